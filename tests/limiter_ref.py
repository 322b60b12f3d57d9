# coding: utf-8
"""The look-ahead peak limiter of include/dv3hip.h (dv3_wave_limit_f32) restated in numpy float64, on numpy alone and
independently of csrc/limiter.hip and of audio.py.  Per span: samples x[0 .. L) (float32), pre-gain g (float32), ceiling
c > 0 (linear), look-ahead A >= 0 samples, release factor rho in [0, 1), and the detector (sample peak, or true peak with
the 3 x 12 table of tests/loudness_ref.py).  Everything between the first and the last line is float64:

    y[n]  = fmul(g, x[n])                                   float32 product, rounded once, then widened; 0 outside the span
    e[n]  = |y[n]|                                          sample-peak detector
            true-peak detector: i_p[m] = sum_j table[p - 1][j] y[m + 6 - j], p = 1 .. 3, m = -1 .. L - 1,
            e[n] = max(|y[n]|, max_p |i_p[n]|, max_p |i_p[n - 1]|)     an interpolant counts for both of its neighbours
    dr[n] = e[n] > c ? 1 - c / e[n] : 0                     the gain reduction this sample demands
    dm[n] = max over j in [n, min(n + A, L - 1)] of dr[j]   look-ahead
    dq[n] = max(dm[n], rho dq[n - 1]),  dq[-1] = 0          instant hold, exponential release
    ds[n] = (1 / (A + 1)) * sum over k in [n - A, n] of dq[max(k, 0)]      attack: a box of the look-ahead's length
    s[n]  = 1 - ds[n]
    out[n] = fmul(y[n], (float) s[n])                       float32, rounded once

Consequences (tests/test_cpu_limiter_ref.py checks each on this file alone):

  ceiling      ds[n] >= dr[n] for every n: every dq[k] of the box, n - A <= k <= n, is at least dm[k], the maximum of dr
               over [k, k + A], and n lies in that window; the clamp max(k, 0) keeps it true for the first A samples
               (dq[0] >= dm[0] >= dr[n] for n <= A).  So s[n] <= c / e[n], and under the sample-peak detector
               |out[n]| = |y[n]| (float) s[n] (1 + d) <= c (1 + 2^-24)^2 <= c (1 + 2^-22): one rounding of s and one of the
               product (plus the rounding of 1 / (A + 1) and of the box sum in float64, far inside the slack);
  no limiting  where nothing exceeds c every table is 0, s is exactly 1 and out[n] = fmul(g, x[n]);
  independence nothing depends on how many spans there are or where a span lies.

The release has two forms here: the sequential recursion, and max over k <= n of dm[k] rho^(n - k) evaluated by doubling
with the powers rho^(2^i) (v[n] = max(v[n], v[n - d] rho^d), d = 1, 2, 4, ..), which is how the device evaluates it: the
same recursion, associative, different only in rounding.

Bounds, derived and not fitted:
  TABLE_TOL  the float64 tables (dq, ds, s) of the device against the sequential form: 1e-12 absolute.  The entries are at
             most 1; the release multiplies at most log2(L) + 11 powers of rho, each rounded once (2^-53 relative), the box
             adds A + 1 <= 513 non-negative terms in a tree of depth <= 10 and multiplies once: a few 1e-15 in all.
  out_bound  against the UNROUNDED product y[n] s[n]: the device rounds its s to float32 (s <= 1: at most 2^-25, bounded
             here by 2^-24) after an error of TABLE_TOL, and rounds the product once (2^-24 relative, of a product that is
             at most |y|): |out - y s| <= |y| (2^-24 + 2^-24 + TABLE_TOL), plus one denormal step."""
import numpy as np

from tests import loudness_ref as LR

TABLE_TOL = 1e-12
COLUMNS = ("gain_min", "over_samples")


def pre(x, g):
    """y = fmul(g, x) in float32, widened"""
    return (np.float32(g) * np.asarray(x, dtype=np.float32)).astype(np.float32).astype(np.float64)


def detector(y, true_peak=False):
    y = np.asarray(y, dtype=np.float64)
    e = np.abs(y)
    if true_peak and y.size:
        t = LR.peak_table().astype(np.float64)
        L = y.size
        pad = np.concatenate([np.zeros(6), y, np.zeros(6)])                 # pad[i + 6] = y[i]
        win = np.stack([pad[11 - j:11 - j + L + 1] for j in range(12)])      # win[j][r] = y[m + 6 - j], m = r - 1
        ip = np.abs(t.dot(win)).max(axis=0)                                  # (L + 1,): m = -1 .. L - 1
        e = np.maximum(e, np.maximum(ip[1:], ip[:-1]))
    return e


def reduction(e, c):
    e = np.asarray(e, dtype=np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(e > c, 1.0 - c / e, 0.0)


def lookahead_max(dr, A):
    dr = np.asarray(dr, dtype=np.float64)
    if dr.size == 0:
        return dr.copy()
    pad = np.concatenate([dr, np.zeros(A)])
    return np.lib.stride_tricks.sliding_window_view(pad, A + 1).max(axis=1)


def release_sequential(dm, rho):
    out = np.empty(len(dm), dtype=np.float64)
    q = 0.0
    for n, v in enumerate(np.asarray(dm, dtype=np.float64).tolist()):
        q = max(v, rho * q)
        out[n] = q
    return out


def rho_powers(rho, count):
    """rho^(2^i), i = 0 .. count - 1, each one float64 pow"""
    return np.array([float(rho) ** (2 ** i) for i in range(count)], dtype=np.float64)


def release_powers(dm, rho):
    """max over k <= n of dm[k] rho^(n - k), by doubling"""
    v = np.array(dm, dtype=np.float64)
    d = 1
    while d < v.size:
        v[d:] = np.maximum(v[d:], v[:-d] * float(rho) ** d)
        d *= 2
    return v


def box(dq, A):
    dq = np.asarray(dq, dtype=np.float64)
    if dq.size == 0:
        return dq.copy()
    pad = np.concatenate([np.full(A, dq[0]), dq])
    return (1.0 / (A + 1)) * np.lib.stride_tricks.sliding_window_view(pad, A + 1).sum(axis=1)


def limit(x, g, c, A, rho, true_peak=False, release="sequential"):
    """one span -> a dict of every table: y, e, dr, dm, dq, ds, s (float64), out (float32), exact (y s, unrounded) and
    report = (gain_min, over_samples)"""
    y = pre(x, g)
    e = detector(y, true_peak)
    dr = reduction(e, float(c))
    dm = lookahead_max(dr, int(A))
    dq = release_sequential(dm, float(rho)) if release == "sequential" else release_powers(dm, float(rho))
    ds = box(dq, int(A))
    s = 1.0 - ds
    out = (y.astype(np.float32) * s.astype(np.float32)).astype(np.float32)
    report = np.array([s.min() if s.size else 1.0, float((dr > 0).sum())], dtype=np.float64)
    return dict(y=y, e=e, dr=dr, dm=dm, dq=dq, ds=ds, s=s, out=out, exact=y * s, report=report)


def out_bound(y):
    return np.abs(y) * (2.0 ** -24 + 2.0 ** -24 + TABLE_TOL) + 2.0 ** -149


# ---- the signals ------------------------------------------------------------------------------------------------------
def spikes(n, seed, at=(), level=0.05, lo=0.5, hi=1.0, extra=4):
    """low-level noise with spikes of lo .. hi (random sign) at the places `at` (those inside [0, n)) and at `extra`
    random ones"""
    rng = np.random.RandomState(seed)
    x = level * rng.randn(n)
    where = [int(i) for i in at if 0 <= int(i) < n]
    if n:
        where += rng.randint(0, n, extra).tolist()
    for i in where:
        x[i] = rng.uniform(lo, hi) * (1.0 if rng.rand() < 0.5 else -1.0)
    return x.astype(np.float32)


SYLLABLES = (0.3, 0.35, 1.0, 0.3, 0.4, 0.3, 0.35, 0.3)


def syllables(fs=22050):
    """eight syllables of 0.22 s -- ten harmonics of 120 Hz, amplitude 1 / sqrt(k + 1), phase 0.7 k^2, under the envelope
    sqrt(sin(pi t / 0.22)) --, each followed by 0.05 s of zeros, amplitudes SYLLABLES (one loud syllable sets the peak),
    the whole scaled to peak 0.5 -> float32 (47624 samples at 22.05 kHz)"""
    n, gap = int(round(0.22 * fs)), int(round(0.05 * fs))
    t = np.arange(n, dtype=np.float64) / float(fs)
    k = np.arange(10, dtype=np.float64)[:, None]
    syl = (np.cos(2.0 * np.pi * 120.0 * (k + 1.0) * t + 0.7 * k * k) / np.sqrt(k + 1.0)).sum(axis=0)
    syl = syl * np.sqrt(np.sin(np.pi * t / 0.22).clip(0.0, None))
    x = np.concatenate([np.concatenate([a * syl, np.zeros(gap)]) for a in SYLLABLES])
    return (0.5 * x / np.abs(x).max()).astype(np.float32)


def integrated(x, fs):
    """BS.1770 integrated loudness of one span by tests/loudness_ref.py"""
    return float(LR.measure([np.asarray(x)], fs)[0][0, 0])


def master(x, fs, target, c, A=None, rho=None, passes=1, true_peak=False, max_gain=10.0 ** 1.5):
    """the mastering chain of audio.master_source on one span in float64: no limiter (A None) -> the static gain
    min(10^((target - L) / 20), c / peak, max_gain); with one the pre-gain min(10^((target - L) / 20), max_gain), re-aimed
    passes - 1 times from the limited loudness, and under the true-peak detector the trim min(1, c / true peak).
    -> the static output, or the list of the outputs after 1, 2, .., passes passes (the passes share their prefix)"""
    x = np.asarray(x, dtype=np.float32)
    g = 10.0 ** ((target - integrated(x, fs)) / 20.0)
    if A is None:
        peak = LR.true_peak(x) if true_peak else float(np.abs(x).max())
        return pre(x, np.float32(min(g, c / peak, max_gain)))
    g = np.float32(min(g, max_gain))
    outs = []
    for p in range(passes):
        if p:
            g = np.float32(min(float(g) * 10.0 ** ((target - integrated(outs[-1], fs)) / 20.0), max_gain))
        outs.append(limit(x, g, c, A, rho, true_peak)["out"])
    trim = lambda o: o.astype(np.float64) * (min(1.0, c / LR.true_peak(o)) if true_peak else 1.0)
    return [trim(o) for o in outs]

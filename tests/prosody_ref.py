# coding: utf-8
"""Float64 restatement of the prosody warp (include/dv3hip.h: dv3_prosody_warp_f32), written from the
definition in the header and not from the kernel.

    out_frames(T, rate, tmin)                      T' = max(tmin, floor((T - 1) / rate + 0.5) + 1)
    split(pos)                                     (floor(pos), the fraction rounded once to fp32), as both axes split
    warp(mag, tlen_in, tlen_out, rate, ratio, W, preserve, T_out, details=False)
        -> out (B, T_out, bins) float64; with details also a dict of the per-element intermediates the error bound needs
    bound(details)                                 the per-element bound of the fp32 kernel's error (derivation below)
    warp_f32_plain(...)                            the ratio == 1 and plain modes in numpy fp32, operation by operation:
                                                   what the kernel must give BIT FOR BIT (no transcendental is involved)
    harmonic_tones(...)                            the pitch-closure fixture of the tests

The fp64 arithmetic here follows the header with one deliberate exception: every product and sum is left unrounded
(float64), only the two fractions and the constant 1e-10 are the fp32 values the kernel uses.
"""
import numpy as np

U = 2.0 ** -24                      # unit roundoff of fp32
FLOOR = float(np.float32(1e-10))    # the kernel's 1e-10f


def out_frames(T, rate, tmin):
    return max(int(tmin), int(np.floor((int(T) - 1) / float(rate) + 0.5)) + 1)


def split(pos):
    pos = np.asarray(pos, dtype=np.float64)
    i0 = np.floor(pos)
    return i0.astype(np.int64), (pos - i0).astype(np.float32).astype(np.float64)


def lerp(a, x, y):
    with np.errstate(invalid="ignore"):
        return np.where(a == 0, x, (1.0 - a) * x + a * y)


def time_split(j, rate, n):
    """output frame(s) j of an item of n frames -> (i0, a, i1)"""
    u = np.minimum(np.asarray(j, dtype=np.float64) * float(rate), float(n - 1))
    i0, a = split(u)
    return i0, a, np.minimum(i0 + 1, n - 1)


def bin_split(bins, ratio):
    """-> (inside bool[bins], s0, fa, s1); outside elements carry (bins - 1, 0, bins - 1)"""
    s = np.arange(bins, dtype=np.float64) / float(ratio)
    inside = s <= bins - 1
    s0, fa = split(np.where(inside, s, float(bins - 1)))
    return inside, s0, fa, np.minimum(s0 + 1, bins - 1)


def envelope(l, W):
    """the triangular moving average of l (bins,), truncated and renormalised at the edges
    -> (E, sum of w |l| / sum of w, number of taps)"""
    wm = _weights(l.shape[0], int(W))
    total = wm.sum(1)
    return wm.dot(l) / total, wm.dot(np.abs(l)) / total, (wm > 0).sum(1).astype(np.float64)


_WEIGHTS = {}


def _weights(bins, W):
    """(bins, bins): row k holds the weights W + 1 - |kk - k| of bin k's window, 0 outside k - W .. k + W"""
    if (bins, W) not in _WEIGHTS:
        k = np.arange(bins)
        _WEIGHTS[(bins, W)] = np.maximum(W + 1 - np.abs(k[None, :] - k[:, None]), 0).astype(np.float64)
    return _WEIGHTS[(bins, W)]


def envelope_literal(l, W):
    """envelope's E, bin by bin as the header writes it (the tests hold the two to each other)"""
    bins = l.shape[0]
    E = np.empty(bins)
    for k in range(bins):
        lo, hi = max(k - W, 0), min(k + W, bins - 1)
        w = (W + 1 - np.abs(np.arange(lo, hi + 1) - k)).astype(np.float64)
        E[k] = (w * l[lo:hi + 1]).sum() / w.sum()
    return E


def _weighted(v, W):
    """the same average of a non-negative row (used for the propagated error of l)"""
    return envelope(v, W)[0]


def warp_frame(x0, x1, a, ratio, W, preserve):
    """one output frame from its two source rows -> dict: out, and the intermediates of the bound"""
    a = float(a)
    m = lerp(a, x0, x1)
    d = {"m": m, "em": np.zeros_like(m) if a == 0 else 3.01 * U * (np.abs((1 - a) * x0) + np.abs(a * x1))}
    if float(ratio) == 1.0:
        d["out"], d["mode"] = m, "copy"
        return d
    inside, s0, fa, s1 = bin_split(m.shape[0], ratio)
    d.update(inside=inside, s0=s0, fa=fa, s1=s1)
    if not preserve:
        d["out"], d["mode"] = np.where(inside, lerp(fa, m[s0], m[s1]), m[-1]), "plain"
        return d
    l = np.log(np.maximum(m, FLOOR))
    E, absE, taps = envelope(l, W)
    X = l - E
    Xs = np.where(inside, lerp(fa, X[s0], X[s1]), 0.0)
    d.update(l=l, E=E, absE=absE, taps=taps, X=X, Xs=Xs, W=W, out=np.exp(E + Xs), mode="envelope")
    return d


def warp(mag, tlen_in, tlen_out, rate, ratio, W, preserve, T_out, details=False):
    mag = np.asarray(mag, dtype=np.float64)
    B, T_in, bins = mag.shape
    tlen_in = [T_in] * B if tlen_in is None else [min(max(int(n), 0), T_in) for n in tlen_in]
    out = np.zeros((B, T_out, bins))
    det = {}
    for b in range(B):
        n = tlen_in[b]
        for j in range(min(max(int(tlen_out[b]), 0), T_out) if n >= 1 else 0):
            i0, a, i1 = time_split(j, rate[b], n)
            d = warp_frame(mag[b, int(i0)], mag[b, int(i1)], a, ratio[b], W, preserve)
            out[b, j] = d["out"]
            d.update(i0=int(i0), a=float(a), i1=int(i1))
            det[(b, j)] = d
    return (out, det) if details else out


# -----------------------------------------------------------------------------------------------------------------------
# The error bound of the fp32 kernel against this file, per element, from the operands (DESIGN.md 4.4's method).
# u = 2^-24.  Every fp32 product, sum and quotient errs by at most u of its result; (1 - a) is itself one rounded
# difference.  The integer / fraction splits are the SAME numbers on both sides (fp64 index arithmetic), so they carry no
# error.  Factors 3.01 / 1.001 absorb the second-order terms ((1 + u)^3 - 1 < 3.01 u).
#
#   lerp(a, x, y), a != 0      three roundings on the x branch ((1 - a), the product, the sum), two on the other:
#                              |err| <= 3.01 u (|(1 - a) x| + |a y|) + (1 - a) err(x) + a err(y);  a == 0: err(x)
#   m                          em = 3.01 u (|(1 - a) x0| + |a x1|)                 (the inputs are exact)
#   copy                       em
#   plain                      lerp's bound on (m[s0], m[s1]) with err = em; outside: em[bins - 1]
#   l = logf(max(m, 1e-10))    the clamp does not enlarge a relative error and log turns it into an absolute one:
#                              el = 3.02 u (0 where em = 0) + 2 u |l|     (logf: documented maximum error 1 ulp <= 2^-23 |l|)
#   E                          n = taps fmaf into a running sum: n u (sum w |l|) / (sum w) (Higham: gamma_n of the sum of
#                              the absolute terms), the quotient u |E|, and the propagated average of el:
#                              eE = avg_w(el) + 1.001 (n u absE + u |E|)
#   X = l - E                  eX = el + eE + 1.001 u |X|
#   X' = lerp(fa, X[s0], X[s1])   lerp's bound with err = eX;  outside: 0, exact
#   arg = E + X'               earg = eE + eX' + 1.001 u |E + X'|
#   out = expf(arg)            out (expm1(earg) + 2 u (1 + earg))            (expf: documented maximum error 1 ulp)
# -----------------------------------------------------------------------------------------------------------------------
def _lerp_bound(fa, v0, v1, e0, e1):
    own = 3.01 * U * (np.abs((1 - fa) * v0) + np.abs(fa * v1))
    return np.where(fa == 0, e0, own + (1 - fa) * e0 + fa * e1)


def frame_bound(d):
    em = d["em"]
    if d["mode"] == "copy":
        return em
    inside, s0, fa, s1 = d["inside"], d["s0"], d["fa"], d["s1"]
    if d["mode"] == "plain":
        m = d["m"]
        return np.where(inside, _lerp_bound(fa, m[s0], m[s1], em[s0], em[s1]), em[-1])
    l, E, X = d["l"], d["E"], d["X"]
    el = np.where(em > 0, 3.02 * U, 0.0) + 2 * U * np.abs(l)
    eE = _weighted(el, d["W"]) + 1.001 * (d["taps"] * U * d["absE"] + U * np.abs(E))
    eX = el + eE + 1.001 * U * np.abs(X)
    eXs = np.where(inside, _lerp_bound(fa, X[s0], X[s1], eX[s0], eX[s1]), 0.0)
    earg = eE + eXs + 1.001 * U * np.abs(E + d["Xs"])
    return d["out"] * (np.expm1(earg) + 2 * U * (1 + earg))


def bound(det, shape):
    """per-element bound for the whole output (zeros where the output is exactly zero)"""
    out = np.zeros(shape)
    for (b, j), d in det.items():
        out[b, j] = frame_bound(d)
    return out


# -----------------------------------------------------------------------------------------------------------------------
# the transcendental-free modes in fp32, operation by operation
# -----------------------------------------------------------------------------------------------------------------------
def _lerp32(a, x, y):
    a = np.asarray(a, dtype=np.float32)
    with np.errstate(invalid="ignore"):
        p0 = (np.float32(1.0) - a) * x
        p1 = a * y
        return np.where(a == 0, x, p0 + p1).astype(np.float32)


def warp_f32_plain(mag, tlen_in, tlen_out, rate, ratio, T_out):
    """preserve_envelope = 0 in numpy fp32 -> (B, T_out, bins) float32, the kernel's output bit for bit"""
    mag = np.asarray(mag, dtype=np.float32)
    B, T_in, bins = mag.shape
    tlen_in = [T_in] * B if tlen_in is None else [min(max(int(n), 0), T_in) for n in tlen_in]
    out = np.zeros((B, T_out, bins), dtype=np.float32)
    for b in range(B):
        n = tlen_in[b]
        for j in range(min(max(int(tlen_out[b]), 0), T_out) if n >= 1 else 0):
            i0, a, i1 = time_split(j, rate[b], n)
            m = _lerp32(np.float32(a), mag[b, int(i0)], mag[b, int(i1)])
            if float(ratio[b]) != 1.0:
                inside, s0, fa, s1 = bin_split(bins, ratio[b])
                m = np.where(inside, _lerp32(fa.astype(np.float32), m[s0], m[s1]), m[-1]).astype(np.float32)
            out[b, j] = m
    return out


# -----------------------------------------------------------------------------------------------------------------------
# the pitch-closure fixture: steady harmonic tones under a formant-like amplitude curve
# -----------------------------------------------------------------------------------------------------------------------
SR, N_FFT, HOP, T_TONES = 22050, 1024, 256, 24
TONE_F0 = (140.0, 205.0)
CLOSURE_SETTINGS = ((4.0, 1.0), (-3.0, 1.0), (0.0, 0.8))           # (semitones, rate)
YIN_LAGS = (SR // 500, -(-SR // 60))                                # tau_min, tau_max
YIN_THRESHOLD = 0.1
CENTS = 25.0


def harmonic_tones(f0s=TONE_F0, T=T_TONES, sr=SR, n_fft=N_FFT, hop=HOP):
    """(len(f0s), (T + 1) hop - n_fft) float64: exactly T lws frames each; harmonics h f0 < 9 kHz with amplitude
    1 / (1 + ((f - 1200) / 500)^2) + 0.05"""
    t = np.arange((T + 1) * hop - n_fft) / float(sr)
    rows = []
    for f0 in f0s:
        x = np.zeros_like(t)
        h = 1
        while h * f0 < 9000.0:
            f = h * f0
            x += (1.0 / (1.0 + ((f - 1200.0) / 500.0) ** 2) + 0.05) * np.sin(2 * np.pi * f * t)
            h += 1
        rows.append(x)
    return np.stack(rows)


def median_f0(f0_rows, Tp):
    """the median over frames 5 .. Tp - 5 of one item's per-frame F0"""
    return float(np.median(np.asarray(f0_rows, dtype=np.float64)[5:Tp - 5]))


def cents(f, g):
    return 1200.0 * np.log2(float(f) / float(g))

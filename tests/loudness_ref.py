# coding: utf-8
"""The loudness measure of include/dv3hip.h (dv3_wave_loudness_f64, dv3_loudness_gate_f64, dv3_loudness_gains_f32)
restated in numpy float64, on numpy alone and independently of csrc/loudness.hip and of audio.py: the K-weighting
coefficients, a sample-by-sample cascade, sub-blocks, blocks and the two gates, the two edge rules, the true-peak table
and estimate, and the gains.  No loudness library is installed, so ITU-R BS.1770's own figures are the anchors
(tests/test_cpu_loudness_ref.py): the coefficient table at 48 kHz and the 997 Hz sine at -3.01 LKFS."""
import math

import numpy as np

COLUMNS = ("lufs", "blocks", "gated_abs", "gated_rel", "momentary_max", "true_peak", "flags")
SHORT, SILENT = 1, 2
NINF = -float("inf")


def step(fs):
    return int(math.floor(0.1 * float(fs) + 0.5))


def coefficients(fs):
    """-> (shelf b, shelf a, high-pass b, high-pass a), each three float64 values with a[0] = 1"""
    fs = float(fs)
    f0, G, Q = 1681.974450955533, 3.999843853973347, 0.7071752369554196
    K = math.tan(math.pi * f0 / fs)
    Vh = 10.0 ** (G / 20.0)
    Vb = Vh ** 0.4996667741545416
    a0 = 1.0 + K / Q + K * K
    sb = np.array([(Vh + Vb * K / Q + K * K) / a0, 2.0 * (K * K - Vh) / a0, (Vh - Vb * K / Q + K * K) / a0])
    sa = np.array([1.0, 2.0 * (K * K - 1.0) / a0, (1.0 - K / Q + K * K) / a0])
    f0, Q = 38.13547087602444, 0.5003270373238773
    K = math.tan(math.pi * f0 / fs)
    a0 = 1.0 + K / Q + K * K
    pb = np.array([1.0, -2.0, 1.0])
    pa = np.array([1.0, 2.0 * (K * K - 1.0) / a0, (1.0 - K / Q + K * K) / a0])
    return sb, sa, pb, pa


def transition(fs):
    """the zero-input transition A of the cascade's state (s1, s2, t1, t2) in transposed direct form II"""
    sb, sa, pb, pa = coefficients(fs)
    return np.array([[-sa[1], 1.0, 0.0, 0.0],
                     [-sa[2], 0.0, 0.0, 0.0],
                     [pb[1] - pa[1] * pb[0], 0.0, -pa[1], 1.0],
                     [pb[2] - pa[2] * pb[0], 0.0, -pa[2], 0.0]])


def cascade(x, fs, state=None):
    """the two biquads sample by sample from `state` (zeros when None) -> (y float64, the end state (4,))"""
    sb, sa, pb, pa = (v.tolist() for v in coefficients(fs))
    s1, s2, t1, t2 = (0.0, 0.0, 0.0, 0.0) if state is None else (float(v) for v in state)
    x = np.asarray(x, dtype=np.float64)
    y = np.empty(x.size, dtype=np.float64)
    for i, v in enumerate(x.tolist()):
        u = sb[0] * v + s1
        s1 = (sb[1] * v - sa[1] * u) + s2
        s2 = sb[2] * v - sa[2] * u
        w = pb[0] * u + t1
        t1 = (pb[1] * u - pa[1] * w) + t2
        t2 = pb[2] * u - pa[2] * w
        y[i] = w
    return y, np.array([s1, s2, t1, t2])


def chunk_states(x, fs):
    """the filter's state before sample k h, k = 0 .. ceil(n / h) - 1, by the sequential filter -> (K, 4)"""
    h = step(fs)
    x = np.asarray(x, dtype=np.float64)
    out, s = [], np.zeros(4)
    for k in range(-(-x.size // h)):
        out.append(s)
        _, s = cascade(x[k * h:(k + 1) * h], fs, s)
    return np.array(out).reshape(-1, 4)


def chunked_states(x, fs):
    """the same by the chunked form: every chunk from a zero state, then s_{k+1} = A^h s_k + e_k"""
    h = step(fs)
    x = np.asarray(x, dtype=np.float64)
    Ah = np.linalg.matrix_power(transition(fs), h)
    out, s = [], np.zeros(4)
    for k in range(-(-x.size // h)):
        out.append(s)
        _, e = cascade(x[k * h:(k + 1) * h], fs)
        s = Ah.dot(s) + e
    return np.array(out).reshape(-1, 4)


def sub_blocks(x, fs):
    """E[k] = the sum of y^2 over samples [k h, (k + 1) h), the last partial sub-block kept -> float64 (ceil(n / h),)"""
    h = step(fs)
    y, _ = cascade(x, fs)
    return np.array([math.fsum((y[k * h:(k + 1) * h] ** 2).tolist()) for k in range(-(-y.size // h))], dtype=np.float64)


def lkfs(z):
    return -0.691 + 10.0 * math.log10(z) if z > 0 else NINF


def blocks(E, n, fs):
    """the z_j of an item of n samples from its sub-block energies -> float64 (J,)"""
    h = step(fs)
    J = (n - 4 * h) // h + 1 if n >= 4 * h else 0
    return np.array([(((E[j] + E[j + 1]) + E[j + 2]) + E[j + 3]) / (4.0 * h) for j in range(J)], dtype=np.float64)


def gate(energies, lengths, fs, peaks=None):
    """one group: its items' sub-block energies and lengths -> (row of COLUMNS, the l_j of the pooled blocks, the
    relative gate or None)"""
    z = np.concatenate([blocks(E, int(n), fs) for E, n in zip(energies, lengths)] + [np.zeros(0)])
    l = np.array([lkfs(v) for v in z])
    peak = max([0.0] + [float(p) for p in (peaks if peaks is not None else [])])
    flags, gamma = 0, None
    n_abs = n_rel = 0
    if z.size == 0:
        flags |= SHORT
        e, n = math.fsum(float(v) for E in energies for v in E), sum(max(int(v), 0) for v in lengths)
        L = lkfs(e / n) if n > 0 and e > 0 else NINF
    else:
        keep = l > -70.0
        n_abs = int(keep.sum())
        if n_abs == 0:
            L = NINF
        else:
            gamma = lkfs(math.fsum(z[keep].tolist()) / n_abs) - 10.0
            keep2 = keep & (l > gamma)
            n_rel = int(keep2.sum())
            L = lkfs(math.fsum(z[keep2].tolist()) / n_rel) if n_rel else NINF
    if L == NINF:
        flags |= SILENT
    row = np.array([L, z.size, n_abs, n_rel, l.max() if l.size else NINF, peak, flags], dtype=np.float64)
    return row, l, gamma


def gate_margin(l, gamma):
    """the distance of the nearest block from either gate, in LU (inf when nothing can flip)"""
    l = np.asarray(l, dtype=np.float64)
    l = l[np.isfinite(l)]
    d = [np.abs(l + 70.0).min()] if l.size else []
    if gamma is not None and l.size:
        d.append(np.abs(l - gamma).min())
    return min(d) if d else float("inf")


def measure(items, fs, groups=None, true_peak_on=False):
    """a list of float32 arrays -> (rows (G, 7), per group (l, gamma), per item E): groups None = every item alone"""
    E = [sub_blocks(x, fs) for x in items]
    pk = [true_peak(x) if true_peak_on else (float(np.abs(x).max()) if len(x) else 0.0) for x in items]
    groups = list(range(len(items) + 1)) if groups is None else list(groups)
    rows, detail = [], []
    for g in range(len(groups) - 1):
        sl = slice(groups[g], groups[g + 1])
        row, l, gamma = gate(E[sl], [len(x) for x in items[sl]], fs, pk[sl])
        rows.append(row)
        detail.append((l, gamma))
    return np.array(rows).reshape(-1, len(COLUMNS)), detail, E


# ---- true peak --------------------------------------------------------------------------------------------------------
def interpolator():
    """g[i] = sinc(i / 4) kaiser(49, 8)[i + 24], i = -24 .. 24, float64 (49,)"""
    i = np.arange(-24, 25, dtype=np.float64)
    return np.sinc(i / 4.0) * np.kaiser(49, 8.0)


def peak_table():
    """phases 1 .. 3 of 12 taps, rounded once to float32: table[p - 1][j] = g[p + 4 (j - 6)] multiplies x[m + 6 - j]"""
    g = interpolator()
    return np.array([[g[24 + p + 4 * (j - 6)] for j in range(12)] for p in (1, 2, 3)]).astype(np.float32)


def true_peak(x, want_abs_sum=False):
    """the largest |.| over the samples and their 3 interpolants each (m = 0 .. n - 1; zeros outside the span), in
    float64 from the float32 table -> the peak (and the largest sum of |tap * sample| of any interpolant)"""
    x = np.asarray(x, dtype=np.float64)
    if x.size == 0:
        return (0.0, 0.0) if want_abs_sum else 0.0
    t = peak_table().astype(np.float64)
    pad = np.concatenate([np.zeros(5), x, np.zeros(6)])                  # pad[m + 5] = x[m]
    win = np.stack([pad[11 - j:11 - j + x.size] for j in range(12)])     # win[j][m] = x[m + 6 - j]
    y = t.dot(win)
    peak = max(float(np.abs(x).max()), float(np.abs(y).max()))
    if want_abs_sum:
        return peak, float(np.abs(t).dot(np.abs(win)).max())
    return peak


# ---- gains ------------------------------------------------------------------------------------------------------------
def gains(rows, goff, target_lufs, ceiling, max_gain):
    """rows (G, 7) -> float32 (B,): float64 throughout, rounded once; ceiling and max_gain linear"""
    rows = np.asarray(rows, dtype=np.float64)
    out = np.zeros(int(goff[-1]), dtype=np.float32)
    for g in range(len(goff) - 1):
        L, P, fl = float(rows[g, 0]), float(rows[g, 5]), int(rows[g, 6])
        q = 1.0
        if not fl & SILENT:
            q = 10.0 ** ((target_lufs - L) / 20.0)
            if P > 0:
                q = min(q, ceiling / P)
            q = min(q, max_gain)
        out[int(goff[g]):int(goff[g + 1])] = np.float32(q)
    return out


# ---- the test signals of the issue ------------------------------------------------------------------------------------
def tone(fs, freq, seconds, dbfs, phase=0.0):
    t = np.arange(int(round(seconds * fs)), dtype=np.float64)
    return 10.0 ** (dbfs / 20.0) * np.sin(2.0 * np.pi * freq * t / fs + phase)


def gating_a(fs):
    """1 kHz at -40 dBFS for 2 s, -20 dBFS for 4 s, -40 dBFS for 2 s"""
    return np.concatenate([tone(fs, 1000.0, 2, -40), tone(fs, 1000.0, 4, -20), tone(fs, 1000.0, 2, -40)]).astype(np.float32)


def gating_b(fs):
    """the -20 dBFS tone for 3 s, 3 s of zeros, 2 s of noise at 1e-5"""
    rng = np.random.RandomState(1770)
    return np.concatenate([tone(fs, 1000.0, 3, -20), np.zeros(3 * int(fs)), 1e-5 * rng.randn(2 * int(fs))]).astype(np.float32)


def faded_tone(fs, freq, phase, amp=0.5, seconds=0.5):
    """amp cos(2 pi freq t + phase), faded in and out over 100 ms (raised cosine)"""
    n = int(round(seconds * fs))
    t = np.arange(n, dtype=np.float64)
    F = int(round(0.1 * fs))
    w = np.ones(n)
    ramp = 0.5 - 0.5 * np.cos(np.pi * (np.arange(F) + 0.5) / F)
    w[:F], w[n - F:] = ramp, ramp[::-1]
    return (amp * w * np.cos(2.0 * np.pi * freq * t / fs + phase)).astype(np.float32)


def interpolator_response(freq_over_fs):
    """|H_p| of the three interpolating phases at a frequency (in units of the sample rate), from the float32 table"""
    t = peak_table().astype(np.float64)
    lag = 6.0 - np.arange(12)                                  # tap j reads x[m + 6 - j]
    return np.abs(t.dot(np.exp(2j * np.pi * freq_over_fs * lag)))


def noise_gain(fs, n):
    """the sum of |impulse response| of the cascade over n samples: the gain from a rounding error to the output"""
    imp = np.zeros(n)
    imp[0] = 1.0
    return float(np.abs(cascade(imp, fs)[0]).sum())


def rounding_gains(fs, n):
    """how a rounding error made INSIDE the cascade spreads: a unit error injected into state variable c at one sample
    moves the later states by the columns of A^m and the later outputs by the cascade's zero-input response.  ->
    (G_state, G_out): the largest row sum over m < n of sum_c |A^m[r][c]|, and sum_m sum_c |y_m from state c| -- the
    sums of |impulse response| from the rounding sites to the states and to the output"""
    A = transition(fs)
    sb, sa, pb, pa = coefficients(fs)
    out_row = np.array([pb[0], 0.0, 1.0, 0.0])                # y = c0 u + t1 with u = s1 at zero input
    P = np.eye(4)
    g_state, g_out = np.zeros(4), 0.0
    for _ in range(int(n)):
        g_state += np.abs(P).sum(axis=1)
        g_out += np.abs(out_row.dot(P)).sum()
        P = A.dot(P)
    return float(g_state.max()), float(g_out)

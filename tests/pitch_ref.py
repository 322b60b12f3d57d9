# coding: utf-8
"""Float64 restatement of the YIN pitch tracker (include/dv3hip.h: dv3_yin_items_f32), written from the
definition in the header and not from the kernel: de Cheveigne & Kawahara 2002, steps 2-5, in the direct difference form.

yin_frames(x, lengths, hop, n_fft, tau_min, tau_max, threshold, sample_rate) -> dict of per-frame arrays over the packed
rows (item b's T_b = lws frames first to last, items in order):
    dprime  (rows, tau_max + 1)   d'(0 .. tau_max)
    lag, f0, ap, power
    a, b, c, D, delta             the parabola's inputs and its vertex
    margin                        the smallest relative gap |p - q| / max(|p|, |q|) by which any comparison of the search
                                  was decided: d'(tau) against the threshold for every tau visited, d'(tau + 1) against
                                  d'(tau) for every step of the descent (the one that stopped it included), and for the
                                  fallback also the gap between the two smallest d' of the range.  0 for an all-zero frame.
    zero                          the frame holds no nonzero sample
    frames                        T_b per item
"""
import numpy as np


def lws_num_frames(length, hop, n_fft):
    pad = n_fft - hop
    return -(-(length + 2 * pad - n_fft) // hop) + 1


def frame_of(x_item, t, hop, n_fft):
    """s[0 .. n_fft): the item with n_fft - hop zeros in front and zeros past its end, from sample t * hop on"""
    L = len(x_item)
    s = np.zeros(n_fft, dtype=np.float64)
    i0 = t * hop - (n_fft - hop)
    lo, hi = max(i0, 0), min(i0 + n_fft, L)
    if hi > lo:
        s[lo - i0:hi - i0] = x_item[lo:hi]
    return s


def _gap(p, q):
    m = max(abs(p), abs(q))
    return abs(p - q) / m if m > 0 else 0.0


def yin_frame(s, tau_min, tau_max, threshold, sample_rate):
    N = len(s)
    W = N - tau_max
    head = s[:W]
    idx = np.arange(W)[:, None] + np.arange(1, tau_max + 1)[None, :]
    diff = head[:, None] - s[idx]
    d = np.concatenate([[0.0], (diff * diff).sum(0)])
    c = np.cumsum(d)
    dp = np.ones(tau_max + 1)
    taus = np.arange(tau_max + 1, dtype=np.float64)
    nz = c > 0
    nz[0] = False
    dp[nz] = d[nz] * taus[nz] / c[nz]
    margin = np.inf
    lag = None
    for tau in range(tau_min, tau_max):
        margin = min(margin, _gap(dp[tau], threshold))
        if dp[tau] < threshold:
            lag = tau
            break
    if lag is not None:
        while lag + 1 < tau_max:
            margin = min(margin, _gap(dp[lag + 1], dp[lag]))
            if not dp[lag + 1] < dp[lag]:
                break
            lag += 1
    else:
        rng = dp[tau_min:tau_max]
        lag = tau_min + int(np.argmin(rng))          # argmin returns the first of equal minima
        two = np.sort(rng)[:2]
        margin = min(margin, _gap(two[0], two[1]))
    a, b, cc = dp[lag - 1], dp[lag], dp[lag + 1]
    D = a - 2.0 * b + cc
    delta = min(max(0.5 * (a - cc) / D, -1.0), 1.0) if D > 0 else 0.0
    zero = not np.any(s)
    return dict(dprime=dp, lag=lag, f0=sample_rate / (lag + delta), ap=b, power=float((s * s).sum() / N), a=a, b=b, c=cc,
                D=D, delta=delta, margin=0.0 if zero else margin, zero=zero)


def yin_frames(x, lengths, hop, n_fft, tau_min, tau_max, threshold, sample_rate):
    x = np.asarray(x, dtype=np.float64)
    rows, frames, o = [], [], 0
    for L in (int(n) for n in lengths):
        T = lws_num_frames(L, hop, n_fft)
        frames.append(T)
        for t in range(T):
            rows.append(yin_frame(frame_of(x[o:o + L], t, hop, n_fft), tau_min, tau_max, threshold, sample_rate))
        o += L
    out = {k: np.array([r[k] for r in rows]) for k in rows[0]}
    out["frames"] = np.array(frames, dtype=np.int64)
    return out


def dprime_bound(n_fft, tau_max):
    """the header's relative bound of d'(tau), at the largest tau: (2 W + tau_max + 8) 2^-24"""
    return (2 * (n_fft - tau_max) + tau_max + 8) * 2.0 ** -24


def pitch_distortion(f0_a, voiced_a, f0_b, voiced_b, path):
    """one item: 1-D tracks and a (P, 2) path with rows of -1 past its end -> the six PITCH_EVAL_COLUMNS as floats"""
    sq, both, err, n = 0.0, 0, 0, 0
    for i, j in np.asarray(path):
        if i < 0 or j < 0:
            continue
        n += 1
        va, vb = bool(voiced_a[i]), bool(voiced_b[j])
        if va and vb:
            both += 1
            sq += (1200.0 * np.log2(float(f0_a[i]) / float(f0_b[j]))) ** 2
        elif va != vb:
            err += 1
    p = np.asarray(path)
    la, lb = int(p[:, 0].max()) + 1, int(p[:, 1].max()) + 1
    return [sq, both, err, n, int(np.sum(np.asarray(voiced_a[:la], dtype=bool))), int(np.sum(np.asarray(voiced_b[:lb], dtype=bool)))]

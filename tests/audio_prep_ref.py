# coding: utf-8
"""fp64 restatements of the two definitions of include/dv3hip.h's ABI 46 entries (numpy / scipy only; this module does
not import the package -- it is what the package is measured against):

  resample(x, up, down)      the rational-ratio band-limited resampler of dv3_resample_items_f32
  trim(y, top_db)            librosa.effects.trim at its defaults (frame_length 2048, hop_length 512, centred frames,
                             reflect padding, ref = max) of dv3_trim_items_f32
"""
import numpy as np
from scipy.special import i0

ZEROS = 64
ROLLOFF = 0.9475937167399596
BETA = 14.769656459379492
FRAME, HOP = 2048, 512


def half_width(up, down):
    """H = ceil(Z / s), s = min(1, up / down), in integers"""
    return ZEROS if up >= down else -(-ZEROS * down // up)


def kernel(t, s):
    """h(t) = s rho sinc(rho s t) w(|t| s / Z), w the Kaiser window (0 from u = 1 on)"""
    t = np.asarray(t, dtype=np.float64)
    u = np.abs(t) * s / ZEROS
    w = np.where(u < 1.0, i0(BETA * np.sqrt(np.clip(1.0 - u * u, 0.0, 1.0))) / i0(BETA), 0.0)
    return s * ROLLOFF * np.sinc(ROLLOFF * s * t) * w


def resample(x, up, down, with_bound=False):
    """y[n] = sum_k x[k] h(n down / up - k), k = i0 - H .. i0 + H + 1 (zeros outside [0, L)), i0 = (n down) div up;
    ceil(L up / down) outputs.  with_bound: also sum_k |h_k x_k| per output (the scale of the fp32 error bound)."""
    x = np.asarray(x, dtype=np.float64)
    L = x.size
    n_out = -(-L * up // down)
    s = min(1.0, up / down)
    H = half_width(up, down)
    T = 2 * H + 2
    xp = np.concatenate([np.zeros(H), x, np.zeros(H + 2 + down)])       # xp[k + H] = x[k]
    y = np.zeros(n_out)
    mag = np.zeros(n_out)
    j = np.arange(T)
    for r in range(min(up, n_out)):                 # outputs n = r, r + up, ... share their coefficients
        n = np.arange(r, n_out, up, dtype=np.int64)
        num = n * down
        i0_ = num // up
        frac = float((r * down) % up) / up
        h = kernel(H - j + frac, s)                 # t = (i0 + frac) - (i0 - H + j)
        seg = xp[i0_[:, None] + j[None, :]]         # x[i0 - H + j]
        y[n] = seg @ h
        mag[n] = np.abs(seg) @ np.abs(h)
    return (y, mag) if with_bound else y


def trim_frame_db(y):
    """the level of each of the 1 + len // 512 frames relative to the loudest one, in dB (fp64)"""
    y = np.asarray(y, dtype=np.float64)
    yp = np.pad(y, FRAME // 2, mode="reflect")
    nf = 1 + y.size // HOP
    mse = np.array([np.mean(yp[f * HOP:f * HOP + FRAME] ** 2) for f in range(nf)])
    db = 10.0 * np.log10(np.maximum(1e-10, mse))
    return db - db.max()


def trim(y, top_db):
    """-> (first sample, length) of the trimmed signal relative to y; y unchanged (0, len) below 1025 samples (it can
    not be reflect-padded); (0, 0) when no frame is above -top_db"""
    n = len(y)
    if n < FRAME // 2 + 1:
        return 0, n
    keep = np.nonzero(trim_frame_db(y) > -top_db)[0]
    if keep.size == 0:
        return 0, 0
    lo = int(keep[0]) * HOP
    hi = min(n, (int(keep[-1]) + 1) * HOP)
    return lo, hi - lo

# coding: utf-8
"""The mel-to-linear estimator of audio.mel_to_linear (include/dv3hip.h: dv3_mel_to_linear_f32),
restated in numpy with a `dtype` argument: float64 is the reference the kernel is compared with, float32 the same
arithmetic at the kernel's precision (the tests take their allowance from the distance of the two).

One item: x (T_b, M) normalised mel, W (M, F) the float32 audio.mel_basis(...) -> (u T_b, F) normalised linear.

  1. time interpolation in the normalised (dB) domain: output frame t reads mel frames i0 = t // u and
     i1 = min(i0 + 1, T_b - 1) with f = (t % u) / u:  x_t = (1 - f) clip(x[i0], 0, 1) + f clip(x[i1], 0, 1)
  2. amplitudes  a_m = 10^((x_t,m (-min_db) + min_db + ref_db) / 20)
  3. start       b = W^T a;  s_k = covered_k (sum_m a_m) / (sum_mk W_mk),  covered_k = (sum_m W_mk > 0)
  4. N updates   r = W s;  d = W^T r;  s <- s * (b / max(d, FLOOR))        (Lee-Seung, the basis fixed)
  5. output      y_k = clip((20 log10(max(10^(min_db / 20), s_k)) - ref_db - min_db) / (-min_db), 0, 1)
"""
import numpy as np

FLOOR = 1e-30


def interpolate(x, u, dtype=np.float64):
    """step 1: (T_b, M) -> (u T_b, M)"""
    x = np.clip(np.asarray(x, dtype=dtype), 0, 1)
    Tb = x.shape[0]
    t = np.arange(u * Tb)
    i0 = t // u
    i1 = np.minimum(i0 + 1, Tb - 1)
    f = ((t % u).astype(dtype) / dtype(u))[:, None]
    return ((dtype(1) - f) * x[i0] + f * x[i1]).astype(dtype)


def amplitudes(x, min_db=-100.0, ref_db=20.0, dtype=np.float64):
    """step 2 (also the inverse of `normalise`): normalised -> amplitude, always > 0"""
    x = np.asarray(x, dtype=dtype)
    e = (x * dtype(-min_db) + dtype(min_db + ref_db)) / dtype(20)
    return np.power(dtype(10), e).astype(dtype)


def normalise(s, min_db=-100.0, ref_db=20.0, dtype=np.float64):
    """step 5: amplitude -> normalised [0, 1] (the db_norm of csrc/audio.hip)"""
    s = np.asarray(s, dtype=dtype)
    floor = np.power(dtype(10), dtype(min_db) / dtype(20)).astype(dtype)
    db = dtype(20) * np.log10(np.maximum(floor, s)) - dtype(ref_db)
    return np.clip((db - dtype(min_db)) / dtype(-min_db), 0, 1).astype(dtype)


def start(a, W):
    """step 3 for amplitudes a (T, M): -> (b (T, F), s (T, F))"""
    colsum = W.sum(axis=0)
    covered = (colsum > 0).astype(W.dtype)
    s = covered[None, :] * (a.sum(axis=1, keepdims=True) / W.sum())
    return a @ W, s.astype(W.dtype)


def update(s, b, W):
    """one update of step 4 on (T, F) rows"""
    d = (s @ W.T) @ W
    return s * (b / np.maximum(d, W.dtype.type(FLOOR)))


def mel_to_magnitude(a, W, n_iter):
    """steps 3-4: amplitudes (T, M) -> the estimate s (T, F) after n_iter updates, in W's dtype"""
    b, s = start(a, W)
    for _ in range(int(n_iter)):
        s = update(s, b, W)
    return s


def mel_to_linear(x, W, u=1, n_iter=32, min_db=-100.0, ref_db=20.0, dtype=np.float64):
    """all five steps for one item: x (T_b, M) -> (u T_b, F) in `dtype`"""
    W = np.asarray(W).astype(dtype)
    x = np.asarray(x)
    if x.shape[0] == 0:
        return np.zeros((0, W.shape[1]), dtype=dtype)
    a = amplitudes(interpolate(x, u, dtype), min_db, ref_db, dtype)
    return normalise(mel_to_magnitude(a, W, n_iter), min_db, ref_db, dtype)


def objective(s, a, W):
    """||W s - a||^2 per frame"""
    return ((s @ W.T - a) ** 2).sum(axis=1)


def mel_of(mag, W, min_db=-100.0, ref_db=20.0, dtype=np.float64):
    """the normalised mel of magnitudes (T, F): what preprocessing writes"""
    return normalise(np.asarray(mag, dtype=dtype) @ np.asarray(W).astype(dtype).T, min_db, ref_db, dtype)


def round_trip(mag, W, n_iter, dtype=np.float64):
    """|norm(W s) - x| per element, x = mel_of(mag): how well the estimate explains the mel it was made from"""
    W = np.asarray(W).astype(dtype)
    x = mel_of(mag, W, dtype=dtype)
    s = mel_to_magnitude(amplitudes(x, dtype=dtype), W, n_iter)
    return np.abs(normalise(s @ W.T, dtype=dtype) - x)


def bin_band(W):
    """brute force: for every bin the [first, last + 1) of the filters whose nonzero band [first bin, last bin] holds it"""
    M, F = W.shape
    lo, hi = np.zeros(M, dtype=np.int64), np.zeros(M, dtype=np.int64)
    for m in range(M):
        nz = np.nonzero(W[m])[0]
        if nz.size:
            lo[m], hi[m] = nz[0], nz[-1] + 1
    out = np.zeros((F, 2), dtype=np.int32)
    for k in range(F):
        ms = [m for m in range(M) if lo[m] <= k < hi[m]]
        if ms:
            assert ms == list(range(ms[0], ms[-1] + 1)), "the filters over bin %d are not a contiguous range" % k
            out[k] = (ms[0], ms[-1] + 1)
    return out


# the framings the tests run: (n_fft, sample_rate, n_mels, fmin, fmax)
CASES = ((1024, 22050, 80, 125.0, 7600.0), (512, 16000, 80, 125.0, 7600.0), (2048, 44100, 80, 125.0, 7600.0),
         (512, 16000, 128, 0.0, 8000.0), (1024, 22050, 20, 0.0, 11025.0), (512, 16000, 13, 55.0, 3000.0))

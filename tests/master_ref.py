# coding: utf-8
"""The three definitions of the mastering stage (include/dv3hip.h: dv3_wave_levels_f32, dv3_wave_gains_f32,
dv3_wave_master_f32) restated in numpy, independently of csrc/master.hip: once in float32 -- every product and sum one
numpy float32 operation, so one rounding each, what the kernel's __fmul_rn / __fadd_rn do; tests/test_gpu_master.py
compares the device bit for bit with it -- and once in float64 (tests/test_cpu_master_ref.py bounds the float32 form's
distance from it).  The dither goes through tests/philox_ref.py.

The reference's whole output stage is one line, audio.save_wav (audio.py:16-18):

    wav *= 32767 / max(0.01, np.max(np.abs(wav)));  wavfile.write(path, sr, wav.astype(np.int16))

Its module cannot be imported here (it needs lws and librosa), so no golden file comes from it: save_wav_samples below
is numpy's own float32 evaluation of that formula as the issue states it, (wav * 32767 / max(0.01, peak)).astype(int16),
and it is the oracle of the "reference" policy."""
import math

import numpy as np

from tests import philox_ref

F32 = np.float32
GAIN_PEAK, GAIN_RMS, GAIN_REFERENCE = 0, 1, 2
MODE_F32, MODE_I16, MODE_I16_REFERENCE = 0, 1, 2
FADE_IN, FADE_OUT = 1, 2


def save_wav_samples(wav):
    """audio.py:17-18 on a float32 array: the int16 samples the reference writes"""
    wav = np.asarray(wav, dtype=np.float32)
    return (wav * 32767 / max(0.01, np.max(np.abs(wav)))).astype(np.int16)


# ---- levels -----------------------------------------------------------------------------------------------------------
def levels_row(x):
    """one item (float32 array) -> (peak, sumsq, sum, over, nonfinite), sumsq and sum EXACTLY rounded (math.fsum of the
    float64 terms; the square of a float32 is exact in float64), plus the sum of |x| over the finite samples"""
    x = np.asarray(x, dtype=np.float32)
    fin = np.isfinite(x)
    xf = x[fin].astype(np.float64)
    peak = float(np.abs(xf).max()) if xf.size else 0.0
    with np.errstate(invalid="ignore"):
        over = int(np.count_nonzero(np.abs(x) >= 1))           # an infinity counts, a NaN does not
    row = (peak, math.fsum((xf * xf).tolist()), math.fsum(xf.tolist()), over, int(np.count_nonzero(~fin)))
    return row, math.fsum(np.abs(xf).tolist())


# ---- gains ------------------------------------------------------------------------------------------------------------
def gains(levels, lengths, goff, policy, target=1.0, ceiling=1.0, max_gain=1.0):
    """levels (B, 5) float64, lengths B ints, goff G + 1 ints -> float32 (B,): float64 throughout, rounded once"""
    levels = np.asarray(levels, dtype=np.float64)
    out = np.zeros(levels.shape[0], dtype=np.float32)
    for g in range(len(goff) - 1):
        b0, b1 = int(goff[g]), int(goff[g + 1])
        P, Q, n = 0.0, 0.0, 0
        for b in range(b0, b1):
            P = max(P, float(levels[b, 0]))
            Q = Q + float(levels[b, 1])                        # ascending item order
            n += max(int(lengths[b]), 0)
        if policy == GAIN_REFERENCE:
            v = max(F32(P), F32(0.01))
        else:
            q = 1.0
            if P > 0 and n > 0 and (policy == GAIN_PEAK or Q > 0):
                q = target / P if policy == GAIN_PEAK else min(target / math.sqrt(Q / float(n)), ceiling / P)
                q = min(q, max_gain)
            v = F32(q)
        out[b0:b1] = v
    return out


# ---- master -----------------------------------------------------------------------------------------------------------
def fade_table(F):
    i = np.arange(int(F), dtype=np.float64)
    return (0.5 - 0.5 * np.cos(np.pi * (i + 0.5) / float(F))).astype(np.float32) if F else np.zeros(0, np.float32)


def dither(n, seed):
    """d(n) for an array of output indices: TPDF from Philox4x32-10, key the two words of seed, counter (n lo, n hi, 0, 0)"""
    n = np.asarray(n, dtype=np.uint64)
    r = philox_ref.philox4x32((n & np.uint64(0xFFFFFFFF), n >> np.uint64(32), 0, 0),
                              (int(seed) & 0xFFFFFFFF, (int(seed) >> 32) & 0xFFFFFFFF))
    u1 = (r[..., 0] >> np.uint32(8)).astype(np.float32) * F32(2.0 ** -24)
    u2 = (r[..., 1] >> np.uint32(8)).astype(np.float32) * F32(2.0 ** -24)
    return u1 - u2


def _weights(L, F, fl, fade, dtype):
    i = np.arange(L)
    w = np.ones(L, dtype=dtype)
    if fl & FADE_IN:
        m = i < F
        w[m] = fade[i[m]]
    if fl & FADE_OUT:
        m = i >= L - F
        w[m] = w[m] * fade[L - 1 - i[m]].astype(dtype)
    return w


def mix(x, src, length, dst, gain, flags, fade, N, dtype=np.float32, reference=False):
    """y[n] of the definition in `dtype` arithmetic (float32: one rounding per operation; float64: the inputs' float32
    values in double) -> (y (N,), the sum of |terms| per sample)"""
    x = np.asarray(x, dtype=np.float32)
    fade = np.asarray(fade, dtype=np.float32)
    F = fade.size
    y, mag, cov = np.zeros(N, dtype=dtype), np.zeros(N, dtype=np.float64), np.zeros(N, dtype=np.int64)
    with np.errstate(all="ignore"):
        for s in range(len(src)):
            L, d = int(length[s]), int(dst[s])
            if L <= 0:
                continue
            xs = x[int(src[s]):int(src[s]) + L].astype(dtype)
            g = dtype(gain[s])
            if reference:
                t = (xs * dtype(32767)) / g
            else:
                t = (g * _weights(L, F, int(flags[s]), fade, dtype)) * xs
            seg = slice(d, d + L)
            y[seg] = np.where(cov[seg] > 0, y[seg] + t, t)
            mag[seg] += np.abs(t.astype(np.float64))
            cov[seg] += 1
    assert cov.max() <= 2
    return y, mag


def master(x, src, length, dst, gain, flags, fade, N, mode, dither_on=False, seed=0):
    """the float32 restatement of dv3_wave_master_f32 -> float32 (N,) or int16 (N,)"""
    y, _ = mix(x, src, length, dst, gain, flags, fade, N, np.float32, mode == MODE_I16_REFERENCE)
    if mode == MODE_F32:
        return y
    with np.errstate(all="ignore"):
        if mode == MODE_I16_REFERENCE:
            r = np.trunc(y)
        else:
            v = y * F32(32767)
            if dither_on:
                v = v + dither(np.arange(N), seed)
            r = np.rint(v)                                     # ties to even
        r = np.where(np.isnan(r), F32(0), np.clip(r, F32(-32768), F32(32767)))
    return r.astype(np.int16)


def issue_layout(F, rng):
    """the segment lengths of the issue {1, F, F + 1, 2F - 1, 5000} with a leading gap, a pause, a crossfade of exactly F
    and the last segment ending at N; sources scattered so that src - dst covers every residue mod 4"""
    length = np.array([1, F, F + 1, 2 * F - 1, 5000], dtype=np.int64)
    flags = np.array([0, 3, 3, 3, 3], dtype=np.int32)
    dst = np.zeros(5, dtype=np.int64)
    dst[0] = 37                                 # a leading gap
    dst[1] = dst[0] + length[0] + 11            # a pause
    dst[2] = dst[1] + length[1]                 # a butt join (a crossfade here would reach back over segment 1's start)
    dst[3] = dst[2] + length[2] + 5
    dst[4] = dst[3] + length[3] - F             # the crossfade of exactly F
    N = int(dst[4] + length[4])
    src = np.zeros(5, dtype=np.int64)
    o = 3
    for s in range(5):
        while (o - dst[s]) % 4 != (s % 4):
            o += 1
        src[s] = o
        o += length[s] + 2
    x = rng.uniform(-1, 1, o + 8).astype(np.float32)
    gain = rng.uniform(0.25, 1.5, 5).astype(np.float32)
    return x, src, length, dst, gain, flags, N

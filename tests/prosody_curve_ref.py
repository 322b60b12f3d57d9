# coding: utf-8
"""Float64 restatement of the prosody marks' three entry points (include/dv3hip.h: dv3_curve_warp_f32,
dv3_curve_plan_f64, dv3_curve_fill_f64), written from the definitions in the header and not from the
kernels.  It reuses tests/prosody_ref.py for what the curve warp shares with the scalar one (warp_frame, frame_bound).

    repair(bounds, nseg, n)                      the bounds as both kernels read them: c_0 .. c_nseg
    seg_frames(c0, c1, rate, last)               len_s
    plan(tlen_in, nseg, bounds, rate, brk, min_frames)              -> (o int64 (B, S + 1), tlen_out int64[B])
    fill(tlen_in, nseg, bounds, rate, semitones, gain_db, brk, o, tlen_out, T_out, R)
                                                 -> (pos, ratio float64, gain float32), each (B, T_out)
    curve_warp(mag, tlen_in, tlen_out, pos, ratio, gain, W, preserve, T_out, details=False)
    curve_bound(details, shape)                  the per-element bound of the fp32 kernel's error
    tables(marks_rows, ...)                      small helper: python rows -> the padded arrays

Python floats are IEEE doubles and every operation below is one rounded operation, as the header writes them, so o,
tlen_out and pos must agree with the kernels BIT FOR BIT; exp2 and pow are library calls on both sides (ratio within
2 ulp; the gain is compared after its rounding to fp32).
"""
import math

import numpy as np

from tests import prosody_ref as P

MAX_RATE, MAX_BREAK = 64, 1048576
U = P.U


def repair(bounds, nseg, n):
    """c_0 = 0, c_s = max(c_{s-1}, min(max(bounds[s], 0), n)), c_nseg = n -> a list of nseg + 1 ints"""
    c = [0]
    for s in range(1, nseg):
        c.append(max(c[-1], min(max(int(bounds[s]), 0), n)))
    c.append(n)
    return c


def _rate(r):
    r = float(r)
    return r if 1.0 / MAX_RATE <= r <= float(MAX_RATE) else 1.0            # (nan fails both tests)


def _brk(v):
    return min(max(int(v), 0), MAX_BREAK)


def seg_frames(c0, c1, rate, last):
    if c1 <= c0:
        return 0
    if last:
        return int(math.floor(float(c1 - 1 - c0) / rate + 0.5)) + 1
    L = float(c1 - c0)
    n = int(math.ceil(L / rate))
    while n > 1 and float(n - 1) * rate >= L:
        n -= 1
    while float(n) * rate < L:
        n += 1
    return n


def _nseg(v, S):
    return min(max(int(v), 1), S)


def plan(tlen_in, nseg, bounds, rate, brk, min_frames):
    B, S = np.asarray(rate).shape
    o = np.zeros((B, S + 1), dtype=np.int64)
    tlen_out = np.zeros(B, dtype=np.int64)
    for b in range(B):
        n, ns = int(tlen_in[b]), _nseg(nseg[b], S)
        c = repair(bounds[b], ns, n)
        at = 0
        for s in range(S):
            if s < ns:
                at += seg_frames(c[s], c[s + 1], _rate(rate[b][s]), c[s + 1] == n) + _brk(brk[b][s])
            o[b, s + 1] = min(at, 2 ** 31 - 1)
        tlen_out[b] = max(int(min_frames), int(o[b, S]))
    return o, tlen_out


def fill(tlen_in, nseg, bounds, rate, semitones, gain_db, brk, o, tlen_out, T_out, R):
    B, S = np.asarray(rate).shape
    pos = np.full((B, T_out), -1.0)
    st = np.zeros((B, T_out))
    db = np.zeros((B, T_out))
    for b in range(B):
        n, ns = int(tlen_in[b]), _nseg(nseg[b], S)
        if n < 1:
            continue
        c = repair(bounds[b], ns, n)
        ob = [int(v) for v in o[b]]
        has = [ob[s + 1] - _brk(brk[b][s]) > ob[s] for s in range(ns)]         # the segment has output frames
        for j in range(min(max(int(tlen_out[b]), 0), T_out)):
            if j >= ob[ns]:                                                    # added by the min_frames clamp
                pos[b, j], st[b, j], db[b, j] = float(n - 1), semitones[b][ns - 1], gain_db[b][ns - 1]
                continue
            s = next(s for s in range(ns) if j < ob[s + 1])
            if j >= ob[s + 1] - _brk(brk[b][s]):
                continue                                                       # in the break: silence
            pos[b, j] = float(c[s]) + float(j - ob[s]) * _rate(rate[b][s])
            st[b, j], db[b, j] = semitones[b][s], gain_db[b][s]
            if R > 0:
                h, lo, first = R // 2, None, 0
                if s + 1 < ns and _brk(brk[b][s]) == 0 and has[s + 1] and j >= ob[s + 1] - h:
                    lo, first = s, ob[s + 1] - h
                elif s > 0 and _brk(brk[b][s - 1]) == 0 and has[s - 1] and j < ob[s] - h + R:
                    lo, first = s - 1, ob[s] - h
                if lo is not None:
                    w = float(j - first + 1) / float(R + 1)
                    st[b, j] = semitones[b][lo] + w * (semitones[b][lo + 1] - semitones[b][lo])
                    db[b, j] = gain_db[b][lo] + w * (gain_db[b][lo + 1] - gain_db[b][lo])
    ratio = np.exp2(st / 12.0)
    gain = np.power(10.0, db / 20.0).astype(np.float32)
    return pos, ratio, gain


def tables(rows, S=None):
    """rows: per item a list of segments (bound of the segment's START, rate, semitones, gain_db, break_frames); the first
    start is ignored (0).  -> dict of the padded arrays: nseg, bounds (B, S + 1), rate, semitones, gain_db, brk (B, S)"""
    B = len(rows)
    S = S or max(len(r) for r in rows)
    t = {"nseg": np.array([len(r) for r in rows], dtype=np.int32), "bounds": np.full((B, S + 1), 2 ** 31 - 1, dtype=np.int32),
         "rate": np.ones((B, S)), "semitones": np.zeros((B, S)), "gain_db": np.zeros((B, S)),
         "brk": np.zeros((B, S), dtype=np.int32)}
    for b, r in enumerate(rows):
        for s, (start, rate, semi, db, brk) in enumerate(r):
            t["bounds"][b, s], t["rate"][b, s], t["semitones"][b, s], t["gain_db"][b, s], t["brk"][b, s] = \
                start, rate, semi, db, brk
    return t


# -----------------------------------------------------------------------------------------------------------------------
# the curve warp
# -----------------------------------------------------------------------------------------------------------------------
def curve_warp(mag, tlen_in, tlen_out, pos, ratio, gain, W, preserve, T_out, details=False):
    """-> out (B, T_out, bins) float64; with details also {(b, j): prosody_ref.warp_frame's dict plus "g" and "v"}.
    The gain enters as the fp32 value the kernel reads; the product is left unrounded."""
    mag = np.asarray(mag, dtype=np.float64)
    B, T_in, bins = mag.shape
    tlen_in = [T_in] * B if tlen_in is None else [min(max(int(n), 0), T_in) for n in tlen_in]
    out = np.zeros((B, T_out, bins))
    det = {}
    for b in range(B):
        n = tlen_in[b]
        for j in range(min(max(int(tlen_out[b]), 0), T_out) if n >= 1 else 0):
            p = float(pos[b][j])
            if not p >= 0.0:
                continue                                                       # silence: the row stays zero
            i0, a = P.split(min(p, float(n - 1)))
            i1 = min(int(i0) + 1, n - 1)
            q = float(ratio[b][j])
            d = P.warp_frame(mag[b, int(i0)], mag[b, i1], a, q if q > 0.0 else 1.0, W, preserve)
            g = float(np.float32(gain[b][j]))
            d.update(i0=int(i0), a=float(a), i1=i1, g=g, v=d["out"])
            out[b, j] = d["v"] if g == 1.0 else d["v"] * g
            det[(b, j)] = d
    return (out, det) if details else out


# The bound: prosody_ref.frame_bound(d) = e bounds the kernel's error on v before the gain.  The kernel then forms ONE
# rounded product fl(v' g) = v' g (1 + delta), |delta| <= u, of its own v' (|v' - v| <= e) with the gain g, which is the
# same fp32 number on both sides.  |fl(v' g) - v g| <= |g| |v' - v| + u |v' g| <= |g| (e + u (|v| + e)).  With g == 1
# there is no product and the bound is e itself.
def curve_frame_bound(d):
    e, g = P.frame_bound(d), abs(d["g"])
    return e if d["g"] == 1.0 else g * (e + U * (np.abs(d["v"]) + e))


def curve_bound(det, shape):
    out = np.zeros(shape)
    for (b, j), d in det.items():
        out[b, j] = curve_frame_bound(d)
    return out


# -----------------------------------------------------------------------------------------------------------------------
# the pitch-closure case of the issue: two parts and a break
# -----------------------------------------------------------------------------------------------------------------------
T_CLOSURE = 48
CLOSURE_ROWS = [(0, 1.0, 0.0, 0.0, 6), (20, 0.8, 4.0, 0.0, 0)]             # [0, 20) plain + 6 silent frames; [20, 48) +4 st at 0.8
CLOSURE_PARTS = ((0, 20, 0.0), (26, 61, 4.0))                              # (first output frame, last + 1, semitones)
CLOSURE_BREAK = (20, 26)
BREAK_DB = 20.0

# coding: utf-8
"""numpy restatements for the guided decode: the guide table of dv3_guide_from_durations_i32 as the header
states it, written as a plain walk over the tokens (not as the kernel's scan + search), and synthesis.fit_durations in
exact rational arithmetic (fractions, not the library's integer quotient / remainder form)."""
from fractions import Fraction

import numpy as np

NEGATIVE, EMPTY, OVER = 1, 2, 4                 # include/dv3hip.h: DV3_GUIDE_*


def guide_table(dur, key_len, T):
    """dur (B, Tk) ints, key_len (B,), T -> (guide (B, T) int32, steps (B,) int32, flags (B,) int32)"""
    dur = np.asarray(dur, dtype=np.int64)
    B, Tk = dur.shape
    guide = np.zeros((B, T), dtype=np.int32)
    steps = np.zeros(B, dtype=np.int32)
    flags = np.zeros(B, dtype=np.int32)
    for b in range(B):
        n_keys = min(max(int(key_len[b]), 1), Tk)
        t, last, total = 0, 0, 0
        for n in range(n_keys):
            d = int(dur[b, n])
            if d < 0:
                flags[b] |= NEGATIVE
                d = 0
            total += d
            for _ in range(d):
                if t < T:
                    guide[b, t] = n
                    last = n
                    t += 1
                else:
                    break
        if total == 0:
            flags[b] |= EMPTY
        if total > T:
            flags[b] |= OVER
        steps[b] = min(total, T)
        guide[b, t:] = last
    return guide, steps, flags


def fit_durations(durations, total_steps, min_steps=0):
    """largest-remainder rounding of min_steps + w[n] * R / sum(w), w = max(d - min_steps, 0), R = total - N * min_steps;
    ties to the earlier token; all-zero weights under min_steps > 0 share R evenly"""
    d = [int(v) for v in durations]
    N, m = len(d), int(min_steps)
    R = int(total_steps) - N * m
    assert N > 0 and min(d) >= 0 and m >= 0 and R >= 0
    w = [max(v - m, 0) for v in d]
    if sum(w) == 0:
        assert m > 0 or R == 0
        w = [1] * N
    share = [Fraction(v * R, sum(w)) for v in w]
    out = [m + int(s // 1) for s in share]
    frac = [s - s // 1 for s in share]
    while sum(out) < int(total_steps):
        n = max(range(N), key=lambda i: (frac[i], -i))
        out[n] += 1
        frac[n] = Fraction(-1)
    return out

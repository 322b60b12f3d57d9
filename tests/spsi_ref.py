# coding: utf-8
"""Float64 restatement of Single Pass Spectrogram Inversion (Beauregard, Harish & Wyse 2015) as audio.spsi_phasor runs it
("A single-pass starting phase"; csrc/spsi.hip): an initial phase for Griffin-Lim built from the
magnitudes alone, without iterating.

Per item an accumulator acc[0 .. F-1] in TURNS (cycles, not radians), zero before the first frame.  Frame t, m = mag[b, t]:

    peak(k)   1 <= k <= F-2 and m[k] > m[k-1] and m[k] >= m[k+1]          (bins 0 and F-1 are never peaks)
    d         0.5 (m[k-1] - m[k+1]) / (m[k-1] - 2 m[k] + m[k+1])          the vertex of the parabola through the three bins;
                                                                          the denominator is < 0 at a peak and |d| <= 0.5
    new[k]    frac(acc[k] + ((hop k) mod n_fft) / n_fft + hop d / n_fft)  the peak's phase advanced by hop x its frequency
    owner(j)  of a non-peak bin: owner(j+1) if j+1 <= F-1 and m[j+1] > m[j] (climb right: a valley goes to the right peak),
              else owner(j-1) if j-1 >= 0 and m[j-1] > m[j] (climb left), else none; a climb that ends on a non-peak
              (a plateau, bin 0, bin F-1) has no owner either
    new[j]    new[owner(j)], 0 without an owner
    acc       <- new  (the whole row, lobes included)
    phasor    (-1)^k exp(2 pi i new[k])

The (-1)^k: both framings of this project reference a frame's transform to the frame's first sample with the window
centred at n_fft / 2, so the bins of one component alternate in sign; the accumulator is kept free of that term.
Frames t >= tlen[b] have the phasor (1, 0) and the turn 0.  The sums are evaluated in the order written, in float64, and
frac(x) = x - floor(x) with a result of 1.0 (x a hair below an integer) taken to 0: the kernel does the same, so the
two agree to the rounding of the final float32 sine and cosine.  tests/test_cpu_spsi_ref.py pins this file;
tests/test_gpu_spsi.py holds the kernel to it."""
import numpy as np


def peaks(m):
    """bool (..., F): the peak bins of each row"""
    m = np.asarray(m, dtype=np.float64)
    p = np.zeros(m.shape, dtype=bool)
    p[..., 1:-1] = (m[..., 1:-1] > m[..., :-2]) & (m[..., 1:-1] >= m[..., 2:])
    return p


def owners_literal(row):
    """int (F,): the owner of every bin of one row by the rule as it is written (a peak owns itself), -1 for none"""
    m = np.asarray(row, dtype=np.float64)
    F = m.shape[0]
    pk = peaks(m)

    def owner(j):
        for _ in range(F + 1):                            # a climb never turns round: at most F - 1 moves
            if pk[j]:
                return j
            if j + 1 <= F - 1 and m[j + 1] > m[j]:
                j += 1
            elif j - 1 >= 0 and m[j - 1] > m[j]:
                j -= 1
            else:
                return -1
        raise AssertionError("a climb did not end")
    return np.array([owner(j) for j in range(F)], dtype=np.int64)


def owners(m):
    """int (..., F): owners_literal for every row at once -- a climb follows a strictly rising (or, leftwards, strictly
    falling) run to its end, and the bin there owns the climber when it is a peak"""
    m = np.asarray(m, dtype=np.float64)
    F = m.shape[-1]
    idx = np.broadcast_to(np.arange(F), m.shape)
    rise = np.zeros(m.shape, dtype=bool)                  # m[j+1] > m[j]
    rise[..., :-1] = m[..., 1:] > m[..., :-1]
    fall = np.zeros(m.shape, dtype=bool)                  # m[j-1] > m[j]
    fall[..., 1:] = m[..., :-1] > m[..., 1:]
    # the end of the rising run from j: the first j' >= j that does not rise
    right = np.minimum.accumulate(np.where(rise, F, idx)[..., ::-1], axis=-1)[..., ::-1]
    # the end, leftwards, of the falling run from j: the last j' <= j with no larger left neighbour
    left = np.maximum.accumulate(np.where(fall, -1, idx), axis=-1)
    end = np.where(rise, right, np.where(fall, left, idx))
    return np.where(np.take_along_axis(peaks(m), end, axis=-1), end, -1)


def _frac(x):
    f = x - np.floor(x)
    return np.where(f >= 1.0, 0.0, f)


def spsi_turns(mag, hop, n_fft, tlen=None):
    """mag (B, T, F = n_fft // 2 + 1) -> (B, T, F) float64: new[k] of every frame, in [0, 1); 0 in frames t >= tlen[b]"""
    mag = np.asarray(mag, dtype=np.float64)
    B, T, F = mag.shape
    assert F == n_fft // 2 + 1 and 0 < hop <= n_fft
    tl = np.full(B, T, dtype=np.int64) if tlen is None else np.asarray(tlen, dtype=np.int64).reshape(B)
    k = np.arange(F)
    base = ((hop * k) % n_fft).astype(np.float64) / n_fft                   # the integer turns of hop k / n_fft removed
    out = np.zeros((B, T, F), dtype=np.float64)
    acc = np.zeros((B, F), dtype=np.float64)
    rows = np.arange(B)[:, None]
    for t in range(T):
        m = mag[:, t]
        pk = peaks(m)
        lo, mid, hi = m[:, :-2], m[:, 1:-1], m[:, 2:]
        den = lo - 2.0 * mid + hi                                           # < 0 at a peak; elsewhere never used
        d = np.zeros((B, F), dtype=np.float64)
        with np.errstate(divide="ignore", invalid="ignore"):
            d[:, 1:-1] = np.where(pk[:, 1:-1], 0.5 * (lo - hi) / den, 0.0)
        new_pk = _frac(acc + base + hop * d / n_fft)
        own = owners(m)
        new = np.where(own >= 0, new_pk[rows, np.maximum(own, 0)], 0.0)
        live = (t < tl)[:, None]
        acc = np.where(live, new, acc)
        out[:, t] = np.where(live, new, 0.0)
    return out


def spsi_phasor(mag, hop, n_fft, tlen=None):
    """-> (B, T, F) complex128 unit phasors: (-1)^k exp(2 pi i new[k]), 1 + 0j in frames t >= tlen[b]"""
    turns = spsi_turns(mag, hop, n_fft, tlen)
    B, T, F = turns.shape
    sign = 1.0 - 2.0 * (np.arange(F) % 2)
    ph = sign * np.exp(2j * np.pi * turns)
    if tlen is not None:
        dead = np.arange(T)[None, :] >= np.asarray(tlen, dtype=np.int64).reshape(B, 1)
        ph = np.where(dead[:, :, None], 1.0 + 0.0j, ph)
    return ph

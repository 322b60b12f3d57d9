# coding: utf-8
"""Float64 restatement of the monotonic alignment search (include/dv3hip.h, dv3_mono_path_f32) -- what
tests/test_gpu_mono_path.py holds the kernels to, itself held to a brute-force enumeration by
tests/test_cpu_mono_ref.py.  Plain loops: every cell is written as the definition reads.

    Pm[t, n] = mean over the layers of attn[l, t, n];   s[t, n] = log(max(Pm[t, n], FLOOR)), a NaN scoring as the floor
    path[0] <= J - 1;   0 <= path[t] - path[t-1] <= J;   path[T-1] >= N - J
    Q[0, n] = s[0, n];   Q[t, n] = s[t, n] + max over 0 <= j <= J of Q[t-1, n-j]
    ties: the smallest advance; among the end keys N - 1 first, a smaller key only when STRICTLY greater.
"""
import numpy as np

COLUMNS = ("feasible", "steps", "keys", "score", "skipped_keys", "longest")
FLOOR = float(np.float32(1e-20))          # DV3_MONO_FLOOR as the kernel holds it
MAX_ADVANCE = 8


def scores(attn):
    """attn (T, N) or (L, T, N) probabilities -> s (T, N) float64; a NaN mean scores as the floor"""
    a = np.asarray(attn, dtype=np.float64)
    if a.ndim == 3:
        m = a[0].copy()
        for l in range(1, a.shape[0]):
            m = m + a[l]
        a = m / a.shape[0]
    a = np.where(np.isnan(a), FLOOR, a)
    return np.log(np.maximum(a, FLOOR))


def search(s, J=1):
    """s: (T, N) float64 scores -> dict(feasible, steps, keys, score, skipped_keys, longest, path, durations): path a
    list of T keys and durations a list of N counts; an infeasible item (T = 0 included) has feasible = 0, score = 0.0,
    an empty path and zero durations"""
    s = np.asarray(s, dtype=np.float64)
    T, N = s.shape
    if not 1 <= J <= MAX_ADVANCE or N < 1:
        raise ValueError("search: J = %d, N = %d" % (J, N))
    none = dict(feasible=0, steps=T, keys=N, score=0.0, skipped_keys=0, longest=0, path=[], durations=[0] * N)
    if T == 0:
        return none
    rows = s.tolist()
    Q = [[None] * N for _ in range(T)]            # None: the cell cannot be reached
    back = [[0] * N for _ in range(T)]
    for n in range(min(J, N)):
        Q[0][n] = rows[0][n]
    for t in range(1, T):
        for n in range(N):
            best, bj = None, 0
            for j in range(0, J + 1):
                if n - j < 0 or Q[t - 1][n - j] is None:
                    continue
                if best is None or Q[t - 1][n - j] > best:
                    best, bj = Q[t - 1][n - j], j
            if best is not None:
                Q[t][n] = rows[t][n] + best
                back[t][n] = bj
    end, ev = None, None
    for n in range(N - 1, max(N - J, 0) - 1, -1):
        if Q[T - 1][n] is not None and (ev is None or Q[T - 1][n] > ev):
            end, ev = n, Q[T - 1][n]
    if end is None:
        return none
    path = [end]
    for t in range(T - 1, 0, -1):
        path.append(path[-1] - back[t][path[-1]])
    path.reverse()
    dur = [0] * N
    for n in path:
        dur[n] += 1
    return dict(feasible=1, steps=T, keys=N, score=ev, skipped_keys=sum(1 for d in dur if d == 0), longest=max(dur),
                path=path, durations=dur)


def mono_path(attn, J=1):
    """attn (T, N) or (L, T, N), already cut to the item's lengths -> the dict of search"""
    return search(scores(attn), J)


def path_ok(path, T, N, J):
    """does `path` (a sequence of keys) satisfy the three rules for T steps over N keys?"""
    p = [int(v) for v in path]
    if len(p) != T or T == 0:
        return False
    if any(v < 0 or v >= N for v in p):
        return False
    if p[0] > J - 1 or p[-1] < N - J:
        return False
    return all(0 <= b - a <= J for a, b in zip(p[:-1], p[1:]))


def path_score(s, path):
    """the scores summed along a path, in float64"""
    return float(sum(s[t, int(n)] for t, n in enumerate(path)))

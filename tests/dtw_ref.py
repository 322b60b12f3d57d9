# coding: utf-8
"""Float64 restatement of the batched DTW and of the mel-cepstral features (include/dv3hip.h,
dv3_dtw_f32) -- what tests/test_gpu_dtw.py holds the kernels to, itself held to hand-worked cases by
tests/test_cpu_dtw_ref.py.  Plain loops: every cell is written as the definition reads.

    d(i, j) = sqrt(sum_k (x[i, k] - y[j, k])^2)
    C(0, 0) = d(0, 0);  C(i, j) = d(i, j) + min(C(i-1, j-1), C(i-1, j), C(i, j-1))
    ties: diagonal, then x advances (from (i-1, j)), then y advances (from (i, j-1)); a later predecessor replaces an
    earlier one only when it is STRICTLY smaller.
"""
import numpy as np

COLUMNS = ("cost", "path_len", "n_diag", "n_x_only", "n_y_only")


def distances(x, y):
    """(Lx, D), (Ly, D) -> (Lx, Ly) float64, from the differences themselves"""
    x = np.asarray(x, dtype=np.float64)
    y = np.asarray(y, dtype=np.float64)
    diff = x[:, None, :] - y[None, :, :]
    return np.sqrt((diff * diff).sum(axis=2))


def dtw_from_distances(d):
    """d: (Lx, Ly) local costs -> dict(cost, path_len, n_diag, n_x_only, n_y_only, path); path is a list of (i, j) from
    (0, 0) to (Lx - 1, Ly - 1), found by backtracking the stored choices.  A zero length: zeros and an empty path."""
    d = np.asarray(d, dtype=np.float64)
    Lx, Ly = d.shape
    if Lx == 0 or Ly == 0:
        return dict(cost=0.0, path_len=0, n_diag=0, n_x_only=0, n_y_only=0, path=[])
    rows = d.tolist()
    C = [[0.0] * Ly for _ in range(Lx)]
    step = [[0] * Ly for _ in range(Lx)]          # 0 diagonal, 1 x advanced, 2 y advanced
    for i in range(Lx):
        for j in range(Ly):
            if i == 0 and j == 0:
                C[0][0] = rows[0][0]
                continue
            best, which = None, 0
            if i > 0 and j > 0:
                best, which = C[i - 1][j - 1], 0
            if i > 0 and (best is None or C[i - 1][j] < best):
                best, which = C[i - 1][j], 1
            if j > 0 and (best is None or C[i][j - 1] < best):
                best, which = C[i][j - 1], 2
            C[i][j] = rows[i][j] + best
            step[i][j] = which
    path = [(Lx - 1, Ly - 1)]
    count = [0, 0, 0]
    i, j = Lx - 1, Ly - 1
    while (i, j) != (0, 0):
        s = step[i][j]
        count[s] += 1
        if s != 2:
            i -= 1
        if s != 1:
            j -= 1
        path.append((i, j))
    path.reverse()
    return dict(cost=C[Lx - 1][Ly - 1], path_len=len(path), n_diag=count[0], n_x_only=count[1], n_y_only=count[2],
                path=path)


def dtw(x, y):
    """x (Lx, D), y (Ly, D) -> the dict of dtw_from_distances"""
    x = np.asarray(x, dtype=np.float64)
    y = np.asarray(y, dtype=np.float64)
    if x.shape[0] == 0 or y.shape[0] == 0:
        return dtw_from_distances(np.zeros((x.shape[0], y.shape[0])))
    return dtw_from_distances(distances(x, y))


def path_cost(d, path):
    """the local costs summed along a path, in float64"""
    return float(sum(d[i, j] for i, j in path))


def mel_cepstra(mel, min_level_db=-100.0, order=13):
    """normalised mel (..., M) in [0, 1] -> (..., order) float64:
    f_k = (1 / sqrt 2) (1 / M) sum_m dB_m cos(pi k (m + 1/2) / M), k = 1 .. order, dB = clip(mel, 0, 1) * (-min) + min"""
    mel = np.asarray(mel, dtype=np.float64)
    M = mel.shape[-1]
    if not 1 <= order <= M - 1:
        raise ValueError("order %d outside [1, %d]" % (order, M - 1))
    db = np.clip(mel, 0.0, 1.0) * (-min_level_db) + min_level_db
    out = np.zeros(mel.shape[:-1] + (order,), dtype=np.float64)
    for k in range(1, order + 1):
        for m in range(M):
            out[..., k - 1] += db[..., m] * np.cos(np.pi * k * (m + 0.5) / M)
    return out / (np.sqrt(2.0) * M)

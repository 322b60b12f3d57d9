# coding: utf-8
"""numpy restatement of dv3_alignment_stats_f32 (include/dv3hip.h), written from the table of its
columns and not from the kernel: one item's stored attention rows -> its 13 statistics.  The fp32 inputs are widened to
float64 for the two focus columns; every other column is an integer."""
import numpy as np

COLUMNS = ("steps", "keys", "focus_mean", "focus_min", "last_key", "furthest_key", "end_step", "tail_steps",
           "covered_keys", "back_steps", "max_jump", "longest_stall", "bad_rows")


def row_path_peak(row):
    """one row over the item's own keys -> (path, peak, bad)"""
    row = np.asarray(row, dtype=np.float64)
    total = row.sum()
    best, arg = -np.inf, None
    for n, v in enumerate(row):
        if v > best:                 # first maximum; a NaN never compares greater
            best, arg = v, n
    if not np.isfinite(total) or total <= 0 or arg is None:
        return 0, 0.0, True
    return arg, best / total, False


def item_stats(attn, steps, key_len):
    """attn (T, Tk) rows of ONE item (anything array-like), steps / key_len: its counts, clamped to [0, T] / [1, Tk]
    -> dict keyed by COLUMNS (Python ints, floats for the focus columns)"""
    attn = np.asarray(attn)
    T, Tk = attn.shape
    Tb = min(max(int(steps), 0), T)
    Nb = min(max(int(key_len), 1), Tk)
    with np.errstate(all="ignore"):
        rows = [row_path_peak(attn[t, :Nb]) for t in range(Tb)]
    path = [r[0] for r in rows]
    peak = [r[1] for r in rows]
    out = dict(steps=Tb, keys=Nb)
    out["focus_mean"] = float(np.mean(peak)) if Tb else 0.0
    out["focus_min"] = float(np.min(peak)) if Tb else 0.0
    out["last_key"] = path[-1] if Tb else 0
    out["furthest_key"] = max(path) if Tb else 0
    ends = [t for t in range(Tb) if path[t] >= Nb - 1]
    out["end_step"] = ends[0] if ends else -1
    out["tail_steps"] = Tb - 1 - ends[0] if ends else 0
    out["covered_keys"] = len(set(path))
    prev = [0] + path[:-1]                       # path[-1] = 0
    out["back_steps"] = sum(1 for t in range(1, Tb) if path[t] < prev[t])
    out["max_jump"] = max([0] + [path[t] - prev[t] for t in range(Tb)])
    longest = run = 0
    for t in range(Tb):
        run = run + 1 if t > 0 and path[t] == path[t - 1] else 1
        longest = max(longest, run)
    out["longest_stall"] = longest
    out["bad_rows"] = sum(1 for r in rows if r[2])
    return out


def batch_stats(attn, steps, key_len, layout="btk"):
    """attn (B, T, Tk) or, layout "tbk", (T, B, Tk) -> one dict per item"""
    attn = np.asarray(attn)
    if layout == "tbk":
        attn = attn.transpose(1, 0, 2)
    return [item_stats(attn[b], steps[b], key_len[b]) for b in range(attn.shape[0])]

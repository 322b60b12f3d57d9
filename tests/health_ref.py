# coding: utf-8
"""numpy / float64 reference of the training-health pieces: the guard rule of the guarded update pass,
the six columns of the per-tensor table from fp32 inputs, and the invariants of the chunk table."""
import numpy as np

COLUMNS = ("grad_sumsq", "grad_absmax", "grad_nonfinite", "param_sumsq", "param_absmax", "update_sumsq")
# relative bound of the three sums: every term is non-negative, so the error is at most (longest chain of fp32
# roundings) * 2^-24 -- the chain is 39 deep at most, the budget 64
SUM_RTOL = 64.0 * 2.0 ** -24


def skips(norm):
    """the guard rule: a pass is refused when the norm word it reads (fp32) is NaN or +-Inf"""
    with np.errstate(over="ignore"):
        return not bool(np.isfinite(np.float32(norm)))


def norm_f32_overflows(g):
    """does the sum of squares of g leave the fp32 range (the norm kernel then writes +Inf for a finite gradient)?"""
    g = np.asarray(g, dtype=np.float64)
    return bool(np.isfinite(g).all() and (g * g).sum() > float(np.finfo(np.float32).max))


def columns(p, g, m, v, hyper, offsets, sizes, grad_prescale=1.0, eps=1e-6, skipped=False):
    """-> float64 [n_tensors][6] from fp32 arenas.  prescale * g is the fp32 product (the kernel takes the maximum of
    it, exactly); squares and sums in float64.  hyper = (lr, 1 - beta1^t, sqrt(1 - beta2^t)) as fp32 words."""
    p, g, m, v = (np.asarray(a, dtype=np.float32) for a in (p, g, m, v))
    h = np.asarray(hyper, dtype=np.float32).astype(np.float64)
    out = np.zeros((len(sizes), len(COLUMNS)), dtype=np.float64)
    for t, (o, n) in enumerate(zip(offsets, sizes)):
        gt, pt = g[o:o + n], p[o:o + n].astype(np.float64)
        ok = np.isfinite(gt)
        x = (np.float32(grad_prescale) * np.abs(gt[ok])).astype(np.float32).astype(np.float64)
        out[t, 0] = (x * x).sum()
        out[t, 1] = x.max() if x.size else 0.0
        out[t, 2] = float(n - int(ok.sum()))
        out[t, 3] = (pt * pt).sum()
        out[t, 4] = np.abs(pt).max()
        if not skipped:
            mt, vt = m[o:o + n].astype(np.float64), v[o:o + n].astype(np.float64)
            d = (h[0] / h[1]) * mt / (np.sqrt(vt) / h[2] + float(np.float32(eps)))
            out[t, 5] = (d * d).sum()
    return out


def check_chunks(chunks, ranges, offsets, sizes, total, chunk=4096):
    """the invariants of train_step.arena_chunks; raises AssertionError with the first one that fails"""
    chunks, ranges = np.asarray(chunks), np.asarray(ranges)
    assert chunks.dtype == np.int64 and ranges.dtype == np.int64
    assert chunks.ndim == 2 and chunks.shape[1] == 3 and ranges.shape == (len(sizes), 2)
    cover = np.zeros(total, dtype=np.int64)
    owner = np.full(total, -1, dtype=np.int64)
    for t, (o, n) in enumerate(zip(offsets, sizes)):
        owner[o:o + n] = t
    for off, length, t in chunks:
        assert off % 4 == 0, "a chunk starts off a 16-byte boundary"
        assert 0 < length <= chunk, "a chunk's length is outside (0, chunk]"
        assert 0 <= off and off + length <= total
        assert (owner[off:off + length] == t).all(), "a chunk crosses a tensor, covers padding or names another tensor"
        cover[off:off + length] += 1
    assert (cover[owner >= 0] == 1).all(), "a tensor element is not covered exactly once"
    assert (cover[owner < 0] == 0).all(), "a padding element is covered"
    row = 0
    for t, (first, count) in enumerate(ranges):
        assert first == row and count == -(-sizes[t] // chunk), "ranges is not the run of the tensor's rows"
        rows = chunks[first:first + count]
        assert (rows[:, 2] == t).all()
        assert rows[0, 0] == offsets[t]
        assert (np.diff(rows[:, 0]) == rows[:-1, 1]).all(), "a tensor's chunks are not contiguous and ascending"
        row += count
    assert row == chunks.shape[0]

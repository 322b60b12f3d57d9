# coding: utf-8
"""No GPU: proves tests/footprint_ref.py, the placements and guard-band checks tests/test_gpu_gemm_footprint.py rests on.

numpy "kernels" that address a placed flat buffer through (base, batch stride, row stride) exactly as the HIP kernels
address a descriptor: a 1 x 1 convolution (sum over channels; output (B, M, T)) and a weight gradient (sum over frames;
output slabs).  The correct kernels are clean under every placement; each mutant -- a store or a load that a real edge
tile could get wrong -- is reported, at the place it happened:

  * a 4-wide store at a row tail that overshoots by 1, 2, 3 elements;      * a store one row past M;
  * a store before the base;                                               * a store into the batch gap;
  * a row written at dense stride into a strided view;
  * a load of 8 elements at a row tail that is MULTIPLIED by a zero mask instead of selected (NaN reaches the output);
  * a load of row Cin (one past the last channel) against a zero weight.

The placements' own claims (the table of footprint_ref.py) are asserted too: the view covers exactly the logical
elements, the base alignment and rs % 4 / bs % 4 are as stated, the bands have the stated size.
"""
import numpy as np
import pytest
import torch

from tests import footprint_ref as FP

CPU = torch.device("cpu")
SHAPE = (3, 5, 13)              # B, C, T: T % 4 == 1 and T % 8 != 0; more than one batch item
M = 6


def _inputs(seed=0):
    rng = np.random.RandomState(seed)
    B, C, T = SHAPE
    x = rng.randint(-7, 8, size=SHAPE).astype(np.float32)
    w = rng.randint(-7, 8, size=(M, C)).astype(np.float32)
    g = rng.randint(-7, 8, size=(B, M, T)).astype(np.float32)
    return x, w, g


def _flat(buf):
    return buf.numpy()          # shares the buffer's memory


def conv_kernel(xbuf, w, ybuf, mutant=None, dense_out=False):
    """y[b, m, t] = sum_c w[m, c] x[b, c, t] on flat buffers"""
    X, Y, xl, yl = _flat(xbuf), _flat(ybuf), xbuf.fp_layout, ybuf.fp_layout
    B, C, T = xl.shape
    Mo = w.shape[0]
    (xbs, xrs), (ybs, yrs) = xl.strides[:2], yl.strides[:2]
    if dense_out:
        ybs, yrs = Mo * T, T
    rows_in = C + 1 if mutant == "row_cin" else C
    wk = np.concatenate([w, np.zeros((Mo, 1), np.float32)], 1) if mutant == "row_cin" else w
    for b in range(B):
        rows = np.stack([X[xl.base + b * xbs + c * xrs: xl.base + b * xbs + c * xrs + T] for c in range(rows_in)])
        with np.errstate(invalid="ignore"):
            acc = (wk[:, :, None] * rows[None]).sum(1).astype(np.float32)       # no BLAS: NaN * 0 must stay NaN
        for m in range(Mo):
            o = yl.base + b * ybs + m * yrs
            Y[o: o + T] = acc[m]
            if mutant in ("tail1", "tail2", "tail3"):
                Y[o + T: o + T + int(mutant[4])] = 0.0
        if mutant == "row_m":
            o = yl.base + b * ybs + Mo * yrs
            Y[o: o + T] = 0.0
        if mutant == "batch_gap" and b + 1 < B:
            Y[yl.base + b * ybs + Mo * yrs] = 0.0
    if mutant == "before_base":
        Y[yl.base - 2] = 0.0


def wgrad_kernel(gbuf, xbuf, obuf, S, mul_mask):
    """out[s][0][m][c] = sum_{b = s mod S} sum_t g[b, m, t] x[b, c, t]; x is read 8 frames at a time, the frames past the row
    end removed by a select (mul_mask False) or by a product with a 0 / 1 mask (True: the mutant)"""
    G, X, O, gl, xl, ol = _flat(gbuf), _flat(xbuf), _flat(obuf), gbuf.fp_layout, xbuf.fp_layout, obuf.fp_layout
    B, Mo, T = gl.shape
    C = xl.shape[1]
    Tp = (T + 7) // 8 * 8
    keep = (np.arange(Tp) < T)
    acc = np.zeros((S, Mo, C), np.float32)
    for b in range(B):
        g = np.stack([G[gl.base + b * gl.strides[0] + m * gl.strides[1]:][:T] for m in range(Mo)])
        xr = np.stack([X[xl.base + b * xl.strides[0] + c * xl.strides[1]:][:Tp] for c in range(C)])
        with np.errstate(invalid="ignore"):
            xr = xr * keep.astype(np.float32) if mul_mask else np.where(keep, xr, np.float32(0))
            acc[b % S] += (g[:, None, :] * xr[None, :, :T]).sum(2) + (0 * xr[None, :, T:]).sum(2)
    s_axis = ol.names.index("s")
    for s in range(S):
        for m in range(Mo):
            idx = {"s": s, "j": 0, "m": m}
            o = ol.base + sum(idx[n] * st for n, st in zip(ol.names[:3], ol.strides[:3]))
            O[o: o + C] = acc[s, m]
    assert s_axis in (0, 2)


def _want(x, w):
    return torch.from_numpy(np.einsum("mc,bct->bmt", w, x))


@pytest.mark.parametrize("placement", FP.PLACEMENTS)
def test_placements_are_what_the_table_says(placement):
    B, C, T = SHAPE
    x = _inputs()[0]
    buf, view = FP.place(x, placement, CPU)
    lay = buf.fp_layout
    assert torch.equal(view, torch.from_numpy(x)) and tuple(view.shape) == SHAPE
    # the view covers exactly the logical elements: they are the words that no longer hold the sentinel
    live = (buf.view(torch.int32) != FP.SENTINEL).nonzero().reshape(-1).numpy()
    assert np.array_equal(live, np.sort(lay.offsets())) and live.size == B * C * T == np.unique(lay.offsets()).size
    bs, rs = view.stride(0), view.stride(1)
    assert view.stride(2) == 1 and (bs, rs) == FP.strides3(SHAPE, placement)
    assert view.data_ptr() % 16 == 4 * FP.base_offset(placement)
    if placement == "strided4":
        assert rs % 4 == 0 and rs > T and bs % 4 == 0 and bs > C * rs
    elif placement == "strided1":
        assert rs % 4 == 1 and rs > T and bs % 4 != 0 and bs > C * rs
    else:
        assert rs == T and bs == C * T
    # the band rule
    need = 256 * rs + 256
    assert FP.band_elems(rs) == need and lay.base >= need and lay.n - (lay.base + lay.span) >= need
    assert FP.violations(buf) == [] and not FP.poisoned(view) and FP.unwritten(view) == 0
    # an output: nothing but the sentinel, every logical word unwritten
    obuf, oview = FP.place(SHAPE, placement, CPU)
    assert FP.unwritten(oview) == B * C * T and FP.poisoned(oview) and FP.violations(obuf) == []


@pytest.mark.parametrize("rows_of_slabs", [False, True])
@pytest.mark.parametrize("placement", FP.PLACEMENTS)
def test_slab_placements(placement, rows_of_slabs):
    S, J, Mo, Cin = 3, 2, 5, 6
    buf, view, ldo = FP.place_slabs(S, J, Mo, Cin, placement, CPU, rows_of_slabs)
    lay = buf.fp_layout
    assert ldo == {"strided4": 12, "strided1": 9}.get(placement, Cin)
    assert tuple(view.shape) == ((J, Mo, S, Cin) if rows_of_slabs else (S, J, Mo, Cin))
    # the strides ops.wgrad_gemm derives from ldo: slab stride / row stride
    if rows_of_slabs:
        assert view.stride() == (Mo * S * ldo, S * ldo, ldo, 1)
    else:
        assert view.stride() == (J * Mo * ldo, Mo * ldo, ldo, 1)
    assert view.data_ptr() % 16 == 4 * FP.base_offset(placement)
    view.copy_(torch.arange(view.numel(), dtype=torch.float32).reshape(view.shape))
    live = (buf.view(torch.int32) != FP.SENTINEL).nonzero().reshape(-1).numpy()
    assert np.array_equal(live, np.sort(lay.offsets())) and live.size == S * J * Mo * Cin
    assert lay.base >= 256 * ldo + 256 and lay.n - (lay.base + lay.span) >= 256 * ldo + 256
    assert FP.violations(buf) == []
    if ldo > Cin:               # a store into the slack of a padded row is named
        _flat(buf)[lay.base + Cin] = 1.0
        v = FP.violations(buf)
        rows = "gap between %s items" % ("s" if rows_of_slabs else "m")       # the axis whose stride is ldo
        assert len(v) == 1 and v[0].where == rows and v[0].distance == 1 and v[0].nearest == (0, 0, 0, Cin - 1)


@pytest.mark.parametrize("placement", FP.PLACEMENTS)
def test_correct_kernels_are_clean(placement):
    x, w, g = _inputs()
    xbuf, _ = FP.place(x, placement, CPU)
    ybuf, y = FP.place((SHAPE[0], M, SHAPE[2]), placement, CPU)
    conv_kernel(xbuf, w, ybuf)
    assert FP.violations(ybuf) == [] and FP.violations(xbuf) == []
    assert not FP.poisoned(y) and FP.unwritten(y) == 0 and torch.equal(y, _want(x, w))
    gbuf, _ = FP.place(g, placement, CPU)
    for rows in (False, True):
        obuf, o, ldo = FP.place_slabs(2, 1, M, SHAPE[1], placement, CPU, rows)
        wgrad_kernel(gbuf, xbuf, obuf, 2, mul_mask=False)
        assert FP.violations(obuf) == [] and not FP.poisoned(o) and FP.unwritten(o) == 0
        got = (o.permute(2, 0, 1, 3) if rows else o).sum(0)[0]
        assert torch.equal(got, torch.from_numpy(np.einsum("bmt,bct->mc", g, x)))


def _mutant(placement, mutant, **kw):
    x, w, _ = _inputs()
    xbuf, _ = FP.place(x, placement, CPU)
    ybuf, y = FP.place((SHAPE[0], M, SHAPE[2]), placement, CPU)
    conv_kernel(xbuf, w, ybuf, mutant, **kw)
    return FP.violations(ybuf), y, _want(x, w)


@pytest.mark.parametrize("over", [1, 2, 3])
@pytest.mark.parametrize("placement", FP.PLACEMENTS)
def test_store_past_a_row_tail_is_reported(placement, over):
    B, C, T = SHAPE
    v, y, want = _mutant(placement, "tail%d" % over)
    last = (B - 1, M - 1, T - 1)
    after = [e for e in v if e.where == "band after"]
    # the last row's overshoot lands in the band behind the tensor, 1 .. over elements past its last element
    assert [(e.nearest, e.distance) for e in after] == [(last, k + 1) for k in range(over)]
    if placement.startswith("strided"):
        # ... and every other row's in the slack behind it: `over` words per row, each right behind its own row
        assert len(v) == B * M * over
        rows = [e for e in v if e.where == "gap between row items"]
        gap = FP.strides3((B, M, T), placement)[1] - T
        # (nearest: the row's own last element, unless the next row's head is closer)
        assert len(rows) == B * (M - 1) * over and all(
            (e.nearest[2] == T - 1 and 1 <= e.distance <= over) or (e.nearest[2] == 0 and e.distance < 0 and
                                                                     gap + e.distance <= over) for e in rows)
        assert sum(e.where == "gap between b items" for e in v) == (B - 1) * over
    else:
        assert len(v) == over         # dense: the other overshoots fall on the next row's head, which that row rewrites
    assert torch.equal(y, want)       # the logical output alone would not have shown it
    assert FP.describe(v).startswith("%d stray words: word " % len(v))
    assert "band after" in repr(after[0]) and "t=%d" % (T - 1) in repr(after[0])


@pytest.mark.parametrize("placement", FP.PLACEMENTS)
def test_store_one_row_past_M_is_reported(placement):
    B, C, T = SHAPE
    v, y, want = _mutant(placement, "row_m")
    after = [e for e in v if e.where == "band after"]
    assert len(after) == T and all(e.nearest == (B - 1, M - 1, T - 1) for e in after)
    rs = FP.strides3((B, M, T), placement)[1]
    assert [e.distance for e in after] == [rs - T + 1 + k for k in range(T)]
    if placement.startswith("strided"):
        # row M of an inner batch item starts in the batch gap (8 / 1 .. 3 words wide) and runs on into the next item's first
        # row, which that item rewrites: the gap words remain
        gap = [e for e in v if e.where == "gap between b items"]
        assert len(gap) > 0 and len(v) == len(after) + len(gap)
    else:
        assert len(v) == T
    assert torch.equal(y, want)


@pytest.mark.parametrize("placement", FP.PLACEMENTS)
def test_store_before_the_base_is_reported(placement):
    v, y, want = _mutant(placement, "before_base")
    assert len(v) == 1 and v[0].where == "band before" and v[0].nearest == (0, 0, 0) and v[0].distance == -2
    assert v[0].bits == 0 and torch.equal(y, want)


@pytest.mark.parametrize("placement", ["strided4", "strided1"])
def test_store_into_the_batch_gap_is_reported(placement):
    B, C, T = SHAPE
    v, y, want = _mutant(placement, "batch_gap")
    bs, rs = FP.strides3((B, M, T), placement)
    assert len(v) == B - 1 and all(e.where == "gap between b items" for e in v)
    # the word right behind the last row's stride slot: nearer to the next item's first element when the gap is short
    for b, e in enumerate(v):
        to_prev, to_next = rs - T + 1, bs - M * rs
        assert (e.nearest, e.distance) == (((b, M - 1, T - 1), to_prev) if to_prev <= to_next else ((b + 1, 0, 0), -to_next))
    assert torch.equal(y, want)


@pytest.mark.parametrize("placement", ["strided4", "strided1"])
def test_row_written_at_dense_stride_into_a_strided_view_is_reported(placement):
    B, C, T = SHAPE
    v, y, want = _mutant(placement, None, dense_out=True)
    assert len(v) > 0 and any(e.where == "gap between row items" for e in v)
    assert FP.unwritten(y) > 0 and FP.poisoned(y)           # the tail of the view was never stored
    assert torch.equal(y[0, 0], want[0, 0])                 # ... while the first row sits where it belongs


@pytest.mark.parametrize("placement", FP.PLACEMENTS)
def test_masked_by_product_load_past_a_row_tail_poisons_the_output(placement):
    B, C, T = SHAPE
    x, w, g = _inputs()
    xbuf, _ = FP.place(x, placement, CPU)
    gbuf, _ = FP.place(g, placement, CPU)
    obuf, o, ldo = FP.place_slabs(1, 1, M, C, placement, CPU)
    wgrad_kernel(gbuf, xbuf, obuf, 1, mul_mask=True)
    assert FP.violations(obuf) == [] and FP.poisoned(o)
    nan = torch.isnan(o[0, 0])
    if placement.startswith("strided"):
        assert bool(nan.all())                               # every row's 8-wide tail reads the slack behind it
    else:
        # dense: only the last row of the last item reads past the tensor -- the others meet the next row's finite values
        assert bool(nan[:, C - 1].all()) and not bool(nan[:, :C - 1].any())


@pytest.mark.parametrize("placement", FP.PLACEMENTS)
def test_load_of_row_cin_poisons_the_output(placement):
    B, C, T = SHAPE
    x, w, _ = _inputs()
    xbuf, _ = FP.place(x, placement, CPU)
    ybuf, y = FP.place((B, M, T), placement, CPU)
    conv_kernel(xbuf, w, ybuf, "row_cin")
    assert FP.violations(ybuf) == [] and FP.poisoned(y)
    nan = torch.isnan(y)
    assert bool(nan[B - 1].all())                            # the last item's row Cin lies in the band behind the tensor
    if placement == "strided4":
        # row Cin of an inner item starts in the batch gap and, T = 13 <= rs - 8 + 8, its first eight words are poison
        assert bool(nan[:B - 1, :, :8].all())
    if not placement.startswith("strided"):
        assert not bool(nan[:B - 1].any())                   # dense: row Cin of an inner item is the next item's row 0
        assert torch.equal(y[:B - 1], _want(x, w)[:B - 1])


def test_the_comparison_is_on_bits():
    """another NaN in a band is a store like any other; the sentinel itself as a VALUE of a logical element is not"""
    buf, view = FP.place(SHAPE, "banded", CPU)
    buf.view(torch.int32)[3] = 0x7fc00000
    v = FP.violations(buf)
    assert len(v) == 1 and v[0].bits == 0x7fc00000 and v[0].where == "band before"
    assert FP.violations(FP.place(SHAPE, "banded", CPU)[0]) == []

# coding: utf-8
"""-m gpu: the batched DTW kernels (dv3_dtw_f32 through ops.dtw) against tests/dtw_ref.py.

Every case is a batch of B = 5 items of mixed lengths -- (1, 1), (1, Ty), (Tx, 1), (Tx, Ty), (Tx - 1, ceil(2 Ty / 3)) --
whose padding past each item's lengths is NaN.

  1. an integer lattice on which every distance and every sum is an exact fp32 integer: cost, counts and the whole path
     bit for bit (the lattice is full of ties: this pins the tie rule), at the tile and wave boundaries and at one
     shape per strip-width instance of the scan kernel;
  2. speech-like random input: the cost to (Lx + Ly + D + 2) half-ulps, the count identities, a valid path that is
     optimal to the same bound;
  3. strided views; 4. two calls, with and without the path; 5. a planted NaN, a zero length; 6. the refusals.
"""
import ctypes
import math
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tests import dtw_ref as DR  # noqa: E402

pytestmark = pytest.mark.gpu

NAN = float("nan")
B = 5


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


def _lengths(Tx, Ty):
    return [(1, 1), (1, Ty), (Tx, 1), (Tx, Ty), (Tx - 1, int(math.ceil(2 * Ty / 3.0)))]


def _pad(items, Tx, Ty, D):
    """items: [(x (Lx, D), y (Ly, D))] -> NaN-padded fp32 (B, Tx, D), (B, Ty, D)"""
    x = np.full((len(items), Tx, D), NAN, dtype=np.float32)
    y = np.full((len(items), Ty, D), NAN, dtype=np.float32)
    for b, (xi, yi) in enumerate(items):
        x[b, :xi.shape[0]] = xi
        y[b, :yi.shape[0]] = yi
    return x, y


_CASES = {}


def _lattice_case(Tx, Ty, D=16):
    key = ("lattice", Tx, Ty, D)
    if key not in _CASES:
        rng = np.random.RandomState(7 * Tx + Ty)
        u = np.zeros(D, dtype=np.float32)
        u[[2, 7, 11]] = (3.0, 4.0, 12.0)                       # |u| = 13: every distance is 13 |a_i - b_j|
        items = []
        for Lx, Ly in _lengths(Tx, Ty):
            a = rng.randint(0, 6, Lx).astype(np.float32)
            c = rng.randint(0, 6, Ly).astype(np.float32)
            items.append((a[:, None] * u, c[:, None] * u))
        _CASES[key] = (items, [DR.dtw(xi, yi) for xi, yi in items])
    return _CASES[key]


def _speech_case(Tx, Ty, D):
    """both sequences cut from one random walk by a random monotone resampling, plus noise"""
    key = ("speech", Tx, Ty, D)
    if key not in _CASES:
        rng = np.random.RandomState(100 * Tx + Ty + D)
        items = []
        for Lx, Ly in _lengths(Tx, Ty):
            n = 2 * max(Lx, Ly) + 3
            walk = np.cumsum(rng.randn(n, D) * 0.3, axis=0)
            ix = np.sort(rng.choice(n, Lx, replace=Lx > n))
            iy = np.sort(rng.choice(n, Ly, replace=Ly > n))
            xi = (walk[ix] + 0.05 * rng.randn(Lx, D)).astype(np.float32)
            yi = (walk[iy] + 0.05 * rng.randn(Ly, D)).astype(np.float32)
            items.append((xi, yi))
        _CASES[key] = (items, [DR.dtw(xi, yi) for xi, yi in items])
    return _CASES[key]


def _run(dev, items, Tx, Ty, D, want_path=True):
    from deepvoice3_pytorch_amd import ops
    x, y = _pad(items, Tx, Ty, D)
    xl = torch.tensor([it[0].shape[0] for it in items], dtype=torch.int32, device=dev)
    yl = torch.tensor([it[1].shape[0] for it in items], dtype=torch.int32, device=dev)
    res = ops.dtw(torch.from_numpy(x).to(dev), torch.from_numpy(y).to(dev), xl, yl, want_path=want_path)
    torch.cuda.synchronize()
    return res


def _bits(t):
    return t.contiguous().view(torch.int32)


def _check_path(path_rows, n, Lx, Ly, counts):
    """the item's (Tx + Ty - 1, 2) path rows: n valid steps, then -1"""
    p = [tuple(int(v) for v in r) for r in path_rows[:n]]
    assert (path_rows[n:] == -1).all()
    if n == 0:
        return p
    assert p[0] == (0, 0) and p[-1] == (Lx - 1, Ly - 1)
    moves = [0, 0, 0]
    for (i0, j0), (i1, j1) in zip(p[:-1], p[1:]):
        step = (i1 - i0, j1 - j0)
        assert step in ((1, 1), (1, 0), (0, 1)), (p, step)
        moves[((1, 1), (1, 0), (0, 1)).index(step)] += 1
    assert tuple(moves) == counts
    return p


# ----------------------------------------------------------------------------------------------------------------------
# 1. the exact lattice
# ----------------------------------------------------------------------------------------------------------------------
LATTICE_SHAPES = [(1, 1), (2, 1), (1, 7), (63, 65), (64, 64), (65, 63), (130, 97), (97, 130), (257, 64),
                  # one shape per strip width instance of the scan kernel: Ty / 64 rounded up = 9 (16), 17 (32), 33 (64)
                  (3, 520), (66, 1040), (2, 2100)]


@pytest.mark.parametrize("Tx,Ty", LATTICE_SHAPES)
def test_lattice_bit_for_bit(dev, Tx, Ty):
    items, want = _lattice_case(Tx, Ty)
    out, path = _run(dev, items, Tx, Ty, 16)
    assert out.shape == (B, 5) and out.dtype == torch.float32
    assert path.shape == (B, Tx + Ty - 1, 2) and path.dtype == torch.int32
    out, path = out.cpu().numpy(), path.cpu().numpy()
    for b, w in enumerate(want):
        got = tuple(float(v) for v in out[b])
        ref = tuple(float(w[k]) for k in DR.COLUMNS)
        print("lattice %4d x %4d item %d: got %s want %s" % (Tx, Ty, b, got, ref))
        assert got == ref, (b, got, ref)
        Lx, Ly = items[b][0].shape[0], items[b][1].shape[0]
        p = _check_path(path[b], w["path_len"], Lx, Ly, (w["n_diag"], w["n_x_only"], w["n_y_only"]))
        assert p == w["path"], b


# ----------------------------------------------------------------------------------------------------------------------
# 2. speech-like input
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("Tx,Ty", [(63, 65), (130, 97), (257, 257)])
@pytest.mark.parametrize("D", [1, 13, 80, 128])
def test_speech_like_within_rounding(dev, D, Tx, Ty):
    items, want = _speech_case(Tx, Ty, D)
    out, path = _run(dev, items, Tx, Ty, D)
    out, path = out.cpu().numpy(), path.cpu().numpy()
    for b, w in enumerate(want):
        Lx, Ly = items[b][0].shape[0], items[b][1].shape[0]
        cost, n, nd, nx, ny = (float(v) for v in out[b])
        # the sum's length times half an ulp, one rounding per addition
        bound = (Lx + Ly + D + 2) * 2.0 ** -24 * w["cost"]
        print("D %3d %3d x %3d item %d: cost %.9g ref %.9g |diff| %.3g bound %.3g; counts %s ref %s" % (
            D, Tx, Ty, b, cost, w["cost"], abs(cost - w["cost"]), bound, (n, nd, nx, ny),
            (w["path_len"], w["n_diag"], w["n_x_only"], w["n_y_only"])))
        assert abs(cost - w["cost"]) <= bound, (b, cost, w["cost"])
        assert n == 1 + nd + nx + ny and nd + nx == Lx - 1 and nd + ny == Ly - 1
        p = _check_path(path[b], int(n), Lx, Ly, (int(nd), int(nx), int(ny)))
        along = DR.path_cost(DR.distances(*items[b]), p)          # the returned path's cost in float64
        assert abs(along - w["cost"]) <= bound, (b, along, w["cost"])


# ----------------------------------------------------------------------------------------------------------------------
# 3. strided views   4. repeatability
# ----------------------------------------------------------------------------------------------------------------------
def test_strided_views_same_bits(dev):
    from deepvoice3_pytorch_amd import ops
    Tx, Ty, D = 130, 97, 13
    items, _ = _speech_case(Tx, Ty, D)
    x, y = _pad(items, Tx, Ty, D)
    xc, yc = torch.from_numpy(x).to(dev), torch.from_numpy(y).to(dev)
    xl = torch.tensor([it[0].shape[0] for it in items], dtype=torch.int32, device=dev)
    yl = torch.tensor([it[1].shape[0] for it in items], dtype=torch.int32, device=dev)
    wide = torch.full((2 * B + 1, Tx + 3, D + 5), NAN, device=dev)
    xv = wide[1:2 * B + 1:2, 2:Tx + 2, 4:D + 4]                   # batch stride 2 rows, time and feature offsets
    xv.copy_(xc)
    ybuf = torch.full((Ty, B, D), NAN, device=dev)
    yv = ybuf.transpose(0, 1)                                     # a (Ty, B, D) buffer viewed as (B, Ty, D)
    yv.copy_(yc)
    assert not xv.is_contiguous() and not yv.is_contiguous() and xv.stride(2) == 1 and yv.stride(2) == 1
    before = _bits(wide).clone()
    o0, p0 = ops.dtw(xc, yc, xl, yl, want_path=True)
    o1, p1 = ops.dtw(xv, yv, xl, yl, want_path=True)
    torch.cuda.synchronize()
    assert torch.equal(_bits(o0), _bits(o1)) and torch.equal(p0, p1)
    assert torch.equal(_bits(wide), before)                       # the inputs are only read
    assert torch.isfinite(o0).all()


@pytest.mark.parametrize("Tx,Ty,D", [(130, 97, 13), (65, 63, 80)])
def test_two_calls_same_bits(dev, Tx, Ty, D):
    items, _ = _speech_case(Tx, Ty, D)
    o0, p0 = _run(dev, items, Tx, Ty, D)
    o1, p1 = _run(dev, items, Tx, Ty, D)
    o2 = _run(dev, items, Tx, Ty, D, want_path=False)
    o3 = _run(dev, items, Tx, Ty, D, want_path=False)
    assert torch.equal(_bits(o0), _bits(o1)) and torch.equal(p0, p1)
    assert torch.equal(_bits(o2), _bits(o3))
    assert torch.equal(_bits(o0), _bits(o2))                      # the table does not depend on want_path


# ----------------------------------------------------------------------------------------------------------------------
# 5. non-finite features, zero lengths
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bad", [NAN, float("inf")])
def test_planted_nonfinite_touches_its_item_only(dev, bad):
    Tx, Ty, D = 130, 97, 13
    items, _ = _speech_case(Tx, Ty, D)
    clean, clean_path = _run(dev, items, Tx, Ty, D)
    planted = [(xi.copy(), yi.copy()) for xi, yi in items]
    planted[3][1][40, 5] = bad                                    # inside item 3's lengths
    out, path = _run(dev, planted, Tx, Ty, D)
    assert math.isnan(float(out[3, 0]))
    keep = [0, 1, 2, 4]
    assert torch.equal(_bits(out[keep]), _bits(clean[keep])) and torch.equal(path[keep], clean_path[keep])
    assert torch.isfinite(clean).all()


def test_zero_lengths_report_zeros(dev):
    from deepvoice3_pytorch_amd import ops
    Tx, Ty, D = 9, 70, 4
    x = torch.full((3, Tx, D), NAN, device=dev)
    y = torch.full((3, Ty, D), NAN, device=dev)
    x[2, :2] = 1.0
    y[2, :3] = 1.0
    xl = torch.tensor([0, 5, 2], dtype=torch.int32, device=dev)      # items 0 and 1 read nothing: all their frames are NaN
    yl = torch.tensor([7, -3, 3], dtype=torch.int32, device=dev)     # a negative length is clamped to 0
    out, path = ops.dtw(x, y, xl, yl, want_path=True)
    torch.cuda.synchronize()
    assert out[:2].tolist() == [[0.0] * 5] * 2
    assert bool((path[:2] == -1).all())
    assert out[2].tolist() == [0.0, 3.0, 1.0, 0.0, 1.0]
    assert path[2, :3].tolist() == [[0, 0], [0, 1], [1, 2]] and bool((path[2, 3:] == -1).all())
    # a length past the buffer is clamped to it
    x = torch.ones(1, 2, 1, device=dev)
    y = torch.zeros(1, 3, 1, device=dev)
    big = torch.tensor([100], dtype=torch.int32, device=dev)
    assert ops.dtw(x, y, big, big).tolist() == [[3.0, 3.0, 1.0, 0.0, 1.0]]


# ----------------------------------------------------------------------------------------------------------------------
# 6. the refusals
# ----------------------------------------------------------------------------------------------------------------------
def test_refusals(dev):
    from deepvoice3_pytorch_amd import _lib, ops
    lib = _lib.lib()
    one = torch.ones(1, dtype=torch.int32, device=dev)

    def z(*shape):
        return torch.zeros(*shape, device=dev)

    for x, y, word in ((z(0, 3, 4), z(0, 3, 4), "B = 0"),
                       (z(1, 4097, 1), z(1, 2, 1), "Tx = 4097"),
                       (z(1, 2, 1), z(1, 4097, 1), "Ty = 4097"),
                       (z(1, 0, 2), z(1, 2, 2), "Tx = 0"),
                       (z(1, 2, 129), z(1, 2, 129), "D = 129"),
                       (z(1, 2, 0), z(1, 2, 0), "D = 0"),
                       (z(1, 2, 8)[:, :, ::2], z(1, 2, 4), "dense")):
        n = x.shape[0]
        with pytest.raises(RuntimeError, match=word):
            ops.dtw(x, y, one[:n], one[:n])
    with pytest.raises(RuntimeError, match="2 x lengths"):
        ops.dtw(z(1, 2, 3), z(1, 2, 3), torch.ones(2, dtype=torch.int32, device=dev), one)
    with pytest.raises(RuntimeError, match="int32"):
        ops.dtw(z(1, 2, 3), z(1, 2, 3), one.long(), one)
    with pytest.raises(RuntimeError, match="non-GPU"):
        ops.dtw(torch.zeros(1, 2, 3), z(1, 2, 3), one, one)
    with pytest.raises(RuntimeError, match=r"\(1, 2, 3\)"):
        ops.dtw(z(1, 2, 3), z(1, 2, 4), one, one)

    # through the descriptor: null pointers and a short scratch; nothing is launched
    x, y = z(2, 3, 4), z(2, 5, 4)
    ln = torch.tensor([3, 3], dtype=torch.int32, device=dev)
    out = torch.full((2, 5), 7.0, device=dev)
    path = torch.full((2, 7, 2), 7, dtype=torch.int32, device=dev)
    need = ctypes.c_int64(-1)
    assert lib.dv3_dtw_scratch_bytes(2, 3, 5, 0, ctypes.byref(need)) == 0 and need.value == 2 * 3 * 5 * 4
    assert lib.dv3_dtw_scratch_bytes(2, 3, 5, 1, ctypes.byref(need)) == 0 and need.value == 2 * 3 * 5 * 5
    assert lib.dv3_dtw_scratch_bytes(64, 4096, 4096, 1, ctypes.byref(need)) == 0 and need.value == 5 * 2 ** 30 > 2 ** 31
    assert lib.dv3_dtw_scratch_bytes(2, 3, 5, 1, None) != 0 and "bytes_out" in lib.dv3_last_error().decode()
    scratch = torch.zeros(150, dtype=torch.uint8, device=dev)

    def desc(**kw):
        d = _lib.STRUCTS["dv3_dtw_desc"]()
        d.x, d.y, d.x_len, d.y_len = x.data_ptr(), y.data_ptr(), ln.data_ptr(), ln.data_ptr()
        d.x_batch_stride, d.x_time_stride, d.x_feat_stride = x.stride()
        d.y_batch_stride, d.y_time_stride, d.y_feat_stride = y.stride()
        d.B, d.Tx, d.Ty, d.D = 2, 3, 5, 4
        d.out, d.path, d.scratch, d.scratch_bytes = out.data_ptr(), path.data_ptr(), scratch.data_ptr(), 150
        for k, v in kw.items():
            setattr(d, k, v)
        return d

    for kw, word in ((dict(x=None), "x is null"), (dict(y=None), "y is null"), (dict(x_len=None), "x_len"),
                     (dict(y_len=None), "y_len"), (dict(out=None), "out is null"), (dict(scratch=None), "scratch is null"),
                     (dict(scratch_bytes=149), "149"), (dict(B=0), "B = 0"), (dict(D=129), "D = 129"),
                     (dict(Ty=4097), "Ty = 4097"), (dict(y_feat_stride=2), "dense"),
                     (dict(out=out.data_ptr() + 2), "aligned")):
        assert lib.dv3_dtw_f32(ctypes.byref(desc(**kw)), None) != 0, kw
        assert word in lib.dv3_last_error().decode(), (kw, lib.dv3_last_error())
    assert lib.dv3_dtw_f32(None, None) != 0
    torch.cuda.synchronize()
    assert bool((out == 7.0).all()) and bool((path == 7).all())           # nothing was launched
    assert lib.dv3_dtw_f32(ctypes.byref(desc(path=None, scratch_bytes=120)), None) == 0    # no path: 4 bytes a cell
    assert lib.dv3_dtw_f32(ctypes.byref(desc()), None) == 0
    torch.cuda.synchronize()
    assert out.tolist() == [[0.0, 3.0, 2.0, 0.0, 0.0]] * 2

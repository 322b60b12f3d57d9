# coding: utf-8
"""tests/weight_norm_ref.py proved without a GPU: the float64 restatements against torch (autograd of
torch._weight_norm, F.conv1d / F.conv_transpose1d and their input gradients), the split-image decode against the host
splits, the preconditions that keep tests/test_gpu_weight_norm.py honest (every shape list reaches the path it names, the
cancelling family cancels, no bound is vacuous), and every bound against an fp32 emulation of the kernels' order."""
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tests import weight_norm_ref as R  # noqa: E402
from tests import decode_step_ref as DR  # noqa: E402
from tests.util import assert_close_elementwise  # noqa: E402

f32 = np.float32
ALL_SHAPES = [(O, I, J, cg, False) for O, I, J, cg in R.NT_SHAPES] + [(O, I, J, 0, True) for I, O, J in R.T_SHAPES]


def _inputs(fam, O, I, J, tr, seed):
    rows, inner = (I, (O, J)) if tr else (O, (I, J))
    return R.family(fam, rows, inner, seed)


# ------------------------------------------------------------------------------------------------------------------
# the reference against torch in float64
# ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ALL_SHAPES)
def test_reference_is_the_autograd_of_weight_norm(case):
    O, I, J, cg, tr = case
    v, g = _inputs("generic", O, I, J, tr, seed=O + I)
    slabs = R.slabs_for("generic", v, 3, O, I, J, tr, seed=1)
    tv = torch.from_numpy(v).double().requires_grad_(True)
    tg = torch.from_numpy(g).double().reshape(-1, 1, 1).requires_grad_(True)
    w = torch._weight_norm(tv, tg, 0)
    assert np.allclose(w.detach().numpy(), R.weight_ref(v, g), rtol=1e-13, atol=0)
    dW, _ = R.dW_ref(slabs, O, I, J, tr)
    (w * torch.from_numpy(dW)).sum().backward()
    ref = R.bwd_ref(slabs, v, g, R.scale_ref(v, g), O, I, J, tr)            # the exact scale, not its fp32 rounding
    assert np.allclose(ref["dv"], tv.grad.numpy(), rtol=1e-10, atol=1e-13 * np.abs(ref["mag_dv"]).max())
    assert np.allclose(ref["dg"], tg.grad.numpy().reshape(-1), rtol=1e-10, atol=1e-13)
    plain = R.bwd_ref(slabs, v, None, None, O, I, J, tr)
    assert np.array_equal(plain["dv"], dW) and plain["dg"] is None


@pytest.mark.parametrize("shape", R.NT_SHAPES)
def test_packs_are_the_operands_of_conv1d_and_its_input_gradient(shape):
    O, I, J, cg = shape
    lay = R.layout(O, I, J, cg, lda_pad=R.NT_LDA_PAD[shape])
    v, g = _inputs("generic", O, I, J, False, seed=O)
    w = R.weight_ref(v, g)
    fwd, own = R.fwd_pack_of(w, lay["lda"], lay["a_half"], cg)
    bwd, _ = R.bwd_pack_of(w, lay["ldb"])
    rs = np.random.RandomState(0)
    B, T, padL = 2, 7, J // 2
    x = torch.from_numpy(rs.standard_normal((B, I, T))).requires_grad_(True)
    xp = F.pad(x, (padL, J - 1 - padL))
    y = F.conv1d(xp, torch.from_numpy(w))
    gy = torch.from_numpy(rs.standard_normal(y.shape))
    (y * gy).sum().backward()
    cols = [R.col_of(o, cg, lay["a_half"]) for o in range(O)]
    xs = xp.detach().numpy()
    mine = sum(np.einsum("im,bit->bmt", fwd[j][:, cols], xs[:, :, j:j + T]) for j in range(J))
    assert np.allclose(mine, y.detach().numpy(), rtol=1e-12, atol=1e-12)
    gp = np.pad(gy.numpy(), ((0, 0), (0, 0), (J - 1 - padL, padL)))          # the DGRAD tap-GEMM: padL' = J - 1 - padL
    dx = sum(np.einsum("oi,bot->bit", bwd[j][:, :I], gp[:, :, j:j + T]) for j in range(J))
    assert np.allclose(dx, x.grad.numpy(), rtol=1e-12, atol=1e-12)
    assert np.isnan(fwd[~own]).all() and own.sum() == O * I * J and np.isnan(bwd[:, :, I:]).all()
    # the forward layout is the one the decode-step tests pack from
    theirs = DR.fwd_pack_of(w.transpose(0, 2, 1).astype(f32), cg, lay["lda"], lay["a_half"])
    assert np.array_equal(theirs, fwd.reshape(J * I, lay["lda"]).astype(f32), equal_nan=True)


@pytest.mark.parametrize("shape", R.T_SHAPES)
def test_transposed_packs_are_the_operands_of_conv_transpose1d(shape):
    I, O, J = shape
    lay = R.layout(O, I, J, transposed=True)
    v, g = _inputs("generic", O, I, J, True, seed=I)
    w = R.weight_ref(v, g)                                                   # [I][O][J]
    fwd, own = R.fwd_pack_of(w, lay["lda"], transposed=True)
    bwd, ownb = R.bwd_pack_of(w, lay["ldb"], transposed=True)
    rs = np.random.RandomState(1)
    B, T = 2, 5
    x = torch.from_numpy(rs.standard_normal((B, I, T))).requires_grad_(True)
    y = F.conv_transpose1d(x, torch.from_numpy(w))
    gy = rs.standard_normal(tuple(y.shape))
    (y * torch.from_numpy(gy)).sum().backward()
    z = np.einsum("im,bit->bmt", fwd[0][:, :J * O], x.detach().numpy())        # [B][J*O][T]: the tap folded in m
    mine = np.zeros(tuple(y.shape))
    dx = np.zeros((B, I, T))
    for j in range(J):
        mine[:, :, j:j + T] += z[:, j * O:(j + 1) * O]
        dx += np.einsum("oi,bot->bit", bwd[0][j * O:(j + 1) * O, :I], gy[:, :, j:j + T])
    assert np.allclose(mine, y.detach().numpy(), rtol=1e-12, atol=1e-12)
    assert np.allclose(dx, x.grad.numpy(), rtol=1e-12, atol=1e-12)
    assert np.isnan(fwd[~own]).all() and np.isnan(bwd[~ownb]).all()


@pytest.mark.parametrize("dtype", ["bf16", "f16"])
def test_split_decode_inverts_the_host_encode(dtype):
    rs = np.random.RandomState(5)
    J, K, lda = 2, 37, 12
    x = (rs.standard_normal((J, K, lda)) * 2.0 ** rs.uniform(-12, 6, (J, K, lda))).astype(f32)
    img = R.encode_split(x, dtype)
    assert img.dtype == np.uint16 and img.size == R.split_words(J, K, lda)
    hi, lo = R.decode_split(img, J, K, lda, dtype)
    eh, el = R.host_split(x, dtype)
    assert np.array_equal(hi[:, :K], eh) and np.array_equal(lo[:, :K], el)
    assert np.all(hi[:, K:] == 0) and np.all(lo[:, K:] == 0)
    # the layout, by hand: element (plane 1, j 1, k 19, m 5) sits at [1][1][19 // 8][5][19 % 8]
    Kp = R.rup(K, 32)
    at = ((((1 * J + 1) * (Kp // 8) + 19 // 8) * lda) + 5) * 8 + 19 % 8
    assert R._from_bits(img[at:at + 1], dtype)[0] == el[1, 19, 5]
    scale = 2.0 ** 8 if dtype == "f16" else 1.0
    assert np.all(np.abs(hi[:, :K] + lo[:, :K] - x.astype(np.float64) * scale) <=
                  np.maximum(2.0 ** -17 * np.abs(x) * scale, 2.0 ** -25))


# ------------------------------------------------------------------------------------------------------------------
# preconditions of the GPU tests
# ------------------------------------------------------------------------------------------------------------------
def test_shape_lists_reach_the_paths_they_name():
    lay = {s: R.layout(*s, lda_pad=R.NT_LDA_PAD[s]) for s in R.NT_SHAPES}
    assert lay[(513, 80, 1, 0)]["lda"] == 516
    assert lay[(12, 36, 3, 6)]["a_half"] == 8 and lay[(12, 36, 3, 6)]["lda"] == 16          # a gap between the halves
    assert lay[(80, 40, 3, 40)]["a_half"] == 40 and lay[(80, 40, 3, 40)]["lda"] == 80       # no pad at all
    assert lay[(66, 33, 2, 33)]["a_half"] == 36
    assert lay[(64, 40, 5, 0)]["lda"] > 64
    assert R.cdiv(257 * 3, 256) == 4 and (257 * 3) % 256 == 3                               # a ragged fourth trip
    assert {R.cdiv(O, 32) * R.cdiv(I, 32) for O, I, J, cg in R.NT_SHAPES} >= {1, 2, 4}        # one block, several
    t = R.layout(3, 5, 2, transposed=True)
    assert t["lda"] == 8 and t["ldb"] == 8 and t["ldb"] > 5
    assert all(I % 32 and (J * O) % 32 for I, O, J in R.T_SHAPES)
    # slab loops: trips of the 8-loop, of the 4-loop, of the tail -- every entry and exit
    trips = {(n // 8, n % 8 // 4, n % 4) for n in R.N_SLABS}
    assert {a for a, b, c in trips} == {0, 1, 2} and {c for a, b, c in trips} == {0, 1, 2, 3}
    assert {(min(a, 1), b) for a, b, c in trips} == {(0, 0), (0, 1), (1, 0), (1, 1)}
    assert [R.dw_depth(n) for n in (1, 8, 13, 16)] == [4, 4, 6, 5]
    # the [O][n_part] loops: per thread (4-accumulator trips, 1-accumulator trips)
    per = {n: {R.part_trips(n, t) for t in range(R.THREADS)} for n in R.N_PART}
    assert per[1] == {(0, 1), (0, 0)} and per[256] == {(0, 1)} and per[257] == {(0, 2), (0, 1)}
    assert per[769] == {(1, 0), (0, 3)} and per[1024] == {(1, 0)}                           # k + 768 < n_part: either side
    assert per[1027] == {(1, 1), (1, 0)} and per[1281] == {(1, 2), (1, 1)}
    assert R.dbias_depth(769, True) == 3 + 2 + 9 and R.dbias_depth(769, False) == 4 + 9
    # rows against bias channels
    kinds = set()
    for I, O, J, tr in R.ROWS_VS_O:
        rows = I if tr else O
        kinds.add("several" if O > 2 * rows else "none" if O < rows else "equal")
    assert kinds == {"several", "none", "equal"}


@pytest.mark.parametrize("case", ALL_SHAPES)
def test_cancelling_family_cancels(case):
    O, I, J, cg, tr = case
    v, g = _inputs("cancel", O, I, J, tr, seed=3)
    ref = R.bwd_ref(R.slabs_for("cancel", v, 5, O, I, J, tr, seed=3), v, g, R.scale_ref(v, g).astype(f32), O, I, J, tr)
    small = np.abs(ref["dv"]) < 1e-3 * ref["mag_dv"]
    assert small.mean() >= 0.9, small.mean()
    assert np.all(ref["E_dv"] < 2.0 ** -12 * ref["mag_dv"])          # and the bound is far below the terms that cancel


def test_no_bound_is_vacuous():
    """bound / |reference| of the generic family, from the reference alone, against weight_norm_ref.VACUITY_CAP"""
    worst = dict((k, 0.0) for k in R.VACUITY_CAP)
    for O, I, J, cg, tr in ALL_SHAPES:
        length = (O if tr else I) * J
        worst["scale"] = max(worst["scale"], R.scale_rel_bound(length))
        worst["pack"] = max(worst["pack"], R.pack_rel_bound(length))
        v, g = _inputs("generic", O, I, J, tr, seed=9)
        ref = R.bwd_ref(R.slabs_for("generic", v, 16, O, I, J, tr, seed=9), v, g, R.scale_ref(v, g).astype(f32), O, I, J, tr)
        for k in ("dW", "dg", "dv"):
            if k == "dv" and length == 1:          # a one-element row: dv = 0 but for the fp32 rounding of `scale`
                assert np.all(np.abs(ref["dv"]) < 2.0 ** -22 * ref["mag_dv"])
                continue
            worst[k] = max(worst[k], float(np.median(ref["E_" + k] / np.abs(ref[k]))))
    rs = np.random.RandomState(2)
    for n in R.N_PART:
        for t in (False, True):
            db, E = R.dbias_ref(rs.standard_normal((13, n) if t else (n, 13)).astype(f32), t)
            worst["dbias"] = max(worst["dbias"], float(np.median(E / np.abs(db))))
    for k, cap in R.VACUITY_CAP.items():
        print("bound / |reference| %-6s %.3g (cap %.3g)" % (k, worst[k], cap))
        assert 0 < worst[k] <= cap, (k, worst[k], cap)


# ------------------------------------------------------------------------------------------------------------------
# the bounds against an fp32 emulation of the kernels' order
# ------------------------------------------------------------------------------------------------------------------
def _block_reduce(acc):
    """[R][256] per-thread fp32 partials -> [R]: the 64-lane xor butterfly, then the four wave partials left to right"""
    w = acc.reshape(acc.shape[0], 4, 64)
    lane = np.arange(64)
    for off in (32, 16, 8, 4, 2, 1):
        w = w + w[:, :, lane ^ off]
    red = w[:, :, 0]
    return ((red[:, 0] + red[:, 1]) + red[:, 2]) + red[:, 3]


def _block_sum(terms):
    """[R][n] fp32 terms, thread t adding elements t, t + 256, ... in order"""
    n = terms.shape[1]
    trips = R.cdiv(n, 256)
    pad = np.zeros((terms.shape[0], trips * 256), f32)
    pad[:, :n] = terms
    acc = np.zeros((terms.shape[0], 256), f32)
    for t in range(trips):
        acc = acc + pad[:, t * 256:(t + 1) * 256]
    assert acc.dtype == f32
    return _block_reduce(acc)


def _emu_scale(v, g):
    if g is None:
        return np.ones(v.shape[0], f32)
    r = v.reshape(v.shape[0], -1)
    return f32(1) / np.sqrt(_block_sum(r * r))


def _emu_dw(s):
    """[S][...] fp32 partials -> their sum in the order of the 8- / 4- / 1-unrolled loops"""
    acc = [np.zeros(s.shape[1:], f32) for _ in range(8)]
    k, S = 0, s.shape[0]
    while k + 8 <= S:
        for u in range(8):
            acc[u] = acc[u] + s[k + u]
        k += 8
    while k + 4 <= S:
        for u in range(4):
            acc[u] = acc[u] + s[k + u]
        k += 4
    while k < S:
        acc[0] = acc[0] + s[k]
        k += 1
    return ((acc[0] + acc[1]) + (acc[2] + acc[3])) + ((acc[4] + acc[5]) + (acc[6] + acc[7]))


def _emu_bwd(slabs, v, g, scale, O, I, J, tr):
    dw = np.ascontiguousarray(R._to_param(_emu_dw(slabs), O, I, J, tr))
    if g is None:
        return dw, None
    rows = v.shape[0]
    dot = _block_sum((dw * v).reshape(rows, -1))
    dg = dot * scale
    c1 = g * scale
    c2 = ((g * scale) * scale) * dg
    return c1[:, None, None] * dw - c2[:, None, None] * v, dg


def _emu_dbias(part, part_t):
    if not part_t:
        return _block_sum(np.ascontiguousarray(part.T))
    Och, n = part.shape
    b = np.zeros((4, Och, 256), f32)
    for tid in range(256):
        k = tid
        while k + 768 < n:
            for u in range(4):
                b[u, :, tid] = b[u, :, tid] + part[:, k + 256 * u]
            k += 1024
        while k < n:
            b[0, :, tid] = b[0, :, tid] + part[:, k]
            k += 256
    return _block_reduce((b[0] + b[1]) + (b[2] + b[3]))


@pytest.mark.parametrize("fam", R.FAMILIES)
@pytest.mark.parametrize("case", ALL_SHAPES)
def test_fp32_emulation_stays_inside_the_forward_bounds(case, fam):
    O, I, J, cg, tr = case
    v, g = _inputs(fam, O, I, J, tr, seed=O * 131 + I * 7 + J)
    sc = _emu_scale(v, g)
    r0 = assert_close_elementwise(sc, R.scale_ref(v, g), R.scale_rel_bound(v[0].size), 0.0, "scale")
    w = (g * sc)[:, None, None] * v
    assert w.dtype == f32
    r1 = assert_close_elementwise(w, R.weight_ref(v, g), R.pack_rel_bound(v[0].size), 0.0, "packed value")
    assert np.array_equal(R.weight_ref(v, None), v.astype(np.float64)) and R.pack_rel_bound(v[0].size, False) == 0.0
    print("worst-ratio emulation forward %s %s %.3g" % (case, fam, max(r0, r1)))


@pytest.mark.parametrize("fam", R.FAMILIES)
@pytest.mark.parametrize("idx", range(len(ALL_SHAPES)))
def test_fp32_emulation_stays_inside_the_backward_bounds(idx, fam):
    O, I, J, cg, tr = ALL_SHAPES[idx]
    worst = 0.0
    for n_slabs in (R.N_SLABS[(idx * 3 + 1) % len(R.N_SLABS)], 16):
        v, g = _inputs(fam, O, I, J, tr, seed=idx)
        scale = R.scale_ref(v, g).astype(f32)
        slabs = R.slabs_for(fam, v, n_slabs, O, I, J, tr, seed=idx)
        ref = R.bwd_ref(slabs, v, g, scale, O, I, J, tr)
        dv, dg = _emu_bwd(slabs, v, g, scale, O, I, J, tr)
        worst = max(worst, assert_close_elementwise(dv, ref["dv"], 0.0, ref["E_dv"], "dv"),
                    assert_close_elementwise(dg, ref["dg"], 0.0, ref["E_dg"], "dg"))
        start = np.random.RandomState(idx).standard_normal(v.shape).astype(f32)
        want, E = R.accumulated(start, ref["dv"], ref["E_dv"])
        worst = max(worst, assert_close_elementwise(start + dv, want, 0.0, E, "dv accumulated"))
        plain = R.bwd_ref(slabs, v, None, None, O, I, J, tr)
        worst = max(worst, assert_close_elementwise(_emu_bwd(slabs, v, None, None, O, I, J, tr)[0], plain["dv"], 0.0,
                                                    plain["E_dv"], "dv of a plain weight"))
    print("worst-ratio emulation backward %s %s %.3g" % (ALL_SHAPES[idx], fam, worst))


@pytest.mark.parametrize("n_slabs", R.N_SLABS)
def test_fp32_emulation_of_the_slab_sum(n_slabs):
    rs = np.random.RandomState(n_slabs)
    O, I, J = 24, 33, 3
    slabs = (rs.standard_normal((n_slabs, J, O, I)) * 2.0 ** rs.uniform(-10, 10, (n_slabs, 1, 1, 1))).astype(f32)
    for rows_of_slabs in (False, True):             # both layouts hold the same logical slabs
        flat, ss, row = R.slab_buffer(slabs, rows_of_slabs, 36)
        assert np.isnan(flat[-64:]).all()
        for s, j, o, i in ((0, 0, 0, 0), (n_slabs - 1, J - 1, O - 1, I - 1), (n_slabs // 2, 1, 7, 32)):
            assert flat[s * ss + (j * O + o) * row + i] == slabs[s, j, o, i]
        assert np.isnan(flat[(n_slabs - 1) * ss + ((J - 1) * O + O - 1) * row + I])        # a pad column
    dW, A = R.dW_ref(slabs, O, I, J, False)
    got = R._to_param(_emu_dw(slabs), O, I, J, False)
    assert_close_elementwise(got, dW, 0.0, R.gamma(R.dw_depth(n_slabs)) * A * R.SLACK, "dW")


@pytest.mark.parametrize("part_t", [False, True])
@pytest.mark.parametrize("n_part", R.N_PART)
def test_fp32_emulation_of_the_bias_sums(n_part, part_t):
    rs = np.random.RandomState(n_part)
    part = (rs.standard_normal((5, n_part) if part_t else (n_part, 5)) * 2.0 ** rs.uniform(-8, 8)).astype(f32)
    want, E = R.dbias_ref(part, part_t)
    r = assert_close_elementwise(_emu_dbias(part, part_t), want, 0.0, E, "dbias")
    print("worst-ratio emulation dbias n_part=%d t=%s %.3g" % (n_part, part_t, r))

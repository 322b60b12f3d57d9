# coding: utf-8
"""tests/gate_ref.py proved without a GPU.

A numpy float32 emulation of every tail expression (the forward GLU / highway of dv3_gate_out, the plain activations
with their residual chain, dv3_gate_deriv, the c8 backward with its bf16 stores), the two hardware operations modelled
as correctly rounded results moved by -1, 0 or +1 ulp and flushed to zero where subnormal.  The faithful emulation must
stay inside the bounds on the G family; each defect model of MUTANTS must leave them (or, for the sub-tile that rounds
a * s + x twice, the bit-identity of the paired channels) on at least one element.  That list is the test of the bounds'
tightness: no bound is tuned to what a kernel returns.
"""
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tests import gate_ref as G  # noqa: E402
from tests import gemm_split_ref as R  # noqa: E402

f32, f64 = np.float32, np.float64
PERTS = [(0, 0), (1, 1), (-1, -1), (1, -1), (-1, 1)]          # ulps added to v_exp_f32's and v_rcp_f32's result
SHAPES = R.EDGE_SHAPES


# ---------------------------------------------------------------------------------------------------------------
# fp32 emulation
# ---------------------------------------------------------------------------------------------------------------
def _nudge(v, n):
    """positive finite fp32 values moved by n ulp; 0 and inf stay"""
    v = np.ascontiguousarray(v, dtype=f32)
    ok = np.isfinite(v) & (v > 0)
    out = np.where(ok, (v.view(np.int32) + np.int32(n)).view(f32), v)
    return np.where(out < f32(2.0 ** -126), f32(0), out).astype(f32)      # a subnormal result is flushed


def hw_exp2(p, n):
    with np.errstate(over="ignore", under="ignore"):
        return _nudge(np.exp2(p.astype(f64)).astype(f32), n)


def hw_rcp(d, n):
    with np.errstate(divide="ignore", over="ignore", under="ignore"):
        return _nudge((1.0 / d.astype(f64)).astype(f32), n)


def fma(a, b, c):
    return (a.astype(f64) * b.astype(f64) + c.astype(f64)).astype(f32)


def emu_sigmoid(g, pert=(0, 0), mutant=None):
    g = np.asarray(g, dtype=f32)
    if mutant == "exp_ratio":                    # exp(g) / (1 + exp(g))
        with np.errstate(over="ignore", invalid="ignore"):
            e = hw_exp2(g * f32(G.L32), pert[0])
            return (e / (f32(1) + e)).astype(f32)
    e = hw_exp2((-g) * f32(G.L32), pert[0])
    s = hw_rcp(f32(1) + e, pert[1])
    if mutant == "clamp16":
        s = np.where(g > 16, f32(1), np.where(g < -16, f32(0), s))
    return s.astype(f32)


def emu_gate_fwd(kind, a, g, x, pert=(0, 0), mutant=None, unfused_rows=None):
    """dv3_gate_out after the tail's sigmoid.  unfused_rows: channels whose a * s + x is rounded twice"""
    a, x = np.asarray(a, dtype=f32), np.asarray(x, dtype=f32)
    s = emu_sigmoid(g, pert, mutant)
    with np.errstate(invalid="ignore", over="ignore"):
        if kind in ("glu", "glu_res"):
            xx = x if kind == "glu_res" else np.zeros_like(a)
            t = fma(a, s, xx)
            if unfused_rows is not None:
                t2 = (a * s).astype(f32) + xx
                t[:, unfused_rows] = t2[:, unfused_rows]
            scale = kind == "glu_res"
            if mutant == "scale_flipped":
                scale = not scale
            return (t * f32(G.RS2_32)).astype(f32) if scale else t
        if mutant == "highway_swapped":
            a, x = x, a
        t = ((f32(1) - s) * x).astype(f32)
        return fma(s, a, t)


def emu_gate_deriv(kind, dy, a, g, x, pert=(0, 0), mutant=None):
    """common.h:89-101 with every product rounded (contraction off)"""
    dy, a = np.asarray(dy, dtype=f32), np.asarray(a, dtype=f32)
    x = np.zeros_like(a) if x is None else np.asarray(x, dtype=f32)
    d = (dy * f32(G.RS2_32)).astype(f32) if kind == "glu_res" else dy
    s = emu_sigmoid(g, pert)
    q = (f32(1) - s).astype(f32)
    t = s if mutant == "t_is_s" else (s * q).astype(f32)
    va = (d * s).astype(f32)
    if kind == "highway":
        vg = ((d * (a - x).astype(f32)).astype(f32) * t).astype(f32)
        vr = d if mutant == "vr_is_d" else (d * q).astype(f32)
    else:
        vg = ((d * a).astype(f32) * t).astype(f32)
        vr = d
    return va, vg, vr


def emu_act_fwd(act, v, r=None, r2=None, pert=(0, 0)):
    v = np.asarray(v, dtype=f32)
    if act == "relu":
        v = np.maximum(v, f32(0))
    elif act == "sigmoid":
        v = emu_sigmoid(v, pert)
    elif act == "softsign":
        v = (v * hw_rcp(f32(1) + np.abs(v), pert[1])).astype(f32)
    for t in (r, r2):
        if t is not None:
            v = ((v + np.asarray(t, dtype=f32)).astype(f32) * f32(G.RS2_32)).astype(f32)
    return v


def _bf16_trunc(v):
    return (np.ascontiguousarray(v, dtype=f32).view(np.int32) & np.int32(-65536)).view(f32).astype(f64)


_cases = {}


def _case(shape, kind):
    """(family, a, g, residual input with the cancelling frames) of one shape and gate kind"""
    key = (shape, kind)
    if key not in _cases:
        C = shape[1]
        f = G.family_g(shape)
        pre = G.pre_gates(f, shape)
        a, g = pre[:, :C], pre[:, C:]
        _cases[key] = (f, a, g, G.with_cancellation(kind, f["r"], a, g, f["pairs"]))
    return _cases[key]


# ---------------------------------------------------------------------------------------------------------------
# the family and the reference
# ---------------------------------------------------------------------------------------------------------------
def test_pre_gates_are_the_same_number_in_every_order_and_operand_form():
    shape = (1, 256, 8, 3, 1, False)
    B, C, T, k, d, causal = shape
    f = G.family_g(shape)
    pre = G.pre_gates(f, shape)
    for form in (("f16", R.F16_ACT_SHIFT), ("bf16",)):
        assert not R.split(f["x"], form)[1].any()
    for form in (("f16", R.F16_WEIGHT_SHIFT), ("bf16",)):
        assert not R.split(f["w"], form)[1].any()
    assert np.array_equal(G.rn_bf16(f["x"]), f["x"].astype(f64)) and np.array_equal(G.rn_bf16(f["w"]), f["w"].astype(f64))
    for seed in (0, 1):          # products added in fp32 in a shuffled order, then the bias: the float64 sum, bit for bit
        got = R.emulate("fwd", f["x"], f["w"], None, None, J=k, dil=d, padL=R.pad_left(k, d, causal),
                        addend=R.bias_bcast(f["bias"]), seed=seed).numpy()
        assert np.array_equal(got, pre)
    assert 2.0 < pre[:, :C][:, f["bias"][:C] == 0].std() < 5.0          # a zero-bias channel sits in the live range
    for i, e in f["pairs"]:
        assert np.array_equal(pre[:, i], pre[:, e]) and np.array_equal(pre[:, C + i], pre[:, C + e])


@pytest.mark.parametrize("C", [8, 16, 24, 40, 64, 96, 128, 256])
def test_pair_channels_straddle_the_last_sub_tile(C):
    pairs = G.pair_channels(C)
    assert len(pairs) == 2
    full = 32 * (C // 32)
    for i, e in pairs:
        assert 0 <= i < e < C
        if full and full < C:
            assert i < full <= e


@pytest.mark.parametrize("kind", G.KINDS)
def test_closed_form_backward_is_the_autograd_of_the_forward(kind):
    rng = np.random.RandomState(3)
    a, g, x, dy = (torch.from_numpy(rng.standard_normal((2, 5, 7)) * sc).requires_grad_(True) for sc in (2, 2, 2, 1))
    y = G.gate_fwd_torch(kind, a, g, x)
    assert np.allclose(y.detach().numpy(), G.gate_fwd(kind, a.detach().numpy(), g.detach().numpy(), x.detach().numpy()),
                       rtol=1e-9, atol=1e-12)
    da, dg, dx = torch.autograd.grad((y * dy.detach()).sum(), (a, g, x), allow_unused=True)
    ra, rg, rr = G.gate_bwd(kind, *(t.detach().numpy() for t in (dy, a, g, x)))
    assert np.allclose(da.numpy(), ra, rtol=1e-13, atol=0) and np.allclose(dg.numpy(), rg, rtol=1e-10, atol=0)
    if kind != "glu":
        assert np.allclose(dx.numpy(), rr, rtol=1e-13, atol=0)


# ---------------------------------------------------------------------------------------------------------------
# the faithful emulation is inside the bounds
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", G.KINDS)
def test_faithful_forward_is_inside_the_bound(kind):
    worst = 0.0
    for shape in SHAPES:
        f, a, g, r = _case(shape, kind)
        ref, bnd = G.fwd_bound(kind, a, g, r)
        for pert in PERTS:
            y = emu_gate_fwd(kind, a, g, r, pert)
            ratio, at = G.worst_ratio(y, ref, bnd)
            assert ratio <= 1.0, (kind, shape, pert, at, ratio)
            assert G.pair_mismatch(y, f["pairs"]) == 0
            worst = max(worst, ratio)
            rb, bb = G.fwd_bound(kind, a, g, G.rn_bf16(r), contracted=False)        # c8 / bf16 tensors
            yb = G.rn_bf16(emu_gate_fwd(kind, a, g, G.rn_bf16(r), pert))
            assert G.worst_ratio(yb, rb, G.to_bf16_bound(rb, bb))[0] <= 1.0
    print("worst-ratio emulated forward %s %.4g" % (kind, worst))
    assert worst > 0.02, "the bound is loose by more than 50 x on its own emulation"


@pytest.mark.parametrize("act", G.ACTS)
def test_faithful_activation_is_inside_the_bound(act):
    for shape in SHAPES:
        C = shape[1]
        f, a, g, _ = _case(shape, "glu")
        r, r2 = f["r"], f["spk3"]
        for rr in ((None, None), (r, None), (r, r2)):
            ref, bnd = G.act_bound(act, a, *rr)
            for pert in PERTS:
                y = emu_act_fwd(act, a, *rr, pert=pert)
                if act in ("linear", "relu") and rr[0] is None:
                    assert np.array_equal(y.astype(f64), ref)
                ratio, at = G.worst_ratio(y, ref, bnd)
                assert ratio <= 1.0, (act, shape, pert, at, ratio)


@pytest.mark.parametrize("kind", G.KINDS)
def test_faithful_backward_is_inside_the_bound(kind):
    worst = 0.0
    for shape in SHAPES:
        f, a, g, r = _case(shape, kind)
        x = r if kind == "highway" else None
        refs, bnds = G.bwd_bound(kind, f["dy"], a, g, x)
        for pert in PERTS:
            outs = emu_gate_deriv(kind, f["dy"], a, g, x, pert)
            for o, ref, bnd in zip(outs, refs, bnds):
                ratio, at = G.worst_ratio(o, ref, bnd)
                assert ratio <= 1.0, (kind, shape, pert, at, ratio)
                worst = max(worst, ratio)
        # the c8 kernel: bf16 inputs, bf16 stores of the same expression
        dyb, ab, gb = G.rn_bf16(f["dy"]), G.rn_bf16(a), G.rn_bf16(g)
        xb = G.rn_bf16(r) if kind == "highway" else None
        refs, bnds = G.bwd_bound(kind, dyb, ab, gb, xb)
        outs = emu_gate_deriv(kind, dyb, ab, gb, xb, (1, -1))
        for o, ref, bnd in zip(outs, refs, bnds):
            assert G.worst_ratio(G.rn_bf16(o), ref, G.to_bf16_bound(ref, bnd))[0] <= 1.0
    print("worst-ratio emulated backward %s %.4g" % (kind, worst))
    assert worst > 0.02


# ---------------------------------------------------------------------------------------------------------------
# the defect models leave them
# ---------------------------------------------------------------------------------------------------------------
def _fwd_fails(kind, mutant=None, g_of=None):
    n = 0
    for shape in SHAPES:
        f, a, g, r = _case(shape, kind)
        ref, bnd = G.fwd_bound(kind, a, g, r)
        gk = g if g_of is None else g_of(f, g, shape)
        y = emu_gate_fwd(kind, a, gk, r, (0, 0), mutant)
        n += G.worst_ratio(y, ref, bnd)[0] > 1.0
    return n


def test_mutant_exp_ratio_gives_nan_at_89():
    f, a, g, r = _case(SHAPES[0], "glu")
    y = emu_gate_fwd("glu", a, g, r, (0, 0), "exp_ratio")
    assert np.isnan(y[g >= 89]).all() and (g >= 89).any()
    assert _fwd_fails("glu", "exp_ratio") and _fwd_fails("highway", "exp_ratio")


@pytest.mark.parametrize("kind", G.KINDS)
def test_mutant_sigmoid_clamped_beyond_16(kind):
    assert _fwd_fails(kind, "clamp16")


@pytest.mark.parametrize("kind", ["glu", "glu_res"])
def test_mutant_output_scale_on_the_wrong_side_of_the_residual_flag(kind):
    assert _fwd_fails(kind, "scale_flipped") == len(SHAPES)


def test_mutant_highway_operands_swapped():
    assert _fwd_fails("highway", "highway_swapped") == len(SHAPES)


@pytest.mark.parametrize("kind", G.KINDS)
def test_mutant_bias_on_the_a_half_only(kind):
    assert _fwd_fails(kind, None, lambda f, g, shape: g - f["bias"][shape[1]:].astype(f64).reshape(1, -1, 1))


def _bwd_fails(kind, mutant, which):
    n = 0
    for shape in SHAPES:
        f, a, g, r = _case(shape, kind)
        x = r if kind == "highway" else None
        refs, bnds = G.bwd_bound(kind, f["dy"], a, g, x)
        outs = emu_gate_deriv(kind, f["dy"], a, g, x, (0, 0), mutant)
        n += G.worst_ratio(outs[which], refs[which], bnds[which])[0] > 1.0
    return n


@pytest.mark.parametrize("kind", G.KINDS)
def test_mutant_gate_derivative_without_one_minus_s(kind):
    assert _bwd_fails(kind, "t_is_s", 1)


def test_mutant_highway_residual_gradient_without_one_minus_s():
    assert _bwd_fails("highway", "vr_is_d", 2)


@pytest.mark.parametrize("kind", ["glu", "glu_res"])
def test_mutant_one_sub_tile_rounds_twice_fails_the_pair_identity_not_the_bound(kind):
    hits = 0
    for shape in SHAPES:
        C = shape[1]
        f, a, g, r = _case(shape, kind)
        edge = [e for _, e in f["pairs"]]
        y = emu_gate_fwd(kind, a, g, r, (0, 0), unfused_rows=edge)
        ref, bnd = G.fwd_bound(kind, a, g, r)
        bnd2 = bnd + G.U * np.abs(a * G.sigmoid64(g)[0])          # the extra rounding of a * s: inside one more u |a s|
        assert G.worst_ratio(y, ref, bnd2)[0] <= 1.0
        hits += G.pair_mismatch(y, f["pairs"]) > 0
    assert hits >= (len(SHAPES) - 3 if kind == "glu_res" else 0)
    if kind == "glu":       # without an addend a * s + 0 is the same number either way: the residual form is the witness
        assert hits == 0


@pytest.mark.parametrize("kind", G.KINDS)
def test_mutant_bf16_store_truncates(kind):
    n = 0
    for shape in SHAPES:
        f, a, g, r = _case(shape, kind)
        rb, bb = G.fwd_bound(kind, a, g, G.rn_bf16(r), contracted=False)
        y = emu_gate_fwd(kind, a, g, G.rn_bf16(r))
        n += G.worst_ratio(_bf16_trunc(y), rb, G.to_bf16_bound(rb, bb))[0] > 1.0
    assert n >= len(SHAPES) - 1


def test_row_sum_depths_restate_the_kernels():
    assert G.depth_gate_bwd(1, True) == 11 and G.depth_gate_bwd(201, False) == 4 + 6
    assert G.depth_gate_bwd(513, True) >= 4 * 3 + 6 and G.depth_gate_bwd_c8(513) == 3 + 20

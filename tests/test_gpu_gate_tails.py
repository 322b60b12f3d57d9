# coding: utf-8
"""-m gpu: the nonlinear tails of every tap-GEMM form, element by element against float64 (tests/gate_ref.py).

The G family gives every GEMM mode, kernel form and summation order THE SAME exact fp32 pre-gate pair (integers times a
power of two; tests/test_cpu_gate_ref.py adds them in shuffled order), with whole channels moved into the sigmoid's
saturation by a bias ladder (|g| up to 200), so what a launch returns is its tail's own arithmetic:
  * the saved pre-gate pair is bit-exact (fp32) or bf16_rn of the exact value (bf16 / c8);
  * the gate output lies inside the per-element bound derived from the tail's fp32 expression;
  * a second identical call returns the same bits, the f16 range counter stays at zero;
  * two channel pairs with identical weight rows, bias and residual rows -- one channel in an interior 32-row sub-tile,
    one in the last (partial) one -- return identical bits (conv_common.h:180-183: the one-ulp difference of round 6);
  * y is compared bit for bit across ALL fp32-output forms and modes of a shape and gate kind: the header promises one
    expression for every fp32 tail (conv_common.h:180-183, :355) and the family one pre-gate, so the first form that
    runs a (shape, kind) sets the bits every later one must return.
Every forced form is asserted from the launch census; a form that is not eligible for a shape is passed over.

The c8 tails (conv_common.h:800-801, both c8 kernels) feed the gate the UNROUNDED fp32 pre-gate pair and store bf16_rn of
it; their a * s + x is contracted by the compiler, not by dv3_gate_out, so the header's promise does not cover them:
they are held to the bound (plus one bf16 rounding) and to each other.

Backward: ops.gate_bwd / ops.gate_bwd_c8 against the closed-form autograd, g from the ladder, a / x / dy from the
magnitude sweeps (0, +-2^-130, N(0, 1) times 2^-6 .. 2^6), with the 16-byte and 4-byte row forms, pair words, a bf16
pre-gate save and both sigmoid forms of the c8 kernel; row sums within depth * u * sum|terms| with the depth restated from
the kernels.  Two fused chains of test_gpu_gate_fuse.py rerun with the producer's bias on the ladder.
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
from tests import test_gpu_gemm_operands as OPS_T  # noqa: E402
from tests import test_gpu_gate_fuse as FUSE_T  # noqa: E402
from tests import test_gpu_kernels as KERN_T  # noqa: E402
from tests.util import rel_err  # noqa: E402

pytestmark = pytest.mark.gpu

SPLIT_FORMS, F32_FORMS, CONV_CASES = OPS_T.SPLIT_FORMS, OPS_T.F32_FORMS, OPS_T.CONV_CASES
_form, _conv_reached = OPS_T._form, OPS_T._conv_reached
MODES = OPS_T.MODES
# (mode, B, C, T) of test_gate_backward_16_byte_rows_of_any_length: head, quads and tail; T = 1, 2, 3; C = 513
_BWD_PARAMS = [m.args[1] for m in KERN_T.test_gate_backward_16_byte_rows_of_any_length.pytestmark
               if m.name == "parametrize" and m.args[0] == "mode,B,C,T"][0]
BWD_SHAPES = sorted(set((B, C, T) for _, B, C, T in _BWD_PARAMS))
BWD_KINDS = G.KINDS + G.ACTS


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


def _lib():
    from deepvoice3_pytorch_amd import ops, _lib
    return ops, _lib.lib()


def _report(what, ratio):
    print("worst-ratio %-72s %.4g" % (what, ratio))


_cache = {}
_first_bits = {}         # (shape, kind) -> (mode, form, bits of y) of the first fp32-output launch


@pytest.fixture(scope="module", autouse=True)
def _release_cache():
    yield
    _cache.clear()
    _first_bits.clear()
    if torch.cuda.is_available():
        torch.cuda.empty_cache()


def _t(a, dev, dtype=torch.float32):
    return torch.from_numpy(np.ascontiguousarray(a)).to(device=dev, dtype=dtype)


def _family(dev, shape):
    key = ("fam", shape)
    if key not in _cache:
        C = shape[1]
        f = G.family_g(shape)
        pre = G.pre_gates(f, shape, device=dev)
        _cache[key] = dict(f=f, pre=pre, a=pre[:, :C], g=pre[:, C:], x=_t(f["x"], dev), w=_t(f["w"], dev),
                           bias=_t(f["bias"], dev))
    return _cache[key]


def _gated_case(dev, shape, kind, spk=None, bf16=False, contracted=True):
    """-> dict(a, g (what the tail holds), r (host) / r_dev, spk_dev, ref, bound) of one shape, gate kind and variant"""
    key = ("gated", shape, kind, spk, bf16, contracted)
    if key not in _cache:
        fam = _family(dev, shape)
        f, a, g = fam["f"], fam["a"], fam["g"]
        s_host = None
        if spk is not None:
            s_host = f[spk]
            a = G.add32(a, s_host if spk == "spk3" else s_host[:, :, None])      # a = rn((acc + bias) + spk): one rounding
        r = G.with_cancellation(kind, f["r"], a, g, f["pairs"], bf16=bf16)
        ref, bnd = G.fwd_bound(kind, a, g, r, contracted=contracted)
        _cache[key] = dict(a=a, g=g, r=r, ref=ref, bnd=bnd, r_dev=_t(r, dev),
                           spk_dev=None if s_host is None else _t(s_host, dev))
    return _cache[key]


def _check_y(got, case, what, pairs, bf16=False):
    """NaN / Inf anywhere fails; -> worst ratio"""
    bnd = G.to_bf16_bound(case["ref"], case["bnd"]) if bf16 else case["bnd"]
    ratio, at = G.worst_ratio(got, case["ref"], bnd)
    assert ratio <= 1.0, "%s: worst at %s: got %r want %r bound %.3g ratio %.3g (a %r g %r r %r)" % (
        what, at, float(got[at]), float(case["ref"][at]), float(bnd[at]), ratio, float(case["a"][at]),
        float(case["g"][at]), float(case["r"][at]))
    n = G.pair_mismatch(np.ascontiguousarray(got), pairs)
    assert n == 0, "%s: %d elements of the paired interior / edge channels differ" % (what, n)
    return ratio


def _mode_consts(ops, kind):
    return (ops.EPI_HIGHWAY if kind == "highway" else ops.EPI_GLU), int(kind == "glu_res")


# ---------------------------------------------------------------------------------------------------------------
# forward: every (mode, form)
# ---------------------------------------------------------------------------------------------------------------
def _run_gated(dev, mode, form, kind, shape):
    """-> worst ratio, or None when the forced form is not eligible for the shape"""
    ops, L = _lib()
    B, C, T, k, d, causal = shape
    M, padL = 2 * C, R.pad_left(k, d, causal)
    fam = _family(dev, shape)
    case = _gated_case(dev, shape, kind)
    hint, switches, sk = (F32_FORMS if mode == "f32" else SPLIT_FORMS)[form]
    pk = ops.pack_weights(fam["w"], None, glu_cg=C, need_bwd=False)
    assert ops.f16_range_events(reset=True) == 0
    epi, residual = _mode_consts(ops, kind)
    outs = []
    with _form(switches, sk):
        for _ in range(2):
            ab = torch.empty(B, M, T, device=dev)
            try:
                y = ops.conv_gemm(fam["x"], pk.fwd, pk.lda, pk.a_half, B=B, Cin=C, Tin=T, M=M, Tout=T, J=k, dil=d,
                                  padL=padL, mode=epi, Cg=C, bias=fam["bias"], residual=residual, ab=ab,
                                  r=None if kind == "glu" else case["r_dev"], a_split=pk.fwd_s, tile_hint=hint)
            except RuntimeError as e:
                assert form != "auto" and ("needs split-bf16" in str(e) or "LDS tile" in str(e)), (form, shape, str(e))
                return None
            census = L.dv3_debug_get(10)
            if not _conv_reached(mode, "gated", form, census, C):
                assert form in ("ksplit", "pp2_streamk"), "%s %s %s %s: census %d" % (kind, mode, form, shape, census)
                return None
            outs.append((y, ab))
    what = "%s %s %s %s" % (kind, mode, form, shape)
    (y, ab), (y2, ab2) = outs
    assert torch.equal(y.view(torch.int32), y2.view(torch.int32)), what + ": a second call differs"
    assert torch.equal(ab.view(torch.int32), ab2.view(torch.int32)), what + ": a second call differs (ab)"
    got_ab = ab.cpu().numpy().astype(np.float64)
    if not np.array_equal(got_ab, fam["pre"]):
        bad = got_ab != fam["pre"]
        i = tuple(int(v) for v in np.argwhere(bad)[0])
        raise AssertionError("%s: %d saved pre-gates are not the exact value; first at %s: got %r want %r" %
                             (what, int(bad.sum()), i, got_ab[i], fam["pre"][i]))
    got = y.cpu().numpy()
    ratio = _check_y(got, case, what, fam["f"]["pairs"])
    bits = got.view(np.int32)
    first = _first_bits.setdefault((shape, kind), (mode, form, bits))
    if first[2] is not bits and not np.array_equal(first[2], bits):
        bad = first[2] != bits
        i = tuple(int(v) for v in np.argwhere(bad)[0])
        raise AssertionError("%s: %d elements differ in their bits from %s %s; first at %s: %r vs %r (a %r g %r r %r)" %
                             (what, int(bad.sum()), first[0], first[1], i, float(got[i]),
                              float(first[2].view(np.float32)[i]), float(case["a"][i]), float(case["g"][i]),
                              float(case["r"][i])))
    return ratio


@pytest.mark.parametrize("mode,form", CONV_CASES)
@pytest.mark.parametrize("kind", G.KINDS)
def test_gated_tail_of_every_form(dev, kind, mode, form):
    """y inside its bound, ab bit-exact, repeatable, paired channels and all fp32-output forms bit-identical"""
    ops, L = _lib()
    prev = ops.set_gemm_precision(mode)
    try:
        ops.f16_range_events(reset=True)
        worst, ran = 0.0, 0
        for shape in (R.STREAMK_SHAPES if form == "pp2_streamk" else R.EDGE_SHAPES):
            r = _run_gated(dev, mode, form, kind, shape)
            assert r is not None or form != "pp2_streamk", "the stream-K form did not take %s" % (shape,)
            if r is not None:
                worst, ran = max(worst, r), ran + 1
        events = ops.f16_range_events(reset=True)
        assert events == 0, "operands inside the fp16 range were counted as outside (%d units)" % events
    finally:
        ops.set_gemm_precision(prev)
    if ran == 0:
        assert form != "auto"
        pytest.skip("%s is not eligible for any edge shape" % form)
    _report("forward fp32 %s %s %s (%d shapes)" % (kind, mode, form, ran), worst)


# ---------------------------------------------------------------------------------------------------------------
# forward: variants on the automatic form
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("spk", ["spk2", "spk3"])
@pytest.mark.parametrize("kind", G.KINDS)
def test_gated_tail_with_speaker_bias(dev, kind, spk, mode):
    """speaker bias (B, C) and (B, C, T), swept in magnitude: a = rn((acc + bias) + spk), saved bit-exact"""
    ops, L = _lib()
    prev = ops.set_gemm_precision(mode)
    worst = 0.0
    try:
        for shape in R.EDGE_SHAPES:
            B, C, T, k, d, causal = shape
            fam, case = _family(dev, shape), _gated_case(dev, shape, kind, spk=spk)
            pk = ops.pack_weights(fam["w"], None, glu_cg=C, need_bwd=False)
            epi, residual = _mode_consts(ops, kind)
            ab = torch.empty(B, 2 * C, T, device=dev)
            s = case["spk_dev"]
            y = ops.conv_gemm(fam["x"], pk.fwd, pk.lda, pk.a_half, B=B, Cin=C, Tin=T, M=2 * C, Tout=T, J=k, dil=d,
                              padL=R.pad_left(k, d, causal), mode=epi, Cg=C, bias=fam["bias"], residual=residual, ab=ab,
                              spk=s, spk_strides=ops._spk_strides(s), r=None if kind == "glu" else case["r_dev"],
                              a_split=pk.fwd_s)
            what = "%s %s %s %s" % (kind, spk, mode, shape)
            want_ab = np.concatenate([case["a"], case["g"]], 1)
            assert np.array_equal(ab.cpu().numpy().astype(np.float64), want_ab), what + ": saved pre-gates"
            worst = max(worst, _check_y(y.cpu().numpy(), case, what, fam["f"]["pairs"]))
        assert ops.f16_range_events(reset=True) == 0
    finally:
        ops.set_gemm_precision(prev)
    _report("forward fp32 %s %s %s" % (kind, spk, mode), worst)


@pytest.mark.parametrize("io", ["ab_bf16", "io_bf16"])
@pytest.mark.parametrize("kind", G.KINDS)
def test_gated_tail_with_bf16_tensors(dev, kind, io):
    """single-term bf16 mode: the pre-gate pair saved as bf16 beside an fp32 output, and bf16 input / residual / output
    tensors (the IOB instantiation of conv_epilogue).  The gate sees the unrounded pair (conv_common.h:249-257)."""
    ops, L = _lib()
    prev = ops.set_gemm_precision("bf16")
    worst, ran = 0.0, 0
    try:
        for shape in R.EDGE_SHAPES:
            B, C, T, k, d, causal = shape
            iob = io == "io_bf16"
            fam, case = _family(dev, shape), _gated_case(dev, shape, kind, bf16=iob)
            pk = ops.pack_weights(fam["w"], None, glu_cg=C, need_bwd=False, split_only=True)
            epi, residual = _mode_consts(ops, kind)
            ab = torch.empty(B, 2 * C, T, device=dev, dtype=torch.bfloat16)
            x = fam["x"].to(torch.bfloat16) if iob else fam["x"]
            r = None if kind == "glu" else (case["r_dev"].to(torch.bfloat16) if iob else case["r_dev"])
            y = ops.conv_gemm(x, pk.fwd, pk.lda, pk.a_half, B=B, Cin=C, Tin=T, M=2 * C, Tout=T, J=k, dil=d,
                              padL=R.pad_left(k, d, causal), mode=epi, Cg=C, bias=fam["bias"], residual=residual, ab=ab,
                              r=r, a_split=pk.fwd_s, out_dtype=torch.bfloat16 if iob else torch.float32)
            what = "%s %s %s" % (kind, io, shape)
            assert y.dtype == (torch.bfloat16 if iob else torch.float32)
            assert np.array_equal(ab.float().cpu().numpy().astype(np.float64), G.rn_bf16(fam["pre"])), what + ": saved pre-gates"
            worst = max(worst, _check_y(y.float().cpu().numpy(), case, what, fam["f"]["pairs"], bf16=iob))
            ran += 1
    finally:
        ops.set_gemm_precision(prev)
    assert ran == len(R.EDGE_SHAPES)
    _report("forward %s %s" % ("bf16" if io == "io_bf16" else "fp32 (bf16 ab)", kind), worst)


C8_SHAPES = [s for s in R.EDGE_SHAPES if s[3] in (1, 3) and (s[3] - 1) * s[4] <= 64 and s[1] % 8 == 0]


@pytest.mark.parametrize("kind", G.KINDS)
def test_gated_tail_of_both_c8_kernels(dev, kind):
    """c8 output, c8 residual, c8 pre-gate save through conv_planes.hip (8xxx) and conv_c8pp.hip (9101): the gate sees the
    UNROUNDED fp32 pre-gates (conv_common.h:790-801), the save is bf16_rn of them, y the fp32 bound plus one bf16 rounding;
    the two kernels return the same bits"""
    ops, L = _lib()
    prev = ops.set_gemm_precision("bf16")
    worst, ran = {"planes": 0.0, "c8pp": 0.0}, {"planes": 0, "c8pp": 0}
    try:
        for shape in C8_SHAPES:
            B, C, T, k, d, causal = shape
            fam, case = _family(dev, shape), _gated_case(dev, shape, kind, bf16=True, contracted=False)
            pk = ops.pack_weights(fam["w"], None, glu_cg=C, need_bwd=False, split_only=True)
            epi, residual = _mode_consts(ops, kind)
            x8 = ops.to_c8(fam["x"])
            r8 = None if kind == "glu" else ops.to_c8(case["r_dev"])
            bits = {}
            for tag, thr in (("planes", 0), ("c8pp", 1)):
                with _form({"DV3_SW_C8PP_MIN_TILES": thr}):
                    ab8 = ops._c8_empty(B, 2 * C, T, dev)
                    y8 = ops.conv_gemm(None, None, pk.lda, pk.a_half, B=B, Cin=C, Tin=T, M=2 * C, Tout=T, J=k, dil=d,
                                       padL=R.pad_left(k, d, causal), mode=epi, Cg=C, bias=fam["bias"], residual=residual,
                                       ab=ab8, r=r8, a_split=pk.fwd_s, x_c8=x8, out_c8=True)
                    census = L.dv3_debug_get(10)
                assert census // 1000 == (8 if tag == "planes" else 9), (tag, shape, census)
                what = "%s c8 %s %s" % (kind, tag, shape)
                with torch.no_grad():
                    y = ops.from_c8(y8, C).cpu().numpy()
                    ab = ops.from_c8(ab8, 2 * C).cpu().numpy()
                assert np.array_equal(ab.astype(np.float64), G.rn_bf16(fam["pre"])), what + ": saved pre-gates"
                worst[tag] = max(worst[tag], _check_y(y, case, what, fam["f"]["pairs"], bf16=True))
                ran[tag] += 1
                bits[tag] = y.view(np.int32)
            assert np.array_equal(bits["planes"], bits["c8pp"]), "%s %s: the two c8 kernels differ" % (kind, shape)
    finally:
        ops.set_gemm_precision(prev)
    assert ran["planes"] == ran["c8pp"] == len(C8_SHAPES)
    for tag in ("planes", "c8pp"):
        _report("forward c8 %s %s (%d shapes)" % (kind, tag, ran[tag]), worst[tag])


def _plain_case(dev, shape, act, chain, il2):
    """plain tail on the (2C, C, k) weights: rows of r / r2 from the sweeps; the interleaved ConvTranspose store reads
    bias[m mod C] for row m"""
    key = ("plain", shape, act, chain, il2)
    if key not in _cache:
        fam = _family(dev, shape)
        f, pre = fam["f"], fam["pre"]
        C = shape[1]
        b64 = f["bias"].astype(np.float64).reshape(1, -1, 1)
        if il2:
            pre = pre - b64 + np.concatenate([b64[:, :C], b64[:, :C]], 1)
        r = np.concatenate([f["r"], f["dy"]], 1) if chain >= 1 else None
        r2 = np.concatenate([f["spk3"], f["r"]], 1) if chain >= 2 else None
        ref, bnd = G.act_bound(act, pre, r, r2)
        _cache[key] = dict(pre=pre, ref=ref, bnd=bnd, r=None if r is None else _t(r, dev),
                           r2=None if r2 is None else _t(r2, dev))
    return _cache[key]


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("variant", ["plain", "r", "r_r2", "interleave2"])
@pytest.mark.parametrize("act", G.ACTS)
def test_plain_tails(dev, act, variant, mode):
    """LINEAR / RELU / SIGMOID / SOFTSIGN, with r, with r and r2, and with the interleaved ConvTranspose store; LINEAR and
    RELU without a residual are exact"""
    ops, L = _lib()
    prev = ops.set_gemm_precision(mode)
    epi = {"linear": ops.EPI_LINEAR, "relu": ops.EPI_RELU, "sigmoid": ops.EPI_SIGMOID, "softsign": ops.EPI_SOFTSIGN}[act]
    chain = {"plain": 0, "r": 1, "r_r2": 2, "interleave2": 0}[variant]
    il2 = variant == "interleave2"
    worst = 0.0
    try:
        for shape in R.EDGE_SHAPES:
            B, C, T, k, d, causal = shape
            fam, case = _family(dev, shape), _plain_case(dev, shape, act, chain, il2)
            pk = ops.pack_weights(fam["w"], None, need_bwd=False)
            y = ops.conv_gemm(fam["x"], pk.fwd, pk.lda, 0, B=B, Cin=C, Tin=T, M=2 * C, Tout=T, J=k, dil=d,
                              padL=R.pad_left(k, d, causal), mode=epi, bias=fam["bias"], r=case["r"], r2=case["r2"],
                              a_split=pk.fwd_s, store_mode=ops.STORE_INTERLEAVE2 if il2 else ops.STORE_BCT)
            got = y.cpu().numpy()
            if il2:         # row m -> channel m mod C, column 2 t + m // C
                assert got.shape == (B, C, 2 * T)
                got = np.concatenate([got[:, :, 0::2], got[:, :, 1::2]], 1)
            what = "%s %s %s %s" % (act, variant, mode, shape)
            if act in ("linear", "relu") and chain == 0:
                assert np.array_equal(got.astype(np.float64), case["ref"]), what + ": not exact"
            ratio, at = G.worst_ratio(got, case["ref"], case["bnd"])
            assert ratio <= 1.0, "%s: worst at %s: got %r want %r bound %.3g ratio %.3g" % (
                what, at, float(got[at]), float(case["ref"][at]), float(case["bnd"][at]), ratio)
            worst = max(worst, ratio)
        assert ops.f16_range_events(reset=True) == 0
    finally:
        ops.set_gemm_precision(prev)
    _report("forward fp32 %s %s %s" % (act, variant, mode), worst)


# ---------------------------------------------------------------------------------------------------------------
# backward
# ---------------------------------------------------------------------------------------------------------------
def _bwd_inputs(B, C, T, kind, bf16):
    """g: the ladder per (b, channel) plus multiples of 2^-5 within +-2; a, x, dy: the magnitude sweeps.  Plain modes: the
    saved activation output y = fp32(act(g)).  bf16: everything the kernel reads as bf16 rounded to bf16 first."""
    key = ("bwd", B, C, T, kind, bf16)
    if key in _cache:
        return _cache[key]
    rng = np.random.RandomState(B * 1000 + C + T)
    lad = np.asarray(G.LADDER)
    g = lad[(np.arange(C).reshape(1, C, 1) + np.arange(B).reshape(B, 1, 1)) % 21] + rng.randint(-64, 65, size=(B, C, T)) * 2.0 ** -5
    a, x, dy = G.sweep(rng, (B, C, T)), G.sweep(rng, (B, C, T)), G.sweep(rng, (B, C, T))
    a = np.roll(a, 5, axis=2) if T > 5 else a              # a, x and dy do not share a frame class
    x = np.roll(x, 11, axis=2) if T > 11 else x
    g = g.astype(np.float32)
    rb = (lambda v: G.rn_bf16(v).astype(np.float32)) if bf16 else (lambda v: v)
    out = dict(dy=dy, a=rb(a), g=rb(g), x=x)
    if bf16 == "c8":
        out["dy"], out["x"] = rb(dy), rb(x)
    if kind in G.ACTS:
        out["y"] = rb(G.act_fwd(kind, g.astype(np.float64)).astype(np.float32))
    _cache[key] = out
    return out


ALPHA = G.RS2_32         # an fp32 number: the reference multiplies by the same value


def _bwd_reference(kind, inp, T, depth):
    """-> list of (name, ref, bound) for dab (B, 2C | C, T), dres, part"""
    dy = inp["dy"].astype(np.float64)
    if kind in G.KINDS:
        x = inp["x"].astype(np.float64) if kind == "highway" else None
        (ra, rg, rr), (ba, bg, br) = G.bwd_bound(kind, dy, inp["a"], inp["g"], x)
        ref, bnd = np.concatenate([ra, rg], 1), np.concatenate([ba, bg], 1)
        dres = (rr, br)
    else:
        ref, bnd = G.act_bwd_bound(kind, dy, None if kind == "linear" else inp["y"], ALPHA)
        dres = None
    part = (ref.sum(2), G.row_sum_bound(np.abs(ref).sum(2), bnd.sum(2), depth))
    return (ref, bnd), dres, part


def _assert_in(got, ref, bnd, what):
    ratio, at = G.worst_ratio(got, ref, bnd)
    assert ratio <= 1.0, "%s: worst at %s: got %r want %r bound %.3g ratio %.3g" % (
        what, at, float(np.asarray(got)[at]), float(ref[at]), float(bnd[at]), ratio)
    return ratio


@pytest.mark.parametrize("B,C,T", BWD_SHAPES)
@pytest.mark.parametrize("kind", BWD_KINDS)
def test_gate_backward_elementwise(dev, kind, B, C, T):
    """ops.gate_bwd against the float64 autograd: 16-byte and 4-byte rows (switch 55), fp32 and pair-word gradients, an
    fp32 and a bf16 pre-gate save"""
    ops, L = _lib()
    gated = kind in G.KINDS
    epi = {"glu": ops.EPI_GLU, "glu_res": ops.EPI_GLU, "highway": ops.EPI_HIGHWAY, "linear": ops.EPI_LINEAR,
           "relu": ops.EPI_RELU, "sigmoid": ops.EPI_SIGMOID, "softsign": ops.EPI_SOFTSIGN}[kind]
    worst = {"fp32": 0.0, "pair": 0.0}
    for ab16 in ((False, True) if gated else (False,)):
        inp = _bwd_inputs(B, C, T, kind, ab16)
        dy = _t(inp["dy"], dev)
        saved = None
        if gated:
            saved = _t(np.concatenate([inp["a"], inp["g"]], 1), dev, torch.bfloat16 if ab16 else torch.float32)
        elif kind != "linear":
            saved = _t(inp["y"], dev)
        x = _t(inp["x"], dev) if kind == "highway" else None
        for sw in (0, 1):
            # the launcher takes the 16-byte form when the switch is on and every row starts at the same 16-byte phase
            depth = max(G.depth_gate_bwd(T, True), G.depth_gate_bwd(T, False)) if sw else G.depth_gate_bwd(T, False)
            (ref, bnd), dres_ref, part_ref = _bwd_reference(kind, inp, T, depth)
            plain = None
            for pair in ((False, True) if gated else (False,)):
                with _form({"DV3_SW_GATE_VEC": sw}):
                    dab, dres, part = ops.gate_bwd(dy, saved, x, B=B, C=C, T=T, mode=epi, residual=int(kind == "glu_res"),
                                                   pair=pair, want_dres=gated, alpha=1.0 if gated else ALPHA)
                    torch.cuda.synchronize()
                what = "%s (%d, %d, %d) switch55=%d pair=%d ab16=%d" % (kind, B, C, T, sw, pair, ab16)
                if pair:
                    words = dab.cpu().numpy().view(np.int32)
                    assert np.array_equal(words, R.pair_words(plain).view(torch.int32).numpy()), what + ": pair words"
                    # hi + lo = v - e, |e| <= 2^-17 |v| (include/dv3hip.h, tests/gemm_split_ref.py: delta), and one bf16
                    # rounding in the subnormal range for lo (the sweeps reach 2^-130, where bf16 numbers are 2^-133 apart)
                    worst["pair"] = max(worst["pair"], _assert_in(G.pair_value(words), ref,
                                                                  bnd + 2.0 ** -17 * (np.abs(ref) + bnd) + G.TINY_B, what))
                else:
                    plain = dab.cpu().numpy()
                    worst["fp32"] = max(worst["fp32"], _assert_in(plain, ref, bnd, what))
                if dres_ref is not None:
                    _assert_in(dres.cpu().numpy(), dres_ref[0], dres_ref[1], what + " dres")
                _assert_in(part.cpu().numpy(), part_ref[0], part_ref[1], what + " row sums")
    _report("backward fp32 %s (%d, %d, %d)" % (kind, B, C, T), worst["fp32"])
    if gated:
        _report("backward pair %s (%d, %d, %d)" % (kind, B, C, T), worst["pair"])


# gated c8 tensors hold whole 8-channel groups (dv3_gate_bwd_f32: C % 8 == 0 in the gated modes)
@pytest.mark.parametrize("kind,B,C,T", [(kd, B, C, T) for kd in BWD_KINDS for (B, C, T) in BWD_SHAPES
                                        if kd in G.ACTS or C % 8 == 0])
def test_gate_backward_c8_elementwise(dev, kind, B, C, T):
    """ops.gate_bwd_c8 on the same inputs rounded to bf16: the v_exp_f32 + v_rcp_f32 sigmoid (switch 56 = 1, default) and
    the libm form (0), each against the same bound plus the bf16 store"""
    ops, L = _lib()
    gated = kind in G.KINDS
    epi = {"glu": ops.EPI_GLU, "glu_res": ops.EPI_GLU, "highway": ops.EPI_HIGHWAY, "linear": ops.EPI_LINEAR,
           "relu": ops.EPI_RELU, "sigmoid": ops.EPI_SIGMOID, "softsign": ops.EPI_SOFTSIGN}[kind]
    inp = _bwd_inputs(B, C, T, kind, "c8")
    (ref, bnd), dres_ref, part_ref = _bwd_reference(kind, inp, T, G.depth_gate_bwd_c8(T))
    dy8 = ops.to_c8(_t(inp["dy"], dev))
    saved = None
    if gated:
        saved = ops.to_c8(_t(np.concatenate([inp["a"], inp["g"]], 1), dev))
    elif kind != "linear":
        saved = ops.to_c8(_t(inp["y"], dev))
    x8 = ops.to_c8(_t(inp["x"], dev)) if kind == "highway" else None
    rows = 2 * C if gated else C
    for fast in (1, 0):
        with _form({"DV3_SW_GATE_C8_FAST": fast}):
            dab8, dres8, part = ops.gate_bwd_c8(dy8, saved, x8, B=B, C=C, T=T, mode=epi, residual=int(kind == "glu_res"),
                                                want_dres=gated, alpha=1.0 if gated else ALPHA)
            torch.cuda.synchronize()
        what = "c8 %s (%d, %d, %d) switch56=%d" % (kind, B, C, T, fast)
        with torch.no_grad():
            dab = ops.from_c8(dab8, rows).cpu().numpy()
            dres = ops.from_c8(dres8, C).cpu().numpy() if dres8 is not None else None
        worst = _assert_in(dab, ref, G.to_bf16_bound(ref, bnd), what)
        if dres_ref is not None:
            _assert_in(dres, dres_ref[0], G.to_bf16_bound(*dres_ref), what + " dres")
        _assert_in(part.cpu().numpy(), part_ref[0], part_ref[1], what + " row sums")
        _report("backward c8 %s %s (%d, %d, %d)" % ("fast" if fast else "libm", kind, B, C, T), worst)


@pytest.mark.parametrize("gemm_mode", ["f16x3", "bf16x3"])
@pytest.mark.parametrize("pkind,ckind,B,C,T,k,d", [FUSE_T.CHAINS[0], FUSE_T.CHAINS[3]])
def test_fused_gate_backward_on_the_ladder(dev, gemm_mode, pkind, ckind, B, C, T, k, d):
    """two chains of test_gpu_gate_fuse.py with the producer's bias on the ladder: the fused tail and the stand-alone
    kernel agree bit for bit in saturation too (the bias gradient by the order of its partial sums only)"""
    ops, L = _lib()
    assert (pkind, B, C, T) in (("glu_res", 3, 64, 150), ("glu_res", 2, 256, 200))
    prev = ops.set_gemm_precision(gemm_mode)
    prev_max, ops.fuse_gate_max_elems = ops.fuse_gate_max_elems, 1 << 40
    try:
        rng = np.random.RandomState(B * 1000 + C + T)
        pv, pg, _ = FUSE_T._gated_params(rng, C, k)
        lad = np.asarray(G.LADDER, dtype=np.float32)
        pb = torch.from_numpy(np.concatenate([lad[(rng.permutation(C) + 3) % 21], lad[rng.permutation(C) % 21]]))
        pcfg = ops.LayerCfg(k=k, dil=d, causal=False, mode=ops.EPI_GLU, residual=True, p=0.1, training=True, site="prod")
        (cv, cg, cb), ccfg = FUSE_T._consumer(ops, rng, ckind, C, k, d)
        x = torch.from_numpy(rng.randn(B, C, T).astype(np.float32))
        tensors = [x, pv, pg, pb, cv, cg, cb]
        wgt = torch.from_numpy(rng.randn(B, C if ckind == "glu" else cv.shape[0], T).astype(np.float32))
        y1, g1, _, st1 = FUSE_T._run_chain(ops, dev, tensors, pcfg, ccfg, wgt, True)
        y0, g0, _, st0 = FUSE_T._run_chain(ops, dev, tensors, pcfg, ccfg, wgt, False)
    finally:
        ops.fuse_gate_max_elems = prev_max
        ops.set_gemm_precision(prev)
    assert st1["fused"] == 1, st1
    assert st0["fused"] == 0 and st0["standalone"] >= 1, st0
    assert torch.equal(y1, y0) and torch.isfinite(y1).all()
    for n, a, b in zip(("dx", "p.dv", "p.dg", "p.dbias", "c.dv", "c.dg", "c.dbias"), g1, g0):
        assert torch.isfinite(a).all(), n
        if n == "p.dbias":
            assert rel_err(a, b) < 2e-6, n
        else:
            assert torch.equal(a, b), "%s differs from the stand-alone gate backward: %g" % (n, rel_err(a, b))

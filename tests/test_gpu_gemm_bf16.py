# coding: utf-8
"""-m gpu: the single-term bf16 GEMMs ("bf16" mode: operands rounded to bf16 at the matrix-core inputs, fp32 accumulate),
fp32 storage and channel-blocked bf16 storage (c8), element by element (tests/gemm_split_ref.py).

Raw GEMM level with plain weights (ops.pack_weights(w, None, ...)), as tests/test_gpu_gemm_operands.py.  Products of two
bf16 values are exact in fp32, so a kernel differs from the float64 GEMM OF THE SAME ROUNDED OPERANDS by fp32 summation
only: (n + c) 2^-24 sum |a| |b| whatever the order, n the accumulation depth and c the roundings of the epilogue, stated
beside every bound below.  A c8 / bf16 output adds exactly one round-to-nearest-even (gemm_split_ref.bf16_out_bound).

EXACT families (E1 .. E5): fp32 outputs equal the exact value, bf16 outputs equal bf16_rn(exact), in every element; the
padding channels of a c8 output are zero.  E5 (fp32 storage) holds bf16 midpoints and their fp32 neighbours, where round
to nearest even, truncation and round-half-away part.  BOUNDED families (B1 .. B5): inside the derived bound.  For c8
tensors the operands are rounded to bf16 on the host first (that is what the tensor holds); fp32 tensors are rounded by
the kernel.  tests/test_cpu_gemm_bf16_ref.py shows what these checks catch.

Every case names a kernel form and asserts from the launch census (dv3_debug_get(10 / 11)) that the form ran; a forced
form that is not eligible for a shape is passed over for that shape, the automatic form never is.  Every launch is made
twice and must return the same bits.  Each case prints its worst ratio to the bound.
"""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tests import gemm_split_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu

MODE = "bf16"
FAMILIES = R.EXACT_BF16 + R.BOUNDED
RS2 = float(np.float32(0.70710678118654752440))           # the sqrt(.5) a residual layer hands to r_scale, as fp32
# fp32 storage, tap-GEMM: form -> tile_hint (tile ids 1 .. 9 of csrc/conv_gemm_bf16x3.hip; the 256 x 256 and k-split kernels
# do not take split_terms == 1)
CONV_FORMS = dict([("auto", 0)] + [("tile%d" % t, t) for t in range(21, 30)])
# fp32 storage, weight gradient: form -> (k_split, masked, switches, census for three taps).  With split_bf16 == 2 the
# dispatcher keeps the two-steps-ahead kernel out (it is a three-term kernel): its switch leads to the per-tap tile
WGRAD_FORMS = {"auto": None, "slabs": (False, False, {}, 4010), "k_split": (True, False, {}, 4030),
               "k_split_masked": (True, True, {}, 4030), "all_taps": (True, False, {"DV3_SW_WGRAD_TILE": 3}, 4030),
               "two_steps_ahead": (True, False, {"DV3_SW_WGRAD_TILE": 4, "DV3_SW_WGRAD_T2_WINDOW": 0}, 4010)}
# c8 tap-GEMM: form -> (switches, census)
C8_FORMS = {"auto": ({}, None), "planes1": ({"DV3_SW_PLANES_TILE": 1}, 8010), "planes2": ({"DV3_SW_PLANES_TILE": 2}, 8020),
            "planes9": ({"DV3_SW_PLANES_TILE": 9}, 8090),
            "c8pp": ({"DV3_SW_C8PP_MIN_TILES": 1, "DV3_SW_C8PP_NW4": 0}, 9101),
            "c8pp_nw4": ({"DV3_SW_C8PP_MIN_TILES": 1, "DV3_SW_C8PP_NW4": 1}, 9111)}


def _wgrad_c8(tr, pf2=None, il=None):
    sw = {"DV3_SW_WGRAD_C8_TR": tr}
    if pf2 is not None:
        sw.update({"DV3_SW_WGRAD_C8_PF2": pf2, "DV3_SW_WGRAD_C8_IL": il})
    return sw


# wgrad_c8: form -> (switches, census without the tap count, + when three taps)
WGRAD_C8_FORMS = {"reg_pf1": (_wgrad_c8(0, 0, 0), 5000, 0), "reg_pf2": (_wgrad_c8(0, 1, 0), 5020, 0),
                  "reg_pf2_il": (_wgrad_c8(0, 1, 1), 5020, 40), "tr": (_wgrad_c8(1), 5100, 0), "tr_il": (_wgrad_c8(2), 5100, 40),
                  "tr_pair": (_wgrad_c8(3), 5300, 0), "tr_pair_il": (_wgrad_c8(4), 5300, 40)}


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


def _lib():
    from deepvoice3_pytorch_amd import ops, _lib
    return ops, _lib.lib()


@pytest.fixture()
def bf16_mode():
    """the GEMM mode and the storage switch as they were (the library's switches: _lib.switches, scoped in each test)"""
    ops, L = _lib()
    prev = (ops.gemm_precision(), ops.bf16_storage)
    ops.set_gemm_precision(MODE)
    try:
        yield ops, L
    finally:
        ops.set_gemm_precision(prev[0])
        ops.bf16_storage = prev[1]


def _switches(switches):
    from deepvoice3_pytorch_amd import _lib
    return _lib.switches(switches)


_by_output = {}


def _note(kind, ratio):
    """worst ratio per kind of output of the running case (an fp32 tail or a bf16 store, whose half ulp nearly fills its bound)"""
    _by_output[kind] = max(_by_output.get(kind, 0.0), ratio)
    return ratio


def _report(what, ratio):
    print("worst-ratio %-72s %.4g" % (what, ratio))
    for kind in sorted(_by_output):
        print("worst-ratio %-72s %.4g" % ("  %s | %s" % (what, kind), _by_output[kind]))
    _by_output.clear()


_cache = {}


@pytest.fixture(scope="module", autouse=True)
def _release_cache():
    yield
    _cache.clear()
    if torch.cuda.is_available():
        torch.cuda.empty_cache()


def _cached(key, make):
    if key not in _cache:
        _cache[key] = make()
    return _cache[key]


def _dims(shape):
    B, C, T, k, d, causal = shape[:6]
    return B, C, T, k, d, R.pad_left(k, d, causal), R.c8_shape_M(shape)


def _operands(dev, fam, gemm, shape, c8):
    """-> (f, act, wgt): the family's operands as the tensors hold them -- c8 activations rounded to bf16 on the host"""
    def make():
        f = R.family(fam, gemm, MODE, shape)
        act, wgt = f["act"], f["wgt"]
        if c8:
            act = R.bf16_rn(act).astype(np.float32)
            if gemm == "wgrad":
                wgt = R.bf16_rn(wgt).astype(np.float32)
        return f, act, wgt
    return _cached(("operands", fam, gemm, shape, c8), make)


def _keep(shape3, seed):
    """a dropout keep mask with p = 0.5: 1 / (1 - p) = 2 is exact"""
    return np.random.RandomState(seed).rand(*shape3) < 0.5


def _expect(dev, key, exact, out_bf16, mm, act, wgt, n, **kw):
    """cached (want, bound) of gemm_split_ref.check_prepared for one expectation"""
    def make():
        tail, bnd = R.expect_bf16(mm, act, wgt, n, device=dev, **kw)
        return R.prepare_bf16(exact, tail, bnd, str(key), out_bf16)
    return _cached(("expect",) + key + (out_bf16,), make)


def _up(a, dev, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    return t if dtype is None else t.to(dtype)


def _to_c8(v, dev):
    """host c8 image of bf16 values -> device tensor bf16 [B][G][T][8]"""
    t = torch.from_numpy(R.c8_pack(v).view(np.int16)).to(dev).view(torch.bfloat16)
    t._dv3_C = v.shape[1]
    return t


def _from_c8(t, C, what):
    """device c8 tensor -> float64 (B, C, T) on its device; the padding channels must be zero"""
    got, pad = R.c8_unpack(t.contiguous().view(torch.int16).cpu().numpy().view(np.uint16), C)
    assert pad == 0.0, "%s: a padding channel of the c8 output holds %r" % (what, pad)
    return torch.from_numpy(got).to(t.device)


def _same_bits(a, b, what):
    ia = a.view(torch.int16) if a.dtype == torch.bfloat16 else a.view(torch.int32)
    ib = b.view(torch.int16) if b.dtype == torch.bfloat16 else b.view(torch.int32)
    assert torch.equal(ia, ib), what + ": a second call differs"


# ---------------------------------------------------------------------------------------------------------------
# fp32 storage: tap-GEMM variants 4xxx
# ---------------------------------------------------------------------------------------------------------------
def _run_conv_f32(dev, form, fam, shape):
    """forward linear, gated through its saved pre-gate pair (fp32 and bf16), input gradient with a keep-bit ymask
    -> worst ratio, or None when the forced tile is not eligible for the shape"""
    ops, L = _lib()
    B, C, T, k, d, padL, M = _dims(shape)
    hint = CONV_FORMS[form]
    exact = fam[0] == "E"
    worst = 0.0
    for gemm in ("fwd", "gated", "gated_ab_bf16", "dgrad"):
        data = "dgrad" if gemm == "dgrad" else "fwd"
        f, act, wgt = _operands(dev, fam, data, shape, False)
        mm = R.make_mm(data, d, padL, k)
        n = R.n_products(data, MODE, J=k, K=(M if data == "dgrad" else C), B=B, T=T)
        x, w = _up(act, dev), _up(wgt, dev)
        bias = None if f["addend"] is None else _up(f["addend"], dev)
        pk = ops.pack_weights(w, None, glu_cg=C if gemm.startswith("gated") else 0, need_bwd=(gemm == "dgrad"))
        if gemm == "dgrad":
            keep = _keep((B, C, T), 11)
            words, rs = R.keep_bits_words(keep)
            ymask = _up(words, dev)
            # n products, + 1: the drop_scale product on the accumulator, + 1: the add of r_scale * r (r = 0 here)
            want, bnd = _expect(dev, (fam, "dgrad_ymask", shape), exact, False, mm, act, wgt, n, out_keep=keep, scale=2.0, ops=2)
        else:
            # n products, + 2: the bias add and the store (gemm_split_ref.EPILOGUE_OPS); a bf16 pre-gate save rounds once more
            want, bnd = _expect(dev, (fam, "fwd", shape), exact, gemm == "gated_ab_bf16", mm, act, wgt, n,
                                addend=R.bias_bcast(f["addend"]), ops=R.EPILOGUE_OPS)
        outs = []
        for _ in range(2):
            try:
                if gemm == "dgrad":
                    y = ops.conv_gemm(x, pk.bwd, pk.ldb, 0, B=B, Cin=M, Tin=T, M=C, Tout=T, J=k, dil=d, padL=(k - 1) * d - padL,
                                      mode=ops.EPI_DGRAD, a_split=pk.bwd_s, tile_hint=hint, ymask=ymask, ymask_rs=rs,
                                      drop_scale=2.0)
                elif gemm == "fwd":
                    y = ops.conv_gemm(x, pk.fwd, pk.lda, 0, B=B, Cin=C, Tin=T, M=M, Tout=T, J=k, dil=d, padL=padL,
                                      mode=ops.EPI_LINEAR, bias=bias, a_split=pk.fwd_s, tile_hint=hint)
                else:
                    y = torch.empty(B, M, T, device=dev, dtype=torch.bfloat16 if gemm == "gated_ab_bf16" else torch.float32)
                    ops.conv_gemm(x, pk.fwd, pk.lda, pk.a_half, B=B, Cin=C, Tin=T, M=M, Tout=T, J=k, dil=d, padL=padL,
                                  mode=ops.EPI_GLU, Cg=C, bias=bias, ab=y, a_split=pk.fwd_s, tile_hint=hint)
            except RuntimeError as e:
                assert form != "auto" and ("needs split-bf16" in str(e) or "LDS tile" in str(e) or "not eligible" in str(e)), \
                    (form, gemm, shape, str(e))
                return None
            census = L.dv3_debug_get(10)
            # family 4 = one bf16 MFMA per product; tile id; + 1: the 8-wave tiles' ping-pong main loop
            assert census // 1000 == 4, (form, gemm, shape, census)
            if form != "auto":
                assert census % 1000 // 10 == hint - 20, (form, gemm, shape, census)
            outs.append(y)
        what = "%s bf16 fp32-storage %s %s %s" % (gemm, form, fam, shape)
        _same_bits(outs[0], outs[1], what)
        worst = max(worst, _note("%s, %s out" % (gemm, "bf16" if gemm == "gated_ab_bf16" else "fp32"),
                                 R.check_prepared(exact, outs[0], want, bnd, what)))
    return worst


@pytest.mark.parametrize("fam", FAMILIES)
@pytest.mark.parametrize("form", list(CONV_FORMS))
def test_fp32_storage_tap_gemm_elementwise(dev, bf16_mode, form, fam):
    worst, ran = 0.0, 0
    for shape in R.EDGE_SHAPES:
        r = _run_conv_f32(dev, form, fam, shape)
        if r is not None:
            worst, ran = max(worst, r), ran + 1
    assert ran > 0, "%s is not eligible for any edge shape" % form
    _report("conv bf16 fp32-storage %s %s (%d shapes)" % (form, fam, ran), worst)


# ---------------------------------------------------------------------------------------------------------------
# fp32 storage: weight gradient, split_bf16 == 2
# ---------------------------------------------------------------------------------------------------------------
def _run_wgrad_f32(dev, form, fam, shape):
    ops, L = _lib()
    B, C, T, k, d, padL, M = _dims(shape)
    small = M <= 64 and C <= 64           # dv3_wgrad_gemm_f32: such layers run the exact fp32 kernel in every mode
    spec = WGRAD_FORMS[form]
    if spec is None:                      # the choice of ops.ConvLayerFn.backward
        x3, S = ops.wgrad_plan(B, M, C, T, k)
        assert x3 == (not small)
        ksplit, masked, switches, want_census = x3, False, {}, None
    else:
        if small:
            return None                   # the single-term forms do not serve these layers
        ksplit, masked, switches, want_census = spec
        S = 3 if ksplit else min(B, 2)
    exact = fam[0] == "E"
    f, act, wgt = _operands(dev, fam, "wgrad", shape, False)
    mm = R.make_mm("wgrad", d, padL, k)
    keep = _keep((B, C, T), 5) if masked else None
    bits = rs = None
    if masked:
        words, rs = R.keep_bits_words(keep)
        bits = _up(words, dev)
    if small:       # the exact fp32 kernel: the float64 GEMM of the fp32 operands, the f32 mode's depth.  (E4 / E5 are built for
        # bf16 operands: their full fp32 products do not add exactly, so here they are held to the bound like B1 .. B5)
        exact = exact and fam not in ("E4", "E5")

        def make():
            n = R.n_products("wgrad", "f32", J=k, K=M, B=B, T=T, n_slabs=S)
            return (R.reference(mm, act, wgt, device=dev), R.bound(mm, act, wgt, None, None, n, device=dev)[0])
        want, bnd = _cached(("expect", fam, "wgrad_small", shape, S), make)
    else:
        # n: the frames of the largest slab (the slabs are added in float64 below), + 1: the drop_scale product of a masked form
        n = R.n_products("wgrad", MODE, J=k, K=M, B=B, T=T, n_slabs=S, k_split=bool(ksplit))
        want, bnd = _expect(dev, (fam, "wgrad", shape, S, bool(ksplit), masked), exact, False, mm, act, wgt, n,
                            wgt_keep=keep, scale=2.0 if masked else 1.0, ops=1 if masked else 0)
    g, x = _up(act, dev), _up(wgt, dev)
    outs = []
    with _switches(switches):
        for _ in range(2):
            o = ops.wgrad_gemm(g, x, B=B, M=M, Cin=C, T=T, Tin=T, J=k, dil=d, padL=padL, n_slabs=S, xmask=bits,
                               xmask_rs=rs or 0, drop_scale=2.0 if masked else 1.0, split_bf16=not small, k_split=ksplit)
            census = L.dv3_debug_get(11)
            outs.append(o)
    # csrc/wgrad_gemm.hip, wgrad_gemm_bf16x3.hip: 1000 the exact kernel of small layers, 4010 the per-tap 128 x 128 tile,
    # 4030 the all-taps kernel (three taps, k-split)
    if small:
        assert census == 1000, (form, shape, census)
    elif want_census is None:
        assert census == (4030 if k == 3 else 4010), (form, shape, census)
    else:
        assert census == (want_census if k == 3 else 4010), (form, shape, census)
    what = "wgrad bf16 fp32-storage %s %s %s" % (form, fam, shape)
    _same_bits(outs[0], outs[1], what)
    assert torch.isfinite(outs[0]).all(), what
    got = outs[0].double().sum(0)         # [S][J][M][C] -> (J, M, C): the slabs added in float64
    return R.check_prepared(exact, got, want, bnd, what)


@pytest.mark.parametrize("fam", FAMILIES)
@pytest.mark.parametrize("form", list(WGRAD_FORMS))
def test_fp32_storage_wgrad_elementwise(dev, bf16_mode, form, fam):
    worst, ran = 0.0, 0
    for shape in R.EDGE_SHAPES:
        r = _run_wgrad_f32(dev, form, fam, shape)
        if r is not None:
            worst, ran = max(worst, r), ran + 1
    assert ran > 0
    _report("wgrad bf16 fp32-storage %s %s (%d shapes)" % (form, fam, ran), worst)


# ---------------------------------------------------------------------------------------------------------------
# c8 storage: tap-GEMM (conv_planes, conv_c8pp; fp32 -> c8 on the 4xxx kernels)
# ---------------------------------------------------------------------------------------------------------------
def _c8_census_ok(census, want):
    return census // 1000 in (8, 9) if want is None else census == want


def _addend_r(dev, fam, shape, f, scale_of):
    """the c8 addend of the input gradient: whole quanta (|m| <= 15) for the exact families, else bf16 values of the
    output's own size"""
    B, C, T = shape[0], shape[1], shape[2]
    rng = np.random.RandomState(23 + C + T)
    if fam[0] == "E":
        return (rng.randint(-15, 16, size=(B, C, T)) * f["quantum"]).astype(np.float32)
    return R.bf16_rn((rng.standard_normal((B, C, T)) * scale_of()).astype(np.float32)).astype(np.float32)


def _run_conv_c8(dev, form, fam, shape, variants=None):
    """every c8 form of the tap-GEMM for one shape -> (worst ratio, {variant: census})"""
    ops, L = _lib()
    B, C, T, k, d, padL, M = _dims(shape)
    switches, want_census = C8_FORMS[form]
    exact = fam[0] == "E"
    gated_ok = len(shape) == 6
    worst, seen = 0.0, {}
    todo = [("fwd", v) for v in ("linear", "glu", "highway", "to_f32", "keep_bytes")] + \
           [("dgrad", v) for v in ("ymask", "ymask_r1", "ymask_r_rs2", "to_f32_ymask")]
    if form == "auto":
        todo.append(("fwd", "from_f32_keep_bits"))          # an fp32 input: the 4xxx kernels, which the c8 switches do not reach
    for gemm, var in todo:
        if var in ("glu", "highway") and not gated_ok:
            continue
        if variants is not None and var not in variants:
            continue
        f, act, wgt = _operands(dev, fam, gemm, shape, True)
        mm = R.make_mm(gemm, d, padL, k)
        n = R.n_products(gemm, MODE, J=k, K=(M if gemm == "dgrad" else C), B=B, T=T)
        w = _up(wgt, dev)
        gated = var in ("glu", "highway")
        pk = ops.pack_weights(w, None, glu_cg=C if gated else 0, need_bwd=(gemm == "dgrad"))
        out_f32 = var.startswith("to_f32")
        kw = dict(B=B, J=k, dil=d, Tin=T, Tout=T)
        if gemm == "fwd":
            bias = None if f["addend"] is None else _up(f["addend"], dev)
            masked = var in ("keep_bytes", "from_f32_keep_bits")
            keep = _keep((B, C, T), 13) if masked else None
            # n products, + 2: the bias add and the store (EPILOGUE_OPS), + 1: the drop_scale product of a masked forward
            want, bnd = _expect(dev, (fam, "fwd", shape, masked), exact, not out_f32, mm, act, wgt, n, act_keep=keep,
                                scale=2.0 if masked else 1.0, addend=R.bias_bcast(f["addend"]),
                                ops=R.EPILOGUE_OPS + (1 if masked else 0))
            kw.update(Cin=C, M=M, padL=padL, bias=bias, a_split=pk.fwd_s, out_c8=not out_f32,
                      drop_scale=2.0 if masked else 1.0)
            if var == "from_f32_keep_bits":
                words, rs = R.keep_bits_words(keep)
                args, kw2 = (_up(act, dev), pk.fwd, pk.lda, 0), dict(mode=ops.EPI_LINEAR, xmask=_up(words, dev), xmask_rs=rs)
            else:
                x8 = _to_c8(act, dev)
                kw2 = dict(x_c8=x8, mode=ops.EPI_LINEAR)
                if masked:
                    kw2["xmask_c8"] = _up(R.keep_bytes(keep), dev)
                if gated:
                    kw2.update(mode=ops.EPI_GLU if var == "glu" else ops.EPI_HIGHWAY, Cg=C,
                               r=x8 if var == "highway" else None)
                args = (None, pk.fwd, pk.lda, pk.a_half if gated else 0)
        else:
            keep = _keep((B, C, T), 17)
            has_r = var in ("ymask_r1", "ymask_r_rs2")
            r_scale = RS2 if var == "ymask_r_rs2" else 0.0          # 0 means 1 (include/dv3hip.h)
            r = None
            if has_r:
                r = _cached(("r", fam, shape), lambda: _addend_r(
                    dev, fam, shape, f, lambda: float(R.expect_bf16(mm, act, wgt, n, device=dev)[0].abs().mean()) + 2.0 ** -100))
            if exact and var == "ymask_r_rs2":
                continue                   # sqrt(.5) r is not a whole number of quanta: the bounded families carry this form
            # n products, + 1: the drop_scale product on the accumulator, + 2 with an addend: the product r_scale * r and the add
            want, bnd = _expect(dev, (fam, "dgrad", shape, var if has_r else "ymask"), exact, not out_f32, mm, act, wgt, n,
                                out_keep=keep, scale=2.0, ops=1 + (2 if has_r else 0),
                                addend=None if r is None else (RS2 if r_scale else 1.0) * r.astype(np.float64))
            kw.update(Cin=M, M=C, padL=(k - 1) * d - padL, a_split=pk.bwd_s, out_c8=not out_f32, drop_scale=2.0,
                      mode=ops.EPI_DGRAD)
            kw2 = dict(x_c8=_to_c8(act, dev))
            if out_f32:
                words, rs = R.keep_bits_words(keep)
                kw2.update(ymask=_up(words, dev), ymask_rs=rs)
            else:
                kw2.update(ymask_c8=_up(R.keep_bytes(keep), dev), r=None if r is None else _to_c8(r, dev), r_scale=r_scale)
            args = (None, pk.bwd, pk.ldb, 0)
        outs = []
        with _switches(switches):
            for _ in range(2):
                ab = ops._c8_empty(B, M, T, dev) if gated else None
                y = ops.conv_gemm(*args, ab=ab, **kw, **kw2)
                census = L.dv3_debug_get(10)
                outs.append(ab if gated else y)
        what = "%s c8 %s %s %s %s" % (gemm, var, form, fam, shape)
        if var == "from_f32_keep_bits":
            assert census // 1000 == 4, (what, census)
        else:
            assert _c8_census_ok(census, want_census), (what, census)
        seen[var] = census
        _same_bits(outs[0], outs[1], what)
        Cout = M if gemm == "fwd" else C
        got = outs[0].double() if out_f32 else _from_c8(outs[0], Cout, what)
        worst = max(worst, _note("%s %s, %s out" % (gemm, var, "fp32" if out_f32 else "c8"),
                                 R.check_prepared(exact, got, want, bnd, what)))
    return worst, seen


@pytest.mark.parametrize("fam", FAMILIES)
@pytest.mark.parametrize("form", list(C8_FORMS))
def test_c8_tap_gemm_elementwise(dev, bf16_mode, form, fam):
    ops, L = bf16_mode
    ops.bf16_storage = True
    worst = 0.0
    for shape in R.C8_SHAPES:
        r, _ = _run_conv_c8(dev, form, fam, shape)
        worst = max(worst, r)
    _report("conv bf16 c8 %s %s (%d shapes)" % (form, fam, len(R.C8_SHAPES)), worst)


def _n_cu(dev):
    ops, L = _lib()
    name = ctypes.create_string_buffer(256)
    n = ctypes.c_int(0)
    assert L.dv3_device_info(dev.index or 0, name, 256, ctypes.byref(n)) == 0
    return n.value


@pytest.mark.parametrize("fam", ["E1", "B1"])
def test_c8_planes_workgroup_walks_two_tiles(dev, bf16_mode, fam):
    """conv_planes is persistent: its grid is min(tiles, n_cu x workgroups per CU) (csrc/conv_planes.hip: two co-resident
    workgroups for the 4-wave tiles 1 and 2, one for the 8-wave tile 9), and a workgroup that walks a second tile prefetches
    it before the first one's epilogue.  The smallest shape of three batch items and two 128-row tiles at which that
    happens for every forced tile: 2 ceil(3 T / 256) > n_cu binds (tile 9); 10923 frames on 256 CUs."""
    ops, L = bf16_mode
    ops.bf16_storage = True
    n_cu = _n_cu(dev)
    B, C, k, d = 3, 128, 3, 3
    T = (n_cu // 2 * 256) // B + 1
    shape = (B, C, T, k, d, False)
    M = 2 * C
    for tile, bn, per_cu in ((1, 128, 2), (2, 64, 2), (9, 256, 1)):
        tiles = -(-M // 128) * -(-(B * T) // bn)          # the dispatcher's grid formula, linear and input-gradient forms alike
        assert tiles > n_cu * per_cu, (tile, tiles, n_cu)
    assert 2 * -(-(B * (T - 1)) // 256) <= n_cu, "one frame fewer would leave tile 9 with one tile per workgroup"
    worst = 0.0
    for form in ("planes1", "planes2", "planes9"):
        r, seen = _run_conv_c8(dev, form, fam, shape, variants=("linear", "keep_bytes", "ymask_r1"))
        assert len(seen) == 3
        worst = max(worst, r)
    for key in [k_ for k_ in _cache if shape in k_]:        # 8 M elements per tensor: not kept for the module
        del _cache[key]
    _report("conv bf16 c8 planes, two tiles per workgroup %s %s" % (fam, shape), worst)
    torch.cuda.empty_cache()


# ---------------------------------------------------------------------------------------------------------------
# c8 storage: weight gradient (wgrad_c8)
# ---------------------------------------------------------------------------------------------------------------
def _run_wgrad_c8(dev, form, fam, shape):
    ops, L = _lib()
    B, C, T, k, d, padL, M = _dims(shape)
    switches, base, il = WGRAD_C8_FORMS[form]
    exact = fam[0] == "E"
    f, act, wgt = _operands(dev, fam, "wgrad", shape, True)
    g8, x8 = _to_c8(act, dev), _to_c8(wgt, dev)
    chunks = B * ((T + 31) // 32)
    worst = 0.0
    with _switches(switches):
        for masked in (False, True):
            keep = _keep((B, C, T), 19) if masked else None
            kb = _up(R.keep_bytes(keep), dev) if masked else None
            for S in (1, 3, 7, chunks + 2):
                def make(S=S, keep=keep):
                    own = R.c8_slabs(B, T, S)
                    # n: the frames of the largest slab, + 1: the drop_scale product of a masked launch
                    n = R.c8_slab_frames(B, T, S)
                    pairs = [R.prepare_bf16(exact, *R.expect_bf16(
                        R.make_mm("wgrad", d, padL, k), act, wgt, n, act_keep=own[s][:, None, :], wgt_keep=keep,
                        scale=2.0 if keep is not None else 1.0, ops=1 if keep is not None else 0, device=dev)) for s in range(S)]
                    want = torch.stack([p[0] for p in pairs])
                    return want, (None if exact else torch.stack([p[1] for p in pairs]))
                want, bnd = _cached(("expect", fam, "wgrad_c8", shape, S, masked), make)
                for rows in (False, True):
                    outs = []
                    for _ in range(2):
                        o = ops.wgrad_gemm_c8(g8, x8, B=B, M=M, Cin=C, T=T, J=k, dil=d, padL=padL, n_slabs=S, xmask_c8=kb,
                                              drop_scale=2.0 if masked else 1.0, rows_of_slabs=rows)
                        census = L.dv3_debug_get(11)
                        outs.append(o)
                    what = "wgrad_c8 %s %s %s S=%d masked=%d rows_of_slabs=%d" % (form, fam, shape, S, masked, rows)
                    assert census == base + k + (il if k == 3 else 0), (what, census)
                    _same_bits(outs[0], outs[1], what)
                    got = outs[0].permute(2, 0, 1, 3) if rows else outs[0]        # [J][M][S][C] -> [S][J][M][C]
                    if S > chunks:
                        assert not bool(got[chunks:].any()), what + ": an empty slab is not zero"
                    # every slab against its own frames' GEMM: nothing is summed away
                    worst = max(worst, R.check_prepared(exact, got, want, bnd, what))
    return worst


@pytest.mark.parametrize("fam", FAMILIES)
@pytest.mark.parametrize("form", list(WGRAD_C8_FORMS))
def test_wgrad_c8_elementwise(dev, bf16_mode, form, fam):
    ops, L = bf16_mode
    ops.bf16_storage = True
    worst = 0.0
    for shape in R.C8_SHAPES:
        worst = max(worst, _run_wgrad_c8(dev, form, fam, shape))
    _report("wgrad bf16 c8 %s %s (%d shapes)" % (form, fam, len(R.C8_SHAPES)), worst)

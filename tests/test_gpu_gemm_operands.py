# coding: utf-8
"""-m gpu: the split-operand GEMMs, element by element, across operand magnitudes (tests/gemm_split_ref.py).

Raw GEMM level: ops.conv_gemm in its linear form, its input-gradient form and the gated form read through its saved
pre-gate pair (linear in x), and ops.wgrad_gemm with the slabs added in float64 on the host -- plain weights
(ops.pack_weights(w, None, ...)), so no weight norm stands between the data and the operand.  Modes f16x3 / bf16x3 / f32.

EXACT families (E1 .. E4): operands are small integers times a power of two, every product and partial sum is exactly
representable, the order of summation cannot matter: torch.equal against the three-term value in float64, every element.
E2 sits in fp16's subnormal and lowest normal binades -- a flush anywhere gives zeros where integers belong; E4 has both
planes live with at most 8 terms per dot product.  BOUNDED families (B1 .. B5): |kernel - float64| <= bound element by
element, the bound derived in gemm_split_ref.py from the header's per-operand statements plus the order-independent fp32
accumulation worst case; nothing here is tuned to what the kernels return.  tests/test_cpu_gemm_split_ref.py shows that a
kernel with flushed fp16 subnormals or one lost lo plane fails these checks.

Every case names a kernel form and asserts, from the launch census (dv3_debug_get(10 / 11)), that it ran that form; a
forced form that is not eligible for a shape is passed over for that shape (and the test skips when no shape took it),
the automatic form never is.  A second identical call must return the same bits.  The stream-K form of the 256 x 256
kernel has shapes of its own (gemm_split_ref.STREAMK_SHAPES: none of the edge shapes has the 2 units per CU it needs), on
which every family runs forward, gated and as input gradient with the form asserted; the benchmarked layer reaches it by
the dispatcher's own rule.
"""
import contextlib
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tests import gemm_split_ref as R  # noqa: E402
from tests.util import assert_close_elementwise  # noqa: E402
from oracle import dv3_oracle as O  # noqa: E402

pytestmark = pytest.mark.gpu

MODES = ("f16x3", "bf16x3", "f32")
FAMILIES = R.EXACT + R.BOUNDED
# form -> (tile_hint, {library switch (include/dv3hip.h, DV3_SWITCHES): value}, ops.streamk)
SPLIT_FORMS = dict([("auto", (0, {}, None))] + [("tile%d" % t, (t, {}, None)) for t in range(21, 30)] +
                   [("pp2", (30, {}, None)), ("pp2_streamk", (30, {"DV3_SW_PP2_SK": 2}, "force")),
                    ("ksplit", (22, {"DV3_SW_X3_KS": 2}, None))])
F32_FORMS = dict([("auto", (0, {}, None))] + [("tile%d" % t, (t, {}, None)) for t in (1, 2, 3, 4, 5, 6, 11, 12, 13, 14, 15, 16)])
CONV_CASES = [(m, f) for m in MODES for f in (F32_FORMS if m == "f32" else SPLIT_FORMS)]
# weight gradient: form -> (split_bf16, k_split, g_pair, masked, switches)
WGRAD_SPLIT_FORMS = {"auto": None, "split_bf16": (True, False, False, False, {}), "k_split": (True, True, False, False, {}),
                     "k_split_masked": (True, True, False, True, {}), "all_taps": (True, True, False, False, {"DV3_SW_WGRAD_TILE": 3}),
                     "two_steps_ahead_per_tap": (True, True, False, False, {"DV3_SW_WGRAD_TILE": 4, "DV3_SW_WGRAD_T2_WINDOW": 0}),
                     "g_pair": (True, True, True, False, {})}
WGRAD_F32_FORMS = {"auto": None, "slabs_masked": (False, False, False, True, {})}
WGRAD_CASES = [(m, f) for m in MODES for f in (WGRAD_F32_FORMS if m == "f32" else WGRAD_SPLIT_FORMS)]


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


@pytest.fixture(scope="module", autouse=True)
def _release_cache():
    yield
    _cache.clear()
    if torch.cuda.is_available():
        torch.cuda.empty_cache()


def _expectation(dev, fam, gemm, mode, shape, keep=None, want_three=True, n_slabs=1, k_split=False):
    """operands on the device and what the kernel must return: (f, act, wgt, bias, want | None, ref, bound), cached for
    the forms that share them.  gemm: "fwd" (also the gated form), "dgrad", "wgrad"; keep: dropout keep mask of the
    weight gradient's x, applied with 1 / (1 - p) = 2 (exact in fp32, so the operand is the same fp32 value on both sides)"""
    key = (fam, gemm, R.forms(gemm, mode), shape, keep is not None, n_slabs, k_split)
    if key in _cache:
        return _cache[key]
    B, C, T, k, d, causal = shape
    padL = R.pad_left(k, d, causal)
    f = R.family(fam, gemm, mode, shape)
    fa, fw = R.forms(gemm, mode)
    mm = R.make_mm(gemm, d, padL, k)
    n = R.n_products(gemm, mode, J=k, K=(C if gemm == "fwd" else 2 * C), B=B, T=T, n_slabs=n_slabs, k_split=k_split)
    bias = R.bias_bcast(f["addend"])
    wgt = f["wgt"] if keep is None else (f["wgt"] * keep.astype(np.float32) * np.float32(2.0))
    ref = R.reference(mm, f["act"], wgt, bias, device=dev)
    bnd = R.bound(mm, f["act"], wgt, fa, fw, n, bias, device=dev)[0]
    want = R.three_term(mm, f["act"], wgt, fa, fw, bias, device=dev) if (fam in R.EXACT and want_three) else None
    out = (f, torch.from_numpy(f["act"]).to(dev), torch.from_numpy(f["wgt"]).to(dev),
           None if f["addend"] is None else torch.from_numpy(f["addend"]).to(dev), want, ref, bnd)
    if B < 64:
        _cache[key] = out
    return out


def _check(fam, got, want, ref, bnd, what):
    """exact families: every element equals the three-term value; bounded families: every element inside its bound"""
    assert torch.isfinite(got).all(), what
    if fam in R.EXACT:
        g64 = got.double()
        if not torch.equal(g64, want):
            bad = (g64 != want)
            i = tuple(int(v) for v in bad.nonzero()[0])
            raise AssertionError("%s: %d of %d elements differ; first at %s: got %r want %r" %
                                 (what, int(bad.sum()), bad.numel(), i, float(g64[i]), float(want[i])))
        if fam != "E4":
            return 0.0
    if got.numel() > (1 << 21):       # the B = 64 shapes: decide on the device, fetch the tensors only to report a failure
        err = (got.double() - ref).abs()
        if bool((err <= bnd).all()):
            return float(torch.where(err == 0, torch.zeros_like(err), err / bnd).max())
    return assert_close_elementwise(got, ref, 0, bnd, what)


@contextlib.contextmanager
def _form(switches, streamk=None):
    """a form's library switches (_lib.switches puts back what was there) and, for the stream-K forms, ops.streamk"""
    from deepvoice3_pytorch_amd import ops, _lib as LIB
    prev_sk = ops.streamk
    if streamk is not None:
        ops.streamk = streamk
    try:
        with LIB.switches(switches):
            yield
    finally:
        ops.streamk = prev_sk


def _conv_reached(mode, gemm, form, census, Kin):
    """did the launch run the form the case names?  (census: csrc/conv_gemm.hip, conv_gemm_bf16x3.hip, conv_gemm_pp2.hip)"""
    if mode == "f32":
        if form == "auto":
            return census // 1000 == 1
        t = int(form[4:])
        return census == (2000 + (t - 10) * 10 if t > 10 else 1000 + t * 10)
    fam_ = 5 if (mode == "f16x3" and gemm != "dgrad") else 3          # scaled fp16 pairs / bf16 pairs
    if census // 1000 != fam_:
        return False
    if form == "auto":
        return True
    if form == "pp2":
        return census % 1000 == 101
    if form == "pp2_streamk":
        return census % 1000 == 102
    if form == "ksplit":                # the rule restated: at least two 32-channel chunks to share between the groups
        assert (census % 10 == 2) == ((Kin + 31) // 32 >= 2) and census % 1000 // 10 == 2, census
        return census % 10 == 2
    return census % 1000 // 10 == int(form[4:]) - 20 and census % 1000 < 100


def _run_conv(dev, gemm, mode, form, fam, shape, want_three=True):
    """-> worst ratio, or None when the forced form is not eligible for the shape"""
    ops, L = _lib()
    B, C, T, k, d, causal = shape
    M, padL = 2 * C, R.pad_left(k, d, causal)
    data_gemm = "dgrad" if gemm == "dgrad" else "fwd"
    f, act, w, bias, want, ref, bnd = _expectation(dev, fam, data_gemm, mode, shape, want_three=want_three)
    hint, switches, sk = (F32_FORMS if mode == "f32" else SPLIT_FORMS)[form]
    pk = ops.pack_weights(w, None, glu_cg=C if gemm == "gated" else 0, need_bwd=(gemm == "dgrad"))
    # the counter is read around the LAUNCHES: packing also builds the forward's fp16 image, which the bf16-range weights
    # of the input gradient's E3 leave on purpose (that image is not used here)
    packed = ops.f16_range_events(reset=True)
    assert packed == 0 or (gemm == "dgrad" and fam == "E3"), "%d units counted while packing in-range weights" % packed
    outs = []
    with _form(switches, sk):
        for _ in range(2):
            try:
                if gemm == "dgrad":
                    y = ops.conv_gemm(act, pk.bwd, pk.ldb, 0, B=B, Cin=M, Tin=T, M=C, Tout=T, J=k, dil=d,
                                      padL=(k - 1) * d - padL, mode=ops.EPI_DGRAD, a_split=pk.bwd_s, tile_hint=hint)
                elif gemm == "gated":
                    y = torch.empty(B, M, T, device=dev)
                    ops.conv_gemm(act, pk.fwd, pk.lda, pk.a_half, B=B, Cin=C, Tin=T, M=M, Tout=T, J=k, dil=d, padL=padL,
                                  mode=ops.EPI_GLU, Cg=C, bias=bias, ab=y, a_split=pk.fwd_s, tile_hint=hint)
                else:
                    y = ops.conv_gemm(act, pk.fwd, pk.lda, 0, B=B, Cin=C, Tin=T, M=M, Tout=T, J=k, dil=d, padL=padL,
                                      mode=ops.EPI_LINEAR, bias=bias, a_split=pk.fwd_s, tile_hint=hint)
            except RuntimeError as e:
                assert form != "auto" and ("needs split-bf16" in str(e) or "LDS tile" in str(e)), (form, shape, str(e))
                return None
            census = L.dv3_debug_get(10)
            if not _conv_reached(mode, gemm, form, census, M if gemm == "dgrad" else C):
                assert form in ("ksplit", "pp2_streamk"), "%s %s %s %s: census %d" % (gemm, mode, form, shape, census)
                return None
            outs.append(y)
    what = "%s %s %s %s %s" % (gemm, mode, form, fam, shape)
    assert torch.equal(outs[0].view(torch.int32), outs[1].view(torch.int32)), what + ": a second call differs"
    return _check(fam, outs[0], want, ref, bnd, what)


@pytest.mark.parametrize("fam", FAMILIES)
@pytest.mark.parametrize("mode,form", CONV_CASES)
@pytest.mark.parametrize("gemm", ["fwd", "gated", "dgrad"])
def test_tap_gemm_elementwise(dev, gemm, mode, form, fam):
    ops, L = _lib()
    prev = ops.set_gemm_precision(mode)
    try:
        ops.f16_range_events(reset=True)
        worst, ran = 0.0, 0
        shapes = R.STREAMK_SHAPES if form == "pp2_streamk" else R.EDGE_SHAPES
        for shape in shapes:
            r = _run_conv(dev, gemm, mode, form, fam, shape)
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
    _report("%s %s %s %s (%d shapes)" % (gemm, mode, form, fam, ran), worst)


def _run_wgrad(dev, mode, form, fam, shape):
    ops, L = _lib()
    B, C, T, k, d, causal = shape
    M, padL = 2 * C, R.pad_left(k, d, causal)
    small = M <= 64 and C <= 64           # dv3_wgrad_gemm_f32: such layers run the exact fp32 kernel in every mode
    eff_mode = "f32" if small else mode
    spec = (WGRAD_F32_FORMS if mode == "f32" else WGRAD_SPLIT_FORMS)[form]
    if spec is None:                      # the choice of ops.ConvLayerFn.backward
        x3, S = ops.wgrad_plan(B, M, C, T, k)
        assert x3 == (eff_mode != "f32")
        split, ksplit, g_pair, masked, switches = x3, x3, False, False, {}
    else:
        split, ksplit, g_pair, masked, switches = spec
        if split and small:
            return None                   # the split forms do not serve these layers
        S = 3 if ksplit else min(B, 2)
    keep = bits = None
    rs = 0
    if masked:
        ops.dropout_state.manual_seed(5)
        bits, rs = ops.dropout_bits(B * C, T, 0.5, dev)
        keep = O.unpack_keep_bits(bits.cpu().numpy().view(np.uint32), B * C, rs, T).reshape(B, C, T)
    f, g, x, _, want, ref, bnd = _expectation(dev, fam, "wgrad", eff_mode, shape, keep=keep, n_slabs=S, k_split=bool(ksplit))
    if g_pair:
        g = R.pair_words(f["act"]).to(dev)
    outs = []
    with _form(switches):
        for _ in range(2):
            o = ops.wgrad_gemm(g, x, B=B, M=M, Cin=C, T=T, Tin=T, J=k, dil=d, padL=padL, n_slabs=S, xmask=bits,
                               xmask_rs=rs, drop_scale=2.0 if masked else 1.0, split_bf16=split, k_split=ksplit,
                               g_pair=g_pair)
            census = L.dv3_debug_get(11)
            outs.append(o)
    # the form the case names (csrc/wgrad_gemm.hip, wgrad_gemm_bf16x3.hip, wgrad_taps2.hip)
    taps2 = k == 3 and (B - 1) * M * T + (M - 1) * T + T >= 8 and (B - 1) * C * T + (C - 1) * T + T >= 8
    if not split:
        expect = (1000, 1010)[not small]
        assert census == expect, (form, shape, census)
    elif form == "split_bf16" or k != 3:
        assert census == 3010, (form, shape, census)
    elif form == "all_taps":
        assert census == 3030, (form, shape, census)
    elif form == "two_steps_ahead_per_tap":
        assert census == (3040 if taps2 else 3010), (form, shape, census)
    else:
        assert census // 10 == (304 if taps2 else 301) and (census % 2 == 1) == (g_pair and taps2), (form, shape, census)
    what = "wgrad %s %s %s %s" % (mode, form, fam, shape)
    assert torch.equal(outs[0].view(torch.int32), outs[1].view(torch.int32)), what + ": a second call differs"
    assert torch.isfinite(outs[0]).all(), what
    got = outs[0].double().sum(0)         # [S][J][M][C] -> (J, M, C): the slabs added in float64
    if fam in R.EXACT:
        if not torch.equal(got, want):
            bad = got != want
            i = tuple(int(v) for v in bad.nonzero()[0])
            raise AssertionError("%s: %d of %d elements differ; first at %s: got %r want %r" %
                                 (what, int(bad.sum()), bad.numel(), i, float(got[i]), float(want[i])))
        if fam != "E4":
            return 0.0
    return assert_close_elementwise(got, ref, 0, bnd, what)


@pytest.mark.parametrize("fam", FAMILIES)
@pytest.mark.parametrize("mode,form", WGRAD_CASES)
def test_wgrad_gemm_elementwise(dev, mode, form, fam):
    ops, L = _lib()
    prev = ops.set_gemm_precision(mode)
    try:
        worst, ran = 0.0, 0
        for shape in R.EDGE_SHAPES:
            r = _run_wgrad(dev, mode, form, fam, shape)
            if r is not None:
                worst, ran = max(worst, r), ran + 1
    finally:
        ops.set_gemm_precision(prev)
    assert ran > 0
    _report("wgrad %s %s %s (%d shapes)" % (mode, form, fam, ran), worst)


# the benchmarked encoder layer (B = 64, C = 512, T = 150, k = 3), bounded families; the float64 references are matrix
# products on the GPU.  d = 1 in every mode; d = 27 in the default mode
@pytest.mark.parametrize("fam", R.BOUNDED)
@pytest.mark.parametrize("mode,shape", [(m, R.BENCH_SHAPES[0]) for m in MODES] + [("f16x3", R.BENCH_SHAPES[1])])
def test_benchmarked_layer_elementwise(dev, mode, shape, fam):
    ops, L = _lib()
    prev = ops.set_gemm_precision(mode)
    try:
        ops.f16_range_events(reset=True)
        for gemm in ("fwd", "gated", "dgrad"):
            r = _run_conv(dev, gemm, mode, "auto", fam, shape)
            census = L.dv3_debug_get(10)
            if mode != "f32" and gemm != "dgrad":
                # 152 tiles of 256 x 256 on 256 CUs: the automatic choice is that kernel, for the gated d = 1 forward in
                # its stream-K form (ops._streamk_ws; test_gpu_kernels.py asserts the same)
                assert census % 1000 in (101, 102), census
                if gemm == "gated" and shape[4] == 1:
                    assert census % 1000 == 102, census
            _report("%s %s auto %s %s [census %d]" % (gemm, mode, fam, shape, census), r)
            torch.cuda.empty_cache()
        r = _run_wgrad(dev, mode, "auto", fam, shape)
        _report("wgrad %s auto %s %s [census %d]" % (mode, fam, shape, L.dv3_debug_get(11)), r)
        assert ops.f16_range_events(reset=True) == 0
    finally:
        ops.set_gemm_precision(prev)
        torch.cuda.empty_cache()

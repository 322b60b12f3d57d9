# coding: utf-8
"""-m gpu: the MEMORY FOOTPRINT of the GEMM kernels -- guard bands, strided and offset views (tests/footprint_ref.py).

tests/test_gpu_gemm_operands.py, test_gpu_gemm_bf16.py, test_gpu_gate_tails.py and test_gpu_c8.py pin the VALUES of every
kernel form on dense, allocator-aligned tensors.  Here the same forms (the form tables are imported from those files, the
census rules too) run with every operand the ABI gives strides for inside a larger buffer the test owns:

  inputs   x, r, r2 (tap-GEMM), g, x (weight gradient): the values in a view, POISON (the quiet NaN 0x7fc0dead) in the
           bands before and after it and in every row / batch gap.  A load outside the tensor that reaches arithmetic
           -- multiplied by a zero weight or a zero mask instead of selected -- turns the output NaN.
  outputs  y, the slabs: a view in a buffer full of the same word as GUARD.  A store outside the logical output changes
           a guard word; footprint_ref.violations names the band or gap, the nearest logical element and the distance.
  dense-only operands (ab, pg, dpg, dpg_res, pg_part, the masks, every c8 tensor) take the `banded` placement only.

Placements (footprint_ref.PLACEMENTS): banded, strided4 (rs % 4 == 0), strided1 (rs % 4 == 1, bs % 4 != 0), offset1 .. 3
(the base 1 .. 3 floats past a 16-byte boundary).  At Tout % 4 == 0 (T = 200) the first two are eligible for the 16-byte
epilogues of csrc/conv_common.h (dv3_wide_epilogue_ok, dv3_wide_glu_ok), the other four must take the narrow ones: the
predicates' pointer & 15, rs & 3 and bs & 3 terms, which dense allocator-aligned tensors never exercise.

For each launch: (1) the census shows the named form; eligibility is decided on the dense launch exactly as the
neighbouring files do and NO PLACEMENT MAY CHANGE IT -- the dispatchers' rules (csrc/conv_gemm.hip, conv_gemm_bf16x3.hip,
conv_gemm_pp2.hip: a_bs == 0, lda % 4 == 0, Tin == Tout, (J - 1) dil <= 64, sizes below 2^30, LDS) hold no alignment
or stride term for x, r, r2, y; the one rule that reads strides, the two-steps-ahead weight gradient's
(B - 1) bs + (rows - 1) rs + T >= 8 of csrc/wgrad_gemm_bf16x3.hip, is restated with the placed strides; (2) no guard
word of any output buffer changed; (3) no sentinel and no NaN in the logical output; (4) the values: family E1 equals
the float64 three-term value in every element, B1 lies inside gemm_split_ref.bound / expect_bf16, unchanged; (5) the
logical output is bit-identical to the same form's launch on dense tensors (conv_common.h: the 16-byte and the narrow
epilogues perform the "same operations per element"; csrc/wgrad_taps2.hip says the same of its re-aligned ends).
One output is exempt from (5): pg_part, the bias partial sums of the fused gate backward, whose 16-byte tail adds a
block's 32 columns in another order than the narrow one (conv_common.h says so; _part_check holds it to its value).

The non-gated forward fills BOTH residual slots.  Its value check is a composition: y0, the launch without residuals, is
held to the float64 reference as above; the launch with r and r2 must equal fp32(fp32(fp32(y0 + r) s + r2) s),
s = fp32(sqrt(.5)), bit for bit -- the two roundings per slot the header's formula states, evaluated in torch fp32.
The input gradient carries its addend r in the reference itself (three_term / bound take an addend).

Every case prints a worst-ratio line and `footprint <case>: N launches, 0 violations`.
"""
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tests import gemm_split_ref as R  # noqa: E402
from tests import footprint_ref as FP  # noqa: E402
from tests import test_gpu_gemm_operands as GO  # noqa: E402
from tests import test_gpu_gemm_bf16 as GB  # noqa: E402

pytestmark = pytest.mark.gpu

FAMILIES = ("E1", "B1")
RS2 = float(np.float32(0.70710678118654752440))
# (mode, form) of the tap-GEMM: the three fp32-storage modes of test_gpu_gemm_operands.py and the single-term mode's tiles
CONV_CASES = GO.CONV_CASES + [("bf16", f) for f in GB.CONV_FORMS]
WGRAD_CASES = GO.WGRAD_CASES + [("bf16", f) for f in GB.WGRAD_FORMS]
GATE_TILES = ("auto", "tile21", "tile22", "tile28", "tile29")    # conv_gemm_bf16x3.hip: the fused gate backward's four tiles


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


_cache = {}
_outs = {}


@pytest.fixture(scope="module", autouse=True)
def _release_cache():
    yield
    _cache.clear()
    _outs.clear()
    GO._cache.clear()
    GB._cache.clear()
    if torch.cuda.is_available():
        torch.cuda.empty_cache()


def _cached(key, make):
    if key not in _cache:
        _cache[key] = make()
    return _cache[key]


def _report(what, ratio, launches):
    print("worst-ratio %-72s %.4g" % (what, ratio))
    print("footprint %s: %d launches, 0 violations" % (what, launches))


def _bits(t):
    return t.contiguous().view(torch.int16 if t.dtype == torch.bfloat16 else torch.int32)


def _placed(dev, key, arr, pl):
    """an input under a placement, cached (inputs are only read; _inputs_intact checks that they were)"""
    return _cached(("in", key, pl), lambda: FP.place(arr, pl, dev))


def _out(dev, shape, pl, tag=""):
    """an output buffer under a placement, every word the sentinel again"""
    key = (tuple(shape), pl, tag)
    if key not in _outs:
        _outs[key] = FP.place(tuple(shape), pl, dev)
    buf, view = _outs[key]
    buf.view(torch.int32).fill_(FP.SENTINEL)
    return buf, view


def _out_slabs(dev, S, J, M, C, pl, rows):
    key = ("slabs", S, J, M, C, pl, rows)
    if key not in _outs:
        _outs[key] = FP.place_slabs(S, J, M, C, pl, dev, rows)
    buf, view, ldo = _outs[key]
    buf.view(torch.int32).fill_(FP.SENTINEL)
    return buf, view, ldo


def _clean(what, **bufs):
    """checks 2 and 3 for the outputs of one launch: name -> (buf, view)"""
    for name, (buf, view) in bufs.items():
        v = FP.violations(buf)
        assert not v, "%s: %s: %s" % (what, name, FP.describe(v))
        n = FP.unwritten(view)
        assert n == 0, "%s: %s: %d logical words were never stored" % (what, name, n)
        assert not FP.poisoned(view), "%s: %s: a NaN reached the logical output" % (what, name)


def _inputs_intact(what):
    for key, val in list(_cache.items()):
        if isinstance(key, tuple) and key and key[0] == "in":
            v = FP.violations(val[0])
            assert not v, "%s: an INPUT buffer was written: %s" % (what, FP.describe(v))


def _residual(shape3, seed, quantum):
    """small whole multiples of the family's quantum (E1: 1), so that acc + r stays exact"""
    return (np.random.RandomState(seed).randint(-15, 16, size=shape3) * (quantum or 2.0 ** -3)).astype(np.float32)


def _expect(dev, fam, data, mode, shape, addend_key, addend, wgt=None, n_slabs=1, k_split=False, wkey=None):
    """(want | None, ref, bound) of gemm_split_ref, unchanged: the float64 reference of the operands (rounded as the mode's
    kernels round them), the three-term value for the exact families, the derived bound"""
    def make():
        B, C, T, k, d, causal = shape
        padL = R.pad_left(k, d, causal)
        f = R.family(fam, data, mode, shape)
        fa, fw = R.forms(data, mode)
        mm = R.make_mm(data, d, padL, k)
        n = R.n_products(data, mode, J=k, K=(C if data == "fwd" else 2 * C), B=B, T=T, n_slabs=n_slabs, k_split=k_split)
        w_ = f["wgt"] if wgt is None else wgt
        ref = R.reference(mm, f["act"], w_, addend, device=dev, form_a=fa, form_w=fw)
        bnd = R.bound(mm, f["act"], w_, fa, fw, n, addend, device=dev)[0]
        want = R.three_term(mm, f["act"], w_, fa, fw, addend, device=dev) if fam in R.EXACT else None
        return want, ref, bnd
    return _cached(("expect", fam, data, R.forms(data, mode), mode == "f32", shape, addend_key, wkey, n_slabs, k_split), make)


def _check(fam, got, exp, what):
    want, ref, bnd = exp
    exact = fam in R.EXACT
    return R.check_prepared(exact, got, want if exact else ref, bnd, what)


# ---------------------------------------------------------------------------------------------------------------
# tap-GEMM: forward, gated forward, input gradient
# ---------------------------------------------------------------------------------------------------------------
def _conv_form(mode, form):
    """-> (tile_hint, switches, ops.streamk)"""
    if mode == "bf16":
        return GB.CONV_FORMS[form], {}, None
    return (GO.F32_FORMS if mode == "f32" else GO.SPLIT_FORMS)[form]


def _reached(mode, gemm, form, census, Kin):
    if mode == "bf16":          # test_gpu_gemm_bf16.py: family 4, the tile id
        assert census // 1000 == 4, (form, gemm, census)
        return form == "auto" or census % 1000 // 10 == GB.CONV_FORMS[form] - 20
    return GO._conv_reached(mode, gemm, form, census, Kin)


def _sk_ws_zero(ops, dev, what):
    """include/dv3hip.h, dv3_conv_desc.sk_ws: the launches leave the first 4 KiB of the workspace zero"""
    e = ops._sk_ws.get((dev.index, ops._stream()))
    assert e is not None, what + ": no stream-K workspace was handed to the launch"
    assert not bool(e[2][:1024].any()), what + ": the stream-K workspace's first 4 KiB are not zero after the launch"


def _run_conv(dev, gemm, mode, form, fam, shape, placements=FP.PLACEMENTS, store_il2=False):
    """-> (worst ratio, launches), or None when the forced form is not eligible for the shape (decided on the dense launch)"""
    ops, L = GO._lib()
    B, C, T, k, d, causal = shape
    M, padL = 2 * C, R.pad_left(k, d, causal)
    data = "dgrad" if gemm == "dgrad" else "fwd"
    hint, switches, sk = _conv_form(mode, form)
    f = R.family(fam, data, mode, shape)
    x_np, w = f["act"], torch.from_numpy(f["wgt"]).to(dev)
    bias = None if f["addend"] is None else torch.from_numpy(f["addend"]).to(dev)
    pk = _cached(("pk", fam, data, mode, shape, gemm == "gated"),
                 lambda: ops.pack_weights(w, None, glu_cg=C if gemm == "gated" else 0, need_bwd=(gemm == "dgrad")))
    ops.f16_range_events(reset=True)
    q = f["quantum"]
    what0 = "%s %s %s %s %s" % (gemm, mode, form, fam, shape)
    ikey = (fam, gemm, R.forms(data, mode), mode == "f32", shape)

    if gemm == "dgrad":
        r_np = _residual((B, C, T), 31 + C + T, q)
        exp = _expect(dev, fam, data, mode, shape, "r", r_np)
        y_shape = (B, C, T)
    elif gemm == "gated":
        r_np = _residual((B, C, T), 37 + C + T, q)
        exp = _expect(dev, fam, data, mode, shape, "bias", R.bias_bcast(f["addend"]))
        y_shape = (B, C, T)
    else:
        r_np, r2_np = _residual((B, M, T), 41 + C + T, q), _residual((B, M, T), 43 + C + T, q)
        y_shape = (B, M // 2, 2 * T) if store_il2 else (B, M, T)
        if store_il2:       # row m -> channel m mod C, column 2 t + m // C; bias[m mod C] (include/dv3hip.h, test_gpu_gate_tails.py)
            r_np = r2_np = None
            b2 = np.concatenate([f["addend"][:C], f["addend"][:C]]).reshape(1, -1, 1)
            exp = _expect(dev, fam, data, mode, shape, "bias_il2", b2)
        else:
            exp = _expect(dev, fam, data, mode, shape, "bias", R.bias_bcast(f["addend"]))

    def launch(pl, with_r=True):
        """one launch with x, r, r2 and y under placement `pl` (None: dense tensors from the allocator)
        -> (y view, {name: (buf, view)} of the placed outputs, ab)"""
        def put(name, arr):
            if arr is None:
                return None
            if pl is None:
                return _cached(("dense", ikey, name), lambda: torch.from_numpy(arr).to(dev))
            return _placed(dev, ikey + (name,), arr, pl)[1]
        x = put("x", x_np)
        bufs = {}
        if pl is None:
            y = torch.full(y_shape, float("nan"), device=dev)
        else:
            bufs["y"] = _out(dev, y_shape, pl)
            y = bufs["y"][1]
        ab = None
        if gemm == "dgrad":
            ops.conv_gemm(x, pk.bwd, pk.ldb, 0, B=B, Cin=M, Tin=T, M=C, Tout=T, J=k, dil=d, padL=(k - 1) * d - padL,
                          mode=ops.EPI_DGRAD, a_split=pk.bwd_s, tile_hint=hint, r=put("r", r_np), y=y)
        elif gemm == "gated":
            bufs["ab"] = _out(dev, (B, M, T), "banded", "ab")
            ab = bufs["ab"][1]
            ops.conv_gemm(x, pk.fwd, pk.lda, pk.a_half, B=B, Cin=C, Tin=T, M=M, Tout=T, J=k, dil=d, padL=padL,
                          mode=ops.EPI_GLU, Cg=C, bias=bias, ab=ab, a_split=pk.fwd_s, tile_hint=hint, residual=1,
                          r=put("r", r_np), y=y)
        else:
            ops.conv_gemm(x, pk.fwd, pk.lda, 0, B=B, Cin=C, Tin=T, M=M, Tout=T, J=k, dil=d, padL=padL,
                          mode=ops.EPI_LINEAR, bias=bias, a_split=pk.fwd_s, tile_hint=hint, y=y,
                          r=put("r", r_np) if with_r else None, r2=put("r2", r2_np) if with_r else None,
                          store_mode=ops.STORE_INTERLEAVE2 if store_il2 else ops.STORE_BCT)
        return y, bufs, ab

    worst, launches = 0.0, 0
    with GO._form(switches, sk):
        # the dense launch decides eligibility, as in test_gpu_gemm_operands.py / test_gpu_gemm_bf16.py
        try:
            yd, _, abd = launch(None)
        except RuntimeError as e:
            assert form != "auto" and ("needs split-bf16" in str(e) or "LDS tile" in str(e) or "not eligible" in str(e)), \
                (form, shape, str(e))
            return None
        census = L.dv3_debug_get(10)
        if not _reached(mode, gemm, form, census, M if gemm == "dgrad" else C):
            assert form in ("ksplit", "pp2_streamk"), "%s: census %d" % (what0, census)
            return None
        launches += 1
        if form == "pp2_streamk":
            _sk_ws_zero(ops, dev, what0 + " dense")
        if abd is not None:
            abd = abd.clone()
        # values of the dense launch
        if gemm == "fwd" and not store_il2:
            y0, _, _ = launch(None, with_r=False)
            assert L.dv3_debug_get(10) == census, what0
            launches += 1
            worst = max(worst, _check(fam, y0, exp, what0 + " dense, no residual"))
            s = torch.tensor(RS2, dtype=torch.float32, device=dev)
            r_d, r2_d = torch.from_numpy(r_np).to(dev), torch.from_numpy(r2_np).to(dev)
            tail = ((y0 + r_d) * s + r2_d) * s
            assert torch.equal(_bits(yd), _bits(tail)), what0 + ": (y0 + r) s + r2) s is not what the residual launch returns"
        elif gemm == "gated":
            worst = max(worst, _check(fam, abd, exp, what0 + " dense, pre-gate pair"))
            assert bool(torch.isfinite(yd).all()), what0
        else:
            got = yd
            if store_il2:
                got = torch.cat([yd[:, :, 0::2], yd[:, :, 1::2]], 1)
            worst = max(worst, _check(fam, got, exp, what0 + " dense"))
        for pl in placements:
            what = "%s [%s]" % (what0, pl)
            y, bufs, ab = launch(pl)      # a RuntimeError here = a placement changed eligibility: the dispatchers hold no such rule
            c2 = L.dv3_debug_get(10)
            assert c2 == census, "%s: census %d, dense %d: the placement changed the kernel form" % (what, c2, census)
            launches += 1
            _clean(what, **bufs)
            if form == "pp2_streamk":
                _sk_ws_zero(ops, dev, what)
            assert torch.equal(_bits(y), _bits(yd)), "%s: differs from the dense launch in %d elements" % (
                what, int((_bits(y) != _bits(yd)).sum()))
            if ab is not None:
                assert torch.equal(_bits(ab), _bits(abd)), what + ": the pre-gate pair differs from the dense launch"
                worst = max(worst, _check(fam, ab, exp, what + " pre-gate pair"))
            elif gemm == "dgrad":
                worst = max(worst, _check(fam, y, exp, what))
            elif store_il2:
                worst = max(worst, _check(fam, torch.cat([y[:, :, 0::2], y[:, :, 1::2]], 1), exp, what))
    events = ops.f16_range_events(reset=True)
    assert events == 0, "%s: operands inside the fp16 range were counted as outside (%d units)" % (what0, events)
    return worst, launches


@pytest.mark.parametrize("mode,form", CONV_CASES)
@pytest.mark.parametrize("gemm", ["fwd", "gated", "dgrad"])
def test_tap_gemm_footprint(dev, gemm, mode, form):
    ops, L = GO._lib()
    prev = ops.set_gemm_precision(mode)
    try:
        worst, ran, launches = 0.0, 0, 0
        shapes = R.STREAMK_SHAPES if form == "pp2_streamk" else R.EDGE_SHAPES
        for shape in shapes:
            for fam in FAMILIES:
                r = _run_conv(dev, gemm, mode, form, fam, shape)
                assert r is not None or form != "pp2_streamk", "the stream-K form did not take %s" % (shape,)
                if r is not None:
                    worst, ran, launches = max(worst, r[0]), ran + 1, launches + r[1]
        _inputs_intact("%s %s %s" % (gemm, mode, form))
    finally:
        ops.set_gemm_precision(prev)
        if form == "pp2_streamk":           # 20 MB tensors: not kept for the module
            _cache.clear()
            _outs.clear()
    if ran == 0:
        assert form != "auto"
        pytest.skip("%s is not eligible for any edge shape (its dispatcher's shape rules, not a placement)" % form)
    _report("%s %s %s (%d shape x family)" % (gemm, mode, form, ran), worst, launches)


@pytest.mark.parametrize("mode", GO.MODES)
def test_interleaved_store_footprint(dev, mode):
    """STORE_INTERLEAVE2 (the ConvTranspose1d k2 s2 store: row m -> channel m mod Mo, column 2 t + m / Mo) under every
    placement of y: rows of 2 T frames, each written by two accumulator rows"""
    ops, L = GO._lib()
    prev = ops.set_gemm_precision(mode)
    try:
        worst, launches = 0.0, 0
        for shape in R.EDGE_SHAPES:
            for fam in FAMILIES:
                r = _run_conv(dev, "fwd", mode, "auto", fam, shape, store_il2=True)
                assert r is not None
                worst, launches = max(worst, r[0]), launches + r[1]
        _inputs_intact("interleave2 " + mode)
    finally:
        ops.set_gemm_precision(prev)
    _report("interleave2 %s auto" % mode, worst, launches)


# ---------------------------------------------------------------------------------------------------------------
# the input gradient with the producer's gate backward in its tail (ops.GateFuse)
# ---------------------------------------------------------------------------------------------------------------
def _part_sums(dab, n_part):
    """float64 sums of the pre-gate gradient over the flat (b, t) columns [32 k, 32 k + 32) -> (sums, sums of magnitudes),
    each [2C][n_part] (include/dv3hip.h: pg_part)"""
    B, C2, T = dab.shape
    flat = dab.double().permute(1, 0, 2).reshape(C2, B * T)
    flat = torch.nn.functional.pad(flat, (0, n_part * 32 - B * T)).reshape(C2, n_part, 32)
    return flat.sum(2), flat.abs().sum(2)


def _part_check(part, psum, what):
    """pg_part is the one output whose SUMMATION ORDER depends on the epilogue form, hence on the placement: the narrow
    tail adds a block's 32 columns across lanes, the 16-byte tail "a sum over four frames + a butterfly over the eight lanes
    of a block" (csrc/conv_common.h, conv_epilogue_wide_block_gate; test_gpu_gate_tails.py compares the bias gradient "by
    the order of its partial sums only").  So it is held to its value, not to the dense launch's bits: 32 fp32 terms in any
    order, 31 additions rounded to nearest -- |part - sum| <= 31 * 2^-24 * sum |dab| (gemm_split_ref's accumulation
    term, first order)."""
    ref, mag = psum
    bnd = 31 * R.U32 * mag
    got = part.reshape(ref.shape).double()
    err = (got - ref).abs()
    assert bool((err <= bnd).all()), "%s: a bias partial sum leaves its bound: worst %g of it" % (
        what, float((err / bnd.clamp_min(1e-300)).max()))
    return float(torch.where(err == 0, torch.zeros_like(err), err / bnd.clamp_min(1e-300)).max())


@pytest.mark.parametrize("pair", [False, True])
@pytest.mark.parametrize("pkind", ["glu", "highway"])
@pytest.mark.parametrize("form", GATE_TILES)
@pytest.mark.parametrize("mode", ["f16x3", "bf16x3"])
def test_fused_gate_backward_footprint(dev, mode, form, pkind, pair):
    """DGRAD launch + GateFuse: y, x, r and the highway producer's input pg_x under every placement; dab / dres / part
    (dense-only: dpg, dpg_res, pg_part) banded.  The tail must leave every guard word alone, agree bit for bit with its own
    dense launch (pg_part: in value, see _part_check), and -- test_gpu_gate_tails.py / test_gpu_gate_fuse.py: "the fused tail and the stand-alone kernel agree bit
    for bit" -- dab / dres must equal ops.gate_bwd of the y it wrote."""
    ops, L = GO._lib()
    prev = ops.set_gemm_precision(mode)
    hint = GO.SPLIT_FORMS[form][0]
    pmode = ops.EPI_GLU if pkind == "glu" else ops.EPI_HIGHWAY
    worst, ran, launches = 0.0, 0, 0
    try:
        for shape in R.EDGE_SHAPES:
            B, C, T, k, d, causal = shape
            M, padL = 2 * C, R.pad_left(k, d, causal)
            for fam in FAMILIES:
                f = R.family(fam, "dgrad", mode, shape)
                w = torch.from_numpy(f["wgt"]).to(dev)
                pk = _cached(("pk", fam, "dgrad", mode, shape, False), lambda: ops.pack_weights(w, None, need_bwd=True))
                r_np = _residual((B, C, T), 31 + C + T, f["quantum"])
                exp = _expect(dev, fam, "dgrad", mode, shape, "r", r_np)
                rng = np.random.RandomState(53 + C + T)
                pab = torch.from_numpy(rng.standard_normal((B, 2 * C, T)).astype(np.float32)).to(dev)      # the producer's pre-gate pair
                px_np = rng.standard_normal((B, C, T)).astype(np.float32)                                   # ... and its input (highway)
                ikey = (fam, "dgrad", R.forms("dgrad", mode), False, shape)
                what0 = "dgrad+gate %s %s %s pair=%d %s %s" % (mode, form, pkind, pair, fam, shape)
                n_part = (B * T + 31) // 32

                def launch(pl):
                    def put(name, arr):
                        if pl is None:
                            return _cached(("dense", ikey, name), lambda: torch.from_numpy(arr).to(dev))
                        return _placed(dev, ikey + (name,), arr, pl)[1]
                    bufs = {}
                    if pl is None:
                        y = torch.full((B, C, T), float("nan"), device=dev)
                    else:
                        bufs["y"] = _out(dev, (B, C, T), pl)
                        y = bufs["y"][1]
                    gate = ops.GateFuse(pab, pmode, 1 if pkind == "glu" else 0, x=put("pg_x", px_np) if pkind == "highway" else None,
                                        pair=pair)
                    bufs["dab"] = _out(dev, (B, 2 * C, T), "banded", "dab")
                    gate.dab = bufs["dab"][1]
                    pbuf = _out(dev, (1, 2 * C, n_part), "banded", "part")
                    bufs["part"] = pbuf
                    gate.part = pbuf[1][0]
                    if pkind == "highway":
                        bufs["dres"] = _out(dev, (B, C, T), "banded", "dres")
                        gate.dres = bufs["dres"][1]
                    ops.conv_gemm(put("x", f["act"]), pk.bwd, pk.ldb, 0, B=B, Cin=M, Tin=T, M=C, Tout=T, J=k, dil=d,
                                  padL=(k - 1) * d - padL, mode=ops.EPI_DGRAD, a_split=pk.bwd_s, tile_hint=hint,
                                  r=put("r", r_np), y=y, gate=gate)
                    assert gate.dab.data_ptr() == bufs["dab"][1].data_ptr() and gate.part.data_ptr() == pbuf[1].data_ptr()
                    return y, bufs, gate

                try:
                    yd, bd, gd = launch(None)
                except RuntimeError as e:
                    # the rule: the fused tail lives in tiles 1, 2, 8, 9 of the bf16-pair kernels (conv_gemm_bf16x3.hip) and
                    # the 256 x 256 kernel; a forced tile the shape's LDS budget rejects declines the shape, not a placement
                    assert form != "auto" and ("not eligible" in str(e) or "LDS tile" in str(e)), (what0, str(e))
                    continue
                census = L.dv3_debug_get(10)
                assert census // 1000 == 3, (what0, census)       # the input gradient runs on bf16 pairs in both split modes
                if form != "auto":
                    assert census % 1000 // 10 in (60 + hint - 20,), (what0, census)
                dense = {n: _bits(v[1]).clone() for n, v in bd.items()}
                launches, ran = launches + 1, ran + 1
                worst = max(worst, _check(fam, yd, exp, what0 + " dense y"))
                # the stand-alone gate backward of the same dy
                sdab, sdres, _ = ops.gate_bwd(yd, pab, gd.x, B=B, C=C, T=T, mode=pmode, residual=gd.residual,
                                              want_dres=pkind == "highway", pair=pair)
                plain = sdab if not pair else ops.gate_bwd(yd, pab, gd.x, B=B, C=C, T=T, mode=pmode, residual=gd.residual)[0]
                psum = _part_sums(plain, n_part)
                worst = max(worst, _part_check(bd["part"][1], psum, what0 + " dense"))
                assert torch.equal(_bits(sdab), dense["dab"]), what0 + ": dab differs from the stand-alone gate backward"
                if pkind == "highway":
                    assert torch.equal(_bits(sdres), dense["dres"]), what0 + ": dres differs from the stand-alone gate backward"
                _clean(what0 + " dense", **{n: v for n, v in bd.items() if not (pair and n == "dab")})
                for pl in FP.PLACEMENTS:
                    what = "%s [%s]" % (what0, pl)
                    y, bufs, gate = launch(pl)
                    assert L.dv3_debug_get(10) == census, (what, census)
                    launches += 1
                    for n, (buf, view) in bufs.items():
                        v = FP.violations(buf)
                        assert not v, "%s: %s: %s" % (what, n, FP.describe(v))
                        assert FP.unwritten(view) == 0, "%s: %s has unwritten words" % (what, n)
                        if not (pair and n == "dab"):           # pair words are bit patterns, not numbers
                            assert not FP.poisoned(view), "%s: a NaN reached %s" % (what, n)
                    assert torch.equal(_bits(y), _bits(yd)), what + ": y differs from the dense launch"
                    for n in dense:
                        if n == "part":     # the one output whose summation order the epilogue form changes (_part_check)
                            worst = max(worst, _part_check(bufs[n][1], psum, what))
                            continue
                        assert torch.equal(_bits(bufs[n][1]), dense[n]), "%s: %s differs from the dense launch" % (what, n)
        _inputs_intact("dgrad+gate %s %s" % (mode, form))
    finally:
        ops.set_gemm_precision(prev)
    assert ran > 0, "no edge shape took the fused gate backward in form %s" % form
    _report("dgrad+gate %s %s %s pair=%d (%d shape x family)" % (mode, form, pkind, pair, ran), worst, launches)


# ---------------------------------------------------------------------------------------------------------------
# weight gradient
# ---------------------------------------------------------------------------------------------------------------
def _wgrad_spec(ops, mode, form, shape, small):
    """-> (split, ksplit, g_pair, masked, switches, S, census rule name) or None when the form does not serve the shape"""
    B, C, T, k, d, causal = shape
    M = 2 * C
    if mode == "bf16":
        spec = GB.WGRAD_FORMS[form]
        if spec is None:
            x3, S = ops.wgrad_plan(B, M, C, T, k)
            assert x3 == (not small)
            return (not small), x3, False, False, {}, S, None
        if small:
            return None
        ksplit, masked, switches, want_census = spec
        return True, ksplit, False, masked, switches, (3 if ksplit else min(B, 2)), want_census
    spec = (GO.WGRAD_F32_FORMS if mode == "f32" else GO.WGRAD_SPLIT_FORMS)[form]
    if spec is None:
        x3, S = ops.wgrad_plan(B, M, C, T, k)
        assert x3 == (("f32" if small else mode) != "f32")
        return x3, x3, False, False, {}, S, None
    split, ksplit, g_pair, masked, switches = spec
    if split and small:
        return None
    return split, ksplit, g_pair, masked, switches, (3 if ksplit else min(B, 2)), None


def _wgrad_census_ok(mode, form, shape, small, split, g_pair, want_census, census, g, x):
    """the census rules of test_gpu_gemm_operands.py / test_gpu_gemm_bf16.py; the two-steps-ahead kernel's own rule
    (csrc/wgrad_gemm_bf16x3.hip) with the strides the launch was given"""
    B, C, T, k, d, causal = shape
    M = 2 * C
    if mode == "bf16":
        if small:
            return census == 1000
        if want_census is None:
            return census == (4030 if k == 3 else 4010)
        return census == (want_census if k == 3 else 4010)
    taps2 = k == 3 and (B - 1) * g.stride(0) + (M - 1) * g.stride(1) + T >= 8 and \
        (B - 1) * x.stride(0) + (C - 1) * x.stride(1) + T >= 8
    if not split:
        return census == (1000, 1010)[not small]
    if form == "split_bf16" or k != 3:
        return census == 3010
    if form == "all_taps":
        return census == 3030
    if form == "two_steps_ahead_per_tap":
        return census == (3040 if taps2 else 3010)
    return census // 10 == (304 if taps2 else 301) and (census % 2 == 1) == (g_pair and taps2)


def _run_wgrad(dev, mode, form, fam, shape):
    ops, L = GO._lib()
    B, C, T, k, d, causal = shape
    M, padL = 2 * C, R.pad_left(k, d, causal)
    small = M <= 64 and C <= 64           # dv3_wgrad_gemm_f32: such layers run the exact fp32 kernel in every mode
    spec = _wgrad_spec(ops, mode, form, shape, small)
    if spec is None:
        return None
    split, ksplit, g_pair, masked, switches, S, want_census = spec
    eff_mode = "f32" if small else mode
    exact = fam in R.EXACT
    f = R.family(fam, "wgrad", eff_mode, shape)
    keep = bits = None
    rs = 0
    if masked:
        keep = GB._keep((B, C, T), 5)
        words, rs = R.keep_bits_words(keep)
        bits = _cached(("keepbits", shape), lambda: torch.from_numpy(words).to(dev))
    if mode == "bf16" and not small:       # test_gpu_gemm_bf16.py: the same-rounding expectation, its depth and roundings
        def make():
            n = R.n_products("wgrad", mode, J=k, K=M, B=B, T=T, n_slabs=S, k_split=bool(ksplit))
            tail, bnd = R.expect_bf16(R.make_mm("wgrad", d, padL, k), f["act"], f["wgt"], n, wgt_keep=keep,
                                      scale=2.0 if masked else 1.0, ops=1 if masked else 0, device=dev)
            want, bnd = R.prepare_bf16(exact, tail, bnd, "wgrad")
            return want, want, bnd
        exp = _cached(("expect_bf16_wgrad", fam, shape, S, bool(ksplit), masked), make)
    else:
        wgt = f["wgt"] if keep is None else (f["wgt"] * keep.astype(np.float32) * np.float32(2.0))
        exp = _expect(dev, fam, "wgrad", eff_mode, shape, None, None, wgt=wgt, n_slabs=S, k_split=bool(ksplit), wkey=masked)
    g_np = f["act"]
    ikey = (fam, "wgrad", R.forms("wgrad", eff_mode), eff_mode == "f32", shape)
    if g_pair:
        g_np = R.pair_words(f["act"]).numpy()
        ikey = ikey + ("pair",)
    what0 = "wgrad %s %s %s %s" % (mode, form, fam, shape)

    def launch(pl, rows):
        if pl is None:
            g = _cached(("dense", ikey, "g"), lambda: torch.from_numpy(g_np).to(dev))
            x = _cached(("dense", ikey, "x"), lambda: torch.from_numpy(f["wgt"]).to(dev))
            out, ldo, bufs = None, None, {}
        else:
            g, x = _placed(dev, ikey + ("g",), g_np, pl)[1], _placed(dev, ikey + ("x",), f["wgt"], pl)[1]
            obuf, out, ldo = _out_slabs(dev, S, k, M, C, pl, rows)
            bufs = {"slabs": (obuf, out)}
        o = ops.wgrad_gemm(g, x, B=B, M=M, Cin=C, T=T, Tin=T, J=k, dil=d, padL=padL, n_slabs=S, xmask=bits, xmask_rs=rs,
                           drop_scale=2.0 if masked else 1.0, split_bf16=split, k_split=ksplit, g_pair=g_pair, out=out,
                           ldo=ldo, rows_of_slabs=rows)
        census = L.dv3_debug_get(11)
        assert _wgrad_census_ok(mode, form, shape, small, split, g_pair, want_census, census, g, x), (what0, pl, census)
        if rows:
            o = o.permute(2, 0, 1, 3)       # [J][M][S][C] -> [S][J][M][C]
        return o, bufs, census

    worst, launches = 0.0, 0
    with GO._form(switches):
        od, _, census = launch(None, False)
        launches += 1
        worst = max(worst, _check(fam, od.double().sum(0), exp, what0 + " dense"))
        for rows in (False, True):
            for pl in FP.PLACEMENTS:
                what = "%s [%s, rows_of_slabs=%d]" % (what0, pl, rows)
                o, bufs, c2 = launch(pl, rows)
                launches += 1
                assert c2 == census, "%s: census %d, dense %d" % (what, c2, census)
                _clean(what, **bufs)
                assert torch.equal(_bits(o), _bits(od)), "%s: differs from the dense launch in %d elements" % (
                    what, int((_bits(o) != _bits(od)).sum()))
                worst = max(worst, _check(fam, o.double().sum(0), exp, what))
    return worst, launches


@pytest.mark.parametrize("mode,form", WGRAD_CASES)
def test_wgrad_gemm_footprint(dev, mode, form):
    ops, L = GO._lib()
    prev = ops.set_gemm_precision(mode)
    try:
        worst, ran, launches = 0.0, 0, 0
        for shape in R.EDGE_SHAPES:
            for fam in FAMILIES:
                r = _run_wgrad(dev, mode, form, fam, shape)
                if r is not None:
                    worst, ran, launches = max(worst, r[0]), ran + 1, launches + r[1]
        _inputs_intact("wgrad %s %s" % (mode, form))
    finally:
        ops.set_gemm_precision(prev)
    assert ran > 0
    _report("wgrad %s %s (%d shape x family)" % (mode, form, ran), worst, launches)


# ---------------------------------------------------------------------------------------------------------------
# each once: the per-batch operand of attention, keep-bit rows with slack
# ---------------------------------------------------------------------------------------------------------------
def test_per_batch_operand_footprint(dev):
    """The per-batch-A form attention uses (a_bs != 0; ops.AttnCoreFn: S[b] = q[b]^T k[b], A = q[b] as [Cin = E][lda = Tq]):
    lda = Tq with Tq % 4 != 0 and `a` itself one float past a 16-byte boundary -- conv_gemm.hip stages such an operand
    element by element (a_scalar).  q sits in a poisoned buffer, k and S under every placement."""
    ops, L = GO._lib()
    prev = ops.set_gemm_precision("f32")
    worst, launches = 0.0, 0
    try:
        for (B, E, Tq, Tk) in [(3, 64, 37, 200), (2, 24, 5, 33), (1, 8, 1, 1), (2, 40, 131, 50)]:
            assert Tq % 4 != 0
            rng = np.random.RandomState(E + Tq + Tk)
            for fam in FAMILIES:
                if fam == "E1":
                    q, kk = rng.randint(-15, 16, size=(B, E, Tq)).astype(np.float32), rng.randint(-15, 16, size=(B, E, Tk)).astype(np.float32)
                else:
                    q, kk = rng.standard_normal((B, E, Tq)).astype(np.float32), rng.standard_normal((B, E, Tk)).astype(np.float32)
                q64, k64 = torch.from_numpy(q).double().to(dev), torch.from_numpy(kk).double().to(dev)
                ref = torch.einsum("bet,ben->btn", q64, k64)
                # E products added in fp32, + 2: gemm_split_ref's epilogue operations (the module docstring's accumulation term)
                bnd = (E + R.EPILOGUE_OPS) * R.U32 * torch.einsum("bet,ben->btn", q64.abs(), k64.abs())
                exp = (ref, ref, bnd)
                qbuf, qv = FP.place(q, "offset1", dev)
                assert qv.data_ptr() % 16 == 4 and qv.is_contiguous()
                what0 = "per-batch A %s (B=%d E=%d Tq=%d Tk=%d)" % (fam, B, E, Tq, Tk)
                kd = torch.from_numpy(kk).to(dev)
                Sd = ops.conv_gemm(kd, torch.from_numpy(q).to(dev), Tq, 0, B=B, Cin=E, Tin=Tk, M=Tq, Tout=Tk, a_bs=E * Tq)
                census = L.dv3_debug_get(10)
                assert census // 1000 == 1, census
                launches += 1
                worst = max(worst, _check(fam, Sd, exp, what0 + " dense"))
                for pl in FP.PLACEMENTS:
                    what = "%s [%s]" % (what0, pl)
                    kbuf, kv = FP.place(kk, pl, dev)
                    ybuf, y = _out(dev, (B, Tq, Tk), pl)
                    ops.conv_gemm(kv, qv, Tq, 0, B=B, Cin=E, Tin=Tk, M=Tq, Tout=Tk, a_bs=E * Tq, y=y)
                    assert L.dv3_debug_get(10) == census, what
                    launches += 1
                    _clean(what, y=(ybuf, y))
                    assert not FP.violations(kbuf) and not FP.violations(qbuf), what
                    assert torch.equal(_bits(y), _bits(Sd)), what + ": differs from the dense launch"
                    worst = max(worst, _check(fam, y, exp, what))
    finally:
        ops.set_gemm_precision(prev)
    _report("per-batch A, lda = Tq, a offset by one float", worst, launches)


def _slack_mask(dev, keep):
    """keep-bit rows [B * C][rs + 1 .. 4]: the words past ceil(T / 32) hold the sentinel, the tensor sits between bands"""
    words, rs = R.keep_bits_words(keep)
    rows = words.shape[0]
    buf, view = FP.place((1, rows, rs), "strided1", dev)
    view.view(torch.int32).copy_(torch.from_numpy(words).to(dev).reshape(1, rows, rs))
    assert view.stride(1) > rs
    return buf, view, view.stride(1)


@pytest.mark.parametrize("mode", GO.MODES + ("bf16",))
def test_keep_bit_rows_with_slack(dev, mode):
    """xmask / ymask with xmask_rs / ymask_rs larger than ceil(T / 32) and sentinel words in the slack and around the
    mask: a kernel that reads a word past the row's last one (or indexes rows with the minimal stride) keeps or drops the
    wrong elements.  Forward (xmask), input gradient (ymask), weight gradient (xmask), automatic forms."""
    ops, L = GO._lib()
    prev = ops.set_gemm_precision(mode)
    worst, launches = 0.0, 0
    try:
        for shape in R.EDGE_SHAPES:
            B, C, T, k, d, causal = shape
            M, padL = 2 * C, R.pad_left(k, d, causal)
            keep = GB._keep((B, C, T), 29)
            mbuf, mview, mrs = _slack_mask(dev, keep)
            kf = keep.astype(np.float32) * np.float32(2.0)
            small = M <= 64 and C <= 64
            for fam in FAMILIES:
                what0 = "keep-bits with slack %s %s %s" % (mode, fam, shape)
                # forward: xd = x * bit * 2 (exact in fp32: the operand is the same fp32 value on both sides)
                f = R.family(fam, "fwd", mode, shape)
                xk = f["act"] * kf
                fa, fw = R.forms("fwd", mode)
                mm = R.make_mm("fwd", d, padL, k)
                n = R.n_products("fwd", mode, J=k, K=C, B=B, T=T)
                bias = R.bias_bcast(f["addend"])
                exp = (R.three_term(mm, xk, f["wgt"], fa, fw, bias, device=dev) if fam in R.EXACT else None,
                       R.reference(mm, xk, f["wgt"], bias, device=dev, form_a=fa, form_w=fw),
                       R.bound(mm, xk, f["wgt"], fa, fw, n, bias, device=dev)[0])
                w = torch.from_numpy(f["wgt"]).to(dev)
                pk = ops.pack_weights(w, None, need_bwd=False)
                ybuf, y = _out(dev, (B, M, T), "banded")
                ops.conv_gemm(torch.from_numpy(f["act"]).to(dev), pk.fwd, pk.lda, 0, B=B, Cin=C, Tin=T, M=M, Tout=T, J=k, dil=d,
                              padL=padL, mode=ops.EPI_LINEAR, bias=torch.from_numpy(f["addend"]).to(dev), a_split=pk.fwd_s,
                              xmask=mview, xmask_rs=mrs, drop_scale=2.0, y=y)
                launches += 1
                _clean(what0 + " fwd", y=(ybuf, y))
                worst = max(worst, _check(fam, y, exp, what0 + " fwd xmask"))
                # input gradient: y = keep ? acc * 2 : 0 (test_gpu_gemm_bf16.py: the scale on the accumulator, one more rounding --
                # the bound below carries EPILOGUE_OPS = 2 as gemm_split_ref.bound always does)
                f = R.family(fam, "dgrad", mode, shape)
                fa, fw = R.forms("dgrad", mode)
                mm = R.make_mm("dgrad", d, padL, k)
                n = R.n_products("dgrad", mode, J=k, K=M, B=B, T=T)
                kd = torch.from_numpy(kf.astype(np.float64)).to(dev)
                want = R.three_term(mm, f["act"], f["wgt"], fa, fw, device=dev) * kd if fam in R.EXACT else None
                exp = (want, R.reference(mm, f["act"], f["wgt"], device=dev, form_a=fa, form_w=fw) * kd,
                       R.bound(mm, f["act"], f["wgt"], fa, fw, n, device=dev)[0] * kd)
                w = torch.from_numpy(f["wgt"]).to(dev)
                pk = ops.pack_weights(w, None, need_bwd=True)
                ybuf, y = _out(dev, (B, C, T), "banded")
                ops.conv_gemm(torch.from_numpy(f["act"]).to(dev), pk.bwd, pk.ldb, 0, B=B, Cin=M, Tin=T, M=C, Tout=T, J=k, dil=d,
                              padL=(k - 1) * d - padL, mode=ops.EPI_DGRAD, a_split=pk.bwd_s, ymask=mview, ymask_rs=mrs,
                              drop_scale=2.0, y=y)
                launches += 1
                _clean(what0 + " dgrad", y=(ybuf, y))
                worst = max(worst, _check(fam, y, exp, what0 + " dgrad ymask"))
                # weight gradient, the automatic plan
                eff = "f32" if small else mode
                f = R.family(fam, "wgrad", eff, shape)
                x3, S = ops.wgrad_plan(B, M, C, T, k)
                exp = _expect(dev, fam, "wgrad", eff, shape, None, None, wgt=f["wgt"] * kf, n_slabs=S, k_split=bool(x3), wkey="slack")
                obuf, out, ldo = _out_slabs(dev, S, k, M, C, "banded", False)
                ops.wgrad_gemm(torch.from_numpy(f["act"]).to(dev), torch.from_numpy(f["wgt"]).to(dev), B=B, M=M, Cin=C, T=T, Tin=T,
                               J=k, dil=d, padL=padL, n_slabs=S, xmask=mview, xmask_rs=mrs, drop_scale=2.0, split_bf16=x3,
                               k_split=x3, out=out, ldo=ldo)
                launches += 1
                _clean(what0 + " wgrad", slabs=(obuf, out))
                worst = max(worst, _check(fam, out.double().sum(0), exp, what0 + " wgrad xmask"))
            assert not FP.violations(mbuf), "the mask buffer was written"
    finally:
        ops.set_gemm_precision(prev)
    _report("keep-bit rows with slack %s" % mode, worst, launches)


# ---------------------------------------------------------------------------------------------------------------
# c8 storage (dense, 16-byte aligned tensors only): bands around every tensor
# ---------------------------------------------------------------------------------------------------------------
@pytest.fixture()
def bf16_mode():
    ops, L = GO._lib()
    prev = (ops.gemm_precision(), ops.bf16_storage)
    ops.set_gemm_precision("bf16")
    ops.bf16_storage = True
    try:
        yield ops, L
    finally:
        ops.set_gemm_precision(prev[0])
        ops.bf16_storage = prev[1]


def _c8_in(dev, key, v, C):
    """bf16 values (B, C, T) -> a c8 tensor in a poisoned buffer (its padding channels zero, as the format requires)"""
    def make():
        buf, view = FP.place_c8(R.c8_pack(v), C, dev)
        view._dv3_C = C
        return buf, view
    return _cached(("in", "c8") + key, make)


def _c8_out(dev, B, C, T, tag):
    key = ("c8out", B, C, T, tag)
    G = R.c8_groups(C)
    if key not in _outs:
        _outs[key] = FP.place_c8((B, G, T, 8), C, dev)
    buf, view = _outs[key]
    buf.fill_(FP.C8_SENTINEL)
    if C % 32:
        view.view(torch.int16)[:, C // 8:] = 0
    view._dv3_C = C
    return buf, view


def _c8_clean(what, C, **bufs):
    """bands intact, no sentinel left in a whole valid group, no NaN; -> {name: float64 (B, C, T)} (padding asserted zero)"""
    out = {}
    for name, (buf, view) in bufs.items():
        v = FP.violations(buf)
        assert not v, "%s: %s: %s" % (what, name, FP.describe(v))
        Cn = C[name]
        left = int((view.view(torch.int16)[:, :Cn // 8] == FP.C8_SENTINEL).sum())
        assert left == 0, "%s: %s: %d elements of whole valid groups were never stored" % (what, name, left)
        out[name] = GB._from_c8(view, Cn, what + " " + name)           # asserts the padding channels are zero
        assert not bool(torch.isnan(out[name]).any()), "%s: a NaN reached %s" % (what, name)
    return out


@pytest.mark.parametrize("form", list(GB.C8_FORMS))
def test_c8_tap_gemm_footprint(dev, bf16_mode, form):
    """planes*, c8pp, c8pp_nw4 and the automatic choice: linear, GLU (y and the saved pair) and the input gradient with
    keep-bytes, c8 in and c8 out"""
    ops, L = bf16_mode
    switches, want_census = GB.C8_FORMS[form]
    worst, launches = 0.0, 0
    for shape in R.C8_SHAPES:
        B, C, T, k, d, padL, M = GB._dims(shape)
        gated_ok = len(shape) == 6
        for fam in FAMILIES:
            exact = fam[0] == "E"
            for var in ("linear", "glu", "dgrad"):
                if var == "glu" and not gated_ok:
                    continue
                gemm = "dgrad" if var == "dgrad" else "fwd"
                f, act, wgt = GB._operands(dev, fam, gemm, shape, True)
                mm = R.make_mm(gemm, d, padL, k)
                n = R.n_products(gemm, "bf16", J=k, K=(M if gemm == "dgrad" else C), B=B, T=T)
                w = GB._up(wgt, dev)
                pk = ops.pack_weights(w, None, glu_cg=C if var == "glu" else 0, need_bwd=(gemm == "dgrad"))
                what = "c8 %s %s %s %s" % (var, form, fam, shape)
                if gemm == "fwd":
                    x8 = _c8_in(dev, (fam, "fwd", shape), act, C)[1]
                    want, bnd = GB._expect(dev, (fam, "fwd", shape, False), exact, True, mm, act, wgt, n, act_keep=None, scale=1.0,
                                           addend=R.bias_bcast(f["addend"]), ops=R.EPILOGUE_OPS)
                    bias = GB._up(f["addend"], dev)
                    if var == "glu":
                        ybuf, y = _c8_out(dev, B, C, T, "y")
                        abuf, ab = _c8_out(dev, B, M, T, "ab")
                        with GB._switches(switches):
                            ops.conv_gemm(None, pk.fwd, pk.lda, pk.a_half, B=B, Cin=C, Tin=T, M=M, Tout=T, J=k, dil=d, padL=padL,
                                          mode=ops.EPI_GLU, Cg=C, bias=bias, ab=ab, a_split=pk.fwd_s, x_c8=x8, out_c8=True, y=y)
                            census = L.dv3_debug_get(10)
                        got = _c8_clean(what, dict(y=C, ab=M), y=(ybuf, y), ab=(abuf, ab))["ab"]
                    else:
                        ybuf, y = _c8_out(dev, B, M, T, "y")
                        with GB._switches(switches):
                            ops.conv_gemm(None, pk.fwd, pk.lda, 0, B=B, Cin=C, Tin=T, M=M, Tout=T, J=k, dil=d, padL=padL,
                                          mode=ops.EPI_LINEAR, bias=bias, a_split=pk.fwd_s, x_c8=x8, out_c8=True, y=y)
                            census = L.dv3_debug_get(10)
                        got = _c8_clean(what, dict(y=M), y=(ybuf, y))["y"]
                else:
                    g8 = _c8_in(dev, (fam, "dgrad", shape), act, M)[1]
                    keep = GB._keep((B, C, T), 17)
                    # n products, + 1: the drop_scale product on the accumulator (test_gpu_gemm_bf16.py, variant "ymask")
                    want, bnd = GB._expect(dev, (fam, "dgrad", shape, "ymask"), exact, True, mm, act, wgt, n, out_keep=keep, scale=2.0,
                                           ops=1, addend=None)
                    ybuf, y = _c8_out(dev, B, C, T, "y")
                    with GB._switches(switches):
                        ops.conv_gemm(None, pk.bwd, pk.ldb, 0, B=B, Cin=M, Tin=T, M=C, Tout=T, J=k, dil=d, padL=(k - 1) * d - padL,
                                      mode=ops.EPI_DGRAD, a_split=pk.bwd_s, x_c8=g8, out_c8=True, drop_scale=2.0,
                                      ymask_c8=GB._up(R.keep_bytes(keep), dev), y=y)
                        census = L.dv3_debug_get(10)
                    got = _c8_clean(what, dict(y=C), y=(ybuf, y))["y"]
                assert GB._c8_census_ok(census, want_census), (what, census)
                launches += 1
                worst = max(worst, R.check_prepared(exact, got, want, bnd, what))
    _inputs_intact("c8 " + form)
    _report("c8 tap-GEMM %s (%d shapes)" % (form, len(R.C8_SHAPES)), worst, launches)


@pytest.mark.parametrize("form", list(GB.WGRAD_C8_FORMS))
def test_wgrad_c8_footprint(dev, bf16_mode, form):
    """every wgrad_c8 form: g8 / x8 in poisoned buffers, the slabs (both layouts) between bands"""
    ops, L = bf16_mode
    switches, base, il = GB.WGRAD_C8_FORMS[form]
    worst, launches = 0.0, 0
    with GB._switches(switches):
        for shape in R.C8_SHAPES:
            B, C, T, k, d, padL, M = GB._dims(shape)
            chunks = B * ((T + 31) // 32)
            for fam in FAMILIES:
                exact = fam[0] == "E"
                f, act, wgt = GB._operands(dev, fam, "wgrad", shape, True)
                g8 = _c8_in(dev, (fam, "wgrad_g", shape), act, M)[1]
                x8 = _c8_in(dev, (fam, "wgrad_x", shape), wgt, C)[1]
                for S in (1, 3):
                    def make(S=S):
                        own = R.c8_slabs(B, T, S)
                        n = R.c8_slab_frames(B, T, S)
                        pairs = [R.prepare_bf16(exact, *R.expect_bf16(R.make_mm("wgrad", d, padL, k), act, wgt, n,
                                                                      act_keep=own[s][:, None, :], ops=0, device=dev)) for s in range(S)]
                        return torch.stack([p[0] for p in pairs]), (None if exact else torch.stack([p[1] for p in pairs]))
                    want, bnd = GB._cached(("expect", fam, "wgrad_c8", shape, S, False), make)
                    for rows in (False, True):
                        what = "wgrad_c8 %s %s %s S=%d rows_of_slabs=%d" % (form, fam, shape, S, rows)
                        obuf, out, ldo = _out_slabs(dev, S, k, M, C, "banded", rows)
                        assert ldo == C and out.is_contiguous()
                        ops.wgrad_gemm_c8(g8, x8, B=B, M=M, Cin=C, T=T, J=k, dil=d, padL=padL, n_slabs=S, rows_of_slabs=rows, out=out)
                        census = L.dv3_debug_get(11)
                        assert census == base + k + (il if k == 3 else 0), (what, census)
                        launches += 1
                        _clean(what, slabs=(obuf, out))
                        got = out.permute(2, 0, 1, 3) if rows else out
                        if S > chunks:
                            assert not bool(got[chunks:].any()), what + ": an empty slab is not zero"
                        worst = max(worst, R.check_prepared(exact, got, want, bnd, what))
    _inputs_intact("c8 " + form)
    _report("wgrad_c8 %s (%d shapes)" % (form, len(R.C8_SHAPES)), worst, launches)

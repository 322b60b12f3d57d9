# coding: utf-8
"""-m gpu: dv3_speaker_bias_fwd_f32 / _bwd_f32 (csrc/speaker_bias.hip) through hand-built dv3_spk_desc / dv3_spk_layer
structs -- out, strides, dout_c8p, scratch and the gradient buffers are the test's -- against the float64 reference of
tests/speaker_bias_ref.py, ELEMENT BY ELEMENT: bit for bit on the EXACT families, inside the derived bounds (none is
measured; tests/test_cpu_speaker_bias_ref.py shows what they catch) on the BOUNDED ones.  tests/test_gpu_speaker_bias.py
keeps the tensor-max checks and the whole-model parity.

The covering selection (an edit that drops an edge shows here).  dout: f = fp32 contiguous, s = the [:, :C, :] slice of a
2 C tensor whose other half is NaN, o = that slice of a view starting ONE element into its storage (row bases 4-byte
aligned only), 8 = a c8 bf16 tensor with dout_c8p = ceil(2 C / 8) and NaN padding channels (run as fp32 as well: same bits).
e: c = contiguous, p = padded batch and row strides and a base one element into its storage.

  #   family      B   E    T   C per layer        g     bias  dout e     edge
  0   dyadic      1  16    1   (1,)               -     -     f    c     T = 1, C = 1: one frame, one row
  1   dyadic      3   5    3   (8, 31)            -     yes   s    p     T = 3 (per-frame loads only), E = 5, two layers
  2   wn          1  16    4   (32,)              yes   yes   o    c     T = 4: exactly one 16-byte load; full row tile
  3   dropped     3   1    5   (33,)              -     -     f    p     T = 5, E = 1, a 1-row second tile, no dbias
  4   dyadic      1  16  255   (65,)              -     yes   s    c     T = 255: the last lane's frames fall back
  5   wn          3   5  256   (1, 8)             yes   -     f    c     T = 256: no tail at all; bias NULL with g
  6   coded       1  16  259   (33, 33)           -     zero  o    c     every element its own value; T = 3 (mod 4) past a chunk
  7   last        3  16  257   (31,)              -     yes   f    c     dout only in the last frame (a 1-frame chunk) and row
  8   dropped     1   5  515   (32, 33)           -     yes   s    p     three chunks, T = 3 (mod 4)
  9   dyadic      1   1    5   (8,) * 16          -     yes   f    c     16 layers in one call
 10   normal      3  16  259   (65, 8)            yes   yes   s    c     BOUNDED
 11   normal      1   5  257   (31, 32, 33)       -     yes   o    p     BOUNDED, plain weights
 12   wide        3  16  515   (33,)              yes   yes   f    c     BOUNDED, dout over 1e-3 .. 1e3
 13   saturated   3  16  256   (32, 1)            yes   yes   s    c     BOUNDED, |out| in {1 - 2^-24, 1 - 2^-12, 1, 0}
 14   normal      1  16    4   (8,) * 16          yes   yes   f    c     BOUNDED, 16 layers
 15-19 dyadic / normal, c8 dout, C in {1, 7, 9, 33, 40}: see C8_CASES
 The forward runs at every row of the table: on the EXACT rows with the forward-exact family of speaker_bias_ref (same
 shapes; wn rows also with their g, bounded), on the BOUNDED rows with the row's own inputs; and at C = 2048, T = 5 (the
 139 KB dynamic-LDS path).  Through ops.speaker_bias_block and autograd: 17 layers (two chunks), and an exact case.

Workspace hygiene in every backward: scratch (sized exactly to dv3_speaker_bias_bwd_scratch_floats) and de start as NaN,
dv / dg / dbias hold known dyadic values, every buffer is followed by a NaN guard.  Every launch is made twice, and once
with debug switch 54 (the one-tile-ahead prefetch) off: identical bits in ALL outputs."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tests import speaker_bias_ref as R  # noqa: E402
from tests.util import assert_close_elementwise  # noqa: E402

pytestmark = pytest.mark.gpu

NAN = float("nan")
GUARD = 256

#        family       B   E    T  Cs             g      bias   dout e
CASES = [("dyadic", 1, 16, 1, (1,), False, False, "f", "c"),
         ("dyadic", 3, 5, 3, (8, 31), False, True, "s", "p"),
         ("wn", 1, 16, 4, (32,), True, True, "o", "c"),
         ("dropped", 3, 1, 5, (33,), False, False, "f", "p"),
         ("dyadic", 1, 16, 255, (65,), False, True, "s", "c"),
         ("wn", 3, 5, 256, (1, 8), True, False, "f", "c"),
         ("coded", 1, 16, 259, (33, 33), False, True, "o", "c"),
         ("last", 3, 16, 257, (31,), False, True, "f", "c"),
         ("dropped", 1, 5, 515, (32, 33), False, True, "s", "p"),
         ("dyadic", 1, 1, 5, (8,) * 16, False, True, "f", "c"),
         ("normal", 3, 16, 259, (65, 8), True, True, "s", "c"),
         ("normal", 1, 5, 257, (31, 32, 33), False, True, "o", "p"),
         ("wide", 3, 16, 515, (33,), True, True, "f", "c"),
         ("saturated", 3, 16, 256, (32, 1), True, True, "s", "c"),
         ("normal", 1, 16, 4, (8,) * 16, True, True, "f", "c")]
#           family     B   E    T  Cs          g
C8_CASES = [("dyadic", 1, 16, 5, (1,), False), ("dyadic", 3, 5, 257, (7, 9), False), ("wn", 1, 16, 259, (33,), True),
            ("normal", 3, 16, 130, (40, 1), True), ("normal", 1, 5, 3, (9, 33), False)]


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


def _env():
    from deepvoice3_pytorch_amd import ops, _lib
    return ops, _lib.lib(), _lib.STRUCTS


def _report(what, ratio, by=None):
    """the worst |error| / bound of a case, and (backward) of each kind of output: de, dv, dg, db"""
    tail = "   " + " ".join("%s %.3g" % kv for kv in sorted(by.items())) if by else ""
    print("worst-ratio %-72s %.4g%s" % (what, ratio, tail))


def _up(dev, a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _guarded(dev, a, pre=0):
    """host array -> device buffer [pre NaN][a][GUARD NaN] and the view of a"""
    a = np.ascontiguousarray(a, dtype=np.float32).reshape(-1)
    t = torch.full((pre + a.size + GUARD,), NAN, device=dev)
    t[pre:pre + a.size] = _up(dev, a)
    return t


def _guard_ok(t, pre, n):
    return bool(torch.isnan(t[:pre]).all()) and bool(torch.isnan(t[pre + n:]).all())


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.int32)


def _e_buffer(dev, e, layout):
    """-> (buffer, pointer, e_bs, e_rs): contiguous, or rows of T + 3 floats, items of E rows + 5 floats, base at element 1;
    everything between the rows is NaN"""
    B, E, T = e.shape
    if layout == "c":
        t = _guarded(dev, e)
        return t, t.data_ptr(), E * T, T
    rs, bs = T + 3, E * (T + 3) + 5
    host = np.full(1 + B * bs + GUARD, NAN, np.float32)
    for b in range(B):
        for k in range(E):
            o = 1 + b * bs + k * rs
            host[o:o + T] = e[b, k]
    t = _up(dev, host)
    return t, t.data_ptr() + 4, bs, rs


def _dout_buffer(dev, d, kind, seed):
    """-> (buffer, pointer, dout_bs, dout_rs, dout_c8p)"""
    B, C, T = d.shape
    if kind == "f":
        t = _guarded(dev, d)
        return t, t.data_ptr(), C * T, T, 0
    if kind in ("s", "o"):
        full = np.full((B, 2 * C, T), NAN, np.float32)
        full[:, :C] = d
        pre = 1 if kind == "o" else 0
        t = _guarded(dev, full, pre=pre)
        return t, t.data_ptr() + 4 * pre, 2 * C * T, T, 0
    words, c8p = R.c8_words(d, seed)
    t = _up(dev, words.view(np.int16).reshape(-1))
    return t, t.data_ptr(), 0, 0, c8p


def _layers_on_device(dev, case):
    keep = []
    for lay in case["layers"]:
        keep.append({k: (_up(dev, lay[k]) if lay.get(k) is not None else None) for k in ("v", "g", "bias")})
    return keep


def _ptr(t):
    return t.data_ptr() if t is not None else None


def _forward(dev, case, e_layout="c"):
    """the raw forward -> [out (B, C, T) host arrays]; every out buffer NaN before, its guard NaN after"""
    ops, L, S = _env()
    B, E, T = case["e"].shape
    n = len(case["layers"])
    eb, ep, e_bs, e_rs = _e_buffer(dev, case["e"], e_layout)
    par = _layers_on_device(dev, case)
    arr = (S["dv3_spk_layer"] * n)()
    outs = []
    for l, p in enumerate(par):
        C = p["v"].shape[0]
        o = torch.full((B * C * T + GUARD,), NAN, device=dev)
        arr[l].v, arr[l].g, arr[l].bias, arr[l].out, arr[l].C = p["v"].data_ptr(), _ptr(p["g"]), _ptr(p["bias"]), o.data_ptr(), C
        outs.append(o)
    d = S["dv3_spk_desc"]()
    d.e, d.e_bs, d.e_rs, d.B, d.E, d.T, d.n_layers = ep, e_bs, e_rs, B, E, T, n
    ops._lib.call("dv3_speaker_bias_fwd_f32", ctypes.byref(d), arr, ops._stream())
    torch.cuda.synchronize()
    res = []
    for o, p in zip(outs, par):
        C = p["v"].shape[0]
        assert _guard_ok(o, 0, B * C * T), "forward wrote beyond out"
        res.append(o[:B * C * T].cpu().numpy().reshape(B, C, T))
    return res


def _check_forward(dev, case, e_layout, what):
    ref = R.forward(case["e"], case["layers"])
    first = _forward(dev, case, e_layout)
    again = _forward(dev, case, e_layout)
    worst = 0.0
    for l, (got, r) in enumerate(zip(first, ref)):
        assert np.array_equal(_bits(got), _bits(again[l])), "%s: layer %d differs between two launches" % (what, l)
        if case["exact"]:
            bad = np.argwhere(_bits(got) != _bits(r["out"].astype(np.float32)))
            assert bad.size == 0, "%s: out of layer %d differs from the exact value at %d elements, first %s" % (
                what, l, len(bad), tuple(bad[0]))
        else:
            worst = max(worst, assert_close_elementwise(got, r["out"], 0.0, r["E_out"], "%s out of layer %d" % (what, l)))
    return worst


def _backward(dev, case, dout_kind, e_layout, prefill, prefetch=1, seed=0, tamper=None):
    """one raw backward on fresh buffers -> dict(rc, de, scratch_ok, layers=[dict(dv, dg, db)]) as host arrays.
    tamper(desc, layer array): alters the call (the refusal tests)."""
    ops, L, S = _env()
    B, E, T = case["e"].shape
    n = len(case["layers"])
    eb, ep, e_bs, e_rs = _e_buffer(dev, case["e"], e_layout)
    par = _layers_on_device(dev, case)
    arr = (S["dv3_spk_layer"] * n)()
    keep, grads = [eb], []
    for l, p in enumerate(par):
        C = p["v"].shape[0]
        o = _guarded(dev, case["outs"][l])
        db_, dp, dbs, drs, c8p = _dout_buffer(dev, case["douts"][l], dout_kind, seed + l)
        y = arr[l]
        y.v, y.g, y.bias, y.out, y.C = p["v"].data_ptr(), _ptr(p["g"]), _ptr(p["bias"]), o.data_ptr(), C
        y.dout, y.dout_bs, y.dout_rs, y.dout_c8p = dp, dbs, drs, c8p
        gv = _guarded(dev, prefill[l]["dv"])
        gg = _guarded(dev, prefill[l]["dg"]) if p["g"] is not None else None
        gb = _guarded(dev, prefill[l]["db"]) if p["bias"] is not None else None
        y.dv, y.dg, y.dbias = gv.data_ptr(), _ptr(gg), _ptr(gb)
        keep += [o, db_]
        grads.append((gv, gg, gb, C))
    d = S["dv3_spk_desc"]()
    d.e, d.e_bs, d.e_rs, d.B, d.E, d.T, d.n_layers = ep, e_bs, e_rs, B, E, T, n
    need = L.dv3_speaker_bias_bwd_scratch_floats(ctypes.byref(d), arr)
    assert need > 0
    scratch = torch.full((need + GUARD,), NAN, device=dev)
    de = torch.full((B * E * T + GUARD,), NAN, device=dev)
    d.de, d.scratch, d.scratch_floats = de.data_ptr(), scratch.data_ptr(), need
    if tamper is not None:
        tamper(d, arr)
    with ops._lib.switches({"DV3_SW_SPK_PREFETCH": prefetch}):
        rc = L.dv3_speaker_bias_bwd_f32(ctypes.byref(d), arr, ops._stream())
        torch.cuda.synchronize()
    res = dict(rc=rc, de=de[:B * E * T].cpu().numpy().reshape(B, E, T), layers=[], need=need,
               de_all=de.cpu().numpy(), scratch=scratch.cpu().numpy())
    assert _guard_ok(de, 0, B * E * T), "de: guard overwritten"
    assert _guard_ok(scratch, 0, need), "scratch: a word beyond dv3_speaker_bias_bwd_scratch_floats was written"
    for (gv, gg, gb, C), p in zip(grads, par):
        assert _guard_ok(gv, 0, C * E) and (gg is None or _guard_ok(gg, 0, C)) and (gb is None or _guard_ok(gb, 0, C))
        res["layers"].append(dict(dv=gv[:C * E].cpu().numpy().reshape(C, E), dg=gg[:C].cpu().numpy() if gg is not None else None,
                                  db=gb[:C].cpu().numpy() if gb is not None else None))
    return res


def _same_bits(a, b, what):
    assert np.array_equal(_bits(a["de"]), _bits(b["de"])), what + ": de differs"
    for l, (x, y) in enumerate(zip(a["layers"], b["layers"])):
        for k in ("dv", "dg", "db"):
            if x[k] is not None:
                assert np.array_equal(_bits(x[k]), _bits(y[k])), "%s: %s of layer %d differs" % (what, k, l)


def _check_against_ref(case, got, prefill, what):
    """every output element by element -> worst ratio to the bound (0 for an EXACT family: bit for bit)"""
    ref = R.backward(case["e"], case["layers"], case["outs"], case["douts"])
    assert got["rc"] == 0
    assert not np.isnan(got["de"]).any(), what + ": NaN in de (a scratch element read before it was written?)"
    worst, by = 0.0, {}
    todo = [("de", got["de"], ref["de"], ref["E_de"])]
    for l, (g_, r) in enumerate(zip(got["layers"], ref["layers"])):
        for k, rk, ek in (("dv", "dv", "E_dv"), ("dg", "dg", "E_dg"), ("db", "db", "E_db")):
            if g_[k] is None:
                continue
            tot, E = R.accumulated(prefill[l][k].reshape(r[rk].shape), r[rk], r[ek])
            todo.append(("%s of layer %d" % (k, l), g_[k], tot, E))
    for name, g_, want, E in todo:
        assert not np.isnan(g_).any(), "%s: NaN in %s" % (what, name)
        if case["exact"]:
            w32 = np.asarray(want, np.float64).astype(np.float32)
            assert np.array_equal(w32.astype(np.float64), want), "%s: %s: the exact value is no fp32 value" % (what, name)
            bad = np.argwhere(g_ != w32)
            assert bad.size == 0, "%s: %s differs from the exact value at %d of %d elements, first at %s: got %r want %r" % (
                what, name, len(bad), g_.size, tuple(bad[0]), float(g_[tuple(bad[0])]), float(w32[tuple(bad[0])]))
        else:
            r = assert_close_elementwise(g_, want, 0.0, E, "%s %s" % (what, name))
            by[name[:2]] = max(by.get(name[:2], 0.0), r)
            worst = max(worst, r)
    _check_against_ref.by = by
    return worst


def _build(fam, B, E, T, Cs, g, bias, seed):
    return R.family(fam, B, E, T, Cs, seed=seed, g=(g if fam not in R.EXACT_FAMILIES else None), bias=bias)


@pytest.mark.parametrize("idx", range(len(CASES)))
def test_backward_every_output_element_by_element(dev, idx):
    fam, B, E, T, Cs, g, bias, dk, ek = CASES[idx]
    case = _build(fam, B, E, T, Cs, g, bias, idx)
    assert (case["layers"][0]["g"] is not None) == g and (case["layers"][0]["bias"] is not None) == bias
    prefill = R.prefill_for(case, idx)
    what = "case %d %s" % (idx, CASES[idx][:5])
    first = _backward(dev, case, dk, ek, prefill)
    worst = _check_against_ref(case, first, prefill, what)
    _same_bits(first, _backward(dev, case, dk, ek, prefill), what + ", second launch")
    by = _check_against_ref.by
    _same_bits(first, _backward(dev, case, dk, ek, prefill, prefetch=0), what + ", switch 54 = 0")
    _report("bwd " + what, worst, by)


@pytest.mark.parametrize("idx", range(len(CASES)))
def test_forward_element_by_element(dev, idx):
    fam, B, E, T, Cs, g, bias, dk, ek = CASES[idx]
    if fam in R.EXACT_FAMILIES:
        case = R.forward_exact_case(B, E, T, Cs, seed=idx, bias=bias)
    else:
        case = _build(fam, B, E, T, Cs, g, bias, idx)
    what = "case %d %s" % (idx, CASES[idx][:5])
    worst = _check_forward(dev, case, ek, what)
    if fam == "wn":            # with g: W is exact there, but 1 + |z| is no power of two: held to the bound
        worst = max(worst, _check_forward(dev, dict(_build(fam, B, E, T, Cs, g, bias, idx), exact=False), ek, what + " (g)"))
    _report("fwd " + what, worst)


def test_forward_at_2048_rows_uses_the_large_dynamic_lds(dev):
    """C = 2048: 2048 * 17 floats = 139 KB of dynamic LDS behind hipFuncSetAttribute; T = 5"""
    worst = 0.0
    for g in (True, False):
        case = R.family("normal", 1, 16, 5, (2048, 33), seed=3, g=g)
        worst = max(worst, _check_forward(dev, case, "p", "C = 2048 g=%s" % g))
    _report("fwd C = 2048, T = 5", worst)


@pytest.mark.parametrize("idx", range(len(C8_CASES)))
def test_backward_c8_gradient_is_the_fp32_path_bit_for_bit(dev, idx):
    """a c8 dout with C not a multiple of 8: NaN padding channels in the last group (the `i < n` guard keeps them out),
    other values in channels C .. 2 C - 1; the same bits as the fp32 path fed the same bf16 values, and the reference"""
    fam, B, E, T, Cs, g = C8_CASES[idx]
    case = _build(fam, B, E, T, Cs, g, True, 100 + idx)
    case["douts"] = [R.bf16_round(d) for d in case["douts"]]
    prefill = R.prefill_for(case, idx)
    what = "c8 case %d %s" % (idx, C8_CASES[idx][:5])
    c8 = _backward(dev, case, "8", "c", prefill, seed=idx)
    worst = _check_against_ref(case, c8, prefill, what)
    by = _check_against_ref.by
    _same_bits(c8, _backward(dev, case, "f", "c", prefill), what + ", fp32 path")
    _same_bits(c8, _backward(dev, case, "8", "c", prefill, seed=idx), what + ", second launch")
    _same_bits(c8, _backward(dev, case, "8", "c", prefill, prefetch=0, seed=idx), what + ", switch 54 = 0")
    _report("bwd " + what, worst, by)


def test_refusals_launch_nothing(dev):
    """the DV3_REQUIRE refusals of fill_args and of the backward's workspace check: an error code, a message, the outputs as
    pre-filled (the requirement is checked on the host before any launch: csrc/speaker_bias.hip, fill_args)"""
    ops, L, S = _env()
    ok = R.family("dyadic", 1, 16, 5, (8, 9), seed=1)
    prefill = R.prefill_for(ok, 1)
    wn = R.family("wn", 1, 16, 5, (8,), seed=1)

    def expect_refused(case, tamper, why, pf=prefill):
        got = _backward(dev, case, "f", "c", pf, tamper=tamper)
        msg = L.dv3_last_error()
        assert got["rc"] != 0 and msg, why + ": accepted"
        assert np.isnan(got["de_all"]).all() and np.isnan(got["scratch"]).all(), why + ": a refused call wrote"
        for l, g_ in enumerate(got["layers"]):
            for k in ("dv", "dg", "db"):
                if g_[k] is not None:
                    assert np.array_equal(g_[k].reshape(-1), pf[l][k].reshape(-1)), why + ": a refused call wrote " + k
        return msg.decode()

    def set_E(d, a):
        d.E = 17
    assert "speaker_embed_dim" in expect_refused(ok, set_E, "E = 17")

    def set_C(d, a):
        a[1].C = 2049
    assert "layer 1" in expect_refused(ok, set_C, "C = 2049")

    def set_n(d, a):
        d.n_layers = 17
    assert "layers per call" in expect_refused(ok, set_n, "17 layers")

    def small(d, a):
        d.scratch_floats = d.scratch_floats - 1
    assert "workspace" in expect_refused(ok, small, "scratch one float short")

    def no_dg(d, a):
        a[0].dg = None
    assert "backward needs" in expect_refused(wn, no_dg, "g without dg", R.prefill_for(wn, 1))

    def c8_short(d, a):
        a[1].dout_c8p = 1                    # 8 channels < C = 9
    assert "c8 gradient" in expect_refused(ok, c8_short, "dout_c8p * 8 < C")
    # the forward's own refusals: nothing written
    B, E, T = ok["e"].shape
    for bad_E, bad_C, bad_n in ((17, 8, 1), (16, 2049, 1), (16, 8, 17)):
        e = _guarded(dev, ok["e"])
        v = _up(dev, np.ones(2049 * 17, np.float32))
        out = torch.full((4096,), NAN, device=dev)
        arr = (S["dv3_spk_layer"] * 17)()
        for y in arr:
            y.v, y.out, y.C = v.data_ptr(), out.data_ptr(), bad_C
        d = S["dv3_spk_desc"]()
        d.e, d.e_bs, d.e_rs, d.B, d.E, d.T, d.n_layers = e.data_ptr(), E * T, T, 1, bad_E, T, bad_n
        assert L.dv3_speaker_bias_fwd_f32(ctypes.byref(d), arr, ops._stream()) != 0 and L.dv3_last_error()
        torch.cuda.synchronize()
        assert bool(torch.isnan(out).all())
    # the accepted neighbour, so that the refusals are the stated ones
    got = _backward(dev, ok, "f", "c", prefill)
    _check_against_ref(ok, got, prefill, "accepted neighbour")


def _through_ops(dev, case, with_slices):
    """ops.speaker_bias_block and autograd -> (outs, dict(de, layers)) as host arrays; e as a padded view"""
    ops, L, S = _env()
    B, E, T = case["e"].shape
    big = torch.full((B, E + 1, T + 3), NAN, device=dev)
    big[:, :E, :T] = _up(dev, case["e"])
    e = big[:, :E, :T].detach().requires_grad_(True)
    layers = []
    for lay in case["layers"]:
        layers.append(tuple((_up(dev, lay[k].reshape(-1, 1) if k == "g" else lay[k]).requires_grad_(True)
                             if lay.get(k) is not None else None) for k in ("v", "g", "bias")))
    outs = ops.speaker_bias_block(e, layers)
    douts = []
    for o, d in zip(outs, case["douts"]):
        if with_slices:
            full = torch.full((B, 2 * d.shape[1], T), NAN, device=dev)
            full[:, :d.shape[1]] = _up(dev, d)
            douts.append(full[:, :d.shape[1], :])
        else:
            douts.append(_up(dev, d))
    torch.autograd.backward(outs, douts)
    torch.cuda.synchronize()
    res = dict(rc=0, de=e.grad.cpu().numpy(), layers=[])
    for v, g, b in layers:
        res["layers"].append(dict(dv=v.grad.cpu().numpy(), dg=g.grad.cpu().numpy().reshape(-1) if g is not None else None,
                                  db=b.grad.cpu().numpy() if b is not None else None))
    return [o.detach().cpu().numpy() for o in outs], res


@pytest.mark.parametrize("fam,B,E,T,Cs,g,bias", [("normal", 3, 16, 33, tuple(range(8, 8 + 17)), True, True),
                                                  ("forward-exact", 1, 5, 257, (33, 1), False, False)])
def test_through_ops_and_autograd(dev, fam, B, E, T, Cs, g, bias):
    """the autograd plumbing: 17 layers (two chunks of the 16-layer entry point; de is the sum of both chunks' -- one
    more rounded addition per element, allowed as half an ulp of the total), g and bias NULL, dout as [:, :C, :] slices,
    e as a padded view.  The backward's reference takes the out tensors the forward RETURNED; in the forward-exact family
    those are on OUT_GRID bit for bit, and with dout on the 1/16 grid the whole backward is exact as well (|W| <= 3,
    e in {0, 1}: the sums of the dyadic family's arithmetic)."""
    if fam == "forward-exact":
        case = R.forward_exact_case(B, E, T, Cs, seed=7, bias=bias)
        rs = np.random.RandomState(5)
        case["douts"] = [R._grid(rs, (B, C, T), -16, 16, 1.0 / 16) for C in Cs]
    else:
        case = _build(fam, B, E, T, Cs, g, bias, 7)
    fwd_ref = R.forward(case["e"], case["layers"])
    outs, got = _through_ops(dev, case, with_slices=True)
    worst = 0.0
    for l, (o, r) in enumerate(zip(outs, fwd_ref)):
        if case["exact"]:
            assert np.array_equal(_bits(o), _bits(r["out"].astype(np.float32))), "ops out of layer %d is not exact" % l
        else:
            worst = max(worst, assert_close_elementwise(o, r["out"], 0.0, r["E_out"], "ops out of layer %d" % l))
    zero = [dict(dv=np.zeros_like(lay["v"]), dg=np.zeros(lay["v"].shape[0], np.float32),
                 db=np.zeros(lay["v"].shape[0], np.float32)) for lay in case["layers"]]
    case["outs"] = outs
    if case["exact"]:
        worst = max(worst, _check_against_ref(case, got, zero, "ops " + fam))
    else:
        chunks = [slice(i, i + 16) for i in range(0, len(Cs), 16)]
        de, E_de = 0.0, 0.0
        for s in chunks:
            ref = R.backward(case["e"], case["layers"][s], case["outs"][s], case["douts"][s])
            for l, r in zip(range(len(Cs))[s], ref["layers"]):
                for k, rk, ek in (("dv", "dv", "E_dv"), ("dg", "dg", "E_dg"), ("db", "db", "E_db")):
                    worst = max(worst, assert_close_elementwise(got["layers"][l][k], r[rk], 0.0, r[ek], "ops %s of layer %d" % (k, l)))
            de, E_de = de + ref["de"], E_de + ref["E_de"]
        worst = max(worst, assert_close_elementwise(got["de"], de, 0.0, E_de + R.U * np.abs(de) * R.SLACK, "ops de"))
    outs2, again = _through_ops(dev, case, with_slices=True)
    _same_bits(got, again, "ops, second run")
    _report("ops %s %s" % (fam, (B, E, T, len(Cs))), worst)

# coding: utf-8
"""-m gpu: the four entry points of csrc/attention.hip called directly, each against the float64 references of
tests/attention_ref.py computed from the same fp32 inputs, element by element (tests.util.assert_close_elementwise).

  (a) dv3_attn_softmax_f32 on scores the test writes: the monotonic window with and without key_len, its edges at 0 and
      Tk, rows off the 4-row workgroup, Tk around the 64-lane stride, a keep mask the test draws itself (tight and wide
      row stride), pd_scale_dev, and pd == NULL;
  (b) dv3_attn_softmax_bwd_f32: dS itself, "dpd only" / "dp_direct only" / both, mask, scale_dev, exact zeros where P is
      zero, a one-hot row;
  (c) dv3_attn_fwd_f32: P, pd and ctx, every exit of its two double-buffered loops, Tq = 1, key_len below the 8 threads
      of a row, the 64 KiB LDS edge, all outputs inside NaN guard regions;
  (d) dv3_attn_argmax_i32: exact ties (the first maximum), all-equal and all-zero rows, rows with a derived gap;
  (e) the documented refusals: a return code and dv3_last_error, nothing launched;
  (f) the fused and the unfused softmax on the same exact scores, and ops.attention_core against the fused kernel.

Every bound is derived in attention_ref.py from the kernels' summation depths -- none is measured; they carry one
hardware assumption (expf to 1 ulp, attention_ref.EXPF_REL).  tests/test_cpu_attention_ref.py proves the references, the
bounds (an fp32 emulation stays inside, fifteen defect models do not) and what the case lists claim.  Every direct case
runs twice and the two runs agree bit for bit (no atomics, a fixed summation order).  Every descriptor is filled through a
helper that checks each buffer's element count against the descriptor's dimensions before the launch."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tests import attention_ref as A  # noqa: E402
from tests.util import assert_close_elementwise  # noqa: E402

pytestmark = pytest.mark.gpu

NAN = float("nan")
GUARD = 1024                 # NaN floats on either side of every output


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


def _env():
    from deepvoice3_pytorch_amd import ops, _lib
    return ops, _lib.lib(), _lib.STRUCTS


def _report(what, ratio):
    print("worst-ratio %-72s %.4g" % (what, ratio))


class Guarded:
    """n floats between two NaN guard regions; .data: the n floats (NaN, or a host array's values)"""

    def __init__(self, dev, n, init=None):
        self.buf = torch.full((n + 2 * GUARD,), NAN, device=dev)
        self.data = self.buf[GUARD:GUARD + n]
        if init is not None:
            self.data.copy_(torch.from_numpy(np.ascontiguousarray(init, dtype=np.float32).reshape(-1)))

    def ptr(self):
        return self.data.data_ptr()

    def intact(self):
        return bool(torch.isnan(self.buf[:GUARD]).all()) and bool(torch.isnan(self.buf[GUARD + self.data.numel():]).all())

    def host(self, *shape):
        return self.data.cpu().numpy().reshape(shape)


def _dev_array(dev, a, dtype):
    """a small input on the device, or None; uint32 words travel as the int32 of the same bits"""
    if a is None:
        return None
    a = np.ascontiguousarray(a)
    if dtype == "u32":
        return torch.from_numpy(a.astype(np.uint32).view(np.int32)).to(dev)
    return torch.from_numpy(a.astype({"i32": np.int32, "f32": np.float32}[dtype])).to(dev)


def _n(t):
    return t.data.numel() if isinstance(t, Guarded) else t.numel()


def _p(t):
    return None if t is None else (t.ptr() if isinstance(t, Guarded) else t.data_ptr())


def _need(t, n, what, optional=False):
    if t is None:
        assert optional, what + " is required"
        return
    assert _n(t) == n, "%s holds %d elements, the descriptor says %d" % (what, _n(t), n)


def _bits_equal(a, b):
    return np.array_equal(np.ascontiguousarray(a).view(np.int32), np.ascontiguousarray(b).view(np.int32))


# ------------------------------------------------------------------------------------------------------------------
# descriptors: every buffer's element count is checked against the dimensions before anything is launched
# ------------------------------------------------------------------------------------------------------------------
def softmax_desc(B, Tq, Tk, s, pd=None, key_len=None, la=None, win=(0, 0), mask=None, mask_rs=0, drop_scale=1.0,
                 pd_scale=1.0, psd=None):
    S = _env()[2]
    _need(s, B * Tq * Tk, "s")
    _need(pd, B * Tq * Tk, "pd", True)
    _need(key_len, B, "key_len", True)
    _need(la, 1, "last_attended", True)
    _need(psd, 1, "pd_scale_dev", True)
    if mask is not None:
        assert mask_rs * 32 >= Tk and pd is not None
        _need(mask, B * Tq * mask_rs, "mask")
    d = S["dv3_softmax_desc"]()
    d.s, d.pd, d.key_len, d.last_attended = _p(s), _p(pd), _p(key_len), _p(la)
    d.mask, d.mask_rs, d.drop_scale, d.pd_scale = _p(mask), mask_rs, float(drop_scale), float(pd_scale)
    d.B, d.Tq, d.Tk, d.win_back, d.win_ahead = B, Tq, Tk, win[0], win[1]
    d.pd_scale_dev = _p(psd)
    return d


def softmax_bwd_desc(B, Tq, Tk, p, ds, dpd=None, dp_direct=None, mask=None, mask_rs=0, drop_scale=1.0, sdev=None):
    S = _env()[2]
    _need(p, B * Tq * Tk, "p")
    _need(ds, B * Tq * Tk, "ds")
    _need(dpd, B * Tq * Tk, "dpd", True)
    _need(dp_direct, B * Tq * Tk, "dp_direct", True)
    _need(sdev, 1, "scale_dev", True)
    assert dpd is not None or dp_direct is not None
    if mask is not None:
        assert mask_rs * 32 >= Tk
        _need(mask, B * Tq * mask_rs, "mask")
    d = S["dv3_softmax_bwd_desc"]()
    d.p, d.dpd, d.dp_direct, d.ds = _p(p), _p(dpd), _p(dp_direct), _p(ds)
    d.mask, d.mask_rs, d.drop_scale = _p(mask), mask_rs, float(drop_scale)
    d.B, d.Tq, d.Tk = B, Tq, Tk
    d.scale_dev = _p(sdev)
    return d


def attn_fwd_desc(B, E, Tq, Tk, q, k, vT, ctx, P, pd, key_len=None, mask=None, mask_rs=0, drop_scale=1.0, pd_scale=1.0,
                  psd=None):
    S = _env()[2]
    _need(q, B * E * Tq, "q")
    _need(k, B * E * Tk, "k")
    _need(vT, B * Tk * E, "vT")
    _need(ctx, B * E * Tq, "ctx")
    _need(P, B * Tq * Tk, "P")
    _need(pd, B * Tq * Tk, "pd")
    _need(key_len, B, "key_len", True)
    _need(psd, 1, "pd_scale_dev", True)
    assert A.fwd_lds_bytes(Tk) <= A.LDS_MAX and B <= 65535
    if mask is not None:
        assert mask_rs * 32 >= Tk
        _need(mask, B * Tq * mask_rs, "mask")
    d = S["dv3_attn_fwd_desc"]()
    d.q, d.k, d.vT, d.key_len = _p(q), _p(k), _p(vT), _p(key_len)
    d.mask, d.mask_rs, d.drop_scale, d.pd_scale = _p(mask), mask_rs, float(drop_scale), float(pd_scale)
    d.ctx, d.P, d.pd = _p(ctx), _p(P), _p(pd)
    d.B, d.E, d.Tq, d.Tk = B, E, Tq, Tk
    d.pd_scale_dev = _p(psd)
    return d


# ------------------------------------------------------------------------------------------------------------------
# (a) dv3_attn_softmax_f32
# ------------------------------------------------------------------------------------------------------------------
def _run_softmax(dev, c, d):
    ops = _env()[0]
    B, Tq, Tk = c["B"], c["Tq"], c["Tk"]
    s = Guarded(dev, B * Tq * Tk, d["s"])
    pd = Guarded(dev, B * Tq * Tk) if c["pd"] else None
    keep = dict(kl=_dev_array(dev, c["key_len"], "i32"), la=_dev_array(dev, None if c["la"] is None else [c["la"]], "i32"),
                mask=_dev_array(dev, d["words"], "u32"), psd=_dev_array(dev, None if d["psd"] is None else [d["psd"]], "f32"))
    desc = softmax_desc(B, Tq, Tk, s, pd, keep["kl"], keep["la"], c["win"], keep["mask"], d["mask_rs"], d["drop_scale"],
                        d["pd_scale"], keep["psd"])
    ops._lib.call("dv3_attn_softmax_f32", ctypes.byref(desc), ops._stream())
    torch.cuda.synchronize()
    assert s.intact() and (pd is None or pd.intact()), "a guard region was written"
    if keep["la"] is not None:
        assert int(keep["la"].item()) == c["la"]
    return s.host(B, Tq, Tk), None if pd is None else pd.host(B, Tq, Tk)


def _assert_zero_outside(got, lo, hi, what):
    g = np.asarray(got).reshape(len(lo), -1)
    for r in range(len(lo)):
        assert not g[r, :lo[r]].any() and not g[r, hi[r]:].any(), "%s row %d: not 0.0 outside [%d, %d)" % (what, r, lo[r], hi[r])


@pytest.mark.parametrize("i", range(len(A.SOFTMAX_CASES)))
def test_softmax_elementwise(dev, i):
    c = A.SOFTMAX_CASES[i]
    what = "attn_softmax " + A.sm_name(c)
    d = A.sm_data(c, i)
    P, pd, ep, epd, lo, hi = A.sm_ref(c, d)
    gP, gpd = _run_softmax(dev, c, d)
    gP2, gpd2 = _run_softmax(dev, c, d)
    assert _bits_equal(gP, gP2) and (gpd is None or _bits_equal(gpd, gpd2)), what + ": two runs differ"
    _assert_zero_outside(gP, lo, hi, what + " P")
    r = assert_close_elementwise(gP, P, 0, ep, what + " P")
    if gpd is not None:
        _assert_zero_outside(gpd, lo, hi, what + " pd")
        assert not gpd[pd == 0].any(), what + ": a dropped element is not 0.0"
        r = max(r, assert_close_elementwise(gpd, pd, 0, epd, what + " pd"))
    _report(what, r)


# ------------------------------------------------------------------------------------------------------------------
# (b) dv3_attn_softmax_bwd_f32
# ------------------------------------------------------------------------------------------------------------------
def _run_bwd(dev, c, d):
    ops = _env()[0]
    B, Tq, Tk = c["B"], c["Tq"], c["Tk"]
    n = B * Tq * Tk
    p = _dev_array(dev, d["P"], "f32")
    dpd, dpx = _dev_array(dev, d["dpd"], "f32"), _dev_array(dev, d["dpx"], "f32")
    mask = _dev_array(dev, d["words"], "u32")
    sdev = _dev_array(dev, None if d["sdev"] is None else [d["sdev"]], "f32")
    ds = Guarded(dev, n)
    desc = softmax_bwd_desc(B, Tq, Tk, p, ds, dpd, dpx, mask, d["mask_rs"], d["drop_scale"], sdev)
    ops._lib.call("dv3_attn_softmax_bwd_f32", ctypes.byref(desc), ops._stream())
    torch.cuda.synchronize()
    assert ds.intact(), "a guard region was written"
    assert _bits_equal(p.cpu().numpy(), d["P"]), "the kernel wrote its input"
    return ds.host(B * Tq, Tk)


@pytest.mark.parametrize("i", range(len(A.SOFTMAX_BWD_CASES)))
def test_softmax_bwd_elementwise(dev, i):
    c = A.SOFTMAX_BWD_CASES[i]
    what = "attn_softmax_bwd " + A.bwd_name(c)
    d = A.bwd_data(c, i)
    dS, bound = A.bwd_ref(c, d)
    g = _run_bwd(dev, c, d)
    assert _bits_equal(g, _run_bwd(dev, c, d)), what + ": two runs differ"
    if c["onehot"] is None:
        _assert_zero_outside(g, d["lo"], d["hi"], what + " dS")
    else:
        assert not g[c["onehot"][0]].any(), what + ": dS of a one-hot row is not identically 0"
    assert not g[d["P"] == 0].any(), what + ": dS is not 0.0 where P is"
    _report(what, assert_close_elementwise(g, dS, 0, bound, what + " dS"))


# ------------------------------------------------------------------------------------------------------------------
# (c) dv3_attn_fwd_f32
# ------------------------------------------------------------------------------------------------------------------
def _run_fwd(dev, c, d):
    ops = _env()[0]
    B, E, Tq, Tk = c["B"], c["E"], c["Tq"], c["Tk"]
    q, k, vT = (_dev_array(dev, d[x], "f32") for x in ("q", "k", "vT"))
    kl, mask = _dev_array(dev, c["key_len"], "i32"), _dev_array(dev, d["words"], "u32")
    psd = _dev_array(dev, None if d["psd"] is None else [d["psd"]], "f32")
    ctx, P, pd = Guarded(dev, B * E * Tq), Guarded(dev, B * Tq * Tk), Guarded(dev, B * Tq * Tk)
    desc = attn_fwd_desc(B, E, Tq, Tk, q, k, vT, ctx, P, pd, kl, mask, d["mask_rs"], d["drop_scale"], d["pd_scale"], psd)
    ops._lib.call("dv3_attn_fwd_f32", ctypes.byref(desc), ops._stream())
    torch.cuda.synchronize()
    assert ctx.intact() and P.intact() and pd.intact(), "a guard region was written"
    return P.host(B, Tq, Tk), pd.host(B, Tq, Tk), ctx.host(B, E, Tq)


def _check_fwd(got, ref, bounds, what):
    (gP, gpd, gctx), (ep, epd, ectx) = got, bounds
    _assert_zero_outside(gP, ref["lo"], ref["hi"], what + " P")
    assert not gpd[ref["pd"] == 0].any(), what + ": pd is not 0.0 beyond key_len / where dropped"
    return max(assert_close_elementwise(gP, ref["P"], 0, ep, what + " P"),
               assert_close_elementwise(gpd, ref["pd"], 0, epd, what + " pd"),
               assert_close_elementwise(gctx, ref["ctx"], 0, ectx, what + " ctx"))


@pytest.mark.parametrize("i", range(len(A.FWD_CASES)))
def test_fwd_elementwise(dev, i):
    c = A.FWD_CASES[i]
    what = "attn_fwd " + A.fwd_name(c)
    d = A.fwd_data(c, i)
    ref, bounds = A.fwd_ref(c, d)
    got = _run_fwd(dev, c, d)
    again = _run_fwd(dev, c, d)
    assert all(_bits_equal(a, b) for a, b in zip(got, again)), what + ": two runs differ"
    _report(what, _check_fwd(got, ref, bounds, what))


# ------------------------------------------------------------------------------------------------------------------
# (d) dv3_attn_argmax_i32
# ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", A.ARGMAX_CASES, ids=lambda c: "%s-Tk%d-%s" % c)
def test_argmax_first_maximum(dev, case):
    ops = _env()[0]
    row, want, margin = A.argmax_row(case)
    assert margin is None or margin > 0
    p = Guarded(dev, case[1], row)
    for _ in range(2):
        out = torch.full((3,), -7, dtype=torch.int32, device=dev)
        ops._lib.call("dv3_attn_argmax_i32", p.ptr(), case[1], out[1:].data_ptr(), ops._stream())
        torch.cuda.synchronize()
        assert out.tolist() == [-7, want, -7], (case, out.tolist())


# ------------------------------------------------------------------------------------------------------------------
# (e) refusals
# ------------------------------------------------------------------------------------------------------------------
def test_refusals(dev):
    """each is rejected by the launcher before any launch: a return code, dv3_last_error names the reason, the outputs
    stay NaN.  The descriptors are built valid by the checked helpers and then changed in one field"""
    ops, L, S = _env()
    B, E, Tq, Tk = 2, 4, 3, 40
    n = B * Tq * Tk
    zeros = lambda m: torch.zeros(m, device=dev)                                           # noqa: E731
    mask = torch.zeros(B * Tq * 2, dtype=torch.int32, device=dev)
    outs = dict(s=Guarded(dev, n), pd=Guarded(dev, n), ds=Guarded(dev, n), ctx=Guarded(dev, B * E * Tq), P=Guarded(dev, n))
    q, k, vT, p, g = zeros(B * E * Tq), zeros(B * E * Tk), zeros(B * Tk * E), zeros(n), zeros(n)

    def fwd(**kw):
        d = attn_fwd_desc(B, E, Tq, Tk, q, k, vT, outs["ctx"], outs["P"], outs["pd"], mask=mask, mask_rs=2)
        for key, v in kw.items():
            setattr(d, key, v)
        return d

    def sm(**kw):
        d = softmax_desc(B, Tq, Tk, outs["s"], outs["pd"], mask=mask, mask_rs=2)
        for key, v in kw.items():
            setattr(d, key, v)
        return d

    def bwd(**kw):
        d = softmax_bwd_desc(B, Tq, Tk, p, outs["ds"], dpd=g)
        for key, v in kw.items():
            setattr(d, key, v)
        return d

    for what, fn, d, text in (("attn_fwd at Tk = 512", "dv3_attn_fwd_f32", fwd(Tk=512, mask_rs=16), "too long"),
                              ("attn_fwd with B = 65536", "dv3_attn_fwd_f32", fwd(B=65536), "bad dims"),
                              ("attn_fwd with mask_rs * 32 < Tk", "dv3_attn_fwd_f32", fwd(mask_rs=1), "row stride"),
                              ("attn_softmax with mask_rs * 32 < Tk", "dv3_attn_softmax_f32", sm(mask_rs=1), "row stride"),
                              ("attn_softmax with a mask and no pd", "dv3_attn_softmax_f32", sm(pd=None), "mask needs pd"),
                              ("attn_softmax_bwd without dpd and dp_direct", "dv3_attn_softmax_bwd_f32", bwd(dpd=None),
                               "bad args")):
        rc = getattr(L, fn)(ctypes.byref(d), ops._stream())
        msg = (L.dv3_last_error() or b"").decode()
        assert rc != 0 and text in msg, (what, rc, msg)
    torch.cuda.synchronize()
    for name, buf in outs.items():
        assert bool(torch.isnan(buf.buf).all()), name + " was written"


# ------------------------------------------------------------------------------------------------------------------
# (f) the fused kernel, the unfused kernel and ops.attention_core on one family X shape
# ------------------------------------------------------------------------------------------------------------------
def test_fused_unfused_and_attention_core_agree(dev):
    """B = 2, E = 33, Tq = 33, Tk = 65, family X: the scores are exact in fp32 in any order, so both kernels run the same
    expf on the same arguments and differ only in the row sum: (ceil(hi / 8) + 3) roundings in the fused kernel,
    (ceil(hi / 64) + 6) in the unfused one, each relative to a sum of positive terms, then one rounding of 1.0f / sum and
    one of the product on either side: |P_fused - P_unfused| <= (d_f + d_u + 4) U P.  Bit identity is NOT expected.
    ops.attention_core takes the fused kernel at this shape and returns its P bit for bit."""
    ops = _env()[0]
    c = A.FWD_CASES[A.CONSISTENCY_CASE]
    B, E, Tq, Tk = c["B"], c["E"], c["Tq"], c["Tk"]
    d = A.fwd_data(c, A.CONSISTENCY_CASE)
    ref, _ = A.fwd_ref(c, d)
    gP, gpd, gctx = _run_fwd(dev, c, d)
    s32 = ref["s"].astype(np.float32)
    assert np.array_equal(s32.astype(np.float64), ref["s"])
    cs = A.sm_case(B, Tq, Tk, "X", key_len=c["key_len"], mask=c["mask"], psd=c["psd"])
    ds = dict(d, s=s32)
    uP, upd = _run_softmax(dev, cs, ds)
    hi = ref["hi"].reshape(B, Tq, 1)
    depth = np.array([A.sum_depth(0, int(h), True) + A.sum_depth(0, int(h), False) + 4 for h in ref["hi"]]).reshape(B, Tq, 1)
    r = assert_close_elementwise(gP, uP.astype(np.float64), 0, 1.001 * depth * A.U * ref["P"] + A.TINY,
                                 "fused P against unfused P")
    # pd: the same three roundings on either side, of values that differ as above
    r = max(r, assert_close_elementwise(gpd, upd.astype(np.float64), 0,
                                        1.001 * (depth + 6) * A.U * np.abs(ref["pd"]) + A.TINY, "fused pd against unfused pd"))
    assert not gP[np.arange(Tk).reshape(1, 1, Tk) >= hi].any()
    _report("fused against unfused softmax, B%d E%d Tq%d Tk%d" % (B, E, Tq, Tk), r)
    q, k = torch.from_numpy(d["q"]).to(dev), torch.from_numpy(d["k"]).to(dev)
    v = torch.from_numpy(np.ascontiguousarray(d["vT"].transpose(0, 2, 1))).to(dev)
    kl = torch.tensor(c["key_len"], dtype=torch.int32, device=dev)
    prev = ops.fused_attention, ops.valid
    ops.fused_attention, ops.valid = True, None          # the defaults: the fused launch, no device-side key count
    try:
        _, Pc = ops.attention_core(q, k, v, kl, None)
        torch.cuda.synchronize()
    finally:
        ops.fused_attention, ops.valid = prev
    assert _bits_equal(Pc.cpu().numpy(), gP), "ops.attention_core does not return the fused kernel's P"

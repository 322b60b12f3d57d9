# coding: utf-8
"""No GPU: proves tests/gemm_split_ref.py (the float64 restatement the GPU test of the split-operand GEMMs rests on) and
the input families of tests/test_gpu_gemm_operands.py.

  * the reference GEMMs are torch's double conv1d and its autograd;
  * the splits meet the per-operand statements of include/dv3hip.h over 2^-30 .. the top of the range;
  * every exact family is exact for every shape the GPU test uses (all partial sums below 2^24 quanta);
  * a split kernel emulated on the host (exact products, fp32 additions in a random order) stays inside `bound`;
  * the same emulation with fp16 subnormals flushed, or with one tap's lo plane lost, leaves the bound by at least 2 x on
    the small-magnitude families and breaks exactness on E2 / E4 -- the condition that keeps the GPU test from being
    vacuous.
"""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import gemm_split_ref as R
from tests.util import assert_close_elementwise

GEMMS = ("fwd", "dgrad", "wgrad")
MODES = ("f16x3", "bf16x3", "f32")
# small enough for the term-by-term emulation; K * J <= 192 so that the accumulation term does not swamp the operand term
EMU_SHAPES = [(2, 32, 9, 1, 1, False), (2, 8, 33, 1, 1, False), (2, 8, 12, 3, 2, True), (1, 40, 7, 2, 4, True),
              (2, 24, 6, 5, 1, False)]
# The lo plane of an fp16 pair is worth 2^-12 of its value, the accumulation term 3 J Kp 2^-24 of sum |w| |x|: ONE tap's lost
# lo plane leaves the bound by 2 x only where few products share an output -- the 1 x 1 shapes (the second one is an edge
# shape of the GPU test).  With more taps E4 catches it, with zero tolerance.
ONE_TAP_SHAPES = EMU_SHAPES[:2]


def _case(fam, gemm, mode, shape):
    B, C, T, k, d, causal = shape
    padL = R.pad_left(k, d, causal)
    f = R.family(fam, gemm, mode, shape)
    fa, fw = R.forms(gemm, mode)
    mm = R.make_mm(gemm, d, padL, k)
    n = R.n_products(gemm, mode, J=k, K=(C if gemm == "fwd" else 2 * C), B=B, T=T)
    return f, fa, fw, mm, n, R.bias_bcast(f["addend"]), dict(J=k, dil=d, padL=padL)


def test_reference_gemms_are_torchs_double_conv1d_and_its_autograd():
    rng = np.random.RandomState(0)
    for (B, C, T, k, d, causal) in R.EDGE_SHAPES:
        padL = R.pad_left(k, d, causal)
        x = torch.from_numpy(rng.standard_normal((B, C, T))).requires_grad_(True)
        w = torch.from_numpy(rng.standard_normal((2 * C, C, k))).requires_grad_(True)
        g = torch.from_numpy(rng.standard_normal((B, 2 * C, T)))
        y = F.conv1d(F.pad(x, (padL, (k - 1) * d - padL)), w, dilation=d)
        dx, dw = torch.autograd.grad((y * g).sum(), (x, w))
        for got, want in ((R.conv_fwd(x.detach(), w.detach(), d, padL), y.detach()),
                          (R.conv_dgrad(g, w.detach(), d, padL), dx),
                          (R.conv_wgrad(g, x.detach(), k, d, padL), dw.permute(2, 0, 1))):
            assert got.shape == want.shape
            assert float((got - want).abs().max()) <= 1e-12 * max(1.0, float(want.abs().max()))


def test_splits_meet_the_headers_statements():
    rng = np.random.RandomState(1)
    for shift in (R.F16_ACT_SHIFT, R.F16_WEIGHT_SHIFT):
        top = 65504.0 * 2.0 ** -shift
        exps = np.arange(-30, 16 - shift)
        v = (rng.uniform(1, 2, size=(exps.size, 4096)) * 2.0 ** exps[:, None] * rng.choice([-1, 1], size=(exps.size, 4096)))
        v = np.concatenate([v.ravel(), 2.0 ** exps, 3 * 2.0 ** exps, [top, -top, 0.0],
                            # exact halves: half-way between neighbouring fp16 values in several binades
                            (1024 + np.arange(0, 64) + 0.5) * 2.0 ** -shift, (1 + 2.0 ** -11) * 2.0 ** exps,
                            2.0 ** -25 * 2.0 ** -shift * np.arange(1, 64)]).astype(np.float32)
        v = v[np.abs(v) <= top]
        hi, lo = R.split_f16(v, shift)
        a = v.astype(np.float64) * 2.0 ** shift
        err = np.abs(a - hi - lo)
        assert np.all(err <= R.delta(v, ("f16", shift)) * 2.0 ** shift)
        # relative while the residual is a NORMAL fp16 value: |r| <= 2^(e-11) >= 2^-14 needs |a| >= 2^-2; below that the
        # residual is an fp16 subnormal and the error absolute (a = 0.22: 2^-25 > 2^-23 a)
        big = np.abs(a) >= 2.0 ** -2
        assert np.all(err[big] <= 2.0 ** -23 * np.abs(a[big])) and np.all(err[~big] <= 2.0 ** -25)
        assert np.all(np.abs(lo) <= 2.0 ** -11 * np.abs(a) + 2.0 ** -25)
        # every plane value is an fp16 value
        for p in (hi, lo):
            assert np.array_equal(p.astype(np.float16).astype(np.float64), p)
        # flush model: only values below the smallest normal change
        fh, fl = R.split_f16(v, shift, flush=True)
        assert np.array_equal(fh[np.abs(hi) >= 2.0 ** -14], hi[np.abs(hi) >= 2.0 ** -14])
        assert np.all(fh[np.abs(hi) < 2.0 ** -14] == 0) and np.all(np.abs(fl[fl != 0]) >= 2.0 ** -14)
    # beyond the range: hi clamps, lo carries the unclamped residual (fp16-accurate to twice the range)
    hi, lo = R.split_f16(np.float32([70000.0 / 16, 131000.0 / 16]), 4)
    assert hi.tolist() == [65504.0, 65504.0] and abs(lo[0] - (70000 - 65504)) <= 2 and abs(lo[1] - (131000 - 65504)) <= 32
    # bf16 pair: 2^-17 |v| over fp32's range (a half-ulp argument: |v - hi| <= 2^-8 * 2^e, |r - lo| <= 2^-17 * 2^e)
    exps = np.arange(-100, 100)
    v = (rng.uniform(1, 2, size=(exps.size, 2048)) * 2.0 ** exps[:, None]).astype(np.float32).ravel()
    v = np.concatenate([v, -v, np.float32(2.0) ** exps, np.float32((1 + 2.0 ** -8)) * np.float32(2.0) ** exps])
    hi, lo = R.split_bf16_pair(v)
    err = np.abs(v.astype(np.float64) - hi - lo)
    assert np.all(err <= 2.0 ** -17 * np.abs(v)) and np.array_equal(err <= R.delta(v, ("bf16",)), np.ones(v.shape, bool))
    assert float((err / np.abs(v)).max()) > 2.0 ** -18, "2^-18 would be too tight a statement: it is reached"
    w = R.pair_words(v).view(torch.int32)
    assert np.array_equal(((w & -65536).view(torch.float32).double() + (w << 16).view(torch.float32).double()).numpy(), hi + lo)


@pytest.mark.parametrize("gemm", GEMMS)
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("fam", R.EXACT)
def test_exact_families_are_exact_for_the_shapes_used(fam, gemm, mode):
    """every product and every partial sum, in any order, is a whole number of quanta below 2^24: fp32 adds them exactly"""
    worst = 0.0
    # the stream-K shapes serve the split tap-GEMMs only
    shapes = R.EDGE_SHAPES + (R.STREAMK_SHAPES if gemm != "wgrad" and mode != "f32" else [])
    for shape in shapes:
        f, fa, fw, mm, n, bias, kw = _case(fam, gemm, mode, shape)
        ah, al, sa = R.split(f["act"], fa)
        wh, wl, sw = R.split(f["wgt"], fw)
        a64, w64 = f["act"].astype(np.float64), f["wgt"].astype(np.float64)
        assert np.array_equal(ah + al, a64 * 2.0 ** sa) and np.array_equal(wh + wl, w64 * 2.0 ** sw), "pairs must be exact"
        if fam == "E4" and fa is not None:
            assert np.any(al != 0) and np.any(wl != 0), "both planes must be live"
        elif fa is not None:
            assert not np.any(al) and not np.any(wl)
        want = R.three_term(mm, f["act"], f["wgt"], fa, fw, bias)
        q = f["quantum"]
        # sum of |terms| (planes taken absolutely) bounds every partial sum of every order
        A = [np.abs(t) * 2.0 ** -s for t, s in ((ah, sa), (al, sa))]
        W = [np.abs(t) * 2.0 ** -s for t, s in ((wh, sw), (wl, sw))]
        tot = mm(R._t64(A[0]), R._t64(W[0])) + mm(R._t64(A[0]), R._t64(W[1])) + mm(R._t64(A[1]), R._t64(W[0]))
        if fa is None:
            tot = mm(R._t64(np.abs(a64)), R._t64(np.abs(w64)))
        if bias is not None:
            tot = tot + torch.from_numpy(np.abs(bias).astype(np.float64))
        quanta = float(tot.max()) / q
        worst = max(worst, quanta)
        # (the masked weight-gradient forms double x -- a keep mask with 1 / (1 - p) = 2: twice the quanta at most)
        assert quanta * (2 if gemm == "wgrad" else 1) < 2.0 ** 24, (shape, quanta)
        wq = (want / q).numpy()
        assert np.array_equal(wq, np.round(wq)), shape
        assert torch.equal(want.float().double(), want), shape
        if fam != "E4" or fa is None:
            assert torch.equal(want, R.reference(mm, f["act"], f["wgt"], bias)), shape
        else:       # the dropped lo lo' is real: the three-term value is NOT the float64 product
            assert not torch.equal(want, R.reference(mm, f["act"], f["wgt"], bias)), shape
        if fam == "E4":
            nz = mm(R._t64((a64 != 0).astype(np.float64)), R._t64((w64 != 0).astype(np.float64)))
            assert float(nz.max()) <= 8, (shape, float(nz.max()))
    print("%s %s %s: largest sum of |terms| = 2^%.1f quanta" % (fam, gemm, mode, np.log2(max(worst, 1.0))))


def _drop_one_tap(gemm, f, shape):
    """defect model: the lo plane of ONE tap is lost -- tap 0 of the weight image (fwd / dgrad); for the weight gradient,
    whose taps share one activation tensor, the lo plane of g in batch item 0 (one slab's worth)"""
    m = np.zeros(f["wgt"].shape if gemm != "wgrad" else f["act"].shape, bool)
    if gemm == "wgrad":
        m[0] = True
        return ("act", m)
    m[:, :, 0] = True
    return ("wgt", m)


@pytest.mark.parametrize("gemm", GEMMS)
@pytest.mark.parametrize("mode", MODES)
def test_emulated_kernel_stays_inside_the_bound_and_defects_do_not(gemm, mode):
    fa, fw = R.forms(gemm, mode)
    for fam in R.EXACT + R.BOUNDED:
        worst, worst_flush, worst_drop = 0.0, 0.0, 0.0
        inexact_flush = inexact_drop = False
        for si, shape in enumerate(EMU_SHAPES):
            f, fa, fw, mm, n, bias, kw = _case(fam, gemm, mode, shape)
            ref = R.reference(mm, f["act"], f["wgt"], bias)
            bnd, op, acc = R.bound(mm, f["act"], f["wgt"], fa, fw, n, bias)
            got = R.emulate(gemm, f["act"], f["wgt"], fa, fw, addend=bias, seed=si, **kw)
            drop = _drop_one_tap(gemm, f, shape)
            if fam in R.EXACT:
                want = R.three_term(mm, f["act"], f["wgt"], fa, fw, bias)
                assert torch.equal(got, want), (fam, shape)
                if fa is not None and fa[0] == "f16" and fam == "E2":
                    inexact_flush |= not torch.equal(
                        R.emulate(gemm, f["act"], f["wgt"], fa, fw, addend=bias, flush=True, seed=si, **kw), want)
                if fa is not None and fam == "E4":
                    inexact_drop |= not torch.equal(
                        R.emulate(gemm, f["act"], f["wgt"], fa, fw, addend=bias, drop_lo=drop, seed=si, **kw), want)
                if fam != "E4":
                    continue            # E4 also has a bound to keep: its reference is the float64 product
            worst = max(worst, assert_close_elementwise(got, ref, 0, bnd, "%s %s %s %s" % (fam, gemm, mode, shape)))
            if fa is None or fam not in R.SMALL_MAGNITUDE:
                continue
            with np.errstate(divide="ignore", invalid="ignore"):
                if fa[0] == "f16":
                    bad = R.emulate(gemm, f["act"], f["wgt"], fa, fw, addend=bias, flush=True, seed=si, **kw)
                    r = float(((bad - ref).abs() / bnd).max())
                    worst_flush = r if worst_flush == 0.0 else min(worst_flush, r)   # EVERY shape must catch it
                if shape in ONE_TAP_SHAPES:
                    bad = R.emulate(gemm, f["act"], f["wgt"], fa, fw, addend=bias, drop_lo=drop, seed=si, **kw)
                    r = float(((bad - ref).abs() / bnd).max())
                    worst_drop = r if worst_drop == 0.0 else min(worst_drop, r)      # each of them must catch it
        line = "%s %s %s: emulated worst ratio %.3f" % (fam, gemm, mode, worst)
        if fam in R.EXACT:
            line += " (bit-exact)"
        assert worst < 1.0
        if fa is not None and fam == "E2" and fa[0] == "f16":
            assert inexact_flush
            line += "; flushed: inexact"
        if fa is not None and fam == "E4":
            assert inexact_drop
            line += "; one tap's lo lost: inexact"
        if fa is not None and fam in R.SMALL_MAGNITUDE:
            if fa[0] == "f16":
                assert worst_flush >= 2.0, (fam, worst_flush)
                line += "; flushed %.1f x (least over the shapes)" % worst_flush
            assert worst_drop >= 2.0, (fam, worst_drop)
            line += "; one tap's lo lost %.1f x (least over the 1 x 1 shapes)" % worst_drop
        print(line)


def test_small_magnitude_edge_shapes_keep_the_operand_term_visible():
    """the GPU test's own shapes: for B2 / B3 in the default mode's forward, flushed fp16 subnormals leave the bound by
    >= 2 x on the edge shapes with K * J <= 192 (three_term as the kernel: exact accumulation, so only the operands differ)"""
    for fam in R.SMALL_MAGNITUDE:
        for shape in [s for s in R.EDGE_SHAPES if s[1] * s[3] <= 192]:
            f, fa, fw, mm, n, bias, kw = _case(fam, "fwd", "f16x3", shape)
            ref = R.reference(mm, f["act"], f["wgt"], bias)
            bnd = R.bound(mm, f["act"], f["wgt"], fa, fw, n, bias)[0]
            ok = R.three_term(mm, f["act"], f["wgt"], fa, fw, bias)
            bad = R.three_term(mm, f["act"], f["wgt"], fa, fw, bias, flush=True)
            r_ok, r_bad = float(((ok - ref).abs() / bnd).max()), float(((bad - ref).abs() / bnd).max())
            print("%s %s: IEEE %.3f, flushed %.1f x the bound" % (fam, shape, r_ok, r_bad))
            assert r_ok < 1.0 and r_bad >= 2.0, (fam, shape, r_ok, r_bad)

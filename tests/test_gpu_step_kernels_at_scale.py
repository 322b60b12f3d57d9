# coding: utf-8
"""The training step's non-GEMM kernels at the bench's B = 64 shapes, against float64 references.

Every kernel here switches to another code path once its input passes a size threshold: a persistent tile walk
(spec_loss_tiled_kernel), grid-stride loops over a capped grid (spec_loss_kernel, guided_attn_kernel,
sqnorm_partial_kernel), several EMB_RANGE passes over one LDS list (embedding_bct_bwd_kernel), the two-stage position-rate
gradient (sincos_pos_bwd_part / _finish), the fused attention forward at 64 KiB of LDS against the unfused softmax.  Each
scale case restates the kernel's threshold formula and asserts that its shape crosses it, so an edit to the shapes can
not silently drop that coverage.

References: the oracle (oracle/dv3_oracle.py, pinned to the reference by tests/golden) evaluated in float64 from the
same fp32 inputs, or a float64 restatement of the reference's expression where the oracle has none.  Element-wise bounds
(tests.util.assert_close_elementwise) are derived from each kernel's arithmetic; a reduced scalar is held to
|got - ref| <= k * 2^-24 * sum|terms| with k its summation depth plus the roundings around it.  Each bound states its
reasoning in one comment line.  u = 2^-24 is the fp32 unit roundoff; an op documented to "1 ulp" errs by <= 2u."""
import math
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tests.util import assert_close_elementwise  # noqa: E402
from oracle import dv3_oracle as O  # noqa: E402

pytestmark = pytest.mark.gpu

U = 2.0 ** -24


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


def _cdiv(a, b):
    return -(-a // b)


def _report(name, ratio):
    print("worst-ratio %-58s %.4g" % (name, ratio))


def _close(got, want, rtol, atol, what):
    _report(what, assert_close_elementwise(got, want, rtol, atol, what))


def _scalar_close(got, want, bound, what):
    got, want, bound = float(got), float(want), float(bound)
    assert abs(got - want) <= bound, "%s: got %r want %r (|err| %.3g > bound %.3g)" % (what, got, want, abs(got - want),
                                                                                         bound)
    _report(what, abs(got - want) / bound if bound > 0 else 0.0)


def _bits_equal(a, b):
    return torch.equal(a.view(torch.int32), b.view(torch.int32))


# ------------------------------------------------------------------------------------------------------------------
# 1. spec_loss / spec_loss_with_grad (csrc/loss.hip)
# ------------------------------------------------------------------------------------------------------------------
def _spec_launch(B, T, D, r, yh_strides, y_strides):
    """-> (tiled, n_blocks, terms per thread) as dv3_spec_loss_f32 chooses them (loss.hip:320-336)"""
    yh_bs, yh_ts, yh_ds = yh_strides
    y_bs, y_ts, y_ds = y_strides
    tiled = yh_ts == 1 and y_ds == 1 and yh_ds > 1 and y_ts > 1                   # loss.hip:325
    if tiled:
        nt = B * _cdiv(T - r, 64) * _cdiv(D, 64)
        nb = min(nt, 1024)                                                         # loss.hip:329
        return True, nb, nt, _cdiv(nt, nb) * 16                                    # 64 x 64 / 256 per tile per thread
    n = B * (T - r) * D
    nb = min(max(_cdiv(n, 256 * 4), 1), 1024)                                      # loss_blocks, loss.hip:299-304
    return False, nb, n, _cdiv(n, nb * 256)


def _spec_inputs(B, T, D, seed, saturate=True):
    rng = np.random.RandomState(seed)
    yh = rng.rand(B, T, D).astype(np.float32)
    y = rng.rand(B, T, D).astype(np.float32)
    if saturate:
        # sigmoid-saturated predictions: exact 0 / 1 and within 1e-7 of them (the binary-divergence gradient is ~1e8 there)
        special = np.array([0.0, 1.0, 5e-8, 1e-7, 1 - 2.0 ** -24, 1 - 1e-7], dtype=np.float32)
        flat = yh.reshape(-1)
        sel = rng.rand(flat.size) < 0.02
        flat[sel] = special[rng.randint(0, len(special), int(sel.sum()))]
        # targets in {0, 1} and in between; some equal to the prediction (|diff| = 0: sign 0)
        ty = y.reshape(-1)
        sel = rng.rand(ty.size) < 0.2
        ty[sel] = np.round(ty[sel])
        sel = rng.rand(ty.size) < 0.01
        ty[sel] = flat[sel]
    return torch.from_numpy(yh), torch.from_numpy(y)


def _t_valid_eff(T, r, tv):
    """spec_t_valid (loss.hip:46-51)"""
    if tv is None or tv >= T:
        return T
    return tv if tv > r else r + 1


def _spec_reference(yh32, y32, lengths, r, wm, wbd, tv, fast_log):
    """O.spec_loss (train.py:547-582) in float64 on y_hat[:, :tv - r] / y[:, r:tv] with the mask sequence_mask(lengths,
    tv)[:, r:] (train.py:261-271, 676-681), its autograd gradient, and the per-term / per-element error bounds of the
    kernel's fp32 arithmetic."""
    B, T, D = yh32.shape
    tve = _t_valid_eff(T, r, tv)
    yh = yh32.detach().cpu().double().contiguous().requires_grad_(True)
    y = y32.detach().cpu().double()
    a_, b_ = yh[:, :tve - r], y[:, r:tve]
    mask = O.sequence_mask(lengths.long().cpu(), tve)[:, r:].unsqueeze(-1).double() if wm > 0 else None
    l1, bd = O.spec_loss(a_, b_, mask, wm, wbd)
    bd = bd.reshape(())
    total = (1 - wbd) * l1 + wbd * bd
    total.backward()
    with torch.no_grad():
        n = a_.numel()
        if wm > 0:
            msum = float(mask.expand_as(a_).sum())
            coef = (1 - wm) / n + wm * mask.expand_as(a_) / msum
        else:
            msum = None
            coef = torch.full_like(a_, 1.0 / n)
        x, t = a_.detach(), b_
        ad = (x - t).abs()
        eps = 1e-8
        A, Bb = x + eps, 1 - x + eps
        la, lb, lab = torch.log(A), torch.log(Bb), torch.log(A + Bb)
        z = -t * (la - lb) + (lab - lb)
        # one logarithm: its argument's rounding (a: u; b = (1 - x) + eps: 2u; a + b: 3u) is an absolute error, plus
        # the log itself: libm logf <= 1 ulp (2u |log|); v_log_f32 (loss.hip:37-40) 1 ulp of log2 x, times LN2 (u), plus
        # an absolute 2^-22 near x = 1 where log2 x -> 0 and the hardware's ulp is that of its internal fixed point
        lrel, labs = (3 * U, 2.0 ** -22) if fast_log else (2 * U, 0.0)
        dla, dlb, dlab = U + lrel * la.abs() + labs, 2 * U + lrel * lb.abs() + labs, 3 * U + lrel * lab.abs() + labs
        Ez = t.abs() * (dla + dlb) + dlab + dlb + U * (2 * (t * (la - lb)).abs() + (lab - lb).abs() + z.abs())
        # gradient: dz = (a * rcp(a + b) - y) * (rcp a + rcp b) (loss.hip:42-43); v_rcp_f32 is 1 ulp (2u)
        s1 = A / (A + Bb)
        T2 = 1 / A + 1 / Bb
        dz = (s1 - t) * T2
        Edz = T2 * 7 * U * (s1.abs() + (s1 - t).abs()) + 6 * U * dz.abs()
        # coef = (1-wm) * fp32(1/n) + wm / msum * m: n and msum converted to float (u each), 1/n, * (1-wm), wm/msum, +
        ec = 4 * U
        Gabs = coef * ((1 - wbd) + wbd * dz.abs())
        Eg = coef * ((1 - wbd) * 2 * U + wbd * Edz) + (ec + 5 * U) * Gabs
        # pad the per-element gradient bound back to (B, T, D): frames >= tv - r have gradient 0 exactly
        Eg_full = torch.zeros_like(yh)
        Eg_full[:, :tve - r] = Eg
        S_l1 = float((coef * ad).sum())
        S_z = float((coef * z).sum())
        S_Ez = float((coef * Ez).sum())
    return dict(l1=float(l1.detach()), bd=float(bd.detach()), total=float(total.detach()), grad=yh.grad, msum=msum, S_l1=S_l1, S_z=S_z,
                S_Ez=S_Ez, Eg=Eg_full, n=n)


# (B, T, D, layout, r, wm, wbd, t_valid, scale): layout 'bct' = a transposed view of a BCT prediction against a BTC
# target (the tiled kernel), 'btc' = both contiguous (the flat kernel).  scale: the case exists for its threshold.
SPEC_CASES = [
    # the bench step's linear loss: 64 x 13 x 9 = 7488 tiles; the last D tile is one column wide
    ("lin_full", 64, 800, 513, "bct", 1, 0.5, 0.1, None, True),
    ("mel_full", 64, 200, 80, "bct", 1, 0.5, 0.1, None, False),
    ("mel_btc", 64, 200, 80, "btc", 1, 0.5, 0.1, None, True),
    # edge shapes past the persistent-grid threshold at a lower CPU cost
    ("tiled_T130_D65", 200, 131, 65, "bct", 1, 1.0, 0.1, None, True),         # T - r = 130 (not a multiple of 64)
    ("tiled_D63_r4", 1030, 9, 63, "bct", 4, 0.5, 0.1, None, True),
    ("tiled_Tr1_D65", 1100, 5, 65, "bct", 4, 0.0, 0.1, None, True),           # T - r = 1
    ("tiled_D513_r4_tvalid", 60, 69, 513, "bct", 4, 0.5, 0.1, 40, True),
    ("tiled_tvalid_r1", 300, 101, 65, "bct", 1, 0.5, 0.0, 2, True),            # t_valid = r + 1
    ("flat_D1", 64, 1101, 1, "bct", 1, 0.5, 0.1, 700, True),                   # D = 1 takes the flat kernel
    ("flat_D65_r4", 300, 70, 65, "btc", 4, 1.0, 0.1, 5, True),                 # t_valid = r + 1
    ("flat_D63", 200, 130, 63, "btc", 1, 0.0, 0.0, None, True),
]


def _spec_lengths(B, T, r, seed):
    rng = np.random.RandomState(seed + 1)
    lens = rng.randint(0, T + 30, B)
    # 0, <= r, exactly T, > T, and at least one non-empty mask
    lens[:5] = [0, r, T, T + 17, max(r + 2, T // 2)]
    return torch.from_numpy(lens.astype(np.int32))


def _make_layout(t, layout, dev):
    t = t.to(dev)
    if layout == "bct":
        return t.transpose(1, 2).contiguous().transpose(1, 2)       # (B, T, D) view of BCT memory
    return t.contiguous()


def _check_spec(name, out4, grad, ref, launch, wm, wbd, gs=1.0):
    tiled, nb, _, per = launch
    depth = per + 6 + 3 + _cdiv(nb, 256) + 6 + 3        # thread serial sum, wave butterfly, 4 waves, finish kernel
    k = depth + 10                                       # + n, msum to float, the divisions and the weighted mixes
    o = out4.detach().cpu().double()
    _scalar_close(o[0], ref["l1"], k * U * ref["S_l1"], name + " l1")
    if wbd > 0:
        _scalar_close(o[1], ref["bd"], k * U * ref["S_z"] + ref["S_Ez"], name + " bd")
    b_tot = (1 - wbd) * k * U * ref["S_l1"] + wbd * (k * U * ref["S_z"] + ref["S_Ez"]) + \
        3 * U * ((1 - wbd) * ref["l1"] + wbd * ref["bd"])
    _scalar_close(o[2], ref["total"], b_tot, name + " total")
    if wm > 0:      # the mask sum is an integer count times D: exact below 2^24, one rounding above
        _scalar_close(o[3], ref["msum"], U * ref["msum"], name + " mask sum")
    # per-element gradient bound of the kernel's arithmetic (see _spec_reference); gs: autograd's dout multiply (u)
    _close(grad, ref["grad"] * gs, 0.0, ref["Eg"] * abs(gs) * (1 + U) + U * (ref["grad"] * gs).abs(), name + " grad")


@pytest.mark.parametrize("case", SPEC_CASES, ids=[c[0] for c in SPEC_CASES])
def test_spec_loss_at_scale(dev, case):
    from deepvoice3_pytorch_amd import ops, _lib
    name, B, T, D, layout, r, wm, wbd, tv, scale = case
    yh32, y32 = _spec_inputs(B, T, D, seed=B + T + D)
    lens = _spec_lengths(B, T, r, seed=B + T)
    yh = _make_layout(yh32, layout, dev)
    y = y32.to(dev).contiguous()
    launch = _spec_launch(B, T, D, r, yh.stride(), y.stride())
    tiled, nb, n_work, per = launch
    if scale:
        if tiled:       # persistent grid: B * ceil((T-r)/64) * ceil(D/64) tiles > 1024 blocks (loss.hip:138, :329)
            assert n_work > 1024 and per > 16, (n_work, per)
        else:           # grid-stride loop with more than one element per thread (loss.hip:78-79, :299-304)
            assert per > 1, (n_work, nb)
    assert tiled == (layout == "bct" and D > 1)
    tv_t = torch.tensor([tv], dtype=torch.int32, device=dev) if tv is not None else None
    lens_d = lens.to(dev) if wm > 0 else None
    modes = (1, 0) if tiled and wbd > 0 else (1,)
    refs = {}
    for fast in modes:
        with _lib.switches({"DV3_SW_LOSS_FAST_LOG": fast}):
            if fast not in refs:
                refs[fast] = _spec_reference(yh32, y32, lens, r, wm, wbd, tv, fast_log=bool(fast) and tiled)
            out4, g = ops.spec_loss_with_grad(yh, y, lens_d, r, wm, wbd, t_valid=tv_t)
            torch.cuda.synchronize()
            assert g.stride() == yh.stride()
            _check_spec("%s[log=%s]" % (name, "fast" if fast else "libm"), out4, g, refs[fast], launch, wm, wbd)
            # determinism: a second identical call returns the same bits (no float atomics)
            out4b, gb = ops.spec_loss_with_grad(yh, y, lens_d, r, wm, wbd, t_valid=tv_t)
            assert _bits_equal(out4, out4b) and _bits_equal(g, gb), name


def test_spec_loss_autograd_gscale(dev):
    """the autograd form: d total / d y_hat scaled by the upstream gradient (gscale != 1), tiled kernel past 1024 tiles"""
    from deepvoice3_pytorch_amd import ops
    B, T, D, r, wm, wbd, gs = 200, 131, 65, 1, 0.5, 0.1, -0.37
    yh32, y32 = _spec_inputs(B, T, D, seed=5)
    lens = _spec_lengths(B, T, r, seed=5)
    yh = _make_layout(yh32, "bct", dev).requires_grad_(True)
    y = y32.to(dev)
    launch = _spec_launch(B, T, D, r, yh.stride(), y.stride())
    assert launch[0] and launch[2] > 1024
    out4 = ops.spec_loss(yh, y, lens.to(dev), r, wm, wbd)
    out4.backward(torch.tensor([0.0, 0.0, gs, 0.0], device=dev))
    ref = _spec_reference(yh32, y32, lens, r, wm, wbd, None, fast_log=True)
    _check_spec("autograd_gscale", out4, yh.grad, ref, launch, wm, wbd, gs=gs)


def test_spec_loss_priority_band(dev):
    """the priority-band pass as train_step.py:394-396 issues it: lin[:, :, :n_pri] against y[:, :, :n_pri], w_bd = 0
    (neither slice is dense: both are copied to BTC and take the flat kernel)"""
    from deepvoice3_pytorch_amd import ops
    B, T, D, r, wm = 16, 300, 513, 1, 0.5
    n_pri = int(3000 / (22050 * 0.5) * D)
    yh32, y32 = _spec_inputs(B, T, D, seed=11)
    lens = _spec_lengths(B, T, r, seed=11)
    lin = _make_layout(yh32, "bct", dev)
    y = y32.to(dev)
    ys, ls = y[:, :, :n_pri], lin[:, :, :n_pri]
    launch = _spec_launch(B, T, n_pri, r, ls.contiguous().stride(), ys.contiguous().stride())
    assert not launch[0] and launch[3] > 1
    out4, g = ops.spec_loss_with_grad(ls, ys, lens.to(dev), r, wm, 0.0)
    ref = _spec_reference(yh32[:, :, :n_pri], y32[:, :, :n_pri], lens, r, wm, 0.0, None, fast_log=False)
    _check_spec("priority_band", out4, g, ref, launch, wm, 0.0)


# ------------------------------------------------------------------------------------------------------------------
# 2. guided attention loss (loss.hip:219-251), L x 64 x 200 x 150
# ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("g", [0.2, 0.4])
@pytest.mark.parametrize("valid", [False, True])
def test_guided_attention_at_scale(dev, g, valid):
    from deepvoice3_pytorch_amd import ops
    L, B, Tq, Tk = 2, 64, 200, 150
    per = B * Tq * Tk
    nb = min(max(_cdiv(per, 1024), 1), 1024)
    assert per > 1024 * 256 and nb == 1024          # grid-stride over B*Tq*Tk on a capped grid (loss.hip:233, :299-304)
    rng = np.random.RandomState(int(g * 10) + valid)
    attn32 = torch.from_numpy(rng.rand(L, B, Tq, Tk).astype(np.float32))
    in_len = rng.randint(1, Tk + 1, B)
    out_len = rng.randint(1, Tq + 1, B)
    in_len[:3], out_len[:3] = [1, Tk, 37], [Tq, 1, 129]
    if valid:       # a batch padded beyond its own maxima (ValidLengths): the mean runs over those maxima
        in_len, out_len = np.minimum(in_len, 121), np.minimum(out_len, 170)
        in_len[1], out_len[0] = 121, 170
    il, ol = torch.from_numpy(in_len.astype(np.int32)), torch.from_numpy(out_len.astype(np.int32))
    W = torch.from_numpy(O.guided_attentions(in_len, out_len, Tq, Tk, g)).double()      # fp32 W, train.py:585-601
    a64 = attn32.double()
    if valid:
        tqv, tkv = int(out_len.max()), int(in_len.max())
        n = L * B * tqv * tkv
        tq_t = torch.tensor([tqv], dtype=torch.int32, device=dev)
        tk_t = torch.tensor([tkv], dtype=torch.int32, device=dev)
    else:
        n, tq_t, tk_t = L * B * Tq * Tk, None, None
    terms = a64 * W
    want = float(terms.sum()) / n
    # depth: per-thread serial sum (ceil(per / (nb*256)) items x L layers), wave (6), 4 waves (3), finish (nb/256 + 9);
    # + attn * fp32(W) (u), * fp32(1/n) (2u: 1/n and the product); W itself is the fp64 -> fp32 cast of train.py
    k = _cdiv(per, nb * 256) * L + 6 + 3 + _cdiv(nb, 256) + 9 + 3
    at = attn32.to(dev)
    for fn in ("grad", "autograd"):
        if fn == "grad":
            out1, dattn = ops.guided_attention_loss_with_grad(at, il.to(dev), ol.to(dev), g, tq_t, tk_t)
        else:
            a = at.clone().requires_grad_(True)
            out1 = ops.guided_attention_loss(a, il.to(dev), ol.to(dev), g, tq_t, tk_t)
            out1.backward()
            dattn = a.grad
        _scalar_close(out1[0].cpu(), want, k * U * float(terms.abs().sum()) / n, "guided g=%g valid=%d %s loss" % (g, valid, fn))
        # gradient = fp32(W) / n: W may differ by 1 ulp (2u: the kernel's g is the fp32 0.2f), fp32(1/n), the product: 4u
        _close(dattn, (W / n).expand(L, B, Tq, Tk), 4 * U, 0.0, "guided g=%g valid=%d %s grad" % (g, valid, fn))
    out1b, dattnb = ops.guided_attention_loss_with_grad(at, il.to(dev), ol.to(dev), g, tq_t, tk_t)
    out1c, dattnc = ops.guided_attention_loss_with_grad(at, il.to(dev), ol.to(dev), g, tq_t, tk_t)
    assert _bits_equal(out1b, out1c) and _bits_equal(dattnb, dattnc)


# ------------------------------------------------------------------------------------------------------------------
# 3. BCE of the done flags (loss.hip:277-297), (64, 200, 1)
# ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("valid", [False, True])
def test_bce_at_scale(dev, valid):
    from deepvoice3_pytorch_amd import ops
    B, T = 64, 200
    rng = np.random.RandomState(17 + valid)
    p = rng.rand(B, T, 1).astype(np.float32)
    t = (rng.rand(B, T, 1) < 0.3).astype(np.float32)
    t[:, ::7] = rng.rand(B, _cdiv(T, 7), 1)             # targets in between too
    special = np.array([0.0, 1.0, 1e-30, 1 - 2.0 ** -24], dtype=np.float32)
    sel = rng.rand(B, T, 1) < 0.05
    p[sel] = special[rng.randint(0, 4, int(sel.sum()))]
    p[0, :4, 0], t[0, :4, 0] = special, [1, 0, 1, 0]     # log clamped at -100 (p = 0, 1) and the 1e-12 gradient clamp
    p32, t32 = torch.from_numpy(p), torch.from_numpy(t)
    tv = 150 if valid else T
    pr = p32[:, :tv].double().requires_grad_(True)
    loss = F.binary_cross_entropy(pr, t32[:, :tv].double())      # torch's own -100 log clamp and 1e-12 denominator
    loss.backward()
    grad = torch.zeros(B, T, 1, dtype=torch.float64)
    grad[:, :tv] = pr.grad
    x, y = pr.detach(), t32[:, :tv].double()
    # one term: logf (<= 1 ulp: 2u |log|) of x or of fp32(1 - x) (an absolute u), * y, the add, the sign: + (1 - y) u
    lx, l1x = torch.clamp(torch.log(x), min=-100), torch.clamp(torch.log1p(-x), min=-100)
    mag = (y * lx).abs() + ((1 - y) * l1x).abs()
    n = x.numel()
    nb = min(max(_cdiv(B * T, 1024), 1), 1024)
    k = _cdiv(B * T, nb * 256) + 6 + 3 + _cdiv(nb, 256) + 9 + 2 + 4     # depth + 1/n, * + per-term 2u|log| + 2 ops
    bound = (k * U * float(mag.sum()) + U * float((1 - y).sum())) / n
    pd = p32.to(dev)
    tv_t = torch.tensor([tv], dtype=torch.int32, device=dev) if valid else None
    out1, dp = ops.bce_loss_with_grad(pd, t32.to(dev), tv_t)
    _scalar_close(out1[0].cpu(), float(loss), bound, "bce valid=%d loss" % valid)
    # gradient (x - y) / max((1 - x) x, 1e-12f) / n: x - y, 1 - x, * x, 1e-12f, the division, fp32(1/n), two products: 8u
    _close(dp, grad, 8 * U, 0.0, "bce valid=%d grad" % valid)
    a = pd.clone().requires_grad_(True)
    out2 = ops.bce_loss(a, t32.to(dev), tv_t)
    out2.backward()
    assert _bits_equal(out2, out1) and _bits_equal(a.grad, dp)


# ------------------------------------------------------------------------------------------------------------------
# 4. embedding_bct forward / backward (elementwise.hip:483-597)
# ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("C,same_id,p", [(256, False, 0.0), (300, False, 0.05), (256, True, 0.05)])
def test_embedding_at_scale(dev, C, same_id, p):
    from deepvoice3_pytorch_amd import ops
    B, T, V = 64, 150, 149
    EMB_RANGE = 4096
    assert B * T > EMB_RANGE       # the index list is built in ceil(B*T / EMB_RANGE) passes (elementwise.hip:544, :559)
    rng = np.random.RandomState(C + same_id)
    idx = rng.randint(1, V, (B, T))
    lens = rng.randint(1, T + 1, B)
    lens[:2] = [1, T]
    for b in range(B):
        idx[b, lens[b]:] = 0                              # padding id 0 at ragged tails
    if same_id:
        idx[:] = 7                                        # every position holds one id: a full LDS list in every pass
    idx_t = torch.from_numpy(idx)
    W32 = torch.from_numpy(rng.randn(V, C).astype(np.float32))
    dout32 = torch.from_numpy(rng.randn(B, C, T).astype(np.float32))
    training = p > 0
    ops.dropout_state.manual_seed(1234)
    ops.dropout_state.record = {}
    try:
        wg = W32.to(dev).requires_grad_(True)
        out = ops.embedding_bct(idx_t.to(dev), wg, p, training, padding_idx=0, site="emb")
        out.backward(dout32.to(dev))
        rec = ops.dropout_state.record.get("emb")
    finally:
        ops.dropout_state.record = None
    if training:
        bits, rows, TT = rec
        keep = torch.from_numpy(O.unpack_keep_bits(bits.cpu().numpy().view(np.uint32), rows, _cdiv(TT, 32), TT))
        keep = keep.view(B, C, T).double()
        assert abs(float(keep.mean()) - (1 - p)) < 0.01
    else:
        keep = torch.ones(B, C, T, dtype=torch.float64)
    # fp64 restatement of nn.Embedding(padding_idx=0) + F.dropout (deepvoice3.py:266-268 of the reference)
    w64 = W32.double().requires_grad_(True)
    ref = F.embedding(idx_t, w64, padding_idx=0).transpose(1, 2) * keep / (1 - p)
    ref.backward(dout32.double())
    # forward: an exact gather times fp32(1/(1-p)) (u) and the product (u)
    _close(out, ref.detach(), 2 * U if training else 0.0, 0.0, "embedding C=%d same=%d fwd" % (C, same_id))
    # backward: a serial sum over the list of each id's positions (count - 1 adds) of dout * fp32(1/(1-p)) (2u)
    counts = torch.bincount(idx_t.view(-1), minlength=V).double()
    counts[0] = 0
    mag = torch.zeros(V, C, dtype=torch.float64)
    mag.index_add_(0, idx_t.view(-1), (dout32.double().abs() * keep / (1 - p)).transpose(1, 2).reshape(-1, C))
    mag[0] = 0
    _close(wg.grad, w64.grad, 0.0, (counts[:, None] + 1) * U * mag, "embedding C=%d same=%d dW" % (C, same_id))
    # determinism
    g1 = wg.grad.clone()
    wg.grad = None
    ops.dropout_state.manual_seed(1234)
    out2 = ops.embedding_bct(idx_t.to(dev), wg, p, training, padding_idx=0, site="emb")
    out2.backward(dout32.to(dev))
    assert _bits_equal(out2, out) and _bits_equal(wg.grad, g1)


# ------------------------------------------------------------------------------------------------------------------
# 5. position encoding with a learnable per-item rate (elementwise.hip:611-706, ops.py:2125-2176)
# ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("T", [200, 150])
@pytest.mark.parametrize("per_item", [True, False])
def test_position_rate_gradient_at_scale(dev, T, per_item):
    from deepvoice3_pytorch_amd import ops
    B, C, n_pos = 64, 256, 1024
    nch = max(1, min(32, (C * T) // 4096))             # ops.py:2170
    assert nch > 1                                     # the rate gradient is split over nch partials per item
    rng = np.random.RandomState(T + per_item)
    table = O.position_encoding_table(n_pos, C, 1.0, sinusoidal=False)       # raw angles, row 0 = padding
    pos = rng.randint(1, n_pos, (B, T))
    pos[:, :3] = [n_pos - 1, 0, 1]                      # max_positions - 1 and a padding position inside the row
    pos[rng.rand(B, T) < 0.05] = 0
    pos_t = torch.from_numpy(pos)
    w32 = torch.from_numpy(rng.uniform(0.2, 2.6, B if per_item else 1).astype(np.float32))
    base32 = torch.from_numpy(rng.randn(B, C, T).astype(np.float32))
    dout32 = torch.from_numpy(rng.randn(B, C, T).astype(np.float32))
    wb = (w32.view(-1, 1).expand(B, 1) if not per_item else w32.view(B, 1))
    tab = table[pos_t]                                                           # (B, T, C) fp32 raw angles
    ang = (wb.view(B, 1, 1) * tab).double()                                      # fp32 product, then exact
    odd = (torch.arange(C) % 2 == 1).view(1, 1, C)
    pad = (pos_t == 0).view(B, T, 1)
    a = tab.double()
    de = torch.where(pad, a, torch.where(odd, -torch.sin(ang) * a, torch.cos(ang) * a))
    if not per_item:
        # the scalar rate sums 64 x C x T terms: with random signs the bound k u sum|terms| dwarfs the value; here every
        # term takes one sign, so that bound is within a small factor of |dw| and a dropped or repeated partial shows
        dout32 = (dout32.abs() * torch.sign(de).transpose(1, 2)).float()
    wd = w32.to(dev).requires_grad_(True)
    out = ops.add_position_encoding(base32.to(dev), pos_t.to(dev), table.to(dev), wd, True)
    out.backward(dout32.to(dev))
    # fp64 restatement of SinusoidalEncoding.forward (modules.py:45-64): the reference computes the angle w * table in
    # fp32 -- that one rounding is repeated here -- then sin (even channels) / cos (odd), row 0 passed through
    enc = torch.where(pad, ang, torch.where(odd, torch.cos(ang), torch.sin(ang)))
    want = base32.double() + enc.transpose(1, 2)
    # sinf / cosf (OCML, <= 2 ulp of a value <= 1: 2^-23 absolute) and the add (u relative)
    _close(out, want, U, 2.0 ** -23, "posenc T=%d per_item=%d fwd" % (T, per_item))
    terms = dout32.double() * de.transpose(1, 2)
    dw_items = terms.sum(dim=(1, 2))
    mag = (dout32.double() * a.transpose(1, 2)).abs().sum(dim=(1, 2))
    per = _cdiv(C * T, nch)
    # per item: trig (2^-23 abs) * a (u), * dout (u): 4u |dout a|; serial thread sum, wave (6), 2 levels, nch partials
    k = 4 + _cdiv(per, 256) + 6 + 2 + nch
    if per_item:
        _close(wd.grad, dw_items, 0.0, k * U * mag, "posenc T=%d per-item dw" % T)
    else:          # + dwb.sum(0) over the B item values (ops.py:2175): torch's order, at most B - 1 levels on those
        _scalar_close(wd.grad[0].cpu(), float(dw_items.sum()),
                      k * U * float(mag.sum()) + (B - 1) * U * float(dw_items.abs().sum()),
                      "posenc T=%d scalar dw" % T)
    g1 = wd.grad.clone()
    wd.grad = None
    out2 = ops.add_position_encoding(base32.to(dev), pos_t.to(dev), table.to(dev), wd, True)
    out2.backward(dout32.to(dev))
    assert _bits_equal(out2, out) and _bits_equal(wd.grad, g1)


# ------------------------------------------------------------------------------------------------------------------
# 6. gradient norm + clip + Adam on a flat arena (optim.hip)
# ------------------------------------------------------------------------------------------------------------------
def _adam_reference_step(st, g, prescale, clip, hyper32, b1, b2, eps, wd, k_norm):
    """one step of O.clip_and_adam (train.py:755-759) in float64 with the data-parallel prescale and weight decay, and a
    first-order error bound of the kernel's fp32 arithmetic carried alongside (Ep, Em, Ev)"""
    p, m, v, Ep, Em, Ev = st
    lr, bc1, bc2s = (float(x) for x in hyper32)
    ge = g * prescale
    total = float(torch.sqrt((ge * ge).sum()))
    c = clip / (total + 1e-6)
    coef = min(1.0, c) if clip > 0 else 1.0
    # coef: the norm (k_norm/2 + 1 u: sqrt of a sum of squares), + 1e-6, the division, * prescale; 0 when not clipped
    ec = (k_norm / 2 + 4) * U if (clip > 0 and c < 1) else 0.0
    gi = ge * coef + wd * p
    Eg = (ec + U) * (ge * coef).abs() + wd * (Ep + 2 * U * p.abs()) + U * gi.abs()     # wd * p and fp32(wd)
    # the kernel's beta constants: beta as fp32 and 1 - fp32(beta) in fp32; the reference's 1 - beta is exact here
    f32 = lambda x: float(np.float32(x))  # noqa: E731
    db1, dc1 = abs(f32(b1) - b1), abs(f32(1 - f32(b1)) - (1 - b1))
    db2, dc2 = abs(f32(b2) - b2), abs(f32(1 - f32(b2)) - (1 - b2))
    m_new = b1 * m + (1 - b1) * gi
    Em = b1 * Em + (1 - b1) * Eg + U * (b1 * m.abs() + (1 - b1) * gi.abs() + m_new.abs()) + db1 * m.abs() + \
        dc1 * gi.abs()
    v_new = b2 * v + (1 - b2) * gi * gi
    Ev = b2 * Ev + (1 - b2) * 2 * gi.abs() * Eg + U * (b2 * v + 2 * (1 - b2) * gi * gi + v_new) + db2 * v + dc2 * gi * gi
    sv = torch.sqrt(v_new)
    denom = sv / bc2s + eps
    # sqrt (u) of v +- Ev, / bc2s (u), + eps (u)
    Esv = torch.minimum(Ev / (2 * sv).clamp_min(1e-300), torch.sqrt(Ev)) + U * sv
    Ed = Esv / bc2s + U * sv / bc2s + U * denom + U * eps       # and fp32(eps)
    step = lr / bc1
    upd = step * m_new / denom
    # step = lr / bc1 (u), m / denom (u), * (u)
    Eu = step * (Em / denom + m_new.abs() * Ed / denom ** 2) + 3 * U * upd.abs()
    p_new = p - upd
    Ep = Ep + Eu + U * p_new.abs()
    return [p_new, m_new, v_new, Ep, Em, Ev], total


@pytest.mark.parametrize("n", [3 * 2 ** 22 + 3, 1, 3, 4, 5])
def test_grad_norm_and_clip_adam(dev, n):
    from deepvoice3_pytorch_amd import ops
    nb = min(max(_cdiv(n, 256 * 4 * 8), 1), 1024)       # optim.hip:83-85, the Trainer's 1024 partials (train_step.py:214)
    if n > 1000:
        assert _cdiv(n, 256 * 4 * 8) > 1024 and n % 4 == 3   # capped grid: several strides per thread, and a scalar tail
    per = _cdiv(n // 4, nb * 256)
    # sum of squares: per thread `per` float4s of 4 terms each (4 adds), the tail, wave (6), 4 waves (3), the finish
    # kernel (nb/256 serial, 6, 3), the squares (u)
    k_norm = 4 * per + 1 + 6 + 3 + _cdiv(nb, 256) + 9 + 1
    rng = np.random.RandomState(n % 1000)
    p0 = torch.from_numpy(rng.randn(n).astype(np.float32))
    partial = torch.empty(1024, dtype=torch.float32, device=dev)       # as Trainer.norm_partial
    out2 = torch.zeros(2, dtype=torch.float32, device=dev)
    hyper = torch.empty(3, dtype=torch.float32, device=dev)
    b1, b2, eps, wd, prescale, lr = 0.5, 0.9, 1e-6, 1e-4, 1.0 / 8, 5e-4
    pg, mg, vg = p0.to(dev), torch.zeros(n, device=dev), torch.zeros(n, device=dev)
    z = torch.zeros(n, dtype=torch.float64)
    st = [p0.double(), z.clone(), z.clone(), z.clone(), z.clone(), z.clone()]
    for step in (1, 2, 3):
        g32 = torch.from_numpy((rng.randn(n) * 0.01 * step).astype(np.float32))
        g64 = g32.double()
        norm_avg = math.sqrt(float((g64 * g64).sum())) * prescale
        clip = 0.25 * norm_avg if step != 2 else 4 * norm_avg        # both sides of the clip threshold
        gg = g32.to(dev)
        ops.grad_sqnorm(gg, partial, out2)
        hv = torch.tensor([lr, 1 - b1 ** step, math.sqrt(1 - b2 ** step)], dtype=torch.float32)
        hyper.copy_(hv)
        ops.clip_adam(pg, gg, mg, vg, out2, clip, hyper, b1, b2, eps, weight_decay=wd, grad_prescale=prescale)
        o = out2.cpu().double()
        sq = float((g64 * g64).sum())
        _scalar_close(o[1], sq, k_norm * U * sq, "sqnorm n=%d step %d sum" % (n, step))
        _scalar_close(o[0], math.sqrt(sq), (k_norm / 2 + 1) * U * math.sqrt(sq), "sqnorm n=%d step %d norm" % (n, step))
        st, total = _adam_reference_step(st, g64, prescale, clip, hv, b1, b2, eps, wd, k_norm)
        assert abs(total - norm_avg) <= 1e-12 * norm_avg
        for got, want, err, nm in ((pg, st[0], st[3], "p"), (mg, st[1], st[4], "m"), (vg, st[2], st[5], "v")):
            _close(got, want, 0.0, err, "adam n=%d step %d %s" % (n, step, nm))
        # determinism of the norm
        o2 = torch.zeros(2, dtype=torch.float32, device=dev)
        ops.grad_sqnorm(gg, partial, o2)
        assert _bits_equal(o2, out2)


# ------------------------------------------------------------------------------------------------------------------
# 7. attention core (attention.hip, ops.py:1933-2020)
# ------------------------------------------------------------------------------------------------------------------
def _q16(rng, shape, scale):
    """values on a 1/16 grid with |x| < 2: every product is a multiple of 2^-8 below 4 and every partial sum of 256
    of them is exact in fp32 (and the bf16 / fp16 hi parts of a split operand are the value itself), so the score
    product contributes no rounding and the bounds below are those of the softmax and of the other operand"""
    return torch.from_numpy(np.clip(np.round(rng.randn(*shape) * scale * 16) / 16, -31 / 16, 31 / 16).astype(np.float32))


@pytest.mark.parametrize("Tq,Tk,p", [(200, 150, 0.0), (200, 511, 0.0), (200, 512, 0.0), (197, 511, 0.05)])
def test_attention_core_at_scale(dev, Tq, Tk, p):
    from deepvoice3_pytorch_amd import ops
    B, E = 64, 256
    prev = ops.set_gemm_precision("f16x3")           # the default gemm mode
    try:
        _attention_at_scale(dev, ops, B, E, Tq, Tk, p)
    finally:
        ops.set_gemm_precision(prev)


def _attention_at_scale(dev, ops, B, E, Tq, Tk, p):
    fused = ops.fused_attention and Tk <= 511         # ops.py:1945: the fused forward holds a [32][Tk + 1] score tile
    assert fused == (Tk != 512)                        # in LDS (64 KiB at Tk = 511); from Tk = 512 the unfused softmax
    rng = np.random.RandomState(Tq + Tk)
    q, k, v = _q16(rng, (B, E, Tq), 0.3), _q16(rng, (B, E, Tk), 0.3), _q16(rng, (B, E, Tk), 0.5)
    key_len = rng.randint(1, Tk + 1, B)
    key_len[:2] = [1, Tk]
    kl = torch.from_numpy(key_len.astype(np.int32))
    dctx = _q16(rng, (B, E, Tq), 0.5)
    dP = torch.from_numpy(rng.randn(B, Tq, Tk).astype(np.float32))
    training = p > 0
    ops.dropout_state.manual_seed(99)
    ops.dropout_state.record = {}
    try:
        gin = [t.to(dev).requires_grad_(True) for t in (q, k, v)]
        cg, Pg = ops.attention_core(gin[0], gin[1], gin[2], kl.to(dev), p=p, training=training, site="att")
        torch.autograd.backward([cg, Pg], [dctx.to(dev), dP.to(dev)])
        rec = ops.dropout_state.record.get("att")
    finally:
        ops.dropout_state.record = None
    if training:
        bits, rows, TT = rec
        keep = torch.from_numpy(O.unpack_keep_bits(bits.cpu().numpy().view(np.uint32), rows, _cdiv(TT, 32), TT))
        keep = keep.view(B, Tq, Tk).double()
    else:
        keep = torch.ones(B, Tq, Tk, dtype=torch.float64)
    # fp64 restatement of deepvoice3.py:143-171 (AttentionLayer.forward, as O.attention_layer computes its core)
    q64, k64, v64 = (t.double().requires_grad_(True) for t in (q, k, v))
    S = torch.bmm(q64.transpose(1, 2), k64)
    mask = torch.arange(Tk)[None, :] >= kl.long()[:, None]
    P = F.softmax(S.masked_fill(mask[:, None, :], -float("inf")), dim=-1)
    scale = Tk * math.sqrt(1.0 / Tk)
    pd = P * keep / (1 - p) * scale
    ctx = torch.bmm(pd, v64.transpose(1, 2)).transpose(1, 2)
    torch.autograd.backward([ctx, P], [dctx.double(), dP.double()])
    with torch.no_grad():
        # P: the scores are exact (_q16); s - max (u |s - max|), expf (2u), the row sum of Tk terms (Tk/64 serial + 6)
        # relative to itself, 1/sum (u), the product (u)
        Sm = S.masked_fill(mask[:, None, :], -float("inf"))
        mx = Sm.max(dim=-1, keepdim=True).values
        dS_ = (Sm - mx).abs().masked_fill(mask[:, None, :], 0)
        eP = U * (dS_ + dS_.max(dim=-1, keepdim=True).values + 2 + _cdiv(Tk, 64) + 6 + 4)
        eP_max = float(eP.max())
        name = "attn Tq=%d Tk=%d p=%g" % (Tq, Tk, p)
        # element-wise relative bound wherever P > 1e-3; below that an absolute 1e-3 * eP
        _close(Pg, P, eP, 1e-3 * eP, name + " P")
        # context: Tk products of exact v and pd (pd: eP plus fp32(1/(1-p)), the scale and two products: 4u) on the fp32
        # matrix cores, a sum of depth <= Tk
        e_ctx = eP_max + 4 * U + (Tk + 1) * U
        ctx_abs = torch.bmm(pd, v64.abs().transpose(1, 2)).transpose(1, 2)
        _close(cg, ctx, 0.0, e_ctx * ctx_abs, name + " ctx")
        # gradients (abs chains of the same products): the four products use the bf16 hi+lo split (ops._attn_split):
        # with one operand exact in bf16 (_q16) a product errs by the other's lo rounding, 2^-18; fp32 sums of depth <=
        # max(Tq, Tk); dpd = dctx^T v is exact (_q16 operands); dS = P (dP - sum P dP) by the softmax backward (row sum of
        # Tk terms: Tk/64 + 6 levels, eP on P, 4u on the drop / scale products)
        pds = keep / (1 - p) * scale
        dpd_abs = torch.bmm(dctx.double().abs().transpose(1, 2), v64.abs())
        dPt_abs = dpd_abs * pds + dP.double().abs()
        dS_abs = P * (dPt_abs + (P * dPt_abs).sum(-1, keepdim=True))
        e_dS = 2 * eP_max + (_cdiv(Tk, 64) + 6 + 6) * U
        e_g = 2.0 ** -18 + (max(Tq, Tk) + 1) * U + e_dS
        dq_abs = torch.bmm(k64.abs(), dS_abs.transpose(1, 2))
        dk_abs = torch.bmm(q64.abs(), dS_abs)
        dv_abs = torch.bmm(dctx.double().abs(), pd)
        _close(gin[0].grad, q64.grad, 0.0, e_g * dq_abs, name + " dq")
        _close(gin[1].grad, k64.grad, 0.0, e_g * dk_abs, name + " dk")
        _close(gin[2].grad, v64.grad, 0.0, (2.0 ** -18 + (Tq + 1) * U + eP_max + 4 * U) * dv_abs, name + " dv")

# coding: utf-8
"""-m gpu: the per-item loss kernels (ops.spec_loss_items, ops.bce_loss_items, ops.guided_attention_loss_items;
csrc/loss.hip) row by row against the float64 restatement of tests/item_losses_ref.py on the same fp32 inputs.
Bound per sum: |err| <= 1e-5 |want| -- what tests/test_gpu_kernels.py::test_losses holds the batch kernels to; counts
exact; two calls bit-equal; and the rows recombine to what the batch kernels return at w_masked = 1."""
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tests import item_losses_ref as R  # noqa: E402
from tests.util import load_golden  # noqa: E402

pytestmark = pytest.mark.gpu
TOL = 1e-5


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


def _i32(a, dev):
    return torch.as_tensor(np.asarray(a), dtype=torch.int32).to(dev)


def _check_rows(got, want, n_sums, what):
    got = got.cpu().numpy().astype(np.float64)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    worst = 0.0
    for b in range(want.shape[0]):
        assert got[b, n_sums] == want[b, n_sums], (what, "count", b, got[b], want[b])
        for k in range(n_sums):
            err = abs(got[b, k] - want[b, k])
            if want[b, k] != 0:
                worst = max(worst, err / abs(want[b, k]))
            assert err <= TOL * abs(want[b, k]), (what, b, k, got[b, k], want[b, k])
    print("%s: worst |err| / |want| = %.3g" % (what, worst))


def _spec_lengths(B, T, r):
    return {5: [0, r, r + 1, T - 1, T], 3: [T, r + 1, r], 1: [T]}[B]


@pytest.mark.parametrize("layout", ["btc", "bct"])
@pytest.mark.parametrize("r", [1, 4])
@pytest.mark.parametrize("B,T,D", [(5, 37, 513), (3, 9, 80), (1, 2, 7)])
def test_spec_items(dev, B, T, D, r, layout):
    from deepvoice3_pytorch_amd import ops
    rng = np.random.RandomState(1000 * B + 10 * T + r)
    y_hat = rng.rand(B, T, D).astype(np.float32) * 0.98 + 0.01
    y = rng.rand(B, T, D).astype(np.float32)
    lengths = _spec_lengths(B, T, r)
    want = R.spec_items(y_hat, y, lengths, r)
    yh = torch.from_numpy(y_hat).to(dev)
    if layout == "bct":
        yh = yh.transpose(1, 2).contiguous().transpose(1, 2)
    yd, ld = torch.from_numpy(y).to(dev), _i32(lengths, dev)
    got = ops.spec_loss_items(yh, yd, ld, r)
    again = ops.spec_loss_items(yh, yd, ld, r)
    assert got.shape == (B, 3) and got.dtype == torch.float32 and not got.requires_grad
    assert torch.equal(got, again)
    _check_rows(got, want, 2, "spec %s %s r=%d" % ((B, T, D), layout, r))
    for b, l in enumerate(lengths):
        if l <= r:
            assert float(got[b].abs().max()) == 0.0
    if T > r:        # (the batch kernel takes no tensor of r frames or fewer; every row above is then zero)
        out4 = ops.spec_loss(yh, yd, ld, r, 1.0, 1.0).cpu().numpy().astype(np.float64)
        rows = got.cpu().numpy().astype(np.float64)
        cnt = rows[:, 2].sum()
        assert out4[3] == cnt
        assert abs(rows[:, 0].sum() / cnt - out4[0]) <= TOL * out4[0]
        assert abs(rows[:, 1].sum() / cnt - out4[1]) <= TOL * out4[1]


@pytest.mark.parametrize("B,T", [(5, 37), (1, 1)])
def test_bce_items(dev, B, T):
    from deepvoice3_pytorch_amd import ops
    rng = np.random.RandomState(B + T)
    p = (rng.rand(B, T).astype(np.float32) * 0.9 + 0.05)
    t = (rng.rand(B, T) > 0.5).astype(np.float32)
    if T > 4:
        p[B - 1, 2], t[B - 1, 2] = 0.0, 1.0        # log clamped at -100, as nn.BCELoss
        p[B - 1, 3], t[B - 1, 3] = 1.0, 1.0
    lengths = [0, 1, 17, T - 1, T] if B == 5 else [T]
    want = R.bce_items(p, t, lengths)
    pd, td, ld = torch.from_numpy(p).to(dev), torch.from_numpy(t).to(dev), _i32(lengths, dev)
    got = ops.bce_loss_items(pd, td, ld)
    assert got.shape == (B, 2) and torch.equal(got, ops.bce_loss_items(pd, td, ld))
    assert torch.equal(got, ops.bce_loss_items(pd.unsqueeze(-1), td.unsqueeze(-1), ld))       # the model's (B, T, 1)
    _check_rows(got, want, 1, "bce %s" % ((B, T),))
    # every item full: the rows recombine to the batch mean
    full = ops.bce_loss_items(pd, td, _i32([T] * B, dev)).cpu().numpy().astype(np.float64)
    mean = float(ops.bce_loss(pd, td).cpu())
    assert abs(full[:, 0].sum() / full[:, 1].sum() - mean) <= TOL * mean


@pytest.mark.parametrize("g", [0.2, 0.4])
@pytest.mark.parametrize("case", ["golden", "one_by_one"])
def test_guided_attention_items(dev, case, g):
    from deepvoice3_pytorch_amd import ops
    fx = load_golden("losses")
    il, ol = (fx["guided/in_len"], fx["guided/out_len"]) if case == "golden" else (np.array([1, 9, 4]), np.array([1, 12, 7]))
    L, B, Tq, Tk = 2, 3, 12, 9
    attn = np.random.RandomState(1).rand(L, B, Tq, Tk).astype(np.float32)
    want = R.guided_items(attn, il, ol, g)
    if case == "golden":        # the restatement's W is the reference's
        W = fx["guided_g%g" % g].astype(np.float64)
        assert np.allclose((attn.astype(np.float64) * W[None]).sum(axis=(0, 2, 3)), want[:, 0], rtol=1e-12, atol=0)
    ad, ild, old = torch.from_numpy(attn).to(dev), _i32(il, dev), _i32(ol, dev)
    got = ops.guided_attention_loss_items(ad, ild, old, g)
    assert got.shape == (B, 2) and torch.equal(got, ops.guided_attention_loss_items(ad, ild, old, g))
    _check_rows(got, want, 1, "guided %s g=%g" % (case, g))
    mean = float(ops.guided_attention_loss(ad, ild, old, g).cpu())
    rows = got.cpu().numpy().astype(np.float64)
    assert abs(rows[:, 0].sum() / attn.size - mean) <= TOL * mean

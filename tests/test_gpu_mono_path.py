# coding: utf-8
"""-m gpu: the monotonic alignment search (dv3_mono_path_f32 through ops.monotonic_path) against
tests/mono_ref.py.

Every case is a batch of B = 5 ragged items whose attention is NaN outside each item's own steps and keys:
  item 0: no steps (infeasible);  item 1: all T steps, key_len past Tk (clamped);  item 2: one step over 2 J keys
  (infeasible by the rules whenever Tk >= 2 J: N > (T + 1) J - 1);  item 3: steps past T (clamped), about T J / 2 keys;
  item 4: T - 1 steps over as many keys as the rules just admit.

  1. softmax rows sharpened around a noisy diagonal, at the wave boundary (Tk 63 / 64 / 65), one key, three registers
     per lane (130), one, two and 67 steps, J = 1 and 3, in all three layouts (the strided ones as genuinely strided
     views).  For a feasible item, tol = 2^-23 T_b (|score_ref| + 2): every score is <= 0, so each partial sum is bounded
     by |score| and each of the T_b additions rounds at 2^-24 relative; logf and the layer mean add about 2^-24
     absolute per step each; the whole doubled.  The device score is within tol of the reference's, and the device PATH,
     scored in float64, within 2 tol of the reference optimum -- not path equality, so that an fp32 near-tie cannot fail
     the test.  The integer columns are exact: feasible, steps and keys against the reference, skipped_keys and longest
     against the device's own durations (they describe the device's path).
  2. exact cases: a planted path, uniform rows (the tie-break alone decides), a row of NaN;
  3. two calls bit for bit, attn unchanged (inside 1.);  4. the refusals.
"""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tests import mono_ref as MR  # noqa: E402

pytestmark = pytest.mark.gpu

NAN = float("nan")
B = 5
COL = {name: i for i, name in enumerate(MR.COLUMNS)}


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


def _bits(t):
    return t.contiguous().view(torch.int32)


def _lengths(T, Tk, J):
    """(steps, key_len) as the caller passes them, and as the kernel clamps them"""
    t4 = max(T - 1, 1)
    steps = [0, T, 1, T + 3, t4]
    keys = [Tk, Tk + 5, min(Tk, 2 * J), min(Tk, max(1, (T * J) // 2 + 1)), max(1, min(Tk - 1, (t4 + 1) * J - 1))]
    clamped = [(min(max(s, 0), T), min(max(k, 1), Tk)) for s, k in zip(steps, keys)]
    return steps, keys, clamped


def _diagonal_rows(rng, Tb, Nb):
    """(Tb, Nb) float64 softmax rows, sharp around a noisy diagonal"""
    t = np.arange(Tb)[:, None]
    centre = t * (Nb - 1) / max(Tb - 1, 1) + rng.randn(Tb, 1) * 1.5
    logits = -0.5 * ((np.arange(Nb)[None, :] - centre) / 1.5) ** 2 + rng.randn(Tb, Nb) * 0.7
    e = np.exp(logits - logits.max(axis=1, keepdims=True))
    return e / e.sum(axis=1, keepdims=True)


_CASES = {}


def _case(T, Tk, J, L):
    """-> attn (L, B, T, Tk) fp32 with NaN outside every item's own steps and keys, steps, keys, clamped lengths and the
    reference's result per item (computed once per shape)"""
    key = (T, Tk, J, L)
    if key not in _CASES:
        rng = np.random.RandomState(1000 * T + 10 * Tk + J + 7 * L)
        steps, keys, clamped = _lengths(T, Tk, J)
        a = np.full((L, B, T, Tk), NAN, dtype=np.float32)
        for b, (Tb, Nb) in enumerate(clamped):
            for l in range(L):
                a[l, b, :Tb, :Nb] = _diagonal_rows(rng, Tb, Nb).astype(np.float32)
        want = [MR.mono_path(a[:, b, :Tb, :Nb].astype(np.float64), J) for b, (Tb, Nb) in enumerate(clamped)]
        _CASES[key] = (a, steps, keys, clamped, want)
    return _CASES[key]


def _place(dev, a, layout):
    """the (L, B, T, Tk) array on the device in `layout` -> (the buffer that holds it, the view ops.monotonic_path gets)"""
    L, _, T, Tk = a.shape
    if layout == "btk":
        buf = torch.from_numpy(a[0]).to(dev)
        return buf, buf
    if layout == "tbk":          # the stacked (T, B, Tk) image inside a larger NaN buffer: no stride is the dense one
        buf = torch.full((T + 1, B + 2, Tk + 3), NAN, device=dev)
        view = buf[:T, 1:B + 1, :Tk]
        view.copy_(torch.from_numpy(a[0]).transpose(0, 1))
    else:
        buf = torch.full((L, B + 1, T + 2, Tk + 3), NAN, device=dev)
        view = buf[:, 1:, 1:T + 1, :Tk]
        view.copy_(torch.from_numpy(a))
    assert not view.is_contiguous()
    return buf, view


def _check_item(tag, row, path, dur, Tb, Nb, J, want, s64):
    """one item of a result against the reference; row, path, dur: numpy rows of the three outputs"""
    assert row[COL["steps"]] == Tb and row[COL["keys"]] == Nb, tag
    assert row[COL["feasible"]] == want["feasible"], tag
    assert (path[Tb:] == -1).all() and (dur[Nb:] == 0).all(), tag
    if not want["feasible"]:
        assert row[COL["score"]] == 0.0 and row[COL["skipped_keys"]] == 0.0 and row[COL["longest"]] == 0.0, tag
        assert (path == -1).all() and (dur == 0).all(), tag
        return
    p = path[:Tb].tolist()
    assert MR.path_ok(p, Tb, Nb, J), (tag, p)
    assert int(dur.sum()) == Tb, tag
    assert dur[:Nb].tolist() == np.bincount(p, minlength=Nb).tolist(), tag
    assert row[COL["skipped_keys"]] == int((dur[:Nb] == 0).sum()) and row[COL["longest"]] == int(dur.max()), tag
    tol = 2.0 ** -23 * Tb * (abs(want["score"]) + 2.0)
    err = abs(float(row[COL["score"]]) - want["score"])
    gap = want["score"] - MR.path_score(s64, p)
    print("%s: T_b %2d N_b %3d score %.9g want %.9g err %.2e gap %.2e tol %.2e%s" % (
        tag, Tb, Nb, row[COL["score"]], want["score"], err, gap, tol, "" if p == want["path"] else "  (another path)"))
    assert err <= tol, (tag, err, tol)
    assert abs(gap) <= 2.0 * tol, (tag, gap, tol)


# ----------------------------------------------------------------------------------------------------------------------
# 1. against the reference
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", ["btk", "tbk", "lbtk"])
@pytest.mark.parametrize("J", [1, 3])
@pytest.mark.parametrize("T", [1, 2, 67])
@pytest.mark.parametrize("Tk", [1, 63, 64, 65, 130])
def test_monotonic_path_against_reference(dev, Tk, T, J, layout):
    from deepvoice3_pytorch_amd import ops
    L = 2 if layout == "lbtk" else 1
    a, steps, keys, clamped, want = _case(T, Tk, J, L)
    assert want[0]["feasible"] == 0                               # no steps
    assert want[2]["feasible"] == (0 if Tk >= 2 * J else 1)       # N > (T + 1) J - 1
    assert want[3]["feasible"] == 1 and want[4]["feasible"] == 1
    buf, view = _place(dev, a, layout)
    before = _bits(buf).clone()
    st = torch.tensor(steps, dtype=torch.int32, device=dev)
    kl = torch.tensor(keys, dtype=torch.int32, device=dev)
    out, path, dur = ops.monotonic_path(view, st, kl, layout, J)
    again = ops.monotonic_path(view, st, kl, layout, J)
    torch.cuda.synchronize()
    assert out.shape == (B, 6) and out.dtype == torch.float32
    assert path.shape == (B, T) and path.dtype == torch.int32 and dur.shape == (B, Tk) and dur.dtype == torch.int32
    for x, y in zip((out, path, dur), again):
        assert torch.equal(_bits(x), _bits(y))                    # two calls, bit for bit
    assert torch.equal(_bits(buf), before)                        # attn is only read
    rows, paths, durs = out.cpu().numpy(), path.cpu().numpy(), dur.cpu().numpy()
    assert np.isfinite(rows).all()
    for b, (Tb, Nb) in enumerate(clamped):                        # every item, none left out
        s64 = MR.scores(a[:, b, :Tb, :Nb].astype(np.float64))
        _check_item("Tk %3d T %2d J %d %s item %d" % (Tk, T, J, layout, b), rows[b], paths[b], durs[b], Tb, Nb, J,
                    want[b], s64)


# ----------------------------------------------------------------------------------------------------------------------
# 2. exact cases
# ----------------------------------------------------------------------------------------------------------------------
def _planted(rng, Tb, Nb, J):
    """a path the rules admit, by random advances within J that reach the last J keys exactly at the end"""
    while True:
        p = [int(rng.randint(0, min(J, Nb)))]
        for t in range(1, Tb):
            left = Tb - 1 - t                                     # steps after this one
            lo = max(0, (Nb - J) - p[-1] - left * J)              # what must be advanced now to still reach the end
            hi = min(J, Nb - 1 - p[-1])
            p.append(p[-1] + int(rng.randint(lo, hi + 1)) if hi >= lo else -1)
            if p[-1] < 0:
                break
        if p[-1] >= 0 and MR.path_ok(p, Tb, Nb, J):
            return p


@pytest.mark.parametrize("J", [1, 3])
def test_planted_path_is_found_exactly(dev, J):
    from deepvoice3_pytorch_amd import ops
    rng = np.random.RandomState(40 + J)
    T, Tk = 67, 130
    sizes = {1: [(67, 60), (40, 33), (9, 7)], 3: [(67, 130), (40, 65), (9, 7)]}[J]
    a = np.full((len(sizes), T, Tk), NAN, dtype=np.float32)
    plans = []
    for b, (Tb, Nb) in enumerate(sizes):
        p = _planted(rng, Tb, Nb, J)
        a[b, :Tb, :Nb] = 0.1 / (Nb - 1)
        a[b, np.arange(Tb), p] = 0.9
        plans.append(p)
    st = torch.tensor([s[0] for s in sizes], dtype=torch.int32, device=dev)
    kl = torch.tensor([s[1] for s in sizes], dtype=torch.int32, device=dev)
    out, path, dur = ops.monotonic_path(torch.from_numpy(a).to(dev), st, kl, "btk", J)
    torch.cuda.synchronize()
    for b, (Tb, Nb) in enumerate(sizes):
        assert out[b, 0].item() == 1.0
        assert path[b, :Tb].tolist() == plans[b], b
        assert (path[b, Tb:] == -1).all()
        assert dur[b].tolist() == np.bincount(plans[b], minlength=Tk).tolist(), b
        assert MR.mono_path(a[b, :Tb, :Nb], J)["path"] == plans[b]          # and the reference agrees
        assert out[b, 4].item() == sum(1 for n in range(Nb) if n not in plans[b])
        assert out[b, 5].item() == np.bincount(plans[b]).max()
    if J == 3:
        assert out[0, 4].item() > 0                               # keys were skipped


@pytest.mark.parametrize("J", [1, 3])
def test_uniform_rows_are_decided_by_the_tie_break(dev, J):
    """every admissible path of an item has the bit-identical score (T_b additions of one constant, in one order)"""
    from deepvoice3_pytorch_amd import ops
    T, Tk = 67, 130
    sizes = {1: [(67, 67), (67, 64), (23, 20), (5, 3), (1, 1)], 3: [(67, 130), (67, 64), (20, 23), (5, 3), (1, 1)]}[J]
    a = np.full((len(sizes), T, Tk), NAN, dtype=np.float32)
    for b, (Tb, Nb) in enumerate(sizes):
        a[b, :Tb, :Nb] = 1.0 / Nb
    st = torch.tensor([s[0] for s in sizes], dtype=torch.int32, device=dev)
    kl = torch.tensor([s[1] for s in sizes], dtype=torch.int32, device=dev)
    out, path, dur = ops.monotonic_path(torch.from_numpy(a).to(dev), st, kl, "btk", J)
    torch.cuda.synchronize()
    for b, (Tb, Nb) in enumerate(sizes):
        want = MR.mono_path(a[b, :Tb, :Nb], J)
        assert want["feasible"] == 1 == out[b, 0].item()
        assert path[b, :Tb].tolist() == want["path"], (b, path[b, :Tb].tolist(), want["path"])
        assert dur[b, :Nb].tolist() == want["durations"], b
        assert out[b, 4].item() == want["skipped_keys"] and out[b, 5].item() == want["longest"]


def test_a_row_of_nan_scores_as_the_floor(dev):
    from deepvoice3_pytorch_amd import ops
    T, Tk, J = 67, 65, 1
    a, steps, keys, clamped, _ = _case(T, Tk, J, 1)
    st = torch.tensor(steps, dtype=torch.int32, device=dev)
    kl = torch.tensor(keys, dtype=torch.int32, device=dev)
    base = ops.monotonic_path(torch.from_numpy(a[0]).to(dev), st, kl, "btk", J)
    hit = a[0].copy()
    Tb, Nb = clamped[3]
    hit[3, Tb // 2, :Nb] = NAN                                    # a whole row inside item 3's lengths
    got = ops.monotonic_path(torch.from_numpy(hit).to(dev), st, kl, "btk", J)
    torch.cuda.synchronize()
    others = [0, 1, 2, 4]
    for x, y in zip(base, got):
        assert torch.equal(_bits(x[others]), _bits(y[others]))    # the other items are unchanged
    want = MR.mono_path(hit[3, :Tb, :Nb].astype(np.float64), J)
    assert want["feasible"] == 1
    _check_item("nan row", got[0][3].cpu().numpy(), got[1][3].cpu().numpy(), got[2][3].cpu().numpy(), Tb, Nb, J, want,
                MR.scores(hit[3, :Tb, :Nb].astype(np.float64)))
    assert abs(want["score"] - (MR.mono_path(a[0, 3, :Tb, :Nb].astype(np.float64), J)["score"])) > 40.0     # log(1e-20) came in


# ----------------------------------------------------------------------------------------------------------------------
# 4. the refusals
# ----------------------------------------------------------------------------------------------------------------------
def test_monotonic_path_refusals(dev):
    from deepvoice3_pytorch_amd import _lib, ops
    lib = _lib.lib()
    Bn, T, Tk = 2, 3, 8
    attn = torch.full((Bn, T, Tk), 1.0 / Tk, device=dev)
    st = torch.tensor([3, 3], dtype=torch.int32, device=dev)
    kl = torch.tensor([3, 2], dtype=torch.int32, device=dev)
    out = torch.full((Bn, 6), 7.0, device=dev)
    path = torch.full((Bn, T), 7, dtype=torch.int32, device=dev)
    dur = torch.full((Bn, Tk), 7, dtype=torch.int32, device=dev)
    need = ctypes.c_int64(0)
    assert lib.dv3_mono_path_scratch_bytes(Bn, T, Tk, ctypes.byref(need)) == 0
    assert need.value == 4 * Bn * T * Tk + Bn * T * Tk
    assert lib.dv3_mono_path_scratch_bytes(1, 3, 3, ctypes.byref(need)) == 0 and need.value == 36 + 12      # 9 bytes -> 12
    need.value = 4 * Bn * T * Tk + Bn * T * Tk
    scratch = torch.zeros(need.value + 8, dtype=torch.uint8, device=dev)

    def call(**kw):
        d = _lib.STRUCTS["dv3_mono_desc"]()
        d.attn, d.steps, d.key_len = attn.data_ptr(), st.data_ptr(), kl.data_ptr()
        d.layer_stride, d.item_stride, d.step_stride = 0, T * Tk, Tk
        d.n_layers, d.B, d.T, d.Tk, d.max_advance = 1, Bn, T, Tk, 1
        d.out, d.path, d.durations = out.data_ptr(), path.data_ptr(), dur.data_ptr()
        d.scratch, d.scratch_bytes = scratch.data_ptr(), need.value
        for k, v in kw.items():
            setattr(d, k, v)
        return lib.dv3_mono_path_f32(ctypes.byref(d), None)

    assert call() == 0
    torch.cuda.synchronize()
    assert out[:, :3].tolist() == [[1.0, 3.0, 3.0], [1.0, 3.0, 2.0]]
    assert path.tolist() == [[0, 1, 2], [0, 1, 1]] and dur[:, :3].tolist() == [[1, 1, 1], [1, 2, 0]]
    out.fill_(7.0)
    path.fill_(7)
    dur.fill_(7)
    EINVAL = _lib.CONSTS["DV3_EINVAL"]
    for kw, word in ((dict(attn=None), "attn"), (dict(steps=None), "steps"), (dict(key_len=None), "key_len"),
                     (dict(out=None), "out"), (dict(path=None), "path"), (dict(durations=None), "durations"),
                     (dict(scratch=None), "scratch"), (dict(B=0), "B = 0"), (dict(B=65536), "B = 65536"),
                     (dict(T=0), "T = 0"), (dict(T=8193), "T = 8193"), (dict(Tk=0), "Tk = 0"), (dict(Tk=2049), "Tk = 2049"),
                     (dict(max_advance=0), "max_advance = 0"), (dict(max_advance=9), "max_advance = 9"),
                     (dict(n_layers=0), "n_layers = 0"), (dict(scratch_bytes=need.value - 1), "scratch_bytes"),
                     (dict(out=out.data_ptr() + 2), "out"), (dict(path=path.data_ptr() + 2), "path"),
                     (dict(durations=dur.data_ptr() + 1), "durations"), (dict(scratch=scratch.data_ptr() + 3), "scratch")):
        assert call(**kw) == EINVAL, kw
        assert word in lib.dv3_last_error().decode(), (kw, lib.dv3_last_error())
    assert lib.dv3_mono_path_f32(None, None) == EINVAL and "descriptor" in lib.dv3_last_error().decode()
    assert lib.dv3_mono_path_scratch_bytes(Bn, T, Tk, None) == EINVAL
    for args in ((0, T, Tk), (Bn, 8193, Tk), (Bn, T, 2049)):
        assert lib.dv3_mono_path_scratch_bytes(*(args + (ctypes.byref(need),))) == EINVAL and need.value == 0
    torch.cuda.synchronize()
    assert bool((out == 7.0).all()) and bool((path == 7).all()) and bool((dur == 7).all())     # nothing was launched
    # and the Python wrapper's own checks
    with pytest.raises(RuntimeError, match="layout"):
        ops.monotonic_path(attn, st, kl, "kbt")
    with pytest.raises(RuntimeError, match="layout"):
        ops.monotonic_path(attn, st, kl, "lbtk")
    with pytest.raises(RuntimeError, match="dense"):
        ops.monotonic_path(attn.transpose(1, 2), st, kl, "btk")
    with pytest.raises(RuntimeError, match="key lengths"):
        ops.monotonic_path(attn, st[:1], kl, "btk")
    with pytest.raises(RuntimeError, match="int32"):
        ops.monotonic_path(attn, st.long(), kl, "btk")
    with pytest.raises(RuntimeError, match="max_advance = 9"):
        ops.monotonic_path(attn, st, kl, "btk", 9)

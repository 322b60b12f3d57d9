# coding: utf-8
"""tests/item_losses_ref.py pinned on the CPU against the oracle's batch losses, and train_step.EvalTotals (pure torch):
the set-level figures do not depend on how a held-out set is cut into batches, nor on how it is split between the
ranks of a process group."""
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tests import item_losses_ref as R  # noqa: E402
from oracle import dv3_oracle as O  # noqa: E402

SET_KEYS = ("mel_l1", "mel_binary_div", "linear_l1", "linear_binary_div", "done", "attn", "loss", "n_items")


@pytest.mark.parametrize("B,T,D,r", [(5, 37, 13, 1), (3, 9, 8, 4), (1, 6, 7, 1)])
def test_spec_items_recombine_to_the_oracles_masked_means(B, T, D, r):
    rng = np.random.RandomState(B * 100 + T)
    y_hat = rng.rand(B, T, D).astype(np.float32) * 0.98 + 0.01
    y = rng.rand(B, T, D).astype(np.float32)
    lengths = np.array(([T, 0, r, r + 1, T - 1] * 2)[:B] if B > 1 else [T])
    rows = R.spec_items(y_hat, y, lengths, r)
    for b in range(B):
        n = max(int(lengths[b]) - r, 0)
        assert rows[b, 2] == n * D
        if n == 0:
            assert rows[b, 0] == 0.0 and rows[b, 1] == 0.0
    mask = O.sequence_mask(torch.from_numpy(lengths), T).unsqueeze(-1)[:, r:].double()
    l1, bd = O.spec_loss(torch.from_numpy(y_hat).double()[:, :-r], torch.from_numpy(y).double()[:, r:], mask,
                         w_masked=1.0, w_bd=0.1)
    assert abs(rows[:, 0].sum() / rows[:, 2].sum() - float(l1)) < 1e-12 * float(l1)
    assert abs(rows[:, 1].sum() / rows[:, 2].sum() - float(bd)) < 1e-12 * float(bd)


def test_spec_items_of_a_tensor_of_r_frames_or_fewer_are_zero_rows():
    rng = np.random.RandomState(0)
    rows = R.spec_items(rng.rand(2, 2, 7), rng.rand(2, 2, 7), [2, 9], 4)
    assert rows.shape == (2, 3) and not rows.any()
    rows = R.spec_items(rng.rand(1, 5, 3), rng.rand(1, 5, 3), [9], 1)       # a length beyond the tensor: clamped to it
    assert rows[0, 2] == 4 * 3


def test_items_against_train_losses():
    """the whole loss block at masked_loss_weight = 1: mel and linear means from the spec rows, the attention term from
    the guided rows over the tensor's element count; done_loss when every item fills the batch"""
    rng = np.random.RandomState(3)
    B, Td, Tk, L, r, ds, Dm, Dl = 4, 12, 9, 2, 1, 4, 5, 7
    hp = dict(outputs_per_step=r, downsample_step=ds, masked_loss_weight=1.0, binary_divergence_weight=0.1,
              use_guided_attention=True, guided_attention_sigma=0.2)
    d = lambda *s: torch.from_numpy(rng.rand(*s) * 0.98 + 0.01)
    mel_out, lin_out, attn, done_hat = d(B, Td, Dm), d(B, Td * ds, Dl), d(L, B, Td, Tk), d(B, Td, 1)
    mel, y = d(B, Td, Dm), d(B, Td * ds, Dl)
    done = torch.from_numpy((rng.rand(B, Td, 1) > 0.5).astype(np.float64))
    il = np.array([9, 1, 5, 7])
    tl = np.array([48, 4, 30, 41])
    dl = tl // r // ds
    _, parts = O.train_losses(None, hp, (mel_out, lin_out, attn, done_hat), mel, y, done, il, tl)
    m = R.spec_items(mel_out.numpy(), mel.numpy(), dl, r)
    l = R.spec_items(lin_out.numpy(), y.numpy(), tl, r)
    a = R.guided_items(attn.numpy(), il, dl, 0.2)
    close = lambda got, want: abs(got - float(want)) < 1e-7 * abs(float(want))      # (the oracle's W is float32)
    assert close(m[:, 0].sum() / m[:, 2].sum(), parts["mel_l1"]) and close(m[:, 1].sum() / m[:, 2].sum(), parts["mel_bd"])
    assert close(l[:, 0].sum() / l[:, 2].sum(), parts["lin_l1"]) and close(l[:, 1].sum() / l[:, 2].sum(), parts["lin_bd"])
    assert close(a[:, 0].sum() / (L * B * Td * Tk), parts["attn_loss"])
    assert list(a[:, 1]) == [L * int(t) * int(n) for t, n in zip(dl, il)]
    full = R.bce_items(done_hat.numpy(), done.numpy(), np.full(B, Td))
    assert close(full[:, 0].sum() / full[:, 1].sum(), parts["done_loss"])
    own = R.bce_items(done_hat.numpy(), done.numpy(), dl)
    assert list(own[:, 1]) == list(dl) and own[1, 0] < full[1, 0]


def _fake_results(cuts, seed=5, n=7):
    """evaluate()-shaped results for the same n items cut into batches of `cuts`: item rows from the restatement on
    random tensors, batch scalars that differ per batch"""
    from deepvoice3_pytorch_amd import train_step
    rng = np.random.RandomState(seed)
    T, D = 11, 6
    lengths = rng.randint(0, T + 1, n)
    spec = lambda: R.spec_items(rng.rand(n, T, D) * 0.9 + 0.05, rng.rand(n, T, D), lengths, 1)
    mel, lin = spec(), spec()
    done = R.bce_items(rng.rand(n, T) * 0.9 + 0.05, (rng.rand(n, T) > 0.5) * 1.0, lengths)
    attn = R.guided_items(rng.rand(2, n, T, 8), rng.randint(1, 9, n), np.maximum(lengths, 1), 0.2)
    table = torch.from_numpy(np.concatenate([mel, lin, done, attn], axis=1))
    assert table.shape == (n, len(train_step.EVAL_ITEM_COLUMNS))
    out, at = [], 0
    for c in cuts:
        res = dict(items=table[at:at + c].to(torch.float32), loss=torch.tensor(0.5 + at), mel_loss=torch.tensor(0.1 * c))
        out.append((res, ["utt%d" % i for i in range(at, at + c)]))
        at += c
    assert at == n
    return out


def _totals(results):
    from deepvoice3_pytorch_amd import train_step
    tot = train_step.EvalTotals(binary_divergence_weight=0.1)
    for res, ids in results:
        tot.add(res, ids)
    return tot


def test_eval_totals_do_not_depend_on_the_batching():
    from deepvoice3_pytorch_amd import train_step
    ref = _totals(_fake_results((7,))).result()
    cols = {c: i for i, c in enumerate(train_step.EVAL_ITEM_COLUMNS)}
    it = ref["items"].numpy()
    assert it.dtype == np.float64 and it.shape == (7, 10) and ref["ids"] == ["utt%d" % i for i in range(7)]
    # the definitions
    assert abs(ref["mel_l1"] - it[:, cols["mel_S1"]].sum() / it[:, cols["mel_cnt"]].sum()) < 1e-12
    assert abs(ref["attn"] - it[:, cols["attn_S"]].sum() / it[:, cols["attn_cnt"]].sum()) < 1e-12
    want = (0.9 * ref["mel_l1"] + 0.1 * ref["mel_binary_div"] + 0.9 * ref["linear_l1"] + 0.1 * ref["linear_binary_div"] +
            ref["done"] + ref["attn"])
    assert abs(ref["loss"] - want) < 1e-12 and ref["n_items"] == 7
    assert abs(ref["batch_mean/loss"] - 0.5) < 1e-12
    for cuts in ((3, 4), (1, 2, 4)):
        got = _totals(_fake_results(cuts)).result()
        for k in SET_KEYS:
            assert abs(got[k] - ref[k]) <= 1e-12 * max(1.0, abs(ref[k])), (cuts, k, got[k], ref[k])
        assert torch.equal(got["items"], ref["items"]) and got["ids"] == ref["ids"]
    # the batch scalars' mean is weighted by the item counts: (3 * 0.5 + 4 * 3.5) / 7
    got = _totals(_fake_results((3, 4))).result()
    assert abs(got["batch_mean/loss"] - (3 * 0.5 + 4 * 3.5) / 7) < 1e-12
    assert abs(got["batch_mean/mel_loss"] - (3 * 0.3 + 4 * 0.4) / 7) < 1e-6      # (0.1 * c went through float32)


def test_eval_totals_refuse_mixed_input():
    from deepvoice3_pytorch_amd import train_step
    (a, ia), (b, ib) = _fake_results((3, 4))
    tot = train_step.EvalTotals()
    with pytest.raises(ValueError):
        tot.result()
    tot.add(a, ia)
    with pytest.raises(ValueError):
        tot.add(b, None)
    with pytest.raises(ValueError):
        tot.add(dict(items=b["items"], loss=b["loss"]), ib)
    with pytest.raises(ValueError):
        tot.add(dict(b, items=b["items"][:, :4]), ib)


def _rank(rank, world, port, q):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
    sys.path.insert(0, ROOT)
    import torch.distributed as dist
    dist.init_process_group(backend="gloo", rank=rank, world_size=world)
    results = _fake_results((1, 2, 4))
    mine = results[:2] if rank == 0 else results[2:]          # items 0-2 on rank 0, 3-6 on rank 1
    res = _totals(mine).result(dist.group.WORLD)
    # ... and a rank whose shard is empty still takes part in the collective, with zeros
    from deepvoice3_pytorch_amd import train_step
    tot = train_step.EvalTotals(0.1, scalar_keys=("loss", "mel_loss"))
    for r_, ids in (results if rank == 0 else []):
        tot.add(r_, ids)
    res["one_sided"] = {k: v for k, v in tot.result(dist.group.WORLD).items() if k not in ("items", "ids")}
    res["items"] = res["items"].numpy()
    q.put((rank, res))
    dist.destroy_process_group()


def _free_port():
    """a port the system hands out for a socket bound here and closed again: free at this moment for the rendezvous"""
    import socket
    with socket.socket(socket.AF_INET, socket.SOCK_STREAM) as sk:
        sk.bind(("127.0.0.1", 0))
        return sk.getsockname()[1]


def _spawn(target, world, port):
    """the children of `target(rank, world, port, q)` -> their results by rank, within the poll's cap"""
    import torch.multiprocessing as mp
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=target, args=(r, world, port, q)) for r in range(world)]
    for p in procs:
        p.start()
    res = []
    for _ in range(120):
        try:
            res.append(q.get(timeout=1.0))
        except Exception:
            if not all(p.is_alive() or p.exitcode == 0 for p in procs):
                break
        if len(res) == world:
            break
    if len(res) != world:
        for p in procs:
            p.kill()
        raise RuntimeError("a rank ended without a result: exit codes %r" % ([p.exitcode for p in procs],))
    for p in procs:
        p.join(60)
        assert p.exitcode == 0
    return [r[1] for r in sorted(res, key=lambda t: t[0])]


def test_eval_totals_under_a_world_2_gloo_group():
    """the items split between two ranks: both ranks report the single-process set-level figures, each keeps its rows"""
    ref = _totals(_fake_results((1, 2, 4))).result()
    r0, r1 = _spawn(_rank, 2, _free_port())
    for got in (r0, r1):
        for k in SET_KEYS + ("batch_mean/loss", "batch_mean/mel_loss"):
            assert abs(got[k] - ref[k]) <= 1e-12 * max(1.0, abs(ref[k])), (k, got[k], ref[k])
    assert np.array_equal(r0["items"], ref["items"].numpy()[:3]) and np.array_equal(r1["items"], ref["items"].numpy()[3:])
    assert r0["ids"] == ref["ids"][:3] and r1["ids"] == ref["ids"][3:]
    for got in (r0["one_sided"], r1["one_sided"]):           # all seven items on rank 0, none on rank 1
        for k in SET_KEYS + ("batch_mean/loss", "batch_mean/mel_loss"):
            assert abs(got[k] - ref[k]) <= 1e-12 * max(1.0, abs(ref[k])), (k, got[k], ref[k])

# coding: utf-8
"""Host side of LatticeReplay under a process group, on a box without a GPU: the collective-free
mode of dist.BucketedAllReduce that the dry warm-up of a newly met shape runs in, the refusal of anything but the
segmented replay, the one-order-per-model check of the host-issued all-reduces, and the hand-back of
ops.dropout_state.dev_offset with several live captures."""
import numpy as np
import pytest
import torch

from deepvoice3_pytorch_amd import dist as dv3dist, ops, train_step
from deepvoice3_pytorch_amd.train_step import FlatArena


def _comm(sizes=(3000, 40, 5000, 7, 2500, 16)):
    params = [torch.nn.Parameter(torch.randn(n)) for n in sizes]
    arena = FlatArena(params)
    comm = dv3dist.BucketedAllReduce(arena, None, bucket_mb=0.02, last_bucket_mb=None)
    assert len(comm.buckets) >= 2
    return params, arena, comm


def _backward_like_the_step(params, comm):
    """what Trainer.forward_backward does to the communicator: arm() right before backward, then every parameter
    reports -- some through autograd's hooks, some through ops.grad_ready_hooks, some through both"""
    comm.arm()
    sum((i + 1.0) * p.sum() for i, p in enumerate(params) if i % 2 == 0).backward()
    for i, p in enumerate(params):
        if i % 2 == 1:
            p.grad.add_(1.0)
        for hook in ops.grad_ready_hooks:
            hook(p)


def test_collective_free_backward_launches_nothing_and_leaves_the_communicator_clean(monkeypatch):
    calls = []
    monkeypatch.setattr(torch.distributed, "all_reduce", lambda *a, **k: calls.append(a))
    params, arena, comm = _comm()
    try:
        # the control: the same backward outside the block launches every bucket (through torch.distributed.all_reduce)
        _backward_like_the_step(params, comm)
        assert len(calls) == len(comm.buckets) and all(comm.launched)
        comm.finish()
        del calls[:]
        with comm.collective_free():
            for _ in range(2):                      # two warm-up passes
                arena.grad.zero_()
                _backward_like_the_step(params, comm)
                assert not comm._armed and not any(comm.launched) and not any(comm.notified)
            # segment capture notes nothing either while the hooks are off
            ops.SideStream.split_capture = True
            try:
                _backward_like_the_step(params, comm)
            finally:
                ops.SideStream.split_capture = False
            assert comm.take_completed() == []
            with pytest.raises(RuntimeError, match="collective_free"):
                comm.launch_after([0], ())
            with pytest.raises(RuntimeError, match="collective_free"):
                comm.finish()
        assert calls == []
        assert comm._works == [] and comm._completed == [] and not comm._armed and not comm._muted
        assert comm.pending == [0] * len(comm.buckets) and comm.launched == [False] * len(comm.buckets)
        assert not any(comm.notified)
        # ... and the next ordinary backward is an ordinary one again
        arena.grad.zero_()
        _backward_like_the_step(params, comm)
        comm.finish()
        assert len(calls) == len(comm.buckets)
    finally:
        comm.close()


def test_collective_free_refuses_to_start_over_all_reduces_in_flight():
    params, arena, comm = _comm()
    try:
        comm._works.append(object())
        with pytest.raises(RuntimeError, match="in flight"):
            with comm.collective_free():
                pass
    finally:
        comm.close()


class _NoPeers(object):
    """a communicator without peers as Trainer sees a dist.RingStandin (which needs a GPU for its scratch buffer)"""
    is_standin = True
    stream = None


def _cpu_trainer():
    from deepvoice3_pytorch_amd import builder
    hp = dict(n_vocab=20, embed_dim=16, mel_dim=8, linear_dim=17, r=1, downsample_step=4, padding_idx=0, dropout=0.0,
              kernel_size=3, encoder_channels=16, decoder_channels=16, converter_channels=16, max_positions=64)
    torch.manual_seed(0)
    return train_step.Trainer(builder.deepvoice3(**hp), train_step.TrainConfig(max_positions=64),
                              process_group=_NoPeers(), bucket_mb=0.01, last_bucket_mb=None)


def test_lattice_replay_under_a_group_without_a_second_stream_is_refused():
    tr = _cpu_trainer()
    try:
        assert tr.comm is not None and tr.side_stream is None
        with pytest.raises(RuntimeError, match="segmented"):
            train_step.LatticeReplay(tr)
        tr.side_stream = object()                    # a second stream, but the segments switched off
        import os
        prev = os.environ.get("DV3_SPLIT_GRAPH")
        os.environ["DV3_SPLIT_GRAPH"] = "0"
        try:
            with pytest.raises(RuntimeError, match="DV3_SPLIT_GRAPH"):
                train_step.LatticeReplay(tr)
        finally:
            if prev is None:
                del os.environ["DV3_SPLIT_GRAPH"]
            else:
                os.environ["DV3_SPLIT_GRAPH"] = prev
        train_step.LatticeReplay(tr).close()         # with both, accepted
    finally:
        tr.side_stream = None
        tr.close()


class _Valid(object):
    def __init__(self, t_in, t_dec):
        self.t_in, self.t_dec = t_in, t_dec


class _Batch(object):
    def __init__(self, t_in, t_dec):
        self.valid, self.text = _Valid(t_in, t_dec), torch.zeros(2, t_in)


def _stub_captures(monkeypatch, orders):
    """GraphedTrainer replaced by its bookkeeping: the dropout offset chain of the real class (its __init__ and close())
    and a bucket schedule per shape taken from `orders` (key -> (seg_buckets, rest_buckets))"""
    made = []

    class Stub(object):
        def __init__(self, trainer, static_batch, warmup=3, split_streams=None, chunk=None, dry_warmup=False, pool=None):
            assert dry_warmup
            self.split = bool(split_streams)
            self.seed_offset = torch.zeros(1, dtype=torch.int64)
            self._prev_offset = ops.dropout_state.dev_offset
            ops.dropout_state.dev_offset = self.seed_offset
            self.seg_buckets, self.rest_buckets = orders.get(train_step.LatticeReplay.key_of(static_batch), ([], []))
            self.segs, self.closed, self.steps = [], False, 0
            made.append(self)

        bucket_order = train_step.GraphedTrainer.bucket_order
        close = train_step.GraphedTrainer.close

        def step(self, batch=None):
            self.steps += 1
            return {}

    monkeypatch.setattr(train_step, "GraphedTrainer", Stub)
    monkeypatch.setattr(train_step, "clone_batch", lambda b: b)
    return made


def test_a_capture_that_would_issue_the_buckets_in_another_order_is_refused(monkeypatch):
    tr = _cpu_trainer()
    n = len(tr.comm.buckets)
    assert n >= 3
    ids = list(range(n))
    a, b, c = _Batch(32, 32), _Batch(32, 24), _Batch(32, 16)
    key = train_step.LatticeReplay.key_of
    orders = {key(a): ([ids[:1], [], ids[1:-1]], ids[-1:]),
              key(b): ([ids[:2], ids[2:-1], []], ids[-1:]),         # buckets move to other segments: the same order
              key(c): ([ids[1:2], ids[:1], ids[2:-1]], ids[-1:])}   # two buckets swapped
    made = _stub_captures(monkeypatch, orders)
    tr.side_stream = object()
    prev = ops.dropout_state.dev_offset
    try:
        rep = train_step.LatticeReplay(tr)
        rep.step(a)
        rep.step(b)
        assert rep.bucket_order == ids and rep.bucket_orders == {key(a): ids, key(b): ids} and all(g.split for g in made)
        with pytest.raises(RuntimeError) as e:
            rep.step(c)
        msg = str(e.value)
        assert repr(key(c)) in msg and repr(ids) in msg and repr([ids[1], ids[0]] + ids[2:]) in msg
        assert key(c) not in rep.graphs and ops.dropout_state.dev_offset is made[1].seed_offset
        rep.step(a)
        assert made[0].steps == 2 and rep.stats["captures"] == 2
        rep.close()
        assert ops.dropout_state.dev_offset is prev
    finally:
        ops.dropout_state.dev_offset = prev
        tr.side_stream = None
        tr.close()


def test_a_capture_that_misses_a_bucket_is_refused(monkeypatch):
    tr = _cpu_trainer()
    ids = list(range(len(tr.comm.buckets)))
    a = _Batch(32, 32)
    _stub_captures(monkeypatch, {train_step.LatticeReplay.key_of(a): ([ids[:1]], ids[2:])})
    tr.side_stream = object()
    prev = ops.dropout_state.dev_offset
    try:
        rep = train_step.LatticeReplay(tr)
        with pytest.raises(RuntimeError, match="every bucket exactly once"):
            rep.step(a)
        assert ops.dropout_state.dev_offset is prev
    finally:
        ops.dropout_state.dev_offset = prev
        tr.side_stream = None
        tr.close()


def test_dropout_offset_goes_back_to_a_live_capture_or_to_the_value_before_the_first(monkeypatch):
    """close() and LRU evictions with several live captures: ops.dropout_state.dev_offset is never left at a closed
    capture's counter"""
    from deepvoice3_pytorch_amd import builder
    hp = dict(n_vocab=20, embed_dim=16, mel_dim=8, linear_dim=17, r=1, downsample_step=4, padding_idx=0, dropout=0.0,
              kernel_size=3, encoder_channels=16, decoder_channels=16, converter_channels=16, max_positions=64)
    tr = train_step.Trainer(builder.deepvoice3(**hp), train_step.TrainConfig(max_positions=64))
    made = _stub_captures(monkeypatch, {})
    before = torch.zeros(1, dtype=torch.int64)         # some value of the process from before the first capture
    prev, ops.dropout_state.dev_offset = ops.dropout_state.dev_offset, before
    a, b, c = _Batch(32, 32), _Batch(32, 24), _Batch(32, 16)
    try:
        rep = train_step.LatticeReplay(tr)
        rep.step(a), rep.step(b), rep.step(c)
        assert ops.dropout_state.dev_offset is made[2].seed_offset
        rep.close()
        assert ops.dropout_state.dev_offset is before and not rep.graphs
        # evictions: the surviving capture's counter
        rep = train_step.LatticeReplay(tr, max_graphs=2)
        rep.step(a), rep.step(b)
        rep.step(a)                                     # a is the most recently used, b the one to go
        rep.step(c)
        g_a, g_b, g_c = made[3:6]
        assert rep.stats["evictions"] == 1 and list(rep.graphs.values()) == [g_a, g_c]
        assert ops.dropout_state.dev_offset is g_c.seed_offset
        rep.step(b)                                     # evicts a while the global is c's: stays at c's (live) ... then b's own
        assert ops.dropout_state.dev_offset is made[6].seed_offset
        # the capture whose counter is installed goes first: the global moves to a live one, not down the closed chain
        ops.dropout_state.dev_offset = g_c.seed_offset
        rep._release(rep.graphs.pop(train_step.LatticeReplay.key_of(c)))
        assert ops.dropout_state.dev_offset is made[6].seed_offset
        rep.close()
        assert ops.dropout_state.dev_offset is before
    finally:
        ops.dropout_state.dev_offset = prev
        tr.close()

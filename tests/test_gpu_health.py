# coding: utf-8
"""-m gpu: training health -- the guarded clip + Adam passes (dv3_clip_adam_guard_f32,
dv3_clip_adam_ema_guard_f32), the per-tensor table (dv3_arena_stats_f32) and what train_step builds on them.

  1. a finite gradient norm: p, m, v (, the average) bit for bit as the unguarded passes write them, health = [0, 0];
  2. a norm that is not finite (a NaN, +Inf or -Inf element, or a finite gradient whose sum of squares leaves the fp32
     range): nothing is touched, health[0] counts it, and the next finite pass applies as the unguarded one does;
  3. the table against tests/health_ref.py (float64 on the same fp32 inputs): maxima and the count exactly, the sums
     within 64 * 2^-24 (a bound from the rounding chain, DESIGN.md 3.7c: 39 roundings at most), the pads never read,
     a skipped pass shows no update, two runs the same bits;
  4. eager trainer: the option leaves clean steps bit for bit as they were and refuses a poisoned one, which the trainer
     without it steps into its parameters;
  5. GraphedTrainer (segmented, single graph) and LatticeReplay refuse it inside the captured step;
  6. Trainer.tensor_stats on the small model."""
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tests import health_ref as H  # noqa: E402

pytestmark = pytest.mark.gpu

# the small model of tests/test_gpu_ema.py (dropout 0: eager steps and replays are comparable bit for bit)
HP = dict(n_vocab=30, embed_dim=32, mel_dim=16, linear_dim=17, r=1, downsample_step=4, padding_idx=0, dropout=0.0,
          kernel_size=3, encoder_channels=64, decoder_channels=32, converter_channels=32, use_memory_mask=False,
          force_monotonic_attention=False, use_decoder_state_for_postnet_input=True, key_projection=True,
          value_projection=True, max_positions=256)
DECAY, STEPS = 0.9, 4
# 4096 * 1024 + 1029: more than one trip of the grid-stride loop at 4 and at 16 bytes per lane, and a scalar tail
BIG = 4096 * 1024 + 1029
SIZES = [1, 3, 4, 5, 1027, BIG]
CASES = [(n, 0) for n in SIZES] + [(1027, 1)]          # (n, offset in elements: 1 = not 16-byte aligned)
BETA1, BETA2, EPS, WD, PRESCALE = 0.5, 0.9, 1e-6, 0.01, 0.125
TABLE_SIZES = [1, 3, 4, 5, 1027, 4096, 4097, 3 * 4096 + 5, 70000]


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


@pytest.fixture(scope="module", autouse=True)
def _range_counter_left_clean(dev):
    """the poisoned backward passes below push NaN through f16x3 operand staging: leave the range counter at zero"""
    yield
    from deepvoice3_pytorch_amd import ops
    torch.cuda.synchronize()
    ops.f16_range_events(reset=True)


def _bits(t):
    t = t.detach().contiguous()
    return t.view(torch.int32) if t.dtype == torch.float32 else t


def _same(a, b):
    if a is None or b is None:
        return a is None and b is None
    return a.shape == b.shape and torch.equal(_bits(a), _bits(b))


def _buf(n, off, dev, gen, kind):
    base = torch.empty(n + off + 3, dtype=torch.float32)
    if kind == "randn":
        base.normal_(generator=gen)
    else:                        # a second moment: not negative
        base.uniform_(0.0, 0.01, generator=gen)
    t = base.to(dev)[off:off + n]
    assert t.data_ptr() % 16 == (4 * off) % 16
    return t


def _hyper(t, one_minus_d, dev):
    return torch.tensor([5e-4 * t, 1.0 - BETA1 ** t, np.sqrt(1.0 - BETA2 ** t), one_minus_d], dtype=torch.float32,
                        device=dev)


def _norm_of(g, dev):
    """ops.grad_sqnorm of a copy (it wants a 16-byte aligned arena) -> the two words the update passes read"""
    from deepvoice3_pytorch_amd import ops
    partial, norm = torch.empty(1024, device=dev), torch.zeros(2, device=dev)
    ops.grad_sqnorm(g.clone(), partial, norm)
    return norm


class _Pair(object):
    """one state stepped four ways: guarded and unguarded, without and with the average"""

    def __init__(self, n, off, dev, gen):
        from deepvoice3_pytorch_amd import ops
        self.ops = ops
        p, m, e = (_buf(n, off, dev, gen, "randn") for _ in range(3))
        v = _buf(n, off, dev, gen, "second")
        m.mul_(0.1)
        c = lambda t: torch.empty(n + off + 3, dtype=torch.float32, device=dev)[off:off + n].copy_(t)   # same alignment
        self.guard = dict(p=c(p), m=c(m), v=c(v))                      # ops.clip_adam(health=)
        self.plain = dict(p=c(p), m=c(m), v=c(v))                      # ops.clip_adam
        self.guard_e = dict(p=c(p), m=c(m), v=c(v), e=c(e))            # ops.clip_adam_ema(health=)
        self.plain_e = dict(p=c(p), m=c(m), v=c(v), e=c(e))            # ops.clip_adam_ema
        self.health = torch.zeros(2, dtype=torch.float32, device=dev)
        self.health_e = torch.zeros(2, dtype=torch.float32, device=dev)

    def snapshot(self):
        return [{k: t.clone() for k, t in s.items()} for s in (self.guard, self.guard_e)]

    def guarded(self, g, norm, clip, hyper):
        o, a, b = self.ops, self.guard, self.guard_e
        epoch = o.param_epoch
        o.clip_adam(a["p"], g, a["m"], a["v"], norm, clip, hyper[:3].clone(), BETA1, BETA2, EPS, WD, PRESCALE,
                    health=self.health)
        o.clip_adam_ema(b["p"], g, b["m"], b["v"], b["e"], norm, clip, hyper, BETA1, BETA2, EPS, WD, PRESCALE,
                        health=self.health_e)
        assert o.param_epoch == epoch + 2            # (unconditional: the host does not know whether a pass skipped)

    def unguarded(self, g, norm, clip, hyper):
        o, a, b = self.ops, self.plain, self.plain_e
        o.clip_adam(a["p"], g, a["m"], a["v"], norm if clip > 0 else None, clip, hyper[:3].clone(), BETA1, BETA2, EPS,
                    WD, PRESCALE)
        o.clip_adam_ema(b["p"], g, b["m"], b["v"], b["e"], norm if clip > 0 else None, clip, hyper, BETA1, BETA2, EPS,
                        WD, PRESCALE)

    def assert_together(self, what):
        torch.cuda.synchronize()
        for x, y in ((self.guard, self.plain), (self.guard_e, self.plain_e)):
            for k in x:
                assert _same(x[k], y[k]), (what, k, len(x))
        assert _same(self.guard["p"], self.guard_e["p"])


# ----------------------------------------------------------------------------------------------------------------
# 1. finite steps are unchanged
# ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,off", CASES)
def test_finite_steps_are_the_unguarded_steps(dev, n, off):
    gen = torch.Generator().manual_seed(n + off)
    pair = _Pair(n, off, dev, gen)
    # clip threshold below / above the gradient norm, and no clipping (the norm is read all the same)
    for t, factor in ((1, 0.5), (2, 2.0), (3, 0.0)):
        g = _buf(n, off, dev, gen, "randn")
        g.mul_(0.1 * t)
        norm = _norm_of(g, dev)
        clip = float(norm[0]) * PRESCALE * factor
        assert (clip > 0) == (factor > 0)
        hyper = _hyper(t, 1.0 - DECAY, dev)
        before = pair.snapshot()
        pair.guarded(g, norm, clip, hyper)
        pair.unguarded(g, norm, clip, hyper)
        pair.assert_together("n=%d off=%d step %d" % (n, off, t))
        assert not _same(pair.guard["p"], before[0]["p"]) and not _same(pair.guard_e["e"], before[1]["e"])
        assert torch.isfinite(pair.guard["p"]).all()
        assert pair.health.tolist() == [0.0, 0.0] and pair.health_e.tolist() == [0.0, 0.0]


def test_guarded_passes_refuse_missing_arguments(dev):
    from deepvoice3_pytorch_amd import ops
    z = lambda k=8: torch.zeros(k, dtype=torch.float32, device=dev)
    p, g, m, v, e, hyper, health = z(), z(), z(), z(), z(), _hyper(1, 0.1, dev), z(2)
    with pytest.raises(RuntimeError, match="norm is required"):
        ops.clip_adam(p, g, m, v, None, 0.0, hyper, BETA1, BETA2, EPS, health=health)
    with pytest.raises(RuntimeError, match="norm is required"):
        ops.clip_adam_ema(p, g, m, v, e, None, 0.0, hyper, BETA1, BETA2, EPS, health=health)
    with pytest.raises(RuntimeError, match="health"):
        ops.clip_adam(p, g, m, v, z(2), 0.0, hyper, BETA1, BETA2, EPS, health=z(1))
    with pytest.raises(RuntimeError, match="expected 8"):
        ops.clip_adam(p, g, m, z(4), z(2), 0.0, hyper, BETA1, BETA2, EPS, health=health)
    with pytest.raises(RuntimeError, match="fp32"):
        ops.clip_adam(p, g, m, v, z(2), 0.0, hyper, BETA1, BETA2, EPS, health=health.double())
    torch.cuda.synchronize()
    assert health.tolist() == [0.0, 0.0] and not p.any()


# ----------------------------------------------------------------------------------------------------------------
# 2. non-finite steps touch nothing
# ----------------------------------------------------------------------------------------------------------------
def _second_trip(n):
    """an index the second trip of the grid-stride loop reaches, in both kernels: clip_adam_kernel runs
    min(4096, ceil(n / 1024)) blocks of 256 lanes, one element per lane and trip; the averaging kernel
    min(2048, ceil(n / 1024)) blocks, four elements per lane and trip (n = 1027 fits its first trip: 2 blocks x 1024)"""
    return 600 if n == 1027 else 2048 * 1024 + 5


POISON = [("nan_first", lambda n: [(0, float("nan"))]),
          ("nan_last", lambda n: [(n - 1, float("nan"))]),               # in the scalar tail
          ("nan_second_trip", lambda n: [(_second_trip(n), float("nan"))]),
          ("plus_inf", lambda n: [(n // 2, float("inf"))]),
          ("minus_inf", lambda n: [(n // 3, float("-inf"))]),
          ("finite_overflow", lambda n: [(1, 3e19), (n - 2, 3e19)])]       # every element finite, the sum of squares not


@pytest.fixture(scope="module")
def poisoned_runs(dev):
    """per size: one state, poisoned passes one after the other (each must leave it alone), then a finite pass.
    Computed once: {n: [(kind, untouched?, health, health_e, norm finite?)], ...} and the final comparison"""
    out = {}
    for n in (1027, BIG):
        gen = torch.Generator().manual_seed(5 * n)
        pair = _Pair(n, 0, dev, gen)
        g0 = _buf(n, 0, dev, gen, "randn")
        g0.mul_(0.1)
        rows = []
        for k, (kind, where) in enumerate(POISON):
            g = g0.clone()
            for i, val in where(n):
                assert 0 <= i < n
                g[i] = val
            norm = _norm_of(g, dev)
            hyper = _hyper(k + 1, 1.0 - DECAY, dev)
            before = pair.snapshot()
            pair.guarded(g, norm, 0.05, hyper)
            torch.cuda.synchronize()
            after = pair.snapshot()
            untouched = all(_same(b[key], a[key]) for b, a in zip(before, after) for key in b)
            rows.append((kind, untouched, pair.health.tolist(), pair.health_e.tolist(), float(norm[0]),
                         bool(torch.isfinite(g).all())))
        # a finite pass on the same buffers: applies, as the unguarded kernels do from the same state
        for s, d in ((pair.guard, pair.plain), (pair.guard_e, pair.plain_e)):
            for key in s:
                d[key].copy_(s[key])
        norm = _norm_of(g0, dev)
        hyper = _hyper(len(POISON) + 1, 1.0 - DECAY, dev)
        before = pair.snapshot()
        pair.guarded(g0, norm, 0.05, hyper)
        pair.unguarded(g0, norm, 0.05, hyper)
        torch.cuda.synchronize()
        together = all(_same(x[key], y[key]) for x, y in ((pair.guard, pair.plain), (pair.guard_e, pair.plain_e))
                       for key in x)
        moved = not _same(pair.guard["p"], before[0]["p"]) and not _same(pair.guard_e["e"], before[1]["e"])
        out[n] = dict(rows=rows, together=together, moved=moved, health=pair.health.tolist(),
                      health_e=pair.health_e.tolist(), finite=bool(torch.isfinite(pair.guard_e["p"]).all()))
    return out


@pytest.mark.parametrize("n", [1027, BIG])
@pytest.mark.parametrize("k", range(len(POISON)), ids=[kind for kind, _ in POISON])
def test_a_step_that_is_not_finite_touches_nothing(poisoned_runs, n, k):
    kind, untouched, health, health_e, norm, g_finite = poisoned_runs[n]["rows"][k]
    assert kind == POISON[k][0]
    assert H.skips(norm), (kind, norm)
    assert g_finite == (kind == "finite_overflow")
    assert untouched, (n, kind)
    assert health == [float(k + 1), 1.0] and health_e == [float(k + 1), 1.0]      # rose by exactly one


@pytest.mark.parametrize("n", [1027, BIG])
def test_the_next_finite_step_applies(poisoned_runs, n):
    r = poisoned_runs[n]
    assert r["together"] and r["moved"] and r["finite"]
    assert r["health"] == [float(len(POISON)), 0.0] and r["health_e"] == [float(len(POISON)), 0.0]


# ----------------------------------------------------------------------------------------------------------------
# 3. the table
# ----------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def table(dev):
    from deepvoice3_pytorch_amd import ops, train_step
    sizes = TABLE_SIZES
    offs, total = [], 0
    for n in sizes:
        offs.append(total)
        total += (n + 3) // 4 * 4
    gen = torch.Generator().manual_seed(99)
    g, p = torch.randn(total, generator=gen), torch.randn(total, generator=gen)
    m = 0.1 * torch.randn(total, generator=gen)
    v = torch.empty(total).uniform_(0.0, 0.01, generator=gen)
    pad = torch.ones(total, dtype=torch.bool)
    for o, n in zip(offs, sizes):
        pad[o:o + n] = False
    assert int(pad.sum()) == total - sum(sizes) > 0
    for a in (g, p, m, v):
        a[pad] = float("nan")                      # the pads are in no chunk: a NaN there must not show anywhere
    at = {n: o for o, n in zip(offs, sizes)}
    g[at[1027] + 1026] = float("nan")
    g[at[4097]] = float("inf")
    g[at[5] + 2] = float("-inf")
    hyper = _hyper(3, 1.0 - DECAY, dev)
    chunks, ranges = train_step.arena_chunks(offs, sizes)
    H.check_chunks(chunks.numpy(), ranges.numpy(), offs, sizes, total)
    dv = [a.to(dev) for a in (p, g, m, v)]
    cd, rd = chunks.to(dev), ranges.to(dev)
    run = lambda health, **kw: ops.arena_stats(dv[0], dv[1], dv[2], dv[3], hyper, health, cd, rd,
                                               grad_prescale=PRESCALE, eps=EPS, **kw)
    scratch = torch.empty(chunks.shape[0] * 6, dtype=torch.float32, device=dev)
    got = dict(none=run(None), again=run(None, scratch=scratch),
               applied=run(torch.tensor([3.0, 0.0], device=dev), scratch=scratch),
               skipped=run(torch.tensor([3.0, 1.0], device=dev), scratch=scratch))
    torch.cuda.synchronize()
    ref = lambda skipped: H.columns(p.numpy(), g.numpy(), m.numpy(), v.numpy(), hyper.cpu().numpy()[:3], offs, sizes,
                                    grad_prescale=PRESCALE, eps=EPS, skipped=skipped)
    return dict(got={k: t.cpu() for k, t in got.items()}, want=ref(False), want_skipped=ref(True), sizes=sizes)


def _check_table(got, want, what):
    got = got.numpy()
    assert got.dtype == np.float64 and got.shape == want.shape
    assert np.isfinite(got).all(), what
    for c in (1, 2, 4):
        assert (got[:, c] == want[:, c]).all(), (what, H.COLUMNS[c], got[:, c], want[:, c])
    for c in (0, 3, 5):
        rel = np.abs(got[:, c] - want[:, c]) / np.maximum(want[:, c], 1e-300)
        rel[want[:, c] == 0] = np.abs(got[:, c])[want[:, c] == 0]
        print("%s %s: worst relative error %.3g (bound %.3g)" % (what, H.COLUMNS[c], rel.max(), H.SUM_RTOL))
        assert (rel <= H.SUM_RTOL).all(), (what, H.COLUMNS[c], rel)


def test_table_against_the_f64_reference(table):
    assert tuple(table["got"]["none"].shape) == (len(TABLE_SIZES), 6)
    _check_table(table["got"]["none"], table["want"], "table")
    bad = table["got"]["none"][:, 2].tolist()
    assert bad == [1.0 if n in (1027, 4097, 5) else 0.0 for n in table["sizes"]]
    assert (table["got"]["none"][:, 5] > 0).all()


def test_table_of_a_skipped_step_shows_no_update(table):
    _check_table(table["got"]["skipped"], table["want_skipped"], "skipped")
    assert (table["got"]["skipped"][:, 5] == 0).all()
    assert torch.equal(table["got"]["skipped"][:, :5], table["got"]["none"][:, :5])


def test_table_is_deterministic(table):
    a = table["got"]["none"]
    for k in ("again", "applied"):
        assert torch.equal(a.view(torch.int64), table["got"][k].view(torch.int64)), k


def test_table_refuses_bad_arguments(dev):
    from deepvoice3_pytorch_amd import ops, train_step
    z = lambda k: torch.zeros(k, dtype=torch.float32, device=dev)
    chunks, ranges = (t.to(dev) for t in train_step.arena_chunks([0, 8], [5, 8]))
    hyper = _hyper(1, 0.1, dev)
    with pytest.raises(RuntimeError, match="expected 16"):
        ops.arena_stats(z(16), z(16), z(12), z(16), hyper, None, chunks, ranges)
    with pytest.raises(RuntimeError, match="int64"):
        ops.arena_stats(z(16), z(16), z(16), z(16), hyper, None, chunks.int(), ranges)
    with pytest.raises(RuntimeError, match="int64"):
        ops.arena_stats(z(16), z(16), z(16), z(16), hyper, None, chunks.cpu(), ranges)
    with pytest.raises(RuntimeError, match="scratch"):
        ops.arena_stats(z(16), z(16), z(16), z(16), hyper, None, chunks, ranges, scratch=z(6))
    with pytest.raises(RuntimeError, match="16-byte"):
        ops.arena_stats(z(17)[1:], z(16), z(16), z(16), hyper, None, chunks, ranges)
    # a row that points outside the arena is read as empty, not followed
    wild = chunks.clone()
    wild[1, 0] = 1 << 40
    out = ops.arena_stats(z(16) + 1, z(16), z(16), z(16) + 1, hyper, None, wild, ranges)
    assert out[:, 3].tolist() == [5.0, 0.0]


# ----------------------------------------------------------------------------------------------------------------
# 4. - 6. the trainers
# ----------------------------------------------------------------------------------------------------------------
def _trainer(dev, seed=0, hp=HP, split=None, **cfg):
    from deepvoice3_pytorch_amd import builder, train_step
    torch.manual_seed(seed)
    model = builder.deepvoice3(**hp).to(dev)
    tc = train_step.TrainConfig(max_positions=hp["max_positions"], outputs_per_step=hp["r"],
                                downsample_step=hp["downsample_step"], **cfg)
    return train_step.Trainer(model, tc, **(split or {}))


def _batch(dev, hp=HP, B=4, seed=3):
    import bench
    from deepvoice3_pytorch_amd import train_step
    rng = np.random.RandomState(seed)
    tl, fl = rng.randint(9, 27, B), rng.randint(40, 117, B)
    bt = bench.synth_batch(rng, B, 0, 0, hp, lengths=(tl, fl))
    return train_step.Batch.from_collate(bt["text"], bt["input_lengths"], bt["mel"], bt["y"], bt["text_positions"],
                                         bt["frame_positions"], bt["done"], bt["target_lengths"], None,
                                         downsample_step=hp["downsample_step"], device=dev, r=hp["r"])


def _poisoned(batch):
    """the same batch with one NaN in its linear target: the target enters only the loss, so the forward GEMM operands
    stay finite and the NaN reaches the step through the loss gradient (frame 5: the loss compares the prediction
    with the target r frames later, so the first r target frames are never read)"""
    from deepvoice3_pytorch_amd import train_step
    b = train_step.clone_batch(batch)
    b.y[0, 5, 0] = float("nan")
    return b


def _state(tr):
    torch.cuda.synchronize()
    a = tr.arena
    return dict(flat=a.flat.clone(), m=a.exp_avg.clone(), v=a.exp_avg_sq.clone(),
                ema=None if a.ema is None else a.ema.clone())


def _states_same(a, b):
    return all(_same(a[k], b[k]) for k in a)


def _finite(st):
    return all(bool(torch.isfinite(t).all()) for t in st.values() if t is not None)


def _scalars(scal):
    return {k: v.detach().clone() for k, v in scal.items()}


@pytest.fixture(scope="module")
def eager(dev):
    """Per averaging setting (off / on): twin trainers from one seed, the guard on and off, over STEPS clean steps, one
    poisoned step and (guard on) one more clean step.  Computed once; the tests below only read it."""
    out = {}
    for name, cfg in (("plain", {}), ("ema", dict(ema_decay=DECAY))):
        on, off = _trainer(dev, skip_nonfinite=True, **cfg), _trainer(dev, **cfg)
        batch = _batch(dev)
        bad = _poisoned(batch)
        r = dict(states_on=[_state(on)], states_off=[_state(off)], scal_on=[], scal_off=[], health=[])
        try:
            for _ in range(STEPS):
                r["scal_on"].append(_scalars(on.step(batch)))
                r["scal_off"].append(_scalars(off.step(batch)))
                r["states_on"].append(_state(on))
                r["states_off"].append(_state(off))
                r["health"].append(on.health())
            names, tab = on.tensor_stats()
            r["names"], r["n_tensors"] = names, len(on.arena.params)
            r["table_clean"] = tab.cpu()
            r["table_clean_again"] = off.tensor_stats()[1].cpu()         # (works without the guard too)
            a = on.arena
            r["arena"] = dict(offsets=list(a.offsets), sizes=list(a.sizes), p=a.flat.cpu().numpy(),
                              g=a.grad.cpu().numpy(), m=a.exp_avg.cpu().numpy(), v=a.exp_avg_sq.cpu().numpy(),
                              hyper=on.hyper.cpu().numpy())
            r["steps_before"] = (on.global_step, on.adam_step)
            r["scal_bad_on"] = _scalars(on.step(bad))
            r["state_bad_on"] = _state(on)
            r["health_bad"] = on.health()
            r["steps_after"] = (on.global_step, on.adam_step)
            r["table_bad"] = on.tensor_stats()[1].cpu()
            r["scal_bad_off"] = _scalars(off.step(bad))
            r["state_bad_off"] = _state(off)
            r["scal_next_on"] = _scalars(on.step(batch))
            r["state_next_on"] = _state(on)
            r["health_next"] = on.health()
            with pytest.raises(RuntimeError, match="guard is off"):
                off.health()
            if on.ema_on:
                with on.averaged():
                    with pytest.raises(RuntimeError, match="averaged"):
                        on.tensor_stats()
        finally:
            on.close()
            off.close()
        out[name] = r
    return out


@pytest.mark.parametrize("avg", ["plain", "ema"])
def test_eager_clean_steps_are_unchanged(eager, avg):
    r = eager[avg]
    for t in range(STEPS + 1):
        assert _states_same(r["states_on"][t], r["states_off"][t]), t
    assert not _same(r["states_on"][STEPS]["flat"], r["states_on"][0]["flat"])
    for s_on, s_off, h in zip(r["scal_on"], r["scal_off"], r["health"]):
        assert sorted(set(s_on) - set(s_off)) == ["step_skipped"] and not set(s_off) - set(s_on)
        for k in s_off:
            assert _same(s_on[k], s_off[k]), k
        assert s_on["step_skipped"].dim() == 0 and float(s_on["step_skipped"]) == 0.0
        assert h == dict(skipped_steps=0, last_step_skipped=False)


@pytest.mark.parametrize("avg", ["plain", "ema"])
def test_eager_poisoned_step_is_refused(eager, avg):
    r = eager[avg]
    assert not np.isfinite(float(r["scal_bad_on"]["grad_norm"]))
    assert _states_same(r["state_bad_on"], r["states_on"][STEPS])
    assert float(r["scal_bad_on"]["step_skipped"]) == 1.0
    assert r["health_bad"] == dict(skipped_steps=1, last_step_skipped=True)
    # the host's counters do not know: they advance as on any other step
    assert r["steps_after"] == (r["steps_before"][0] + 1, r["steps_before"][1] + 1)
    # the following clean step applies, and everything stays finite
    assert not _same(r["state_next_on"]["flat"], r["state_bad_on"]["flat"])
    assert _finite(r["state_next_on"])
    assert float(r["scal_next_on"]["step_skipped"]) == 0.0 and np.isfinite(float(r["scal_next_on"]["loss"]))
    assert r["health_next"] == dict(skipped_steps=1, last_step_skipped=False)
    # without the option the same step ends in the parameters (today's behaviour: the test has teeth)
    assert "step_skipped" not in r["scal_bad_off"]
    assert not torch.isfinite(r["state_bad_off"]["flat"]).all()
    if avg == "ema":
        assert not torch.isfinite(r["state_bad_off"]["ema"]).all()


@pytest.mark.parametrize("form", ["segments", "single"])
def test_graphed_trainer_refuses_the_poisoned_replay(dev, form):
    """one warm-up step (eager, in the constructor), then a clean, a poisoned and a clean replay"""
    from deepvoice3_pytorch_amd import train_step
    tr = _trainer(dev, skip_nonfinite=True, ema_decay=DECAY)
    if form == "segments" and tr.side_stream is None:
        tr.close()
        pytest.skip("no second stream: the step is not captured in segments here")
    batch = _batch(dev)
    bad = _poisoned(batch)
    g = train_step.GraphedTrainer(tr, train_step.clone_batch(batch), warmup=1, split_streams=(form == "segments"))
    try:
        assert g.split == (form == "segments")
        s1 = g.step(batch)
        assert float(s1["step_skipped"]) == 0.0
        before = _state(tr)
        s2 = g.step(bad)
        after = _state(tr)
        assert float(s2["step_skipped"]) == 1.0 and not np.isfinite(float(s2["grad_norm"]))
        assert g.health() == dict(skipped_steps=1, last_step_skipped=True)
        names, tab = g.tensor_stats()
        tab = tab.cpu()
        s3 = g.step(batch)
        final = _state(tr)
        assert float(s3["step_skipped"]) == 0.0
        assert g.health() == dict(skipped_steps=1, last_step_skipped=False)
    finally:
        g.close()
        tr.close()
    assert _states_same(before, after)
    assert _finite(final) and not _same(final["flat"], after["flat"])
    assert len(names) == tab.shape[0] and (tab[:, 5] == 0).all() and (tab[:, 2] > 0).any()
    if form == "single":
        # an eager trainer driven through the same batches: the warm-up step, then what the three replays were given
        tw = _trainer(dev, skip_nonfinite=True, ema_decay=DECAY)
        try:
            for b in (batch, batch, bad, batch):
                tw.step(b)
            want = _state(tw)
            assert tw.health() == dict(skipped_steps=1, last_step_skipped=False)
        finally:
            tw.close()
        assert _states_same(final, want)


def test_lattice_replay_refuses_the_poisoned_replay(dev):
    from deepvoice3_pytorch_amd import data, train_step
    rng = np.random.RandomState(11)
    items = []
    for tl, fl in ((20, 100), (25, 90)):
        text = np.concatenate([rng.randint(2, HP["n_vocab"], tl - 1), [1]]).astype(np.int32)
        items.append((text, rng.rand(fl, HP["mel_dim"]).astype(np.float32), rng.rand(fl, HP["linear_dim"]).astype(np.float32)))
    tr = _trainer(dev, seed=1, skip_nonfinite=True, ema_decay=DECAY)
    rep = train_step.LatticeReplay(tr)
    try:
        b = data.device_collate(data.pack_batch(items), dev, 1, 4, lattice=(16, 8))
        bad = _poisoned(b)
        s1 = rep.step(b)
        assert float(s1["step_skipped"]) == 0.0
        before = _state(tr)
        s2 = rep.step(bad)
        after = _state(tr)
        assert float(s2["step_skipped"]) == 1.0
        rep.step(b)
        final = _state(tr)
        assert rep.stats["captures"] == 1 and rep.stats["replays"] == 3
        assert rep.health() == dict(skipped_steps=1, last_step_skipped=False)
        names, tab = rep.tensor_stats()
        assert len(names) == len(tr.arena.params) and (tab[:, 5] > 0).all()
    finally:
        rep.close()
        tr.close()
    assert _states_same(before, after)
    assert _finite(final) and not _same(final["flat"], after["flat"])


@pytest.mark.parametrize("avg", ["plain", "ema"])
def test_tensor_stats_on_the_small_model(eager, avg):
    r = eager[avg]
    tab = r["table_clean"]
    assert len(r["names"]) == r["n_tensors"] == tab.shape[0] and tab.shape[1] == 6 and tab.dtype == torch.float64
    assert len(set(r["names"])) == len(r["names"])
    assert torch.equal(tab, r["table_clean_again"])          # the twin without the guard: the same state, the same table
    a = r["arena"]
    want = H.columns(a["p"], a["g"], a["m"], a["v"], a["hyper"][:3], a["offsets"], a["sizes"], grad_prescale=1.0,
                     eps=1e-6)
    _check_table(tab, want, "small model")
    # the sum of column 0 and the step's grad_norm are sums of the same squares in different orders
    total = float(tab[:, 0].sum())
    gn2 = float(r["scal_on"][-1]["grad_norm"].double()) ** 2
    g64 = float((a["g"].astype(np.float64) ** 2).sum())
    print("sum of grad_sumsq %.9g, grad_norm^2 %.9g, float64 %.9g" % (total, gn2, g64))
    assert abs(total - g64) <= H.SUM_RTOL * g64
    assert abs(total - gn2) <= H.SUM_RTOL * gn2
    assert (tab[:, 2] == 0).all()
    assert (tab[:, 5] > 0).all(), [n for n, u in zip(r["names"], tab[:, 5].tolist()) if not u > 0]
    # after the poisoned step, refused: the non-finite elements show per tensor, and nothing moved
    bad = r["table_bad"]
    assert any(c > 0 for n, c in zip(r["names"], bad[:, 2].tolist()) if n.startswith("postnet."))
    assert (bad[:, 5] == 0).all()
    assert torch.equal(bad[:, 3:5], tab[:, 3:5])             # the parameters are those of the last clean step

# coding: utf-8
"""-m gpu: weight averaging -- the moving average of the parameters taken inside the fused clip + Adam
pass (dv3_clip_adam_ema_f32), the in-place exchange (dv3_swap_f32) and what train_step builds on them.

  1. kernel: p, m, v bit for bit as ops.clip_adam writes them, the average within 4 * 2^-24 * max(|e|, |p'|) of the
     float64 update (tests/ema_ref.py: three fp32 roundings; the kernel's FMA drops one);
  2. the end points 1 - d = 0 and 1 - d = 1, exactly;
  3. the exchange: exact, its own inverse, the same or overlapping buffers refused;
  4. eager trainer: averaging on leaves the trajectory bit for bit as it was, the average follows the float64 recursion;
  5. GraphedTrainer (segmented, single graph) and LatticeReplay carry the average, each step with its own decay;
  6. averaged(): evaluation and synthesis see the average, the raw weights return bit for bit;
  7. resume from a checkpoint; 8. a split training mode."""
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tests import ema_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu

# the small model of tests/test_gpu_valid_lengths.py / test_gpu_evaluate.py (dropout 0: eager steps and replays then
# need no seed bookkeeping to be comparable bit for bit)
HP = dict(n_vocab=30, embed_dim=32, mel_dim=16, linear_dim=17, r=1, downsample_step=4, padding_idx=0, dropout=0.0,
          kernel_size=3, encoder_channels=64, decoder_channels=32, converter_channels=32, use_memory_mask=False,
          force_monotonic_attention=False, use_decoder_state_for_postnet_input=True, key_projection=True,
          value_projection=True, max_positions=256)
DECAY, STEPS = 0.9, 4
# 4096 * 1024 + 1029: more than one trip of the grid-stride loop at 4 and at 16 bytes per lane, and a scalar tail
SIZES = [1, 3, 4, 5, 1027, 4096 * 1024 + 1029]
CASES = [(n, 0) for n in SIZES] + [(1027, 1)]          # (n, offset in elements: 1 = not 16-byte aligned)
BETA1, BETA2, EPS, WD, PRESCALE = 0.5, 0.9, 1e-6, 0.01, 0.125


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


def _bits(t):
    t = t.detach().contiguous()
    return t.view(torch.int32) if t.dtype == torch.float32 else t


def _same(a, b):
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


def _check_average(e_new, e_old, p_new, w32, what):
    """|e' - float64 update| <= 4 * 2^-24 * max(|e|, |p'|), element-wise, from the kernel's own p' and the previous e"""
    e0, p1 = e_old.cpu().numpy(), p_new.cpu().numpy()
    err = np.abs(e_new.cpu().numpy().astype(np.float64) - R.update(e0, p1, float(w32)))
    bound = R.bound(e0, p1)
    worst = float((err / np.maximum(bound, 1e-300)).max())
    print("%s: worst |e' - f64| / bound = %.3f" % (what, worst))
    assert (err <= bound).all(), (what, worst)


# ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,off", CASES)
def test_kernel_matches_clip_adam_and_the_f64_average(dev, n, off):
    from deepvoice3_pytorch_amd import ops
    gen = torch.Generator().manual_seed(n + off)
    p, m, e = (_buf(n, off, dev, gen, "randn") for _ in range(3))
    v = _buf(n, off, dev, gen, "second")
    m.mul_(0.1)
    p0, m0, v0 = p.clone(), m.clone(), v.clone()           # the copies ops.clip_adam steps
    partial, norm = torch.empty(1024, device=dev), torch.zeros(2, device=dev)
    for t, factor in ((1, 0.5), (2, 2.0), (3, 0.25)):       # clip threshold below / above / below the gradient norm
        g = _buf(n, off, dev, gen, "randn")
        g.mul_(0.1 * t)
        ops.grad_sqnorm(g.clone(), partial, norm)           # (of a copy: grad_sqnorm wants a 16-byte aligned arena)
        clip = float(norm[0]) * PRESCALE * factor
        assert clip > 0
        hyper = _hyper(t, 1.0 - R.decay_at(t, DECAY), dev)
        e_old = e.clone()
        epoch = ops.param_epoch
        ops.clip_adam_ema(p, g, m, v, e, norm, clip, hyper, BETA1, BETA2, EPS, WD, PRESCALE)
        assert ops.param_epoch == epoch + 1
        ops.clip_adam(p0, g, m0, v0, norm, clip, hyper[:3].clone(), BETA1, BETA2, EPS, WD, PRESCALE)
        torch.cuda.synchronize()
        assert _same(p, p0) and _same(m, m0) and _same(v, v0), (n, off, t)
        assert torch.isfinite(p).all()
        _check_average(e, e_old, p, hyper[3].item(), "n=%d off=%d step %d" % (n, off, t))
        assert not _same(e, e_old)


@pytest.mark.parametrize("n,off", [(5, 0), (1027, 0), (1027, 1)])
def test_kernel_end_points(dev, n, off):
    """hyper[3] = 0 leaves the average bit-unchanged, hyper[3] = 1 makes it the updated parameter"""
    from deepvoice3_pytorch_amd import ops
    gen = torch.Generator().manual_seed(7 * n + off)
    p, m, e, g = (_buf(n, off, dev, gen, "randn") for _ in range(4))
    v = _buf(n, off, dev, gen, "second")
    e.mul_(1e-3)                # far from p: e + (p' - e) would round
    e_old = e.clone()
    ops.clip_adam_ema(p, g, m, v, e, None, 0.0, _hyper(1, 0.0, dev), BETA1, BETA2, EPS, WD, 1.0)
    assert _same(e, e_old) and not _same(p, e)
    ops.clip_adam_ema(p, g, m, v, e, None, 0.0, _hyper(2, 1.0, dev), BETA1, BETA2, EPS, WD, 1.0)
    assert _same(e, p)


@pytest.mark.parametrize("n,off", CASES)
def test_swap_is_exact_and_its_own_inverse(dev, n, off):
    from deepvoice3_pytorch_amd import ops
    gen = torch.Generator().manual_seed(3 * n + off)
    a, b = _buf(n, off, dev, gen, "randn"), _buf(n, off, dev, gen, "randn")
    a0, b0 = a.clone(), b.clone()
    epoch = ops.param_epoch
    ops.swap_(a, b)
    assert ops.param_epoch == epoch + 1
    assert _same(a, b0) and _same(b, a0)
    ops.swap_(a, b)
    assert _same(a, a0) and _same(b, b0)


def test_swap_refuses_the_same_or_overlapping_buffers(dev):
    from deepvoice3_pytorch_amd import ops
    base = torch.arange(64, dtype=torch.float32, device=dev)
    want = base.clone()
    with pytest.raises(RuntimeError, match="same or overlap"):
        ops.swap_(base[:32], base[:32])
    with pytest.raises(RuntimeError, match="same or overlap"):
        ops.swap_(base[:32], base[4:36])
    with pytest.raises(RuntimeError):
        ops.swap_(base[:32], base[32:63])
    with pytest.raises(RuntimeError, match="overlaps"):
        ops.clip_adam_ema(base[:32], base[32:], base[32:], base[32:], base[8:40], None, 0.0, base[:4], BETA1, BETA2, EPS)
    assert torch.equal(base, want)


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


def _state(tr):
    torch.cuda.synchronize()
    a = tr.arena
    return dict(flat=a.flat.clone(), m=a.exp_avg.clone(), v=a.exp_avg_sq.clone(),
                ema=None if a.ema is None else a.ema.clone())


def _scalars(scal):
    return {k: v.detach().clone() for k, v in scal.items()}


@pytest.fixture(scope="module")
def eager(dev):
    """STEPS eager steps on one batch, averaging on and (a twin from the same seed) off: the state after every step.
    Computed once; the tests below only read it."""
    out = {}
    for name, cfg in (("on", dict(ema_decay=DECAY)), ("off", {})):
        tr = _trainer(dev, **cfg)
        batch = _batch(dev)
        states, scalars = [_state(tr)], []
        for _ in range(STEPS):
            scalars.append(_scalars(tr.step(batch)))
            states.append(_state(tr))
        tr.close()
        out[name] = (states, scalars)
    return out


def test_eager_trainer_same_trajectory_and_the_f64_recursion(dev, eager):
    (on, s_on), (off, s_off) = eager["on"], eager["off"]
    assert off[0]["ema"] is None and _same(on[0]["ema"], on[0]["flat"])
    for t in range(1, STEPS + 1):
        for k in ("flat", "m", "v"):
            assert _same(on[t][k], off[t][k]), (t, k)
        assert sorted(s_on[t - 1]) == sorted(s_off[t - 1])
        for k in s_on[t - 1]:
            assert _same(s_on[t - 1][k], s_off[t - 1][k]), (t, k)
        w32 = np.float32(1.0 - R.decay_at(t, DECAY))
        _check_average(on[t]["ema"], on[t - 1]["ema"], on[t]["flat"], w32, "eager step %d" % t)
    assert not _same(on[STEPS]["ema"], on[STEPS]["flat"]) and not _same(on[STEPS]["flat"], on[0]["flat"])


@pytest.mark.parametrize("form", ["segments", "single"])
def test_graphed_trainer_carries_the_average(dev, eager, form):
    """one warm-up step (eager, in the constructor) and STEPS - 1 replays: a decay captured as a constant would show in
    the first replay (d_1 = 2/11, d_2 = 3/12, ...)"""
    from deepvoice3_pytorch_amd import train_step
    tr = _trainer(dev, ema_decay=DECAY)
    if form == "segments" and tr.side_stream is None:
        tr.close()
        pytest.skip("no second stream: the step is not captured in segments here")
    g = train_step.GraphedTrainer(tr, _batch(dev), warmup=1, split_streams=(form == "segments"))
    try:
        assert g.split == (form == "segments")
        for _ in range(STEPS - 1):
            g.step()
        got = _state(tr)
        assert tr.adam_step == STEPS
    finally:
        g.close()
        tr.close()
    want = eager["on"][0][STEPS]
    assert _same(got["flat"], want["flat"])
    assert _same(got["ema"], want["ema"])


def test_lattice_replay_carries_the_average(dev):
    """STEPS steps over batches of two lattice shapes, replayed, against eager steps on the same padded batches"""
    from deepvoice3_pytorch_amd import data, train_step
    rng = np.random.RandomState(11)
    items = []
    for tl, fl in ((20, 100), (25, 90), (13, 50), (12, 44)):
        text = np.concatenate([rng.randint(2, HP["n_vocab"], tl - 1), [1]]).astype(np.int32)
        items.append((text, rng.rand(fl, HP["mel_dim"]).astype(np.float32), rng.rand(fl, HP["linear_dim"]).astype(np.float32)))
    groups = [items[0:2], items[2:4], items[0:2], items[2:4]]
    assert len(groups) == STEPS
    results = []
    for mode in ("eager", "lattice"):
        tr = _trainer(dev, seed=1, ema_decay=DECAY)
        rep = train_step.LatticeReplay(tr) if mode == "lattice" else None
        try:
            for grp in groups:
                b = data.device_collate(data.pack_batch(grp), dev, 1, 4, lattice=(16, 8))
                (rep or tr).step(b)
            results.append(_state(tr))
            if rep is not None:
                assert rep.stats["captures"] == 2 and rep.stats["replays"] == STEPS
                with tr.averaged():
                    with pytest.raises(RuntimeError, match="averaged"):
                        rep.step(b)
        finally:
            if rep is not None:
                rep.close()
            tr.close()
    want, got = results
    assert not _same(want["ema"], want["flat"])
    assert _same(got["flat"], want["flat"])
    assert _same(got["ema"], want["ema"])


# ----------------------------------------------------------------------------------------------------------------
def test_averaged_weights_in_use(dev, tmp_path):
    from deepvoice3_pytorch_amd import audio, builder, ops, synthesis, train_step
    hp = dict(HP, linear_dim=257)                     # tts_batch inverts the spectrogram: 512-point frames
    cfg = dict(lr_schedule=None, initial_learning_rate=2e-3)
    acfg = audio.AudioConfig(fft_size=512, hop_size=128, griffin_lim_iters=1)
    seqs = [[5, 9, 3, 17, 22, 4, 1], [11, 2, 8, 1]]
    tr = _trainer(dev, hp=hp, ema_decay=DECAY, **cfg)
    twin = _trainer(dev, hp=hp, ema_decay=DECAY, **cfg)
    batch = _batch(dev, hp=hp)

    def synth(model):
        dec = model.seq2seq.decoder
        dec.min_decoder_steps = dec.max_decoder_steps = 7
        res = synthesis.tts_batch(model, seqs, audio_cfg=acfg)
        torch.cuda.synchronize()
        return [r[0].clone() for r in res]

    try:
        for _ in range(3):
            tr.step(batch)
            twin.step(batch)
        a = tr.arena
        before = _state(tr)
        mel_raw = synth(tr.model)                     # (fills the packed decode weights from the raw parameters)
        ev_raw = tr.evaluate(batch)
        ev_avg = tr.evaluate(batch, averaged=True)
        assert _same(a.flat, before["flat"]) and _same(a.ema, before["ema"])
        path = str(tmp_path / "averaged.pth")
        train_step.export_averaged(tr, path)
        with tr.averaged():
            assert _same(a.flat, before["ema"]) and _same(a.ema, before["flat"])
            for p, o, n in zip(a.params, a.offsets, a.sizes):
                assert _same(p.detach().reshape(-1), before["ema"][o:o + n])
            ev_in = tr.evaluate(batch)
            mel_in = synth(tr.model)
            with pytest.raises(RuntimeError, match="averaged"):
                tr.step(batch)
            with pytest.raises(RuntimeError, match="nest"):
                tr.evaluate(batch, averaged=True)
        torch.cuda.synchronize()
        assert _same(a.flat, before["flat"]) and _same(a.ema, before["ema"])
        for p, o, n in zip(a.params, a.offsets, a.sizes):
            assert _same(p.detach().reshape(-1), before["flat"][o:o + n])
        mel_back = synth(tr.model)
        # a fresh model loaded from the exported file
        torch.manual_seed(123)
        t2 = train_step.Trainer(builder.deepvoice3(**hp).to(dev), train_step.TrainConfig(
            max_positions=hp["max_positions"], outputs_per_step=1, downsample_step=4, **cfg))
        try:
            train_step.load_checkpoint(path, t2, reset_optimizer=True)
            ev_file = t2.evaluate(batch)
            mel_file = synth(t2.model)
        finally:
            t2.close()
        assert sorted(ev_in) == sorted(ev_avg) == sorted(ev_file)
        for k in ev_in:
            assert _same(ev_in[k], ev_avg[k]) and _same(ev_in[k], ev_file[k]), k
        assert not _same(ev_in["loss"], ev_raw["loss"])
        for x, y, z, w in zip(mel_in, mel_file, mel_raw, mel_back):
            assert x.shape[0] >= 1 and x.shape[1] == hp["mel_dim"] and torch.isfinite(x).all()
            assert _same(x, y)                        # the exchange reached the packed decode weights ...
            assert not _same(x, z)                    # ... which held the raw parameters before ...
            assert _same(z, w)                        # ... and hold them again afterwards
        # the next step: as the twin's, which never exchanged anything
        s1, s2 = _scalars(tr.step(batch)), _scalars(twin.step(batch))
        got, want = _state(tr), _state(twin)
        for k in got:
            assert _same(got[k], want[k]), k
        for k in s1:
            assert _same(s1[k], s2[k]), k
    finally:
        tr.close()
        twin.close()


def test_resume_from_a_checkpoint(dev, eager):
    from deepvoice3_pytorch_amd import train_step
    tr = _trainer(dev, ema_decay=DECAY)
    batch = _batch(dev)
    try:
        for _ in range(2):
            tr.step(batch)
        ck = train_step.checkpoint_dict(tr)
    finally:
        tr.close()
    assert "ema_state_dict" in ck
    t2 = _trainer(dev, seed=5, ema_decay=DECAY)
    try:
        train_step.load_checkpoint(ck, t2)
        assert t2.adam_step == 2 and t2.global_step == 2
        for _ in range(STEPS - 2):
            t2.step(batch)
        got = _state(t2)
    finally:
        t2.close()
    want = eager["on"][0][STEPS]
    for o, n in zip(t2.arena.offsets, t2.arena.sizes):         # (the alignment pads are not state)
        assert _same(got["flat"][o:o + n], want["flat"][o:o + n])
        assert _same(got["ema"][o:o + n], want["ema"][o:o + n])


def test_split_mode_averages_the_trained_part_only(dev):
    tr = _trainer(dev, ema_decay=DECAY, split=dict(train_seq2seq=False), lr_schedule=None, initial_learning_rate=2e-3)
    batch = _batch(dev)
    try:
        s2s = [p.detach().clone() for p in tr.model.seq2seq.parameters()]
        for _ in range(2):
            tr.step(batch)
        st = _state(tr)
        assert not _same(st["ema"], st["flat"])
        post = set(id(p) for p in tr.model.postnet.parameters())
        assert all(id(p) in post for p in tr.arena.params)
        with tr.averaged():
            for p, q in zip(tr.model.seq2seq.parameters(), s2s):
                assert _same(p, q)
            for p, o, n in zip(tr.arena.params, tr.arena.offsets, tr.arena.sizes):
                assert _same(p.detach().reshape(-1), st["ema"][o:o + n])
        assert _same(tr.arena.flat, st["flat"])
    finally:
        tr.close()

# coding: utf-8
"""-m gpu: token timings through the synthesis entry points and forced alignment of a training batch.

  1. tts_batch(timings=True) on toy models of both decoder families: every timing dict is ops.monotonic_path on the
     utterance's own returned alignment, bit for bit, and the dict the utterance gets in a batch of one; the spans end
     at steps x seconds_per_step; with diagnostics the dict is the sixth element; timings=False changes nothing;
  2. RollingSynthesizer(timings=True) with fewer slots than utterances: per ticket the dicts of tts_batch;
  3. train_step.align_batch on a Trainer and on a LatticeReplay over a two-item ragged batch: the search over the
     attention of an eval-mode forward of the same batch, nothing of the training state touched, the next step's scalars
     as without the call.
"""
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tests.test_gpu_rolling_decode import NY_HP, DV3_HP  # noqa: E402  (the toy hyper-parameters)

pytestmark = pytest.mark.gpu

KEYS = ("durations", "end", "path", "start", "summary")
STEPS = 40                                      # every utterance decodes STEPS + 1 steps: the done flag is out of the rule
LENS = [31, 9, 23, 4, 17, 12]


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


def _toy(family, dev):
    from deepvoice3_pytorch_amd import builder, audio
    torch.manual_seed(3)
    make, hp = dict(nyanko=(builder.nyanko, NY_HP), deepvoice3=(builder.deepvoice3, DV3_HP))[family]
    hp = dict(hp, linear_dim=257)                                 # the bins of a 512-point FFT: results end in Griffin-Lim
    model = make(**hp).to(dev).eval()
    dec = model.seq2seq.decoder
    dec.min_decoder_steps = dec.max_decoder_steps = STEPS
    cfg = audio.AudioConfig(fft_size=512, hop_size=128, sample_rate=16000, griffin_lim_iters=2)
    return model, hp, cfg


def _seqs(hp):
    rng = np.random.RandomState(5)
    return [rng.randint(2, hp["n_vocab"], s).tolist() for s in LENS]


def _bits(t):
    t = t.contiguous()
    return t.view(torch.int64) if t.dtype == torch.float64 else t.view(torch.int32)


def _same(a, b, what):
    assert sorted(a) == sorted(b) == list(KEYS), what
    for k in KEYS:
        assert a[k].dtype == b[k].dtype and a[k].shape == b[k].shape, (what, k, a[k].shape, b[k].shape)
        if not torch.equal(_bits(a[k]), _bits(b[k])):
            print("%s %s:\n  %s\n  %s" % (what, k, a[k].tolist(), b[k].tolist()))
        assert torch.equal(_bits(a[k]), _bits(b[k])), (what, k)


# ----------------------------------------------------------------------------------------------------------------------
# 1. tts_batch
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("family,advance", [("nyanko", 1), ("deepvoice3", 1), ("deepvoice3", 3)])
def test_tts_batch_timings(dev, family, advance):
    from deepvoice3_pytorch_amd import ops, synthesis
    model, hp, cfg = _toy(family, dev)
    seqs = _seqs(hp)
    up = max(hp["downsample_step"] // hp["r"], 1)                  # the converter's time upsampling (builder._dv3)
    sps = hp["r"] * up * 128 / 16000.0                             # one decoder step: r mel frames of `up` hops of 128
    plain = synthesis.tts_batch(model, seqs, audio_cfg=cfg)
    timed = synthesis.tts_batch(model, seqs, audio_cfg=cfg, timings=True, timing_advance=advance)
    both = synthesis.tts_batch(model, seqs, audio_cfg=cfg, diagnostics=True, timings=True, timing_advance=advance)
    assert len(plain) == len(timed) == len(both) == len(seqs)
    for b, (p, t, d) in enumerate(zip(plain, timed, both)):
        assert len(p) == 4 and len(t) == 5 and len(d) == 6
        for x, y, z in zip(p, t[:4], d[:4]):
            assert torch.equal(x, y) and torch.equal(x, z), (family, b)        # timings=True changes no result
        ali, tm = t[2], t[4]
        steps, n = ali.shape
        assert (steps, n) == (STEPS + 1, LENS[b])
        assert "flags" in d[4]
        _same(tm, d[5], "with diagnostics, item %d" % b)                        # the sixth element
        # the search on the utterance's own returned alignment, alone
        one = lambda v: torch.tensor([v], dtype=torch.int32, device=dev)
        out, path, dur = ops.monotonic_path(ali[None].contiguous(), one(steps), one(n), "btk", advance)
        start, end = synthesis.token_spans(dur, sps)
        alone = {"path": path[0], "durations": dur[0], "start": start[0], "end": end[0], "summary": out[0]}
        _same(tm, alone, "%s item %d against its own alignment" % (family, b))
        assert tm["path"].shape == (steps,) and tm["durations"].shape == (n,) and tm["summary"].shape == (6,)
        row = dict(zip(synthesis.TIMING_COLUMNS, tm["summary"].tolist()))
        print(family, advance, b, row, tm["durations"].tolist())
        assert row["feasible"] == 1.0 and row["steps"] == steps and row["keys"] == n
        assert int(tm["durations"].sum()) == steps
        assert tm["end"][-1].item() == steps * sps                              # exactly
        assert t[0].shape[0] == steps * hp["r"] and t[1].shape[0] == steps * hp["r"] * up
        assert tm["end"][-1].item() == t[1].shape[0] * 128 / 16000.0            # the linear frames' own time
        assert tm["start"][0].item() == 0.0 and torch.equal(tm["start"][1:], tm["end"][:-1])
        # the same utterance in a batch of one
        single = synthesis.tts_batch(model, [seqs[b]], audio_cfg=cfg, timings=True, timing_advance=advance)[0]
        _same(tm, single[4], "%s item %d against a batch of one" % (family, b))


# ----------------------------------------------------------------------------------------------------------------------
# 2. rolling admission
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("family", ["nyanko", "deepvoice3"])
def test_rolling_timings_equal_tts_batch(dev, family):
    from deepvoice3_pytorch_amd import synthesis
    model, hp, cfg = _toy(family, dev)
    seqs = _seqs(hp)
    want = synthesis.tts_batch(model, seqs, audio_cfg=cfg, timings=True)
    rs = synthesis.RollingSynthesizer(model, slots=4, max_text_len=max(LENS), audio_cfg=cfg, chunk=8, timings=True)
    tickets = [rs.submit(s) for s in seqs]
    got = {res[0]: res for res in rs.drain()}
    assert sorted(got) == tickets
    for tk in tickets:
        assert len(got[tk]) == 6
        assert got[tk][3].shape == want[tk][2].shape
        _same(got[tk][5], want[tk][4], "%s ticket %d" % (family, tk))
    # with diagnostics the dict comes after the statistics; off, the result is the five of before
    both = {r[0]: r for r in synthesis.tts_stream(model, seqs[:3], slots=2, audio_cfg=cfg, diagnostics=True, timings=True)}
    for tk in range(3):
        assert len(both[tk]) == 7 and "flags" in both[tk][5]
        _same(both[tk][6], want[tk][4], "%s stream ticket %d" % (family, tk))
    assert all(len(r) == 5 for r in synthesis.tts_stream(model, seqs[:3], slots=2, audio_cfg=cfg))
    # a program whose stored rows carry a scale (three or more attention layers) is searched on the scaled copy it
    # returns, not in place: the dict is still that of the returned alignment
    from deepvoice3_pytorch_amd import ops
    rs = synthesis.RollingSynthesizer(model, slots=4, max_text_len=max(LENS), audio_cfg=cfg, chunk=8, timings=True)
    assert rs.prog.align_scale == 1.0                             # (so the runs above read the stacked buffer in place)
    rs.prog.align_scale = 0.75
    for s in seqs[:4]:
        rs.submit(s)
    one = lambda v: torch.tensor([v], dtype=torch.int32, device=dev)
    for res in rs.drain():
        ali, tm = res[3], res[5]
        assert torch.equal(ali, want[res[0]][2] * 0.75)
        out, path, dur = ops.monotonic_path(ali[None].contiguous(), one(ali.shape[0]), one(ali.shape[1]), "btk", 1)
        assert torch.equal(tm["summary"].view(torch.int32), out[0].view(torch.int32))
        assert torch.equal(tm["path"], path[0]) and torch.equal(tm["durations"], dur[0])
        assert tm["summary"][3].item() != want[res[0]][4]["summary"][3].item()     # log 0.75 per step came in


# ----------------------------------------------------------------------------------------------------------------------
# 3. forced alignment of a training batch
# ----------------------------------------------------------------------------------------------------------------------
LHP = dict(n_vocab=30, embed_dim=32, mel_dim=16, linear_dim=17, r=1, downsample_step=4, padding_idx=0, dropout=0.05,
           kernel_size=3, encoder_channels=64, decoder_channels=32, converter_channels=32, use_memory_mask=True,
           force_monotonic_attention=False, use_decoder_state_for_postnet_input=True, key_projection=True,
           value_projection=True, max_positions=256)


def _batch(dev):
    from deepvoice3_pytorch_amd import data
    rng = np.random.RandomState(11)
    items = []
    for tl, fl in ((13, 100), (9, 62)):
        text = np.concatenate([rng.randint(2, LHP["n_vocab"], tl - 1), [1]]).astype(np.int32)
        items.append((text, rng.rand(fl, LHP["mel_dim"]).astype(np.float32), rng.rand(fl, LHP["linear_dim"]).astype(np.float32)))
    return data.device_collate(data.pack_batch(items), dev, 1, 4, lattice=(16, 8))


def _run(dev, kind, with_align):
    """step, (align_batch,) step from one initial state -> the second step's scalars, the arena, the alignment"""
    from deepvoice3_pytorch_amd import builder, ops, train_step
    ops.dropout_state.manual_seed(7)
    torch.manual_seed(0)
    model = builder.deepvoice3(**LHP).to(dev)
    trainer = train_step.Trainer(model, train_step.TrainConfig(max_positions=256, outputs_per_step=1, downsample_step=4))
    runner = train_step.LatticeReplay(trainer) if kind == "lattice" else trainer
    batch = _batch(dev)
    res = None
    try:
        runner.step(batch)
        if with_align:
            torch.cuda.synchronize()
            a = trainer.arena
            before = (trainer.global_step, trainer.adam_step, trainer._hyper_slot, ops.dropout_state.site,
                      ops.dropout_state.seed, ops.param_epoch, ops.mask_plan.plan, ops.mask_plan.last)
            state = [t.clone() for t in (a.flat, a.grad, a.exp_avg, a.exp_avg_sq)]
            flags = [m.training for m in model.modules()]
            assert model.training
            res = train_step.align_batch(runner, batch)
            torch.cuda.synchronize()
            assert before == (trainer.global_step, trainer.adam_step, trainer._hyper_slot, ops.dropout_state.site,
                              ops.dropout_state.seed, ops.param_epoch, ops.mask_plan.plan, ops.mask_plan.last)
            for x, y in zip(state, (a.flat, a.grad, a.exp_avg, a.exp_avg_sq)):
                assert torch.equal(x, y)
            assert flags == [m.training for m in model.modules()] and ops.valid is None
            # the same search on the attention of an eval-mode forward of the same batch
            model.eval()
            try:
                with torch.no_grad():
                    ops.valid = batch.valid
                    attn = model(batch.text, batch.mel, speaker_ids=None, text_positions=batch.text_positions,
                                 frame_positions=batch.frame_positions, input_lengths=batch.input_lengths)[2]
            finally:
                ops.valid = None
                for m, f in zip(model.modules(), flags):
                    m.training = f
            assert attn.dim() == 4 and attn.shape[1] == 2
            want = ops.monotonic_path(attn, batch.decoder_lengths, batch.input_lengths, "lbtk", 1)
            wide = train_step.align_batch(runner, batch, max_advance=2)
            torch.cuda.synchronize()
            for x, y in zip(res, want):
                assert torch.equal(x.view(torch.int32), y.view(torch.int32))
            out, path, dur = (t.cpu() for t in res)
            tl, dl = batch.input_lengths.tolist(), batch.decoder_lengths.tolist()
            print(kind, "layers", attn.shape[0], "out", out.tolist(), "wide", wide[0].tolist())
            assert out.shape == (2, 6) and path.shape == (2, attn.shape[2]) and dur.shape == (2, attn.shape[3])
            for b in range(2):
                assert out[b, :3].tolist() == [1.0, dl[b], tl[b]]
                assert int(dur[b].sum()) == dl[b] and not dur[b, tl[b]:].any() and (path[b, dl[b]:] == -1).all()
                assert path[b, 0] == 0 and path[b, dl[b] - 1] == tl[b] - 1
            assert (wide[0][:, 3] >= res[0][:, 3]).all()                 # more paths admitted: the best cannot get worse
        scal = {k: v.detach().cpu().numpy().copy() for k, v in runner.step(batch).items()}
        torch.cuda.synchronize()
        a = trainer.arena
        return scal, [t.detach().cpu().numpy().copy() for t in (a.flat, a.exp_avg, a.exp_avg_sq)]
    finally:
        if runner is not trainer:
            runner.close()
        trainer.close()


@pytest.mark.parametrize("kind", ["trainer", "lattice"])
def test_align_batch_between_two_steps(dev, kind):
    s0, p0 = _run(dev, kind, with_align=False)
    s1, p1 = _run(dev, kind, with_align=True)
    assert sorted(s0) == sorted(s1)
    for k in s0:
        assert np.array_equal(s0[k].view(np.int32) if s0[k].dtype == np.float32 else s0[k],
                              s1[k].view(np.int32) if s1[k].dtype == np.float32 else s1[k]), k
    for x, y in zip(p0, p1):
        assert np.array_equal(x, y)


def test_align_batch_refusals(dev, monkeypatch):
    from deepvoice3_pytorch_amd import builder, train_step
    torch.manual_seed(0)
    model = builder.deepvoice3(**LHP).to(dev)
    tc = train_step.TrainConfig(max_positions=256, outputs_per_step=1, downsample_step=4)
    postnet_only = train_step.Trainer(model, tc, train_seq2seq=False)
    try:
        with pytest.raises(ValueError, match="train_seq2seq=False"):
            train_step.align_batch(postnet_only, _batch(dev))
    finally:
        postnet_only.close()
    trainer = train_step.Trainer(model, tc)
    try:
        with pytest.raises(ValueError, match="averaging is off"):
            train_step.align_batch(trainer, _batch(dev), averaged=True)
        monkeypatch.setattr(torch.cuda, "is_current_stream_capturing", lambda: True)
        with pytest.raises(RuntimeError, match="capture"):
            train_step.align_batch(trainer, _batch(dev))
        monkeypatch.undo()
    finally:
        trainer.close()

# coding: utf-8
"""-m gpu: vocoding the decoder's mel (`from_mel=`) on the three synthesis entry points, with a small
random deepvoice3 (r = 2, the post-net upsamples by 2) and a small random nyanko (r = 1, by 4) in eval mode and three
utterances of different lengths.

  1. tts_batch(from_mel=True): the mel and alignment bits of the plain run; `linear` is audio.mel_to_linear of that
     item's mel alone at the upsampling derived from the post-net's layers (which is the plain run's linear / mel frame
     ratio), `wav` is its inv_spectrogram_batch; a forward hook on model.postnet counts 0 calls; diagnostics and timings
     are still appended and equal those of the plain run; a MelInverse instance is used as given.  The model's
     linear_dim is not consulted.
  2. RollingSynthesizer(from_mel=True) and tts_stream give, per ticket, the tensors of tts_batch.
  3. synthesize_batch(postnet=False) returns None for `linear` and the plain run's other results.
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

STEPS = 12                                      # every utterance decodes STEPS + 1 steps: the done flag is out of the rule
LENS = [17, 5, 11]
FAMILIES = ("deepvoice3", "nyanko")


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


def _toy(family, dev, linear_dim=257):
    from deepvoice3_pytorch_amd import builder, audio
    torch.manual_seed(3)
    make, hp = dict(nyanko=(builder.nyanko, NY_HP), deepvoice3=(builder.deepvoice3, DV3_HP))[family]
    hp = dict(hp, linear_dim=linear_dim)
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


def _same(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(_bits(a), _bits(b))


class _Calls(object):
    def __init__(self, module):
        self.n = 0
        self.handle = module.register_forward_hook(self)

    def __call__(self, *a):
        self.n += 1


@pytest.mark.parametrize("family", FAMILIES)
def test_tts_batch_from_mel(dev, family):
    from deepvoice3_pytorch_amd import audio, synthesis
    model, hp, cfg = _toy(family, dev)
    seqs = _seqs(hp)
    opt = audio.MelInverse(fmin=55.0, fmax=7600.0)            # mel_dim = 20 bands
    plain = synthesis.tts_batch(model, seqs, audio_cfg=cfg, diagnostics=True, timings=True)
    calls = _Calls(model.postnet)
    try:
        voc = synthesis.tts_batch(model, seqs, audio_cfg=cfg, diagnostics=True, timings=True, from_mel=opt)
        bare = synthesis.tts_batch(model, seqs, audio_cfg=cfg, from_mel=True)
        assert calls.n == 0, "the post-net ran"
        synthesis.tts_batch(model, seqs[:1], audio_cfg=cfg)
        assert calls.n == 1                                  # (the hook does count a plain run)
    finally:
        calls.handle.remove()
    up = synthesis.postnet_upsampling(model)
    assert up == max(hp["downsample_step"] // hp["r"], 1)
    for b, (p, v, q) in enumerate(zip(plain, voc, bare)):
        assert len(p) == len(v) == 6 and len(q) == 4
        assert _same(v[0], p[0]) and _same(v[2], p[2]) and _same(q[0], p[0]) and _same(q[2], p[2]), (family, b)
        assert p[1].shape[0] == up * p[0].shape[0]            # the derived upsampling is the post-net's own
        assert v[1].shape == (up * v[0].shape[0], 257)
        for res, o in ((v, opt), (q, audio.MelInverse())):
            alone = audio.mel_to_linear(res[0][None].contiguous(), cfg, None, up, o)
            assert _same(res[1], alone[0]), "%s item %d: linear is not mel_to_linear of its own mel" % (family, b)
            wav, n = audio.inv_spectrogram_batch(alone, cfg, None, [alone.shape[1]])
            assert _same(res[3], wav[0, :int(n[0])]), "%s item %d: wav is not the inversion of its linear" % (family, b)
        assert not _same(v[1], q[1])                          # another band edge, another estimate
        assert v[4] == p[4]                                   # the statistics dict, flags included
        assert sorted(v[5]) == sorted(p[5]) and all(_same(v[5][k], p[5][k]) for k in p[5])
    # the bins are audio_cfg's: a model whose linear_dim fits no FFT size is refused without from_mel, vocoded with it
    odd, hp2, _ = _toy(family, dev, linear_dim=33)
    with pytest.raises(ValueError):
        synthesis.tts_batch(odd, seqs[:1], audio_cfg=cfg)
    res = synthesis.tts_batch(odd, seqs[:1], audio_cfg=cfg, from_mel=True)[0]
    assert res[1].shape == (up * res[0].shape[0], 257) and bool(torch.isfinite(res[3]).all())
    with pytest.raises(ValueError):
        synthesis.tts_batch(model, seqs[:1], audio_cfg=cfg, from_mel=32)


@pytest.mark.parametrize("family", FAMILIES)
def test_rolling_and_stream_from_mel_equal_tts_batch(dev, family):
    from deepvoice3_pytorch_amd import synthesis
    model, hp, cfg = _toy(family, dev)
    seqs = _seqs(hp)
    want = synthesis.tts_batch(model, seqs, audio_cfg=cfg, from_mel=True)
    calls = _Calls(model.postnet)
    try:
        rs = synthesis.RollingSynthesizer(model, slots=2, max_text_len=max(LENS), audio_cfg=cfg, chunk=8, from_mel=True)
        tickets = [rs.submit(s) for s in seqs]
        got = {res[0]: res for res in rs.drain()}
        streamed = {res[0]: res for res in synthesis.tts_stream(model, seqs, slots=2, audio_cfg=cfg, from_mel=True)}
        assert calls.n == 0, "the post-net ran"
    finally:
        calls.handle.remove()
    assert sorted(got) == sorted(streamed) == tickets == [0, 1, 2]
    for tk in tickets:
        for res in (got[tk], streamed[tk]):
            assert len(res) == 5
            for i, (x, y) in enumerate(zip(res[1:], want[tk])):
                assert _same(x, y), (family, tk, i)


@pytest.mark.parametrize("family", FAMILIES)
def test_synthesize_batch_without_postnet(dev, family):
    model, hp, cfg = _toy(family, dev)
    seqs = _seqs(hp)
    text = torch.zeros(len(seqs), max(LENS), dtype=torch.long)
    for b, s in enumerate(seqs):
        text[b, :len(s)] = torch.as_tensor(s)
    text = text.to(dev)
    full = model.synthesize_batch(text, LENS)
    calls = _Calls(model.postnet)
    try:
        part = model.synthesize_batch(text, LENS, postnet=False)
        assert calls.n == 0
    finally:
        calls.handle.remove()
    assert part[1] is None and full[1] is not None
    assert _same(part[0], full[0]) and _same(part[2], full[2]) and torch.equal(part[4], full[4])
    assert len(part[3]) == len(full[3]) and all(_same(a, b) for a, b in zip(part[3], full[3]))

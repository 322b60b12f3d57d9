# coding: utf-8
"""-m gpu: speaking rate and pitch at vocoding (csrc/prosody.hip; include/dv3hip.h:
dv3_prosody_warp_f32) against the float64 restatement of tests/prosody_ref.py.

  1. the entry point element by element against float64 under a bound derived from the operands; the padding;
  2. the integer / fraction split of both axes: the transcendental-free modes bit for bit against their fp32 restatement;
  3. identity items and batch independence, bit for bit; the refusals;
  4. inv_spectrogram_batch with the keyword is the by-hand composition, bit for bit, also on mel_to_linear's output;
  5. the pitch moves by the requested interval: stft -> inverse with the option -> yin_items;
  6. through synthesis: tts_batch, RollingSynthesizer.submit, tts_stream, timings, from_mel."""
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tests import prosody_ref as P  # noqa: E402

pytestmark = pytest.mark.gpu

TMIN = 4                                        # min_frames at hop = fft_size / 4 on the lws framing
ST = lambda s: 2.0 ** (s / 12.0)
# (tlen_in, rate, ratio): the ragged batch of the issue, and the long stretch with the extreme shifts
OPERANDS = {
    "ragged": ((12, 7, TMIN), (1.0, 0.8, 1.25), (1.0, ST(4), ST(-3))),
    "stretch": ((12, 7), (0.3, 0.3), (ST(24), ST(-24))),
}


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


def _magnitudes(B, T, bins, tlen, seed):
    """fp32 magnitudes over and beyond the range magnitudes() makes (10^-5.6 .. 10^1.4), a few zeros and values under the
    kernel's floor of 1e-10 among them; frames at or beyond tlen[b] are NaN"""
    rng = np.random.RandomState(seed)
    m = 10.0 ** rng.uniform(-5.6, 1.4, (B, T, bins))
    wild = rng.rand(B, T, bins)
    m = np.where(wild < 0.01, 0.0, np.where(wild < 0.02, 1e-12, np.where(wild < 0.03, 1e3, np.where(wild < 0.04, 3e-8, m))))
    m = m.astype(np.float32)
    for b, n in enumerate(tlen):
        m[b, n:] = np.nan
    return m


def _raw(dev, mag, tlen_in, tlen_out, rate, ratio, W, preserve, T_out, fill=-7.0):
    """dv3_prosody_warp_f32 itself -> (B, T_out, bins) float32 numpy"""
    from deepvoice3_pytorch_amd import _lib
    x = torch.from_numpy(np.ascontiguousarray(mag, dtype=np.float32)).to(dev)
    B, T_in, bins = x.shape
    out = torch.full((B, T_out, bins), fill, dtype=torch.float32, device=dev)
    ti = torch.tensor(list(tlen_in), dtype=torch.int32, device=dev) if tlen_in is not None else None
    to = torch.tensor(list(tlen_out), dtype=torch.int32, device=dev)
    r = torch.tensor(list(rate), dtype=torch.float64, device=dev)
    q = torch.tensor(list(ratio), dtype=torch.float64, device=dev)
    _lib.call("dv3_prosody_warp_f32", x.data_ptr(), out.data_ptr(), B, T_in, T_out, bins,
              ti.data_ptr() if ti is not None else None, to.data_ptr(), r.data_ptr(), q.data_ptr(), int(W), int(preserve),
              torch.cuda.current_stream().cuda_stream)
    return out.cpu().numpy()


# ----------------------------------------------------------------------------------------------------------------------
# 1. element by element
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("preserve,W", [(1, 1), (1, 19), (1, 64), (0, 19)])
@pytest.mark.parametrize("bins", [257, 513, 1025])
def test_elementwise_against_float64(dev, bins, preserve, W):
    """Every element within prosody_ref.bound of the float64 restatement -- the bound is derived there, next to the
    formula, from the operands and the rounding of each fp32 operation (two interpolations, logf, the 2 W + 1 accumulated
    products and their quotient, expf), as DESIGN.md 4.4 derives its bounds; nothing in it was fitted to the kernel.
    No NaN of the padded input frames reaches the output; rows past tlen_out are exact zeros (the buffer starts at -7).
    The largest ratio of error to bound is printed; DESIGN.md 3.6i records the worst one measured."""
    worst = 0.0
    for name, (tin, rate, ratio) in sorted(OPERANDS.items()):
        B, T_in = len(tin), max(tin) + 2
        tout = [P.out_frames(n, r, TMIN) for n, r in zip(tin, rate)]
        T_out = max(tout) + 1
        if name == "stretch":
            assert T_out > T_in
        mag = _magnitudes(B, T_in, bins, tin, seed=bins + W)
        got = _raw(dev, mag, tin, tout, rate, ratio, W, preserve, T_out).astype(np.float64)
        want, det = P.warp(mag.astype(np.float64), tin, tout, rate, ratio, W, preserve, T_out, details=True)
        assert np.isfinite(got).all(), "a padded frame was read"
        for b, n in enumerate(tout):
            assert not got[b, n:].any() and got[b, :n].shape == (n, bins)
        lim = P.bound(det, want.shape)
        err = np.abs(got - want)
        live = lim > 0
        assert (err[~live] == 0).all()                            # copies and zero rows: exact
        r = float((err[live] / lim[live]).max())
        worst = max(worst, r)
        print("bins %d W %d preserve %d %s: largest error / bound %.3f (largest relative error %.2e)"
              % (bins, W, preserve, name, r, float((err[live] / np.maximum(np.abs(want[live]), 1e-300)).max())))
        assert (err <= lim).all(), (name, r)
    print("bins %d W %d preserve %d: worst error / bound %.3f" % (bins, W, preserve, worst))


def test_tlen_in_null_means_all_frames(dev):
    mag = _magnitudes(2, 9, 257, (9, 9), seed=3)
    args = ((12, 12), (0.8, 0.8), (ST(4), ST(4)), 19, 1, 12)
    assert np.array_equal(_raw(dev, mag, None, *args), _raw(dev, mag, (9, 9), *args))


# ----------------------------------------------------------------------------------------------------------------------
# 2. the split of both axes
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bins", [257, 513, 1025])
def test_the_split_of_both_axes_is_the_restatements(dev, bins):
    """A staircase whose value encodes its frame and bin, 2^i (k + 1)^2: strictly convex along the bins, so an
    interpolated value lies between two neighbouring squares and decodes to ONE (s0, fa); the power of two rides through
    every fp32 operation exactly.  With ratio != 1 and rate 1 the output must decode to the restatement's s0, and with
    the plain warp -- which involves no transcendental -- the whole output, staircase and random, must equal the fp32
    restatement built from the restatement's (i0, a, s0, fa) BIT FOR BIT: one ulp of difference in either fraction
    would show."""
    T = 12
    i, k = np.arange(T, dtype=np.float64)[:, None], np.arange(bins, dtype=np.float64)[None, :]
    stairs = (2.0 ** i * (k + 1.0) ** 2)[None].astype(np.float32)
    for ratio in (ST(4), ST(-3), ST(24), ST(-24), 1.5):
        got = _raw(dev, stairs, (T,), (T,), (1.0,), (ratio,), 19, 0, T)[0].astype(np.float64)
        inside, s0, fa, s1 = P.bin_split(bins, ratio)
        root = np.sqrt(got / 2.0 ** i)
        away = (fa > 1e-3) & (fa < 1.0 - 1e-3) | (fa == 0)                 # an fp32 rounding cannot cross a square there
        assert np.array_equal((np.floor(root + 1e-9).astype(np.int64) - 1)[:, away], np.tile(s0[away], (T, 1))), ratio
    tin, rate, ratio = (T, 7, TMIN, T), (1.0, 0.8, 1.25, 0.3), (1.5, ST(4), ST(-3), 1.0)
    tout = [P.out_frames(n, r, TMIN) for n, r in zip(tin, rate)]
    for mag in (np.tile(stairs, (4, 1, 1)), _magnitudes(4, T, bins, tin, seed=bins)):
        got = _raw(dev, mag, tin, tout, rate, ratio, 19, 0, max(tout))
        want = P.warp_f32_plain(mag, tin, tout, rate, ratio, max(tout))
        assert np.array_equal(got.view(np.int32), want.view(np.int32)), float(np.abs(got - want).max())


# ----------------------------------------------------------------------------------------------------------------------
# 3. identity, batch independence, refusals
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("preserve", [0, 1])
def test_identity_items_come_back_bit_for_bit(dev, preserve):
    bins, tin = 513, (12, 7, 9)
    mag = _magnitudes(3, 12, bins, tin, seed=7)
    rate, ratio = (1.0, 0.8, 1.0), (1.0, ST(4), 1.0)
    tout = [P.out_frames(n, r, TMIN) for n, r in zip(tin, rate)]
    got = _raw(dev, mag, tin, tout, rate, ratio, 19, preserve, max(tout))
    for b in (0, 2):
        assert np.array_equal(got[b, :tin[b]].view(np.int32), mag[b, :tin[b]].view(np.int32))
        assert not got[b, tin[b]:].any()
    assert not np.array_equal(got[1, :7], mag[1, :7])


@pytest.mark.parametrize("preserve", [0, 1])
def test_every_item_equals_its_b1_call(dev, preserve):
    from deepvoice3_pytorch_amd import audio
    cfg = audio.AudioConfig(fft_size=512, hop_size=128, sample_rate=16000)
    tin = [12, 7, TMIN, 10]
    mag = torch.from_numpy(_magnitudes(4, 12, 257, tin, seed=11)).to(dev)
    p = audio.Prosody(rate=[1.0, 0.8, 1.25, 0.3], semitones=[4.0, 0.0, -3.0, 7.0], preserve_envelope=bool(preserve))
    out, lens = audio.warp_magnitudes(mag, tin, cfg, p)
    assert lens.tolist() == [P.out_frames(n, r, TMIN) for n, r in zip(tin, p.rate)] and out.shape[1] == int(lens.max())
    raw = _raw(dev, mag.cpu().numpy(), tin, lens.tolist(), p.rate, [ST(s) for s in p.semitones], p.half_width(cfg), preserve,
               int(lens.max()))
    assert np.array_equal(out.cpu().numpy().view(np.int32), raw.view(np.int32))      # the wrapper is the entry point's call
    for b in range(4):
        one = audio.Prosody(p.rate[b], p.semitones[b], bool(preserve))
        alone, n = audio.warp_magnitudes(mag[b:b + 1, :tin[b]].contiguous(), None, cfg, one)
        assert int(n[0]) == int(lens[b]) and torch.equal(alone[0].view(torch.int32), out[b, :int(n[0])].view(torch.int32))
        assert not out[b, int(n[0]):].any()


def test_refusals(dev):
    from deepvoice3_pytorch_amd import _lib, audio
    h = _lib.lib()
    x = torch.ones(1, 4, 257, device=dev)
    out = torch.empty_like(x)
    tl = torch.full((1,), 4, dtype=torch.int32, device=dev)
    one = torch.ones(1, dtype=torch.float64, device=dev)
    good = [x.data_ptr(), out.data_ptr(), 1, 4, 4, 257, None, tl.data_ptr(), one.data_ptr(), one.data_ptr(), 19, 1, None]
    assert h.dv3_prosody_warp_f32(*good) == 0
    for pos, bad in ((0, None), (1, None), (1, x.data_ptr()), (7, None), (8, None), (9, None), (2, 0), (2, 65536), (3, 0),
                     (4, 0), (5, 0), (5, 1026), (10, 0), (10, 65), (11, 2)):
        args = list(good)
        args[pos] = bad
        assert h.dv3_prosody_warp_f32(*args) == _lib.CONSTS["DV3_EINVAL"], (pos, bad)
        assert h.dv3_last_error().decode().startswith("prosody_warp:")
    torch.cuda.synchronize()
    cfg = audio.AudioConfig(fft_size=512, hop_size=128, sample_rate=16000)
    with pytest.raises(ValueError, match="bins"):
        audio.warp_magnitudes(torch.ones(1, 4, 513, device=dev), None, cfg, audio.Prosody(0.8))
    with pytest.raises(ValueError, match="frame lengths"):
        audio.warp_magnitudes(x, [5], cfg, audio.Prosody(0.8))
    with pytest.raises(ValueError, match="rate"):
        audio.warp_magnitudes(x, None, cfg, audio.Prosody([0.8, 0.9]))
    with pytest.raises(ValueError, match="init_phasor"):
        audio.inv_spectrogram_batch(x, cfg, init_phasor=torch.ones(1, 4, 257, 2, device=dev), prosody=audio.Prosody(0.8))


# ----------------------------------------------------------------------------------------------------------------------
# 4. composition
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("init", ["zero", "spsi"])
def test_the_keyword_is_the_by_hand_composition(dev, init):
    """inv_spectrogram_batch(x, cfg, frame_lengths=fl, prosody=p) is magnitudes -> warp_magnitudes -> (spsi_phasor) ->
    griffin_lim -> the per-item de-emphasis, bit for bit, with sample lengths num_samples(T'_b); without frame_lengths every
    item has T frames; None and an all-neutral Prosody() are today's call."""
    from deepvoice3_pytorch_amd import _lib, audio
    cfg = audio.AudioConfig(fft_size=512, hop_size=128, sample_rate=16000, griffin_lim_iters=3, griffin_lim_momentum=0.99,
                            griffin_lim_init=init)
    B, T, fl = 3, 14, [14, 9, 5]
    x = torch.from_numpy(np.random.RandomState(5).rand(B, T, 257).astype(np.float32)).to(dev)
    p = audio.Prosody(rate=[0.8, 1.0, 1.25], semitones=[0.0, 3.0, -2.0])
    for lengths in (fl, None):
        got, samples = audio.inv_spectrogram_batch(x, cfg, frame_lengths=lengths, prosody=p)
        mag, tp = audio.warp_magnitudes(audio.magnitudes(x, cfg), lengths, cfg, p)
        assert tp.tolist() == [audio.warped_frames(n, r, cfg) for n, r in zip(lengths or [T] * B, p.rate)]
        tlen = tp.to(torch.int32).to(dev)
        ph = audio.spsi_phasor(mag, 128, tlen, 512) if init == "spsi" else None
        y = audio.griffin_lim(mag, 128, 3, ph, "lws", cfg.window_scale, tlen, 512, 0.99)
        want_n = [audio.num_samples(int(n), 128, "lws", 512) for n in tp]
        want = torch.empty_like(y)
        _lib.call("dv3_deemphasis_items_f32", y.data_ptr(), want.data_ptr(), B, y.shape[1],
                  torch.tensor(want_n, dtype=torch.int32, device=dev).data_ptr(), 0.97, torch.cuda.current_stream().cuda_stream)
        assert samples.tolist() == want_n and torch.equal(got.view(torch.int32), want.view(torch.int32))
    for neutral in (None, audio.Prosody(), audio.Prosody(rate=[1.0] * B, semitones=[0.0] * B)):
        a, n = audio.inv_spectrogram_batch(x, cfg, frame_lengths=fl, prosody=neutral)
        b, m = audio.inv_spectrogram_batch(x, cfg, frame_lengths=fl)
        assert torch.equal(a, b) and torch.equal(n, m)
        plain = audio.inv_spectrogram_batch(x, cfg, prosody=neutral)
        assert isinstance(plain, torch.Tensor) and torch.equal(plain, audio.inv_spectrogram_batch(x, cfg))


def test_a_mel_is_vocoded_with_the_keyword_through_mel_to_linear(dev):
    """inv_melspectrogram_batch keeps its parameters; its documented composition, mel_to_linear followed by
    inv_spectrogram_batch, takes the keyword: the warp runs on the magnitudes of the inverted mel, item by item (each item
    equals its own B = 1 call on its own frames bit for bit), the sample lengths are num_samples(T'_b), and without the
    keyword, or with a neutral Prosody(), the composition is inv_melspectrogram_batch itself."""
    from deepvoice3_pytorch_amd import audio
    cfg = audio.AudioConfig(fft_size=512, hop_size=128, sample_rate=16000, griffin_lim_iters=2)
    opt = audio.MelInverse(iters=4)
    mel = torch.from_numpy(np.random.RandomState(6).rand(2, 6, 20).astype(np.float32)).to(dev)
    p = audio.Prosody(rate=[0.8, 1.25], semitones=[2.0, 0.0], preserve_envelope=False)
    for fl in ([6, 3], None):
        lin = audio.mel_to_linear(mel, cfg, fl, 2, opt)
        frames = [2 * v for v in (fl or [6, 6])]
        got, n = audio.inv_spectrogram_batch(lin, cfg, frame_lengths=frames if fl else None, prosody=p)
        assert n.tolist() == [audio.num_samples(audio.warped_frames(t, r, cfg), 128, "lws", 512)
                              for t, r in zip(frames, p.rate)]
        for b in range(2):
            one = audio.Prosody(p.rate[b], p.semitones[b], False)
            alone, k = audio.inv_spectrogram_batch(lin[b:b + 1, :frames[b]].contiguous(), cfg, prosody=one)
            assert int(k[0]) == int(n[b]) and torch.equal(alone[0], got[b, :int(n[b])]) and not got[b, int(n[b]):].any()
    lin = audio.mel_to_linear(mel, cfg, [6, 3], 2, opt)
    want, m = audio.inv_melspectrogram_batch(mel, cfg, [6, 3], 2, opt)
    for neutral in (None, audio.Prosody()):
        a, n = audio.inv_spectrogram_batch(lin, cfg, frame_lengths=[12, 6], prosody=neutral)
        assert torch.equal(a, want) and torch.equal(n, m)


# ----------------------------------------------------------------------------------------------------------------------
# 5. the pitch moves by the requested interval
# ----------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def tone_spectrogram(dev):
    """the CPU fixture's tones -> audio.stft magnitudes -> the normalised spectrogram the inverse takes, under a config
    whose magnitudes() returns them: power 1, no de-emphasis, a reference level that leaves room for the peaks"""
    from deepvoice3_pytorch_amd import audio
    cfg = audio.AudioConfig(preemphasis=0.0, power=1.0, ref_level_db=60, griffin_lim_iters=30, griffin_lim_momentum=0.99)
    y = torch.from_numpy(P.harmonic_tones().astype(np.float32)).to(dev)
    _, spec = audio.stft(y, P.T_TONES, P.HOP, want_phasor=False, want_spec=True, convention="lws",
                         window_scale=cfg.window_scale)
    mag = torch.sqrt(spec[..., 0] ** 2 + spec[..., 1] ** 2)
    assert float(mag.max()) < 10.0 ** (cfg.ref_level_db / 20.0)
    db = 20.0 * torch.log10(mag.clamp(min=1e-5)) - cfg.ref_level_db
    return ((db - cfg.min_level_db) / -cfg.min_level_db).clamp(0.0, 1.0).contiguous(), cfg


@pytest.mark.parametrize("preserve", [True, False])
@pytest.mark.parametrize("semitones,rate", P.CLOSURE_SETTINGS)
def test_pitch_closure_on_the_device(dev, tone_spectrogram, semitones, rate, preserve):
    """the condition of tests/test_cpu_prosody_ref.py::test_pitch_closure_in_float64 for the kernels: the median F0
    over frames 5 .. T' - 5 of the inverted waveform within 25 cents of f0 x ratio"""
    from deepvoice3_pytorch_amd import audio
    lin, cfg = tone_spectrogram
    B = lin.shape[0]
    p = audio.Prosody(rate=rate, semitones=semitones, preserve_envelope=preserve)
    wav, n = audio.inv_spectrogram_batch(lin, cfg, prosody=p)
    Tp = audio.warped_frames(P.T_TONES, rate, cfg)
    assert n.tolist() == [audio.num_samples(Tp, P.HOP, "lws", P.N_FFT)] * B and wav.shape == (B, int(n[0]))
    f0, _, _, frames = audio.yin_items(wav.reshape(-1).contiguous(), n.numpy(), cfg,
                                       audio.PitchConfig(fmin=60.0, fmax=500.0, threshold=P.YIN_THRESHOLD))
    assert frames.tolist() == [Tp] * B
    f0 = f0.cpu().numpy()
    for b, tone in enumerate(P.TONE_F0):
        got = P.median_f0(f0[b * Tp:(b + 1) * Tp], Tp)
        c = P.cents(got, tone * ST(semitones))
        print("f0 %g Hz, %+g st, rate %g, preserve %d: median %.2f Hz, %+.2f cents" % (tone, semitones, rate, preserve, got, c))
        assert abs(c) <= P.CENTS, (tone, semitones, rate, preserve, got, c)


# ----------------------------------------------------------------------------------------------------------------------
# 6. through synthesis
# ----------------------------------------------------------------------------------------------------------------------
E2E_HP = dict(n_vocab=40, embed_dim=32, mel_dim=20, linear_dim=257, r=1, downsample_step=4, padding_idx=0, dropout=0.05,
              kernel_size=3, encoder_channels=64, decoder_channels=32, converter_channels=32, use_memory_mask=True,
              force_monotonic_attention=True, use_decoder_state_for_postnet_input=True, key_projection=True,
              value_projection=True, max_positions=128)


@pytest.mark.parametrize("from_mel", [False, True])
def test_through_synthesis(dev, from_mel):
    """the tiny random model of the synthesis tests at 512 / 128: with rate and semitones per utterance, mel, linear and
    alignment are the plain call's and only wav changes, to num_samples(T'_b) samples -- the waveform of the by-hand
    inverse of the utterance's own spectrogram; token spans are the plain call's divided by the rate;
    RollingSynthesizer.submit and tts_stream give the same waveform bit for bit; from_mel composes."""
    from deepvoice3_pytorch_amd import audio, builder, synthesis
    torch.manual_seed(0)
    model = builder.deepvoice3(**E2E_HP).to(dev).eval()
    dec = model.seq2seq.decoder
    dec.min_decoder_steps = dec.max_decoder_steps = 11
    rng = np.random.RandomState(2)
    ids = [rng.randint(2, 40, 9).tolist(), rng.randint(2, 40, 14).tolist()]
    cfg = audio.AudioConfig(fft_size=512, hop_size=128, sample_rate=16000, griffin_lim_iters=3)
    rate, semis = [0.8, 1.0], [0.0, 3.0]
    plain = synthesis.tts_batch(model, ids, audio_cfg=cfg, timings=True, from_mel=from_mel)
    res = synthesis.tts_batch(model, ids, audio_cfg=cfg, timings=True, from_mel=from_mel, rate=rate, semitones=semis)
    assert len(res) == len(plain) == 2
    for b in range(2):
        for i in range(3):
            assert torch.equal(res[b][i], plain[b][i]), (b, i)
        lin, wav = res[b][1], res[b][3]
        Tp = audio.warped_frames(lin.shape[0], rate[b], cfg)
        assert wav.shape == (audio.num_samples(Tp, 128, "lws", 512),)
        assert not torch.equal(wav, plain[b][3][:wav.numel()]) if wav.numel() <= plain[b][3].numel() else True
        by_hand, _ = audio.inv_spectrogram_batch(lin[None].contiguous(), cfg,
                                                 prosody=audio.Prosody(rate=rate[b], semitones=semis[b]))
        assert torch.equal(wav, by_hand[0]), (b, float((wav - by_hand[0]).abs().max()))
        for key in ("start", "end"):
            assert res[b][4][key].dtype == torch.float64
            assert torch.equal(res[b][4][key], plain[b][4][key] / rate[b]), (b, key)
        for key in ("path", "durations", "summary"):
            assert torch.equal(res[b][4][key], plain[b][4][key]), (b, key)
    same = synthesis.tts_batch(model, ids, audio_cfg=cfg, from_mel=from_mel, rate=1.0, semitones=[0, 0],
                               prosody=audio.Prosody())
    for b in range(2):
        assert torch.equal(same[b][3], plain[b][3])
    got = {r[0]: r for r in synthesis.tts_stream(model, ids, slots=2, audio_cfg=cfg, from_mel=from_mel, timings=True,
                                                 rate=rate, semitones=semis)}
    assert sorted(got) == [0, 1]
    for b in range(2):
        assert torch.equal(got[b][4], res[b][3]), (b, "tts_stream")
        assert torch.equal(got[b][5]["end"], res[b][4]["end"]) and torch.equal(got[b][2], res[b][1])
    rs = synthesis.RollingSynthesizer(model, slots=2, max_text_len=14, audio_cfg=cfg, from_mel=from_mel)
    plainer = audio.Prosody(preserve_envelope=False)                   # another envelope setting in the same group
    tickets = [rs.submit(ids[0], rate=rate[0], semitones=semis[0]), rs.submit(ids[1], semitones=semis[1], prosody=plainer)]
    rolled = {r[0]: r[4] for r in rs.drain()}
    assert torch.equal(rolled[tickets[0]], res[0][3])
    other = synthesis.tts_batch(model, ids[1:], audio_cfg=cfg, from_mel=from_mel, semitones=semis[1], prosody=plainer)
    assert torch.equal(rolled[tickets[1]], other[0][3]) and not torch.equal(other[0][3], res[1][3])
    with pytest.raises(ValueError, match="rate"):
        rs.submit(ids[0], rate=[0.8, 1.0])
    with pytest.raises(ValueError, match="rate"):
        synthesis.tts_batch(model, ids, audio_cfg=cfg, rate=[0.8, 1.0, 1.2])

# coding: utf-8
"""-m gpu: Single Pass Spectrogram Inversion (csrc/spsi.hip; include/dv3hip.h: dv3_spsi_phasor_f32)
against the float64 restatement of tests/spsi_ref.py.

  1. audio.spsi_phasor against the restatement: three frame sizes, two hops, three frame counts, speech-like and noise
     magnitudes; rows whose climbs span several of the kernel's 64-bin segments;
  2. every item of a ragged batch as its own B = 1 call, bit for bit, (1, 0) past its frames;
  3. the buffer's edges and the refusals through the raw entry point;
  4. through inv_spectrogram_batch, SPSI + 10 iterations at 0.99 end below the restatement's 60 plain ones;
  5. "zero" is the call without the option and "spsi" the call with the phasor passed by hand, bit for bit;
  6. tts_batch and tts_stream carry the option, from_mel=True included."""
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tests import fast_gl_ref as R  # noqa: E402
from tests import spsi_ref as S  # noqa: E402

pytestmark = pytest.mark.gpu

SIZES = [512, 1024, 2048]
RATE = {512: 16000, 1024: 22050, 2048: 48000}
SENTINEL = -12345.0


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


def _noise(dev, n, hop, B, T):
    """the clipped-normal draw of tests/test_gpu_fast_gl.py::_draw through audio.magnitudes: many narrow peaks"""
    from deepvoice3_pytorch_amd import audio
    rng = np.random.RandomState(15 + hop)
    lin = torch.from_numpy(np.clip(0.55 + 0.25 * rng.randn(B, T, n // 2 + 1), -0.2, 1.2).astype(np.float32))
    return audio.magnitudes(lin.to(dev), audio.AudioConfig(fft_size=n, hop_size=hop, sample_rate=RATE[n]))


def _pairs(ph):
    """complex (B, T, F) -> float64 (B, T, F, 2)"""
    return np.stack([ph.real, ph.imag], axis=-1)


# ----------------------------------------------------------------------------------------------------------------------
# 1. against the restatement
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", SIZES)
def test_kernel_matches_the_restatement(dev, n):
    """Bound: 2e-6 absolute per component.  The magnitudes are fp32 values on both sides and every comparison of the
    algorithm is exact, so the peak sets and owners are identical by construction; the angle is formed in fp64 in the
    same order on both sides; what is left is one fp32 rounding of a turn in [0, 1) (at most 2^-25 turns, 1.9e-7 rad;
    4e-7 rad with the doubling counted against it) and an accurate fp32 sine and cosine (a few 1e-7).
    Measured on an MI355X, the largest error over the hops, frame counts and both kinds of magnitudes: 1.93e-07,
    1.93e-07 and 1.95e-07 at 512, 1024 and 2048."""
    from deepvoice3_pytorch_amd import audio
    B, worst = 3, 0.0
    for hop in (n // 4, 3 * n // 16):
        for T in (audio.min_frames(hop, "lws", n), 13, 40):
            speech = torch.from_numpy(R.speechlike_magnitudes(n, hop, B=B, T=T).astype(np.float32)).to(dev)
            for kind, mag in (("speech", speech), ("noise", _noise(dev, n, hop, B, T))):
                got = audio.spsi_phasor(mag, hop, fft_size=n)
                assert tuple(got.shape) == (B, T, n // 2 + 1, 2) and got.dtype == torch.float32
                m64 = mag.cpu().numpy().astype(np.float64)
                want = _pairs(S.spsi_phasor(m64, hop, n))
                e = float(np.abs(got.cpu().numpy().astype(np.float64) - want).max())
                worst = max(worst, e)
                print("n %d hop %d T %d %s: %d peaks, largest error %.2e" % (n, hop, T, kind, int(S.peaks(m64).sum()), e))
                assert e < 2e-6, (hop, T, kind, e)
    print("n %d: largest error %.2e" % (n, worst))


@pytest.mark.parametrize("n", SIZES)
def test_long_runs_cross_the_wave_segments(dev, n):
    """The kernel finds the end of a climb by ballots over 64-bin segments and goes on into the next segment when a run
    leaves its own.  Rows whose runs span many segments in both directions: lobes 60 to 600 bins wide (with and without
    a ripple that breaks them up), one rising ramp over all bins (it ends on bin F - 1: no owner anywhere) and one falling
    ramp (it ends on bin 0).  The bound of test_kernel_matches_the_restatement; measured on an MI355X: 1.49e-07,
    1.79e-07 and 1.81e-07 at 512, 1024 and 2048, with climbs of up to 179, 213 and 313 bins."""
    from deepvoice3_pytorch_amd import audio
    F, T, hop = n // 2 + 1, 6, n // 4
    rng = np.random.RandomState(n)
    k = np.arange(F, dtype=np.float64)
    rows = np.empty((4, T, F))
    for t in range(T):
        width = rng.uniform(20, 200)
        rows[0, t] = np.abs(np.sin((k + rng.uniform(0, 50)) / width)) + 0.01
        rows[1, t] = rows[0, t] + 2e-3 * rng.rand(F) * (t % 2)
        rows[2, t] = 1.0 + np.cumsum(rng.rand(F))
        rows[3, t] = rows[2, t][::-1]
    m64 = rows.astype(np.float32).astype(np.float64)
    own = S.owners(m64)
    longest = int(np.abs(own[:2] - k)[own[:2] >= 0].max())
    assert longest > 128 and not (own[2:] >= 0).any(), longest                # climbs of more than two segments
    got = audio.spsi_phasor(torch.from_numpy(m64.astype(np.float32)).to(dev), hop, fft_size=n)
    e = float(np.abs(got.cpu().numpy().astype(np.float64) - _pairs(S.spsi_phasor(m64, hop, n))).max())
    print("n %d: longest climb %d bins, largest error %.2e" % (n, longest, e))
    assert e < 2e-6, e


# ----------------------------------------------------------------------------------------------------------------------
# 2. ragged batches
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", SIZES)
def test_per_item_equals_b1(dev, n):
    from deepvoice3_pytorch_amd import audio
    hop, T = 3 * n // 16, 13
    frames = [T, 7, audio.min_frames(hop, "lws", n), 1, 0]
    B = len(frames)
    mag = _noise(dev, n, hop, B, T)
    tlen = torch.tensor(frames, dtype=torch.int32, device=dev)
    got = audio.spsi_phasor(mag, hop, tlen, n)
    one = torch.tensor([1.0, 0.0], device=dev)
    for b, k in enumerate(frames):
        assert bool((got[b, k:] == one).all()), (b, "rows past the item's frames are not (1, 0)")
        if k:
            want = audio.spsi_phasor(mag[b:b + 1, :k].contiguous(), hop, fft_size=n)[0]
            assert torch.equal(got[b, :k], want), (b, float((got[b, :k] - want).abs().max()))
    full = torch.full((B,), T, dtype=torch.int32, device=dev)
    assert torch.equal(audio.spsi_phasor(mag, hop, full, n), audio.spsi_phasor(mag, hop, fft_size=n))
    # the restatement's rows too, the ragged form included
    want = _pairs(S.spsi_phasor(mag.cpu().numpy().astype(np.float64), hop, n, frames))
    assert float(np.abs(got.cpu().numpy() - want).max()) < 2e-6


# ----------------------------------------------------------------------------------------------------------------------
# 3. edges and refusals, through the raw entry point
# ----------------------------------------------------------------------------------------------------------------------
def test_buffer_edges_and_refusals(dev):
    """The largest F (1025) at T = min_frames, B = 2, in a buffer framed by sentinels: with and without tlen nothing
    outside (B, T, F, 2) is written and everything inside is.  A frame size of 4096 is DV3_EINVAL with the sibling
    kernels' message; the other refusals launch nothing either."""
    from deepvoice3_pytorch_amd import audio, _lib
    from deepvoice3_pytorch_amd.ops import _stream
    h = _lib.lib()
    n, hop, B = 2048, 512, 2
    T, F = audio.min_frames(hop, "lws", n), n // 2 + 1
    assert T == 4
    mag = _noise(dev, n, hop, B, T)
    size, margin = B * T * F * 2, 2 * F * 2               # two frame rows of sentinels on either side
    st = _stream()
    for tl in (None, [T, 1]):
        tlen = None if tl is None else torch.tensor(tl, dtype=torch.int32, device=dev)
        buf = torch.full((margin + size + margin,), SENTINEL, dtype=torch.float32, device=dev)
        inner = buf[margin:margin + size]
        assert inner.data_ptr() % 8 == 0
        rc = h.dv3_spsi_phasor_f32(mag.data_ptr(), inner.data_ptr(), B, T, hop, tlen.data_ptr() if tl else None, n, st)
        assert rc == 0, h.dv3_last_error()
        torch.cuda.synchronize()
        assert bool((buf[:margin] == SENTINEL).all()) and bool((buf[margin + size:] == SENTINEL).all()), tl
        got = inner.reshape(B, T, F, 2)
        assert bool((got != SENTINEL).all()), tl
        assert torch.equal(got, audio.spsi_phasor(mag, hop, tlen, n)), tl
        assert float(((got ** 2).sum(-1) - 1.0).abs().max()) < 1e-6
    einval = _lib.CONSTS["DV3_EINVAL"]
    out = torch.full((size,), SENTINEL, dtype=torch.float32, device=dev)

    def call(mag_ptr=mag.data_ptr(), out_ptr=out.data_ptr(), B=B, T=T, hop=hop, nf=n):
        return h.dv3_spsi_phasor_f32(mag_ptr, out_ptr, B, T, hop, None, nf, st)
    for kw, needle in ((dict(nf=4096), "n_fft = 4096 is not supported: the FFT kernels are built for 512, 1024 and 2048"),
                       (dict(nf=1000), "n_fft = 1000"), (dict(mag_ptr=None), "mag"), (dict(out_ptr=None), "phasor"),
                       (dict(out_ptr=out.data_ptr() + 4), "aligned"), (dict(B=0), "B = 0"), (dict(T=0), "T = 0"),
                       (dict(hop=0), "hop = 0"), (dict(hop=n + 1), "hop = 2049")):
        assert call(**kw) == einval, kw
        assert needle in h.dv3_last_error().decode(), (kw, h.dv3_last_error().decode())
    torch.cuda.synchronize()
    assert bool((out == SENTINEL).all())
    with pytest.raises(ValueError, match="fft_size=4096"):
        audio.spsi_phasor(torch.zeros(1, 4, 2049, device=dev), 1024, fft_size=4096)
    with pytest.raises(ValueError, match="513 bins"):
        audio.spsi_phasor(torch.zeros(1, 4, 513, device=dev), 512, fft_size=2048)
    with pytest.raises(ValueError, match="tlen"):
        audio.spsi_phasor(mag, hop, torch.tensor([T, 1], device=dev), n)              # int64
    with pytest.raises(ValueError, match="hop=0"):
        audio.spsi_phasor(mag, 0, fft_size=n)


# ----------------------------------------------------------------------------------------------------------------------
# 4. convergence on the device, through inv_spectrogram_batch
# ----------------------------------------------------------------------------------------------------------------------
def _features(m64, dev, n, hop, **kw):
    """A config under which inv_spectrogram_batch returns Griffin-Lim's own signal on given magnitudes (power 1, no
    de-emphasis, a 200 dB range below 1000 so that nothing is clipped), and the normalised features that hold them
    -> (cfg, lin on the device)"""
    from deepvoice3_pytorch_amd import audio
    cfg = audio.AudioConfig(fft_size=n, hop_size=hop, sample_rate=RATE[n], preemphasis=0.0, min_level_db=-200,
                            ref_level_db=60, power=1.0, **kw)
    lin = (20.0 * np.log10(np.maximum(m64, 1e-7)) - 60.0 + 200.0) / 200.0
    assert lin.min() >= 0.0 and lin.max() <= 1.0
    return cfg, torch.from_numpy(lin.astype(np.float32)).to(dev)


@pytest.mark.parametrize("n,hop", R.CONVERGENCE_CASES)
def test_spsi_and_ten_momentum_iterations_beat_sixty_plain_ones_on_the_device(dev, n, hop):
    """tests/test_cpu_spsi_ref.py's condition with the device in the restatement's place: SPSI + 10 iterations at 0.99
    through inv_spectrogram_batch against the RESTATEMENT's 60 plain iterations from zero phase (0.1098, 0.1123,
    0.0849).  The magnitudes go in as normalised features (see _features); what audio.magnitudes makes of them is within
    1e-4 of the fixture and is what the spectral convergence is measured against.
    Measured on an MI355X: 0.0769, 0.0776, 0.0714 (the restatement's own figures to four digits)."""
    from deepvoice3_pytorch_amd import audio
    m64 = R.speechlike_magnitudes(n, hop)
    cfg, lin = _features(m64, dev, n, hop, griffin_lim_init="spsi", griffin_lim_iters=10, griffin_lim_momentum=0.99)
    held = audio.magnitudes(lin, cfg).cpu().numpy().astype(np.float64)
    assert np.abs(held - m64).max() < 1e-4 * m64.max()
    y = audio.inv_spectrogram_batch(lin, cfg).cpu().numpy()
    s, ref = R.spectral_convergence(y, held, hop, n), R.plain60(n, hop)
    print("n %d hop %d: device spsi + 10 x 0.99 %.4f, restatement 60 plain %.4f, ratio %.3f" % (n, hop, s, ref, s / ref))
    assert s < ref, (s, ref)


# ----------------------------------------------------------------------------------------------------------------------
# 5. bit identity of the two settings
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", SIZES)
def test_zero_is_the_plain_call_and_spsi_the_call_by_hand(dev, n):
    from deepvoice3_pytorch_amd import audio
    hop, B, T = n // 4, 2, 13
    frames = [T, 9]
    lin = torch.rand(B, T, n // 2 + 1, generator=torch.Generator().manual_seed(n)).to(dev)
    kw = dict(fft_size=n, hop_size=hop, sample_rate=RATE[n], griffin_lim_iters=3, griffin_lim_momentum=0.99)
    plain, zero, on = audio.AudioConfig(**kw), audio.AudioConfig(griffin_lim_init="zero", **kw), \
        audio.AudioConfig(griffin_lim_init="spsi", **kw)
    mag = audio.magnitudes(lin, plain)
    tlen = torch.tensor(frames, dtype=torch.int32, device=dev)
    # the batch path
    w = audio.inv_spectrogram_batch(lin, plain)
    assert torch.equal(audio.inv_spectrogram_batch(lin, zero), w)
    s = audio.inv_spectrogram_batch(lin, on)
    assert not torch.equal(s, w)
    assert torch.equal(s, audio.inv_spectrogram_batch(lin, plain, init_phasor=audio.spsi_phasor(mag, hop, fft_size=n)))
    mine = audio.spsi_phasor(mag.flip(1).contiguous(), hop, fft_size=n)               # an explicit init_phasor wins
    assert torch.equal(audio.inv_spectrogram_batch(lin, on, init_phasor=mine),
                       audio.inv_spectrogram_batch(lin, plain, init_phasor=mine))
    # the items path
    w, n0 = audio.inv_spectrogram_batch(lin, plain, frame_lengths=frames)
    z, n1 = audio.inv_spectrogram_batch(lin, zero, frame_lengths=frames)
    assert torch.equal(z, w) and torch.equal(n0, n1)
    s, n2 = audio.inv_spectrogram_batch(lin, on, frame_lengths=frames)
    assert not torch.equal(s, w) and torch.equal(n0, n2)
    by_hand, _ = audio.inv_spectrogram_batch(lin, plain, init_phasor=audio.spsi_phasor(mag, hop, tlen, n),
                                             frame_lengths=frames)
    assert torch.equal(s, by_hand)
    for b, k in enumerate(frames):                                                    # and each item as if alone
        alone = audio.inv_spectrogram_batch(lin[b:b + 1, :k].contiguous(), on)[0]
        assert torch.equal(s[b, :alone.numel()], alone) and not s[b, alone.numel():].any(), b
    # from a mel: inv_melspectrogram_batch is inv_spectrogram_batch of mel_to_linear
    mel = torch.rand(B, T, 20, generator=torch.Generator().manual_seed(n + 1)).to(dev)
    opt = audio.MelInverse(iters=4)
    lin2 = audio.mel_to_linear(mel, plain, options=opt)
    got = audio.inv_melspectrogram_batch(mel, on, options=opt)
    assert torch.equal(got, audio.inv_spectrogram_batch(lin2, on))
    assert not torch.equal(got, audio.inv_melspectrogram_batch(mel, plain, options=opt))
    got, _ = audio.inv_melspectrogram_batch(mel, on, frames, options=opt)
    want, _ = audio.inv_spectrogram_batch(audio.mel_to_linear(mel, plain, frames, options=opt), on, frame_lengths=frames)
    assert torch.equal(got, want)


# ----------------------------------------------------------------------------------------------------------------------
# 6. synthesis carries the option
# ----------------------------------------------------------------------------------------------------------------------
E2E_HP = dict(n_vocab=40, embed_dim=32, mel_dim=20, linear_dim=257, r=1, downsample_step=4, padding_idx=0, dropout=0.05,
              kernel_size=3, encoder_channels=64, decoder_channels=32, converter_channels=32, use_memory_mask=True,
              force_monotonic_attention=True, use_decoder_state_for_postnet_input=True, key_projection=True,
              value_projection=True, max_positions=128)


def test_synthesis_carries_the_option(dev):
    """the tiny model of tests/test_gpu_fast_gl.py at 512 / 128: tts_batch and tts_stream with a config that carries
    griffin_lim_init="spsi" give, per utterance, the waveform of the by-hand call on the utterance's own spectrogram
    (bit for bit: each item is inverted as if alone), which is not the zero start's; from_mel=True the same."""
    from deepvoice3_pytorch_amd import audio, builder, synthesis
    torch.manual_seed(0)
    model = builder.deepvoice3(**E2E_HP).to(dev).eval()
    dec = model.seq2seq.decoder
    dec.min_decoder_steps = dec.max_decoder_steps = 11
    rng = np.random.RandomState(2)
    ids = [rng.randint(2, 40, 9).tolist(), rng.randint(2, 40, 14).tolist()]
    kw = dict(fft_size=512, hop_size=128, sample_rate=16000, griffin_lim_iters=3, griffin_lim_momentum=0.99)
    zero, on = audio.AudioConfig(**kw), audio.AudioConfig(griffin_lim_init="spsi", **kw)
    for from_mel in (False, True):
        res = synthesis.tts_batch(model, ids, audio_cfg=on, from_mel=from_mel)
        base = synthesis.tts_batch(model, ids, audio_cfg=zero, from_mel=from_mel)
        assert len(res) == len(base) == 2
        for b in range(2):
            lin, wav = res[b][1], res[b][3]
            assert torch.equal(lin, base[b][1]) and wav.shape == base[b][3].shape
            assert not torch.equal(wav, base[b][3]), (from_mel, b)
            one = lin[None].contiguous()
            ph = audio.spsi_phasor(audio.magnitudes(one, zero), 128, fft_size=512)
            by_hand = audio.inv_spectrogram_batch(one, zero, init_phasor=ph)[0]
            assert torch.equal(wav, by_hand), (from_mel, b, float((wav - by_hand).abs().max()))
        got = {r[0]: r[4] for r in synthesis.tts_stream(model, ids, slots=2, audio_cfg=on, from_mel=from_mel)}
        assert sorted(got) == [0, 1]
        for b in range(2):
            assert torch.equal(got[b], res[b][3]), (from_mel, b)

# coding: utf-8
"""-m gpu: fast Griffin-Lim (csrc/audio.hip: gl_project2_kernel<N, LWS, true>; include/dv3hip.h:
dv3_gl_project_momentum_f32) against the float64 restatement of tests/fast_gl_ref.py.

  1. audio.griffin_lim(momentum=) against the restatement: three frame sizes, two hops, an even and an odd frame count
     (the unpaired last frame), both framings, alpha 0.5 and 0.99, 1 / 2 / 5 / 8 iterations;
  2. momentum = 0 is the call without the argument, bit for bit;
  3. every item of a ragged batch as its own B = 1 call, bit for bit;
  4. the scratch buffer's edges through the raw entry point: nothing outside an item's own rows is touched, the rows
     hold the STFT, the first call does not read the buffer;
  5. on the device 30 iterations at 0.99 end below 0.8 x the restatement's 60 plain ones;
  6. tts_batch, tts_stream and torch.ops.dv3hip.griffin_lim carry the option;
  7. refusals."""
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tests import fast_gl_ref as R  # noqa: E402
from oracle import audio_oracle as A  # noqa: E402

pytestmark = pytest.mark.gpu

SIZES = [512, 1024, 2048]
RATE = {512: 16000, 1024: 22050, 2048: 48000}
SENTINEL = -12345.0


def _f(n):
    """the depth factor of tests/test_gpu_fft_sizes.py on the bounds of tests/test_audio.py"""
    return max(1.0, np.log2(n) / 10.0)


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


def _rel(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return float(np.abs(a - b).max() / np.abs(b).max())


def _draw(dev, n, hop, B, T):
    """the input of test_griffin_lim_matches_the_restatement_and_converges (tests/test_gpu_fft_sizes.py): clipped normal
    features through audio.magnitudes, a random initial phase -> (mag on the device, its fp64 copy, phasor, init)"""
    from deepvoice3_pytorch_amd import audio
    F = n // 2 + 1
    rng = np.random.RandomState(15 + hop)
    lin = torch.from_numpy(np.clip(0.55 + 0.25 * rng.randn(B, T, F), -0.2, 1.2).astype(np.float32))
    mag = audio.magnitudes(lin.to(dev), audio.AudioConfig(fft_size=n, hop_size=hop, sample_rate=RATE[n]))
    phz = rng.uniform(-np.pi, np.pi, (B, T, F)).astype(np.float32)
    phasor = torch.from_numpy(np.stack([np.cos(phz), np.sin(phz)], axis=-1)).to(dev)
    return mag, mag.cpu().numpy().astype(np.float64), phasor, np.exp(1j * phz.astype(np.float64))


# ----------------------------------------------------------------------------------------------------------------------
# 1. against the restatement
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", SIZES)
def test_momentum_matches_the_restatement(dev, n):
    """Bound: the project's own for Griffin-Lim, 5e-4 * max(1, log2(n) / 10) of the maximum (an fp32 emulation of the
    algorithm on these draws stays below 5e-6).  Measured on an MI355X, the largest error over the hops, frame counts,
    alphas and iteration counts: lws 9.4e-07 / 9.0e-06 / 2.3e-06 and torch 2.1e-05 / 2.1e-06 / 2.4e-05 at 512 / 1024 /
    2048 (the largest ones after 8 iterations: a bin whose t is small takes its phase from rounding, and the following
    iterations carry the difference on)."""
    from deepvoice3_pytorch_amd import audio
    B, iters, worst = 2, (1, 2, 5, 8), {"lws": 0.0, "torch": 0.0}
    for hop in (n // 4, 3 * n // 16):
        for T in (12, 13):
            mag, m64, phasor, init = _draw(dev, n, hop, B, T)
            for alpha in (0.5, 0.99):
                for conv in ("lws", "torch"):
                    want = R.fast_griffin_lim(m64, max(iters), hop, n, alpha, init, conv, at=iters)
                    for k in iters:
                        got = audio.griffin_lim(mag, hop, k, phasor, convention=conv, fft_size=n, momentum=alpha)
                        assert tuple(got.shape) == want[k].shape == (B, audio.num_samples(T, hop, conv, n))
                        e = _rel(got.cpu().numpy(), want[k])
                        worst[conv] = max(worst[conv], e)
                        print("n %d hop %d T %d alpha %.2f %s iterations %d: %.2e" % (n, hop, T, alpha, conv, k, e))
                        assert e < 5e-4 * _f(n), (hop, T, alpha, conv, k, e)
    print("n %d: largest error lws %.2e torch %.2e" % (n, worst["lws"], worst["torch"]))


# ----------------------------------------------------------------------------------------------------------------------
# 2. momentum = 0 is the plain call
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", SIZES)
def test_momentum_zero_is_the_plain_call(dev, n):
    from deepvoice3_pytorch_amd import audio
    hop, B, T = n // 4, 2, 13
    mag, _, phasor, _ = _draw(dev, n, hop, B, T)
    for conv in ("lws", "torch"):
        tlen = torch.tensor([T, max(9, audio.min_frames(hop, conv, n))], dtype=torch.int32, device=dev)
        for tl in (None, tlen):
            want = audio.griffin_lim(mag, hop, 3, phasor, conv, None, tl, n)
            got = audio.griffin_lim(mag, hop, 3, phasor, conv, None, tl, n, 0.0)
            assert torch.equal(got, want), (conv, tl is None)
            assert not torch.equal(audio.griffin_lim(mag, hop, 3, phasor, conv, None, tl, n, 0.99), want)
    lin = torch.rand(B, T, n // 2 + 1, generator=torch.Generator().manual_seed(n)).to(dev)
    kw = dict(fft_size=n, hop_size=hop, sample_rate=RATE[n], griffin_lim_iters=3)
    w0, s0 = audio.inv_spectrogram_batch(lin, audio.AudioConfig(**kw), frame_lengths=[T, 9])
    w1, s1 = audio.inv_spectrogram_batch(lin, audio.AudioConfig(griffin_lim_momentum=0.0, **kw), frame_lengths=[T, 9])
    assert torch.equal(w0, w1) and torch.equal(s0, s1)


# ----------------------------------------------------------------------------------------------------------------------
# 3. each item as if alone
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("convention", ["lws", "torch"])
@pytest.mark.parametrize("n", SIZES)
def test_per_item_equals_b1(dev, n, convention):
    from deepvoice3_pytorch_amd import audio
    g = torch.Generator().manual_seed(7 + n)
    for hop in (n // 4, 3 * n // 16):
        frames = [13, 10, audio.min_frames(hop, convention, n)]
        B, T = len(frames), max(frames)
        lin = torch.rand(B, T, n // 2 + 1, generator=g).to(dev)
        cfg = audio.AudioConfig(fft_size=n, hop_size=hop, sample_rate=RATE[n], griffin_lim_iters=4, convention=convention,
                                griffin_lim_momentum=0.99)
        wav, samples = audio.inv_spectrogram_batch(lin, cfg, frame_lengths=frames)
        assert wav.shape == (B, audio.num_samples(T, hop, convention, n))
        for b, k in enumerate(frames):
            want = audio.inv_spectrogram_batch(lin[b:b + 1, :k].contiguous(), cfg)[0]
            assert int(samples[b]) == want.numel() == audio.num_samples(k, hop, convention, n), (hop, b)
            assert torch.equal(wav[b, :want.numel()], want), (hop, b, float((wav[b, :want.numel()] - want).abs().max()))
            assert not wav[b, want.numel():].any(), (hop, b)


# ----------------------------------------------------------------------------------------------------------------------
# 4. the scratch buffer's edges
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("convention", ["lws", "torch"])
@pytest.mark.parametrize("n", [1024, 2048])
def test_scratch_buffer_edges(dev, n, convention):
    """B = 2, T = 13, tlen = (13, 9): both items end in an unpaired frame.  The phantom partner of item 1's is row 9, which
    is not the item's own; in the whole-batch form (tlen NULL) the phantom partner of the last item's frame 12 is the
    row behind the buffer, where a margin of one frame row stands.  Rows at and past tlen[b] and the margin keep their
    sentinel over two launches; the rows below hold the STFT of y (audio.stft's bound in tests/test_audio.py and
    tests/test_gpu_fft_sizes.py: 2e-6 * max(1, log2(n) / 10) of the maximum); a first call gives the same frames whatever
    the buffer held."""
    from deepvoice3_pytorch_amd import audio, _lib
    from deepvoice3_pytorch_amd.ops import _stream
    lws = convention == "lws"
    hop, B, T, F = n // 4, 2, 13, n // 2 + 1
    tl = [13, 9]
    tlen = torch.tensor(tl, dtype=torch.int32, device=dev)
    rng = np.random.RandomState(n + lws)
    L = audio.num_samples(T, hop, convention, n)
    ys = [torch.from_numpy(rng.randn(B, L).astype(np.float32)).to(dev) for _ in range(2)]
    mag = torch.from_numpy(rng.rand(B, T, F).astype(np.float32)).to(dev)
    awin, swin = audio.lws_windows(dev, hop, None, n) if lws else (None, None)

    def launch(y, buf, first, tlen_ptr=tlen.data_ptr(), alpha=0.99):
        frames = torch.full((B, T, n), SENTINEL, dtype=torch.float32, device=dev)
        _lib.call("dv3_gl_project_momentum_f32", y.data_ptr(), mag.data_ptr(), awin.data_ptr() if lws else None,
                  swin.data_ptr() if lws else None, buf.data_ptr(), frames.data_ptr(), B, T, hop, tlen_ptr, int(lws), n,
                  alpha, first, _stream())
        return frames

    def fresh(fill):
        buf = torch.full((B * T + 1, F, 2), fill, dtype=torch.float32, device=dev)      # the last row: the margin
        for b in range(B):
            buf[b * T + tl[b]:(b + 1) * T] = SENTINEL
        buf[B * T] = SENTINEL
        return buf

    def check(buf, y, what):
        rows = buf[:B * T].reshape(B, T, F, 2)
        assert bool((buf[B * T] == SENTINEL).all()), (what, "the margin behind the buffer was written")
        for b in range(B):
            assert bool((rows[b, tl[b]:] == SENTINEL).all()), (what, b, "rows past the item's frames were written")
            Lb = audio.num_samples(tl[b], hop, convention, n)
            _, sp = audio.stft(y[b:b + 1, :Lb].contiguous(), tl[b], hop, want_phasor=False, want_spec=True,
                               convention=convention, fft_size=n)
            e = _rel(rows[b, :tl[b]].cpu().numpy(), sp[0].cpu().numpy())
            print("n %d %s %s item %d: cprev against audio.stft %.2e" % (n, convention, what, b, e))
            assert e < 2e-6 * _f(n), (what, b, e)

    nan_buf, zero_buf = fresh(float("nan")), fresh(0.0)
    f_nan, f_zero = launch(ys[0], nan_buf, 1), launch(ys[0], zero_buf, 1)
    torch.cuda.synchronize()
    assert torch.equal(f_nan, f_zero), "a first call read the scratch buffer"
    for b in range(B):
        assert bool(torch.isfinite(f_nan[b, :tl[b]]).all()) and bool((f_nan[b, :tl[b]] != SENTINEL).any())
        assert bool((f_nan[b, tl[b]:] == SENTINEL).all()), (b, "frames past the item's own were written")
    check(nan_buf, ys[0], "first")
    # a first call projects as the plain per-item entry does (t = c): the same frames up to the rounding of one FMA
    plain = torch.full((B, T, n), SENTINEL, dtype=torch.float32, device=dev)
    _lib.call("dv3_gl_project_items_f32_n", ys[0].data_ptr(), mag.data_ptr(), awin.data_ptr() if lws else None,
              swin.data_ptr() if lws else None, plain.data_ptr(), B, T, hop, tlen.data_ptr(), int(lws), n, _stream())
    for b in range(B):
        assert _rel(f_nan[b, :tl[b]].cpu().numpy(), plain[b, :tl[b]].cpu().numpy()) < 1e-5, b
    c0 = torch.view_as_complex(nan_buf[:T].cpu().double().contiguous()).numpy()[None]     # item 0's rows, as the next call reads them
    f2 = launch(ys[1], nan_buf, 0)
    torch.cuda.synchronize()
    check(nan_buf, ys[1], "second")
    for b in range(B):
        assert bool(torch.isfinite(f2[b, :tl[b]]).all()) and bool((f2[b, tl[b]:] == SENTINEL).all()), b
    # the second call used what the first left: item 0's frames against fp64 on the fp32 spectra the buffer held
    c1 = torch.view_as_complex(nan_buf[:T].cpu().double().contiguous()).numpy()[None]
    t = c1 + 0.99 * (c1 - c0)
    spec = mag[:1].cpu().double().numpy() * (t / np.maximum(np.abs(t), 1e-8))
    if lws:
        want = np.fft.irfft(spec, n=n, axis=-1) * A.lws_windows(n, hop)[1]
    else:
        want = np.fft.irfft(spec, n=n, axis=-1) * (0.5 - 0.5 * np.cos(2 * np.pi * np.arange(n) / n))
    e = _rel(f2[0].cpu().numpy(), want[0])
    print("n %d %s: frames of the second call against fp64 %.2e" % (n, convention, e))
    assert e < 5e-4 * _f(n), e
    # the whole-batch form (tlen NULL) on a buffer of exactly B * T rows plus the margin
    full = torch.full((B * T + 1, F, 2), float("nan"), dtype=torch.float32, device=dev)
    full[B * T] = SENTINEL
    launch(ys[0], full, 1, None)
    launch(ys[1], full, 0, None)
    torch.cuda.synchronize()
    assert bool((full[B * T] == SENTINEL).all()) and bool(torch.isfinite(full[:B * T]).all())
    _, sp = audio.stft(ys[1], T, hop, want_phasor=False, want_spec=True, convention=convention, fft_size=n)
    assert _rel(full[:B * T].reshape(B, T, F, 2).cpu().numpy(), sp.cpu().numpy()) < 2e-6 * _f(n)


# ----------------------------------------------------------------------------------------------------------------------
# 5. convergence on the device
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,hop", R.CONVERGENCE_CASES)
def test_thirty_momentum_iterations_beat_sixty_plain_ones_on_the_device(dev, n, hop):
    """tests/test_cpu_fast_gl.py's condition with the device in the restatement's place: its 30 iterations at 0.99 against
    0.8 x the RESTATEMENT's 60 plain ones (0.1098, 0.1123, 0.0849).  Measured on an MI355X: 0.0583, 0.0611, 0.0564 (the
    restatement's own figures to four digits); the device's 60 plain iterations: 0.1098, 0.1123, 0.0849."""
    from deepvoice3_pytorch_amd import audio
    m64 = R.speechlike_magnitudes(n, hop)
    mag = torch.from_numpy(m64.astype(np.float32)).to(dev)
    fast = audio.griffin_lim(mag, hop, 30, None, "lws", fft_size=n, momentum=0.99).cpu().numpy()
    plain = audio.griffin_lim(mag, hop, 60, None, "lws", fft_size=n).cpu().numpy()
    s_fast, s_plain = R.spectral_convergence(fast, m64, hop, n), R.spectral_convergence(plain, m64, hop, n)
    ref = R.plain60(n, hop)
    print("n %d hop %d: device 30 x 0.99 %.4f, device 60 plain %.4f, restatement 60 plain %.4f, ratio %.3f"
          % (n, hop, s_fast, s_plain, ref, s_fast / ref))
    assert s_fast < 0.8 * ref, (s_fast, ref)


# ----------------------------------------------------------------------------------------------------------------------
# 6. the public paths
# ----------------------------------------------------------------------------------------------------------------------
E2E_HP = dict(n_vocab=40, embed_dim=32, mel_dim=20, linear_dim=1025, r=1, downsample_step=4, padding_idx=0, dropout=0.05,
              kernel_size=3, encoder_channels=64, decoder_channels=32, converter_channels=32, use_memory_mask=True,
              force_monotonic_attention=True, use_decoder_state_for_postnet_input=True, key_projection=True,
              value_projection=True, max_positions=128)


def test_public_paths_carry_the_momentum(dev):
    """the tiny model of test_tts_at_2048 (tests/test_gpu_fft_sizes.py) and that test's tolerance, 1e-3"""
    from deepvoice3_pytorch_amd import audio, builder, synthesis, torch_ops  # noqa: F401 (registers torch.ops.dv3hip)
    torch.manual_seed(0)
    model = builder.deepvoice3(**E2E_HP).to(dev).eval()
    dec = model.seq2seq.decoder
    dec.min_decoder_steps = dec.max_decoder_steps = 11
    rng = np.random.RandomState(2)
    ids = [rng.randint(2, 40, 9).tolist(), rng.randint(2, 40, 14).tolist()]
    cfg = audio.AudioConfig(fft_size=2048, hop_size=512, sample_rate=48000, griffin_lim_iters=4, griffin_lim_momentum=0.99)
    res = synthesis.tts_batch(model, ids, audio_cfg=cfg)
    assert len(res) == 2
    for b, (mel, lin, ali, wav) in enumerate(res):
        m64 = A.magnitudes(lin.cpu().numpy()[None])
        want = A.inv_preemphasis(R.fast_griffin_lim(m64, 4, 512, 2048, 0.99), 0.97)[0]
        plain = A.inv_preemphasis(A.lws_griffin_lim(m64, 4, 512), 0.97)[0]
        assert want.shape == tuple(wav.shape)
        e, d = _rel(wav.cpu().numpy(), want), _rel(plain, want)
        print("utterance %d: waveform error %.2e (the plain algorithm's waveform is %.2e away)" % (b, e, d))
        assert e < 1e-3 and d > 10 * e, (b, e, d)
    got = {i: wav for i, _, _, _, wav in synthesis.tts_stream(model, ids, slots=2, audio_cfg=cfg)}
    assert sorted(got) == [0, 1]
    for b in range(2):
        assert torch.equal(got[b], res[b][3]), (b, float((got[b] - res[b][3]).abs().max()))
    mag = torch.rand(2, 13, 513, generator=torch.Generator().manual_seed(1)).to(dev)
    w0 = audio.griffin_lim(mag, 256, 5, momentum=0.99)
    w1 = torch.ops.dv3hip.griffin_lim(mag, 256, 5, 1024, 0.99)
    assert torch.equal(w0, w1) and not torch.equal(w0, torch.ops.dv3hip.griffin_lim(mag, 256, 5))


# ----------------------------------------------------------------------------------------------------------------------
# 7. refusals
# ----------------------------------------------------------------------------------------------------------------------
def test_refusals(dev):
    from deepvoice3_pytorch_amd import audio, _lib, torch_ops  # noqa: F401
    from deepvoice3_pytorch_amd.ops import _stream
    n, hop, B, T = 1024, 256, 1, 12
    mag = torch.rand(B, T, 513, device=dev)
    for bad in (1.0, -0.1, float("nan")):
        with pytest.raises(ValueError, match=r"\[0, 1\)"):
            audio.griffin_lim(mag, hop, 2, momentum=bad)
    with pytest.raises((ValueError, RuntimeError)):
        torch.ops.dv3hip.griffin_lim(mag, hop, 2, 1024, 1.0)
    h = _lib.lib()
    y = torch.zeros(B, hop * (T + 1), device=dev)
    out = torch.full((B * T * n,), 7.0, dtype=torch.float32, device=dev)
    cp = torch.full((B * T * 513 * 2,), 7.0, dtype=torch.float32, device=dev)
    aw, sw = audio.lws_windows(dev, hop, None, n)
    st = _stream()

    def call(alpha=0.99, cprev=cp.data_ptr(), nf=n, T=T, hop=hop, lws=1):
        return h.dv3_gl_project_momentum_f32(y.data_ptr(), mag.data_ptr(), aw.data_ptr(), sw.data_ptr(), cprev,
                                             out.data_ptr(), B, T, hop, None, lws, nf, alpha, 1, st)
    einval = _lib.CONSTS["DV3_EINVAL"]
    for kw, needle in ((dict(alpha=1.0), "alpha = 1"), (dict(alpha=-0.1), "alpha = -0.1"), (dict(alpha=float("nan")), "alpha"),
                       (dict(cprev=None), "cprev"), (dict(nf=4096), "n_fft = 4096"), (dict(T=3), "fewer"),
                       (dict(T=3, lws=0), "fewer"), (dict(hop=1025), "bad arguments")):
        assert call(**kw) == einval, kw
        assert needle in h.dv3_last_error().decode(), (kw, h.dv3_last_error().decode())
    torch.cuda.synchronize()
    assert bool((out == 7.0).all()) and bool((cp == 7.0).all())
    assert call() == 0                                              # and the same call with a momentum it takes runs
    torch.cuda.synchronize()
    assert bool((out != 7.0).any()) and bool((cp != 7.0).all())

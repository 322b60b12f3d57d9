# coding: utf-8
"""The audio kernels at fft_size 512 and 2048 (csrc/audio.hip: fft_lds<N, SIGN> and the frame kernels templated on N;
include/dv3hip.h: the `_n` entry points), next to the 1024 the rest of the suite runs.

  1. known answers of the transform: a unit impulse and two cosines through the torch-framing STFT;
  2. tests/test_audio.py's GPU tests mirrored at the new sizes, lengths and hops scaled by n / 1024, same bounds times
     max(1, log2(n) / 10) (the transform's rounding grows with its depth): 1.0 at 512, 1.1 at 2048;
  3. every item of a ragged batch as if alone, bit for bit (inverse and features);
  4. refusals: a spectrogram of the wrong width, n_fft = 4096 at every sibling, too few frames;
  5. end to end: tts_batch and RollingSynthesizer with a linear_dim = 1025 model at 2048 / 512 / 48 kHz;
  6. the LJSpeech preprocessor at 512 / 128 / 16 kHz.

Shapes: B <= 3, at most 12 frames, two hops per size -- n/4 and 3n/16, which does not divide the frame (six frames
overlap a sample)."""
import json
import os

import numpy as np
import pytest
import torch

from oracle import audio_oracle as A

pytestmark = pytest.mark.gpu

SIZES = [512, 2048]
RATE = {512: 16000, 1024: 22050, 2048: 48000}


def _f(n):
    """the depth factor on tests/test_audio.py's bounds"""
    return max(1.0, np.log2(n) / 10.0)


def _hops(n):
    return (n // 4, 3 * n // 16)


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


def _rel(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return float(np.abs(a - b).max() / np.abs(b).max())


def _cplx(t):
    return torch.view_as_complex(t.detach().cpu().double().contiguous()).numpy()


# ----------------------------------------------------------------------------------------------------------------------
# 1. known answers
# ----------------------------------------------------------------------------------------------------------------------
def _hann_dft(j, n):
    """sum_m hann_periodic[m] exp(-2 pi i j m / n) for integer j: n/2 at j = 0, -n/4 at j = +-1 (mod n), else 0"""
    j = j % n
    return 0.5 * n * (j == 0) - 0.25 * n * ((j == 1) | (j == n - 1))


@pytest.mark.parametrize("n", SIZES)
def test_transform_known_answers(dev, n):
    """Torch framing (periodic Hann w, frame t = samples [t hop - n/2, t hop + n/2)); only frames that lie inside the
    signal are looked at, so no reflection enters.  A unit impulse at offset m of a frame gives w[m] exp(-2 pi i k m / n);
    a cosine of amplitude 4 / n on bin kb gives exp(i phi) in bin kb, -1/2 exp(i phi) in kb +- 1 and nothing elsewhere
    (Nyquist, where both halves of the cosine meet: amplitude 2 / n gives +-1 in bin n/2 and -+1/2 in n/2 - 1).  A misplaced radix-2 pass or a
    wrong twiddle index moves or scales single bins, which these spectra show and a relative norm over noise can hide.
    Bound: 1e-6 absolute, spectra of unit scale."""
    from deepvoice3_pytorch_amd import audio
    T = 12
    k = np.arange(n // 2 + 1)
    w = 0.5 - 0.5 * np.cos(2 * np.pi * np.arange(n) / n)
    for hop in _hops(n):
        L = hop * (T - 1)
        starts = np.arange(T) * hop - n // 2
        inside = [t for t in range(T) if starts[t] >= 0 and starts[t] + n <= L]
        assert len(inside) >= 2
        t0 = inside[0]
        sigs, wants = [], []
        for n0 in (1, n // 2 + 3):                                  # impulses, placed by their offset in frame t0
            x = np.zeros(L)
            p = starts[t0] + n0
            x[p] = 1.0
            want = np.zeros((T, n // 2 + 1), dtype=np.complex128)
            for t in inside:
                m = p - starts[t]
                if 0 <= m < n:
                    want[t] = w[m] * np.exp(-2j * np.pi * k * m / n)
            assert abs(abs(want[t0, 5]) - w[n0]) < 1e-15
            sigs.append(x)
            wants.append(want)
        for kb in (n // 2, n // 4 + 1):                             # cosines on a bin
            amp = (2.0 if kb == n // 2 else 4.0) / n
            x = amp * np.cos(2 * np.pi * kb * np.arange(L) / n)
            want = np.zeros((T, n // 2 + 1), dtype=np.complex128)
            for t in inside:
                ph = np.exp(2j * np.pi * kb * starts[t] / n)
                want[t] = 0.5 * amp * (ph * _hann_dft(k - kb, n) + np.conj(ph) * _hann_dft(k + kb, n))
            peak = np.abs(want[inside]).max(axis=1)
            assert np.allclose(peak, 1.0) and np.abs(want[inside]).argmax(axis=1).tolist() == [kb] * len(inside)
            sigs.append(x)
            wants.append(want)
        y = torch.from_numpy(np.stack(sigs).astype(np.float32)).to(dev)
        _, sp = audio.stft(y, T, hop, want_phasor=False, want_spec=True, convention="torch", fft_size=n)
        got = _cplx(sp)
        for i, want in enumerate(wants):
            # the fp32 input carries its own rounding (the cosines'): the expectation is the fp32 signal's, to first order
            err = float(np.abs(got[i][inside] - want[inside]).max())
            print("n %d hop %d signal %d: max abs err %.2e" % (n, hop, i, err))
            assert err < 1e-6, (n, hop, i, err)


# ----------------------------------------------------------------------------------------------------------------------
# 2. the 1024 tests of tests/test_audio.py at the new sizes
# ----------------------------------------------------------------------------------------------------------------------
def _torch_cases(n):
    return [(1, 9, n // 4), (3, 12, n // 4), (2, 12, 3 * n // 16)]


@pytest.mark.parametrize("n", SIZES)
def test_stft_istft_match_torch_fft(dev, n):
    """test_hip_stft_istft_match_torch_fft: 2e-6 (spectrum), 1e-3 (phasor where |Z| > 1e-3 max), 2e-5 (inverses)"""
    from deepvoice3_pytorch_amd import audio
    F, f = n // 2 + 1, _f(n)
    for B, T, hop in _torch_cases(n):
        rng = np.random.RandomState(B * 100 + T + n)
        y = torch.from_numpy(rng.randn(B, hop * (T - 1)).astype(np.float32))
        ph, sp = audio.stft(y.to(dev), T, hop, want_phasor=True, want_spec=True, fft_size=n)
        Z = A.stft(y.double(), hop, n)
        got = torch.view_as_complex(sp.cpu().double().contiguous())
        assert got.shape == Z.shape == (B, T, F)
        e = _rel(torch.view_as_real(got).numpy(), torch.view_as_real(Z).numpy())
        gph = torch.view_as_complex(ph.cpu().double().contiguous())
        big = Z.abs() > 1e-3 * Z.abs().max()
        ep = float(((gph - Z / Z.abs())[big]).abs().max())
        mag = torch.from_numpy(rng.rand(B, T, F).astype(np.float32))
        phz = torch.from_numpy(rng.uniform(-np.pi, np.pi, (B, T, F)).astype(np.float32))
        phasor = torch.stack([torch.cos(phz), torch.sin(phz)], dim=-1)
        yg = audio.istft(mag.to(dev), phasor.to(dev), hop, fft_size=n)
        want = A.istft(mag.double() * torch.view_as_complex(phasor.double().contiguous()), hop, n)
        ei = _rel(yg.cpu().numpy(), want.numpy())
        yz = audio.istft(mag.to(dev), None, hop, fft_size=n)
        ez = _rel(yz.cpu().numpy(), A.istft(mag.double().to(torch.complex128), hop, n).numpy())
        print("n %d B %d T %d hop %d: stft %.2e phasor %.2e istft %.2e zero-phase %.2e" % (n, B, T, hop, e, ep, ei, ez))
        assert e < 2e-6 * f and ep < 1e-3 * f and ei < 2e-5 * f and ez < 2e-5 * f, (B, T, hop)


def _lws_cases(n):
    """2560, 256 * 37, 5000 and 1000 samples at 1024 / 256, scaled and cut to at most 12 frames: a hop multiple, a length
    that is none, one shorter than the frame, and one at the hop that does not divide the frame"""
    h = n // 4
    return [(1, 8 * h, h), (3, 7 * h + 37, h), (2, n - 3 * n // 128, h), (2, 20 * n // 16 + 5, 3 * n // 16)]


@pytest.mark.parametrize("n", SIZES)
def test_lws_framing_matches_the_restatement(dev, n):
    """test_hip_lws_framing_matches_the_restatement: 2e-6, 1e-3, 2e-5 (round trip), 2e-5 (inverses)"""
    from deepvoice3_pytorch_amd import audio
    F, f = n // 2 + 1, _f(n)
    for B, L, hop in _lws_cases(n):
        rng = np.random.RandomState(L + B)
        y = rng.randn(B, L).astype(np.float32)
        T = audio.lws_num_frames(L, hop, n)
        assert T <= 12
        ph, sp = audio.stft(torch.from_numpy(y).to(dev), T, hop, want_phasor=True, want_spec=True, convention="lws",
                            fft_size=n)
        Z = A.lws_stft(y.astype(np.float64), n, hop)
        got = _cplx(sp)
        assert got.shape == Z.shape == (B, T, F)
        e = float(np.abs(got - Z).max() / np.abs(Z).max())
        gph = _cplx(ph)
        big = np.abs(Z) > 1e-3 * np.abs(Z).max()
        ep = float(np.abs((gph - Z / np.maximum(np.abs(Z), 1e-30))[big]).max())
        mag = torch.from_numpy(np.abs(Z).astype(np.float32)).to(dev)
        back = audio.istft(mag, ph, hop, convention="lws", fft_size=n).cpu().numpy()
        assert back.shape[1] == audio.lws_num_samples(T, hop, n) >= L
        er = float(np.abs(back[:, :L] - y).max() / np.abs(y).max())
        m2 = rng.rand(B, T, F).astype(np.float32)
        phz = rng.uniform(-np.pi, np.pi, (B, T, F)).astype(np.float32)
        phasor = torch.from_numpy(np.stack([np.cos(phz), np.sin(phz)], axis=-1))
        yg = audio.istft(torch.from_numpy(m2).to(dev), phasor.to(dev), hop, convention="lws", fft_size=n).cpu().numpy()
        ei = _rel(yg, A.lws_istft(m2.astype(np.float64) * np.exp(1j * phz.astype(np.float64)), hop))
        yz = audio.istft(torch.from_numpy(m2).to(dev), None, hop, convention="lws", fft_size=n).cpu().numpy()
        ez = _rel(yz, A.lws_istft(m2.astype(np.complex128), hop))
        print("n %d B %d L %d hop %d T %d: stft %.2e phasor %.2e round trip %.2e istft %.2e zero-phase %.2e"
              % (n, B, L, hop, T, e, ep, er, ei, ez))
        assert e < 2e-6 * f and ep < 1e-3 * f and er < 2e-5 * f and ei < 2e-5 * f and ez < 2e-5 * f, (B, L, hop)


def _torch_gl(mag, n_iter, hop, n, init):
    """oracle.griffin_lim at n_fft = n (the oracle's own is fixed at 1024; its stft / istft take the size)"""
    y = A.istft(mag * init, hop, n)
    for _ in range(n_iter):
        Z = A.stft(y, hop, n)
        y = A.istft(mag * (Z / torch.clamp(Z.abs(), min=1e-8)), hop, n)
    return y


@pytest.mark.parametrize("n", SIZES)
def test_griffin_lim_matches_the_restatement_and_converges(dev, n):
    """test_hip_lws_griffin_lim_matches_the_restatement_and_converges and test_hip_griffin_lim_matches_oracle_and_converges:
    5e-4 after 0, 1 and 5 iterations on both framings at both hops; on the lws framing the spectral convergence falls
    with the iterations, and a consistent magnitude is approached at least twice as closely after 60 of them"""
    from deepvoice3_pytorch_amd import audio
    F, f = n // 2 + 1, _f(n)
    B, T = 2, 12
    for hop in _hops(n):
        rng = np.random.RandomState(15 + hop)
        lin = torch.from_numpy(np.clip(0.55 + 0.25 * rng.randn(B, T, F), -0.2, 1.2).astype(np.float32))
        cfg = audio.AudioConfig(fft_size=n, hop_size=hop, sample_rate=RATE[n])
        mag = audio.magnitudes(lin.to(dev), cfg)
        assert _rel(mag.cpu().numpy(), A.magnitudes(lin.numpy())) < 2e-5
        m64 = mag.cpu().numpy().astype(np.float64)
        phz = rng.uniform(-np.pi, np.pi, (B, T, F)).astype(np.float32)
        phasor = torch.from_numpy(np.stack([np.cos(phz), np.sin(phz)], axis=-1)).to(dev)
        init = np.exp(1j * phz.astype(np.float64))
        for n_iter in (0, 1, 5):
            got = audio.griffin_lim(mag, hop, n_iter, phasor, convention="lws", fft_size=n).cpu().numpy()
            want = A.lws_griffin_lim(m64, n_iter, hop, init)
            assert got.shape == want.shape == (B, (T + 1) * hop - n)
            e = _rel(got, want)
            gt = audio.griffin_lim(mag, hop, n_iter, phasor, convention="torch", fft_size=n).cpu().numpy()
            wt = _torch_gl(torch.from_numpy(m64), n_iter, hop, n, torch.from_numpy(init)).numpy()
            assert gt.shape == wt.shape == (B, hop * (T - 1))
            et = _rel(gt, wt)
            print("n %d hop %d iterations %d: lws %.2e torch %.2e" % (n, hop, n_iter, e, et))
            assert e < 5e-4 * f and et < 5e-4 * f, (hop, n_iter)

        def sc(y, m):
            Z = np.abs(A.lws_stft(y.astype(np.float64), n, hop))
            return float(np.linalg.norm(Z - m) / np.linalg.norm(m))
        s = [sc(audio.griffin_lim(mag, hop, k, phasor, convention="lws", fft_size=n).cpu().numpy(), m64) for k in (0, 10, 40)]
        assert s[2] < s[1] < s[0], s
        sig = np.cumsum(rng.randn(B, audio.lws_num_samples(T, hop, n)), axis=1) * 0.05
        cm = np.abs(A.lws_stft(sig, n, hop))
        assert cm.shape == (B, T, F)
        cmag = torch.from_numpy(cm.astype(np.float32)).to(dev)
        s = [sc(audio.griffin_lim(cmag, hop, k, phasor, convention="lws", fft_size=n).cpu().numpy(), cm) for k in (0, 60)]
        print("n %d hop %d: spectral convergence of a consistent magnitude %.3f -> %.3f" % (n, hop, s[0], s[1]))
        assert s[1] < 0.5 * s[0], s


def _speechlike(n, L, B, rng):
    """test_hip_spectrogram_and_melspectrogram's signal with its time axis scaled by n / 1024: 0.3 sin on bin 20.4 + 0.05 noise"""
    t = np.arange(L) / (22050.0 * n / 1024)
    return (0.3 * np.sin(2 * np.pi * 440 * t)[None] + 0.05 * rng.randn(B, L)).astype(np.float32)


def _lws_features(wav64, n, hop, sr, gain=None):
    """audio.spectrogram / audio.melspectrogram (audio.py:31-35,46-51) on the lws framing, composed from the oracle's
    steps (its lws_spectrogram / lws_melspectrogram are fixed at 1024) -> (lin (B, T, F), mel (B, T, 80))"""
    D = np.abs(A.lws_stft(A.preemphasis(wav64), n, hop))
    lin = A.normalize(A.amp_to_db(D) - 20, -100)
    M = np.einsum("mf,btf->btm", A.slaney_mel_basis(sr=sr, n_fft=n, n_mels=80, fmin=125.0, fmax=7600.0), D)
    return lin, A.normalize(A.amp_to_db(M) - 20, -100)


def _lin_errs(got, want, axis):
    """linear rows in [0, 1] against the oracle's, bins along `axis` -> (max error over every bin, max error over the
    bins of at least 1e-3 of their frame's peak, max amplitude error / frame peak over every bin); the last two are what
    tests/test_gpu_wav_features.py holds the ragged rows to"""
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    amp = lambda x: 10.0 ** ((x * 100.0 - 100.0 + 20.0) / 20.0)               # undo the normalisation (clipped bins too)
    peak = amp(want).max(axis=axis, keepdims=True)
    big = amp(want) >= 1e-3 * peak
    e = np.abs(got - want)
    return float(e.max()), float(e[big].max()), float((np.abs(amp(got) - amp(want)) / peak).max())


GEMM_MODES = ("f16x3", "bf16x3", "f32")


def feature_errors(dev, n, hop):
    """test_hip_spectrogram_and_melspectrogram's checks at frame size n: its signal (RandomState(8): 0.3 sin on bin 20.4
    + 0.05 noise, B = 2) with the time axis scaled by n / 1024 and cut to 12 torch frames; the lws framing on a hop
    multiple and on a length that is none (9 to 11 frames); the mel rows of the batch path under the three GEMM
    precision modes; the ragged path (features_items) on the same items without and with the rescaling gain.
    -> dict of the maximum errors, every one over EVERY bin unless its name says otherwise"""
    from deepvoice3_pytorch_amd import audio, ops
    F, sr = n // 2 + 1, RATE[n]
    rng = np.random.RandomState(8)
    B, T = 2, 12
    wav = _speechlike(n, hop * (T - 1), B, rng)
    w64 = wav.astype(np.float64)
    tcfg = audio.AudioConfig(fft_size=n, hop_size=hop, sample_rate=sr, convention="torch")
    lcfg = audio.AudioConfig(fft_size=n, hop_size=hop, sample_rate=sr)
    basis = A.slaney_mel_basis(sr=sr, n_fft=n, n_mels=80, fmin=125.0, fmax=7600.0)
    D = A.stft(torch.from_numpy(A.preemphasis(w64)), hop, n).abs().numpy().transpose(0, 2, 1)
    want = A.normalize(A.amp_to_db(D) - 20, -100)
    wantm = A.normalize(A.amp_to_db(np.einsum("mf,bft->bmt", basis, D)) - 20, -100)
    S = audio.spectrogram_batch(torch.from_numpy(wav).to(dev), tcfg)
    assert S.shape == (B, F, T)
    out = {}
    out["torch lin"], out["torch lin, bins >= 1e-3 peak"], out["torch lin, amplitude"] = _lin_errs(S.cpu().numpy(), want, 1)
    cuts = [np.ascontiguousarray(wav[:, :hop * 6]), np.ascontiguousarray(wav[:, :hop * 6 + 11])]
    lws_want = [_lws_features(wv.astype(np.float64), n, hop, sr) for wv in cuts]
    for mode in GEMM_MODES:                                       # the filterbank product: Cin = n / 2 + 1 on the tap-GEMM
        prev = ops.set_gemm_precision(mode)
        try:
            M = audio.melspectrogram_batch(torch.from_numpy(wav).to(dev), tcfg)
            Ml = audio.melspectrogram_batch(torch.from_numpy(cuts[1]).to(dev), lcfg)
        finally:
            ops.set_gemm_precision(prev)
        assert M.shape == (B, 80, T) and Ml.shape == (B, 80, lws_want[1][1].shape[1])
        out["torch mel " + mode] = float(np.abs(M.cpu().numpy() - wantm).max())
        out["lws mel " + mode] = float(np.abs(Ml.cpu().numpy() - lws_want[1][1].transpose(0, 2, 1)).max())
    lin_e, mel_e = [], []
    for wv, (wl, wm) in zip(cuts, lws_want):
        S = audio.spectrogram_batch(torch.from_numpy(wv).to(dev), lcfg).cpu().numpy()
        Tl = A.lws_num_frames(wv.shape[1], n, hop)
        assert S.shape == (B, F, Tl) and Tl <= 12
        lin_e.append(_lin_errs(S, wl.transpose(0, 2, 1), 1))
        # the ragged path: both items in one launch, without and with the rescaling gain
        for rmax in (None, 0.999):
            lin, mel, frames = audio.features_from_arrays(list(wv), lcfg, dev, rescaling=rmax)
            assert list(frames) == [Tl] * B and lin.shape == (B * Tl, F) and mel.shape == (B * Tl, 80)
            if rmax is None:
                gl, gm = wl, wm
                assert np.array_equal(lin.cpu().numpy().reshape(B, Tl, F).transpose(0, 2, 1), S)   # the batch path's bits
            else:
                g = np.array([np.float32(rmax) / np.abs(w).max() for w in wv], dtype=np.float32)
                scaled = (wv * g[:, None]).astype(np.float32)        # the fp32 products the kernel forms
                gl, gm = _lws_features(scaled.astype(np.float64), n, hop, sr)
            lin_e.append(_lin_errs(lin.cpu().numpy().reshape(B, Tl, F), gl, 2))
            mel_e.append(float(np.abs(mel.cpu().numpy().reshape(B, Tl, 80) - gm).max()))
    out["lws lin"], out["lws lin, bins >= 1e-3 peak"], out["lws lin, amplitude"] = (max(e[i] for e in lin_e) for i in range(3))
    out["ragged mel"] = max(mel_e)
    return out


@pytest.mark.parametrize("n", SIZES)
def test_spectrogram_and_melspectrogram(dev, n):
    """test_hip_spectrogram_and_melspectrogram at the new sizes, its bounds over EVERY bin: 2e-5 on the torch framing,
    5e-5 on the lws one (values live in [0, 1]), linear and mel, the mel rows under the three GEMM modes, on the batch
    path and through features_items without and with the rescaling gain -- times max(1, log2(n) / 10).  On top of that,
    what tests/test_gpu_wav_features.py holds linear rows to: the same bound on the bins of at least 1e-3 of their
    frame's peak, and 1e-5 of the frame's peak in amplitude for every bin.
    Measured over every bin (hops n/4, 3n/16): torch framing 1.07e-5, 1.33e-5 at 512 and 1.79e-5, 1.30e-5 at 2048; lws
    framing 2.6e-6, 2.11e-5 at 512 and 2.1e-6, 3.1e-6 at 2048; mel rows at most 1.5e-6 in every mode.  The 1024 kernel on
    the same scaled input (feature_errors(dev, 1024, hop)): torch 7.34e-5, 1.19e-5; lws 2.5e-6, 3.79e-5 -- the every-bin
    figure follows the smallest noise bin of the input, at every size."""
    f = _f(n)
    for hop in _hops(n):
        e = feature_errors(dev, n, hop)
        print("n %d hop %d: %s" % (n, hop, ", ".join("%s %.2e" % kv for kv in e.items())))
        for k, v in e.items():
            bound = 1e-5 if k.endswith("amplitude") else (2e-5 if k.startswith("torch") else 5e-5) * f
            assert v < bound, (n, hop, k, v, bound)


@pytest.mark.parametrize("n", SIZES)
def test_inv_spectrogram(dev, n):
    """test_hip_deemphasis_and_inv_spectrogram, end to end in the reference's calling convention: 1e-3"""
    from deepvoice3_pytorch_amd import audio
    F, f, hop = n // 2 + 1, _f(n), n // 4
    rng = np.random.RandomState(6 + n)
    spec = np.clip(0.5 + 0.2 * rng.randn(F, 12), 0, 1).astype(np.float32)
    mag = A.magnitudes(spec.T[None])
    wav = audio.inv_spectrogram(spec, audio.AudioConfig(fft_size=n, hop_size=hop, sample_rate=RATE[n], griffin_lim_iters=3,
                                                        convention="torch"))
    want = A.inv_preemphasis(_torch_gl(torch.from_numpy(mag), 3, hop, n, torch.ones(1, 12, F, dtype=torch.complex128)).numpy(),
                             0.97)[0]
    assert wav.shape == (hop * 11,) and np.isfinite(wav).all() and _rel(wav, want) < 1e-3 * f
    wav = audio.inv_spectrogram(spec, audio.AudioConfig(fft_size=n, hop_size=hop, sample_rate=RATE[n], griffin_lim_iters=3))
    want = A.inv_preemphasis(A.lws_griffin_lim(mag, 3, hop), 0.97)[0]
    assert wav.shape == (13 * hop - n,) and np.isfinite(wav).all() and _rel(wav, want) < 1e-3 * f


# ----------------------------------------------------------------------------------------------------------------------
# 3. each item as if alone
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("convention", ["lws", "torch"])
@pytest.mark.parametrize("n", SIZES)
def test_inverse_per_item_equals_b1(dev, n, convention):
    from deepvoice3_pytorch_amd import audio
    g = torch.Generator().manual_seed(5 + n)
    for hop in _hops(n):
        tmin = audio.min_frames(hop, convention, n)
        frames = [12, tmin, 7]
        B, T = len(frames), max(frames)
        lin = torch.rand(B, T, n // 2 + 1, generator=g).to(dev)
        cfg = audio.AudioConfig(fft_size=n, hop_size=hop, sample_rate=RATE[n], griffin_lim_iters=3, convention=convention)
        wav, samples = audio.inv_spectrogram_batch(lin, cfg, frame_lengths=frames)
        assert wav.shape == (B, audio.num_samples(T, hop, convention, n))
        for b, k in enumerate(frames):
            want = audio.inv_spectrogram_batch(lin[b:b + 1, :k].contiguous(), cfg)[0]
            assert int(samples[b]) == want.numel() == audio.num_samples(k, hop, convention, n), (hop, b)
            assert torch.equal(wav[b, :want.numel()], want), (hop, b, float((wav[b, :want.numel()] - want).abs().max()))
            assert not wav[b, want.numel():].any(), (hop, b)


@pytest.mark.parametrize("n", SIZES)
def test_features_per_item_equal_b1(dev, n):
    from deepvoice3_pytorch_amd import audio
    rng = np.random.RandomState(3 + n)
    for hop in _hops(n):
        cfg = audio.AudioConfig(fft_size=n, hop_size=hop, sample_rate=RATE[n])
        lengths = [6 * hop, n - 1, 5 * hop + 13]                 # a hop multiple, shorter than one frame, neither
        wavs = [_speechlike(n, L, 1, rng)[0] * s for L, s in zip(lengths, (1.0, 0.2, 2.0))]
        for rmax in (None, 0.999):
            lin, mel, frames = audio.features_from_arrays(wavs, cfg, dev, rescaling=rmax)
            assert list(frames) == [audio.lws_num_frames(L, hop, n) for L in lengths] and max(frames) <= 12
            o = np.concatenate([[0], np.cumsum(frames)])
            for b, w in enumerate(wavs):
                l1, m1, f1 = audio.features_from_arrays([w], cfg, dev, rescaling=rmax)
                assert list(f1) == [frames[b]] and l1.shape == (frames[b], n // 2 + 1)
                assert torch.equal(lin[o[b]:o[b + 1]], l1) and torch.equal(mel[o[b]:o[b + 1]], m1), (hop, rmax, b)


# ----------------------------------------------------------------------------------------------------------------------
# 4. refusals
# ----------------------------------------------------------------------------------------------------------------------
def test_refusals(dev):
    from deepvoice3_pytorch_amd import audio, _lib
    from deepvoice3_pytorch_amd.ops import _stream
    cfg = audio.AudioConfig(fft_size=2048, hop_size=512, sample_rate=48000, griffin_lim_iters=1)
    with pytest.raises(ValueError, match="513.*1025"):
        audio.inv_spectrogram_batch(torch.rand(2, 12, 513, device=dev), cfg)
    with pytest.raises(ValueError, match="513.*1025"):
        audio.inv_spectrogram_batch(torch.rand(2, 12, 513, device=dev), cfg, frame_lengths=[12, 9])
    with pytest.raises(ValueError, match="1025.*513"):
        audio.inv_spectrogram_batch(torch.rand(2, 12, 1025, device=dev))           # and the other way round
    with pytest.raises(ValueError, match="fft_size=4096"):
        audio.istft(torch.rand(1, 12, 2049, device=dev), None, 1024, fft_size=4096)
    # too few frames: (T + 1) * 512 - 2048 > 0 needs T >= 4 on the lws framing, 512 * (T - 1) > 1024 needs T >= 4 on the torch one
    assert audio.min_frames(512, "lws", 2048) == 4 and audio.min_frames(512, "torch", 2048) == 4
    with pytest.raises(ValueError, match=r"frame lengths in \[4, 12\]"):
        audio.inv_spectrogram_batch(torch.rand(2, 12, 1025, device=dev), cfg, frame_lengths=[12, 3])
    # the siblings themselves: DV3_EINVAL before anything is launched (the sentinel in the output survives)
    h = _lib.lib()
    B, T, hop = 1, 12, 512
    z = torch.zeros(B * T * 2049 * 2, dtype=torch.float32, device=dev)           # input enough for every call at 4096
    out = torch.full((B * T * 4096,), 7.0, dtype=torch.float32, device=dev)
    i32 = torch.full((4,), T, dtype=torch.int32, device=dev)
    i64 = torch.zeros(4, dtype=torch.int64, device=dev)
    p, o, st = z.data_ptr(), out.data_ptr(), _stream()

    def calls(nf, T=T):
        return {
            "dv3_istft_frames_f32_n": (p, p, o, B, T, nf, st),
            "dv3_overlap_add_f32_n": (p, o, B, T, hop, nf, st),
            "dv3_gl_project_f32_n": (p, p, o, B, T, hop, nf, st),
            "dv3_stft_phase_f32_n": (p, o, None, None, B, T, hop, nf, st),
            "dv3_lws_stft_f32_n": (p, p, o, None, None, B, T, hop, (T + 1) * hop - nf, nf, st),
            "dv3_lws_istft_frames_f32_n": (p, p, p, o, B, T, nf, st),
            "dv3_lws_overlap_add_f32_n": (p, o, B, T, hop, nf, st),
            "dv3_lws_gl_project_f32_n": (p, p, p, p, o, B, T, hop, nf, st),
            "dv3_gl_istft_items_f32_n": (p, p, p, o, B, T, hop, i32.data_ptr(), 1, nf, st),
            "dv3_overlap_add_items_f32_n": (p, o, B, T, hop, i32.data_ptr(), 1, nf, st),
            "dv3_gl_project_items_f32_n": (p, p, p, p, o, B, T, hop, i32.data_ptr(), 1, nf, st),
            "dv3_analysis_items_f32_n": (p, i64.data_ptr(), i32.data_ptr(), B, T, hop, 0.97, p, None, p, None, 80, -100.0,
                                         20.0, o, None, nf, st),
        }
    for bad in (4096, 768, 256, 0, -1024):
        for name, args in calls(bad).items():
            assert getattr(h, name)(*args) == _lib.CONSTS["DV3_EINVAL"], (name, bad)
            msg = h.dv3_last_error().decode()
            assert "n_fft = %d" % bad in msg and "512, 1024 and 2048" in msg, (name, msg)
    # T below the framing's minimum at a size the kernels take: refused on the host as well
    short = calls(2048, T=3)
    for name in ("dv3_overlap_add_f32_n", "dv3_lws_istft_frames_f32_n", "dv3_istft_frames_f32_n", "dv3_analysis_items_f32_n"):
        short.pop(name)                                              # these do not depend on the signal length
    for name, args in short.items():
        assert getattr(h, name)(*args) == _lib.CONSTS["DV3_EINVAL"], name
    torch.cuda.synchronize()
    assert bool((out == 7.0).all())


# ----------------------------------------------------------------------------------------------------------------------
# 5. end to end
# ----------------------------------------------------------------------------------------------------------------------
E2E_HP = dict(n_vocab=40, embed_dim=32, mel_dim=20, linear_dim=1025, r=1, downsample_step=4, padding_idx=0, dropout=0.05,
              kernel_size=3, encoder_channels=64, decoder_channels=32, converter_channels=32, use_memory_mask=True,
              force_monotonic_attention=True, use_decoder_state_for_postnet_input=True, key_projection=True,
              value_projection=True, max_positions=128)


def test_tts_at_2048(dev):
    from deepvoice3_pytorch_amd import audio, builder, synthesis
    torch.manual_seed(0)
    model = builder.deepvoice3(**E2E_HP).to(dev).eval()
    dec = model.seq2seq.decoder
    dec.min_decoder_steps = dec.max_decoder_steps = 11            # 12 steps: a random-weight done flag stays out of the rule
    rng = np.random.RandomState(2)
    ids = [rng.randint(2, 40, 9).tolist(), rng.randint(2, 40, 14).tolist()]
    cfg = audio.AudioConfig(fft_size=2048, hop_size=512, sample_rate=48000, griffin_lim_iters=3)
    res = synthesis.tts_batch(model, ids, audio_cfg=cfg)
    assert len(res) == 2
    for b, (mel, lin, ali, wav) in enumerate(res):
        Tb = lin.shape[0]
        assert lin.shape == (Tb, 1025) and Tb == 4 * mel.shape[0] == 48
        assert wav.shape == ((Tb + 1) * 512 - 2048,)
        want = A.inv_preemphasis(A.lws_griffin_lim(A.magnitudes(lin.cpu().numpy()[None]), cfg.griffin_lim_iters, 512), 0.97)[0]
        assert want.shape == wav.shape
        e = _rel(wav.cpu().numpy(), want)
        print("utterance %d: %d linear frames, waveform error %.2e" % (b, Tb, e))
        assert e < 1e-3, (b, e)
    rs = synthesis.RollingSynthesizer(model, slots=2, max_text_len=16, audio_cfg=cfg)
    tickets = [rs.submit(s) for s in ids]
    got = {tk: wav for tk, _, _, _, wav in rs.drain()}
    assert sorted(got) == tickets
    for b, tk in enumerate(tickets):
        assert got[tk].shape == res[b][3].shape and torch.equal(got[tk], res[b][3]), \
            (b, float((got[tk] - res[b][3]).abs().max()))
    # a model of 513 bins under this config: refused once, before any decode, with both numbers
    small = builder.deepvoice3(**dict(E2E_HP, linear_dim=513)).to(dev).eval()
    small.seq2seq.decoder.min_decoder_steps = small.seq2seq.decoder.max_decoder_steps = 11
    with pytest.raises(ValueError, match="513.*2048.*1025"):
        synthesis.tts_batch(small, ids, audio_cfg=cfg)
    with pytest.raises(ValueError, match="513.*2048.*1025"):
        synthesis.RollingSynthesizer(small, slots=2, max_text_len=16, audio_cfg=cfg)
    with pytest.raises(ValueError, match="1025.*1024.*513"):
        synthesis.tts_batch(model, ids)                                              # and the default config with this one


# ----------------------------------------------------------------------------------------------------------------------
# 6. the preprocessor at 512 / 128 / 16 kHz
# ----------------------------------------------------------------------------------------------------------------------
def test_preprocess_at_512(dev, tmp_path):
    from scipy.io import wavfile
    from deepvoice3_pytorch_amd import audio, data, preprocess
    n, hop, sr = 512, 128, 16000
    in_dir, out_dir = str(tmp_path / "corpus"), str(tmp_path / "out")
    os.makedirs(os.path.join(in_dir, "wavs"))
    rng = np.random.RandomState(4)
    L = int(0.3 * sr)
    pcm, lines = [], []
    for i in range(2):
        x = _speechlike(n, L, 1, rng)[0]
        pcm.append((x * 32767).astype(np.int16))
        wavfile.write(os.path.join(in_dir, "wavs", "U%d.wav" % i), sr, pcm[-1])
        lines.append("U%d|raw|utterance number %d, long enough to keep" % (i, i))
    with open(os.path.join(in_dir, "metadata.csv"), "w", encoding="utf-8") as f:
        f.write("\n".join(lines) + "\n")
    cfg = audio.AudioConfig(fft_size=n, hop_size=hop, sample_rate=sr)
    md = preprocess.build_from_path(in_dir, out_dir, cfg, device=dev)
    T = A.lws_num_frames(L, n, hop)
    assert [m[2] for m in md] == [T, T]
    for i, m in enumerate(md):
        spec, mel = np.load(os.path.join(out_dir, m[0])), np.load(os.path.join(out_dir, m[1]))
        assert spec.shape == (T, 257) and mel.shape == (T, 80) and spec.dtype == mel.dtype == np.float32
        x64 = (pcm[i].astype(np.float32) / np.float32(32768.0)).astype(np.float64)[None]
        wl, wm = _lws_features(x64, n, hop, sr)
        (el, el_big, ela), em = _lin_errs(spec, wl[0], 1), float(np.abs(mel - wm[0]).max())
        print("utterance %d: lin %.2e (bins >= 1e-3 peak %.2e, amplitude %.2e) mel %.2e" % (i, el, el_big, ela, em))
        assert el < 5e-5 and ela < 1e-5 and em < 5e-5, (i, el, ela, em)           # every bin
    with open(os.path.join(out_dir, "audio_config.json")) as f:
        js = json.load(f)
    assert (js["fft_size"], js["hop_size"], js["sample_rate"]) == (512, 128, 16000)
    assert data.read_audio_config(out_dir) == js
    ds = data.PreprocessedDataset(out_dir, lambda t: [2 + ord(c) % 38 for c in t])
    with open(os.path.join(out_dir, "train.txt"), encoding="utf-8") as f:
        rows = [ln.split("|") for ln in f.read().splitlines()]
    assert ds.frame_lengths == [int(r[2]) for r in rows] == [T, T]
    _, mel0, spec0 = ds[0]
    assert spec0.shape == (T, 257) and mel0.shape == (T, 80)
    # a file at another rate is refused by name (no resampling on this path)
    with pytest.raises(ValueError, match="sample rate 16000, expected 22050"):
        preprocess.load_wav(os.path.join(in_dir, "wavs", "U0.wav"), 22050)

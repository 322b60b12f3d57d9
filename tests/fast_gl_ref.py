# coding: utf-8
"""Float64 restatement of the fast Griffin-Lim algorithm (Perraudin, Balazs & Sondergaard 2013) as audio.griffin_lim runs
it with momentum = alpha, on the transforms of oracle/audio_oracle.py:

    y_0 = iSTFT(mag * init)
    for n = 1 .. n_iter:
        c_n = STFT(y_{n-1})
        t_n = c_n                          if n == 1
              c_n + alpha (c_n - c_{n-1})  otherwise
        y_n = iSTFT(mag * t_n / max(|t_n|, 1e-8))

alpha = 0 is oracle.lws_griffin_lim / oracle.griffin_lim, and so is one iteration at any alpha.  The lws framing uses the
oracle's lws_stft / lws_istft, the torch framing its stft / istft at any n_fft (as _torch_gl of
tests/test_gpu_fft_sizes.py does).  tests/test_cpu_fast_gl.py pins this file; tests/test_gpu_fast_gl.py holds the kernels
to it."""
import numpy as np
import torch

from oracle import audio_oracle as A


def fast_griffin_lim(mag, n_iter, hop, n_fft, alpha, init=None, convention="lws", at=None):
    """mag real (B, T, n_fft / 2 + 1), init complex unit phasors of that shape or None (zero phase) -> y (B, L) float64
    numpy: L = (T + 1) * hop - n_fft on the lws framing, hop * (T - 1) on the torch one.
    at (iteration counts <= n_iter): -> {k: y_k} instead, the signal after each of those counts from one run"""
    if not 0.0 <= alpha < 1.0:
        raise ValueError("alpha=%r must lie in [0, 1)" % (alpha,))
    mag = np.asarray(mag, dtype=np.float64)
    assert mag.shape[-1] == n_fft // 2 + 1
    if convention == "lws":
        ph = np.ones(mag.shape, dtype=np.complex128) if init is None else np.asarray(init, dtype=np.complex128)
        y = A.lws_istft(mag * ph, hop)
        prev, kept = None, {0: y}
        for i in range(n_iter):
            c = A.lws_stft(y, n_fft, hop)
            t = c if prev is None else c + alpha * (c - prev)
            prev = c
            y = kept[i + 1] = A.lws_istft(mag * (t / np.maximum(np.abs(t), 1e-8)), hop)
        return y if at is None else {k: kept[k] for k in at}
    m = torch.from_numpy(mag)
    ph = torch.ones(m.shape, dtype=torch.complex128) if init is None else torch.as_tensor(init).to(torch.complex128)
    y = A.istft(m * ph, hop, n_fft)
    prev, kept = None, {0: y}
    for i in range(n_iter):
        c = A.stft(y, hop, n_fft)
        t = c if prev is None else c + alpha * (c - prev)
        prev = c
        y = kept[i + 1] = A.istft(m * (t / torch.clamp(t.abs(), min=1e-8)), hop, n_fft)
    return y.numpy() if at is None else {k: kept[k].numpy() for k in at}


def spectral_convergence(y, mag, hop, n_fft):
    """|| |STFT(y)| - mag ||_F / || mag ||_F over the whole batch, the fp64 lws STFT"""
    Z = np.abs(A.lws_stft(np.asarray(y, dtype=np.float64), n_fft, hop))
    mag = np.asarray(mag, dtype=np.float64)
    return float(np.linalg.norm(Z - mag) / np.linalg.norm(mag))


def speechlike(n_fft, hop, B=2, T=40, seed=3):
    """A voiced, vibrato-carrying, amplitude-modulated harmonic signal with a little noise, its time axis scaled with the
    frame size (sample rate 22050 n_fft / 1024) -> (B, (T + 1) * hop - n_fft) float64: exactly T lws frames.
    Row b: f0 = 110 + 30 b + 40 sin(2 pi 1.5 t + b) Hz, phi its running phase,
           x = 0.1 * [sum_{k=1..19} sin(k phi) / k * (0.5 + 0.5 sin(2 pi 3 t)) + 0.05 randn]"""
    rng = np.random.RandomState(seed)
    L = (T + 1) * hop - n_fft
    sr = 22050.0 * n_fft / 1024
    t = np.arange(L) / sr
    rows = []
    for b in range(B):
        f0 = 110.0 + 30.0 * b + 40.0 * np.sin(2 * np.pi * 1.5 * t + b)
        phi = 2 * np.pi * np.cumsum(f0) / sr
        voiced = sum(np.sin(k * phi) / k for k in range(1, 20)) * (0.5 + 0.5 * np.sin(2 * np.pi * 3 * t))
        rows.append(0.1 * (voiced + 0.05 * rng.randn(L)))
    return np.stack(rows)


def speechlike_magnitudes(n_fft, hop, B=2, T=40, seed=3):
    """|lws STFT| of speechlike(...), rounded through fp32 (what a device holds) -> (B, T, n_fft / 2 + 1) float64"""
    m = np.abs(A.lws_stft(speechlike(n_fft, hop, B, T, seed), n_fft, hop))
    assert m.shape == (B, T, n_fft // 2 + 1)
    return m.astype(np.float32).astype(np.float64)


CONVERGENCE_CASES = ((512, 128), (1024, 256), (2048, 512))
_PLAIN60 = {}


def plain60(n_fft, hop):
    """spectral convergence of 60 plain iterations of the restatement on speechlike_magnitudes from zero phase, computed
    once per process and shared by the tests that compare with it"""
    key = (n_fft, hop)
    if key not in _PLAIN60:
        mag = speechlike_magnitudes(n_fft, hop)
        _PLAIN60[key] = spectral_convergence(fast_griffin_lim(mag, 60, hop, n_fft, 0.0), mag, hop, n_fft)
    return _PLAIN60[key]

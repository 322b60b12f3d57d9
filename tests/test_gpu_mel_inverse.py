# coding: utf-8
"""-m gpu: the mel-to-linear inversion kernel (dv3_mel_to_linear_f32 through audio.mel_to_linear)
against the float64 restatement tests/mel_inverse_ref.py, element by element.

Cases: the six framings of mel_inverse_ref.CASES (three FFT sizes; 13, 20, 80 and 128 bands; bands 142 bins wide with the
last bin covered; bins under no filter at both ends), each with upsample 1, 4 and 3 and 0, 1 and 32 iterations, once
with per-item lengths (9, 1, 2, 0) of T = 9 -- the frames past a length hold NaN, which must not reach the output -- and
once without lengths.  Items 0, 1 and 3 are the mel of fast_gl_ref.speechlike_magnitudes, item 2 is uniform noise in
[-0.3, 1.3] (the kernel clips).

Allowance: for every call the test computes E32 = max |ref(float32) - ref(float64)| over the batch itself -- the error
of the same arithmetic at the kernel's precision -- and the device must stay within 4 E32 of the float64 reference: the factor covers
another summation order and the hardware's log / exp2.  Bins under no filter and rows past a length must be exactly 0.0.
The output buffer is pre-filled with NaN (an unwritten element shows) inside a larger one whose margins must keep their
canary bits.  Bit for bit: each item against its own B = 1 call on the trimmed mel, the batch in reversed order,
upsample = 4 rows 0, 4, ... against the upsample = 1 rows, audio.mel_to_linear against the direct call, and
inv_melspectrogram_batch against the composition it is defined as.
"""
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tests import fast_gl_ref as GL  # noqa: E402
from tests import mel_inverse_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu

B, T = 4, 9
LENGTHS = (9, 1, 2, 0)
CANARY, MARGIN = 0x5ca1ab1e, 4096
FACTOR = 4.0


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


def _cfg(case, **kw):
    from deepvoice3_pytorch_amd import audio
    n_fft, sr = case[0], case[1]
    return audio.AudioConfig(fft_size=n_fft, hop_size=n_fft // 4, sample_rate=sr, **kw)


_INPUTS = {}


def _inputs(case):
    """(W float32 (M, F), x float32 (B, T, M)) of a case, made once"""
    from deepvoice3_pytorch_amd import audio
    if case not in _INPUTS:
        n_fft, sr, M, fmin, fmax = case
        W = audio.mel_basis(sr, n_fft, M, fmin, fmax)
        mag = GL.speechlike_magnitudes(n_fft, n_fft // 4)                   # (2, 40, F)
        mel = R.mel_of(mag.reshape(-1, mag.shape[-1]), W).astype(np.float32)   # 80 frames
        x = np.stack([mel[3:3 + T], mel[30:30 + T], mel[0:T], mel[50:50 + T]])
        x[2] = np.random.RandomState(7).uniform(-0.3, 1.3, (T, M)).astype(np.float32)
        _INPUTS[case] = (W, x)
    return _INPUTS[case]


def _direct(dev, case, x, lengths, u, iters):
    """the entry point itself on a case's tables"""
    from deepvoice3_pytorch_amd import audio
    n_fft, sr, M, fmin, fmax = case
    return _launch(dev, audio.mel_inverse_tables(dev, sr, M, fmin, fmax, n_fft), x, lengths, u, iters)


def _launch(dev, tables, x, lengths, u, iters):
    """the entry point into a NaN-filled buffer between two canary margins -> (B, T u, F) (a view of it)"""
    from deepvoice3_pytorch_amd import _lib
    from deepvoice3_pytorch_amd.ops import _stream
    basis, band, bins, inv_sum = tables
    M, F = basis.shape
    nb = x.shape[0]
    n = nb * x.shape[1] * u * F
    buf = torch.full((n + 2 * MARGIN,), float("nan"), dtype=torch.float32, device=dev)
    bits = buf.view(torch.int32)
    bits[:MARGIN] = CANARY
    bits[MARGIN + n:] = CANARY
    tlen = None if lengths is None else torch.tensor(lengths, dtype=torch.int32).to(dev)
    out = buf[MARGIN:MARGIN + n]
    _lib.call("dv3_mel_to_linear_f32", x.data_ptr(), tlen.data_ptr() if tlen is not None else None, basis.data_ptr(),
              band.data_ptr(), bins.data_ptr(), inv_sum, out.data_ptr(), nb, x.shape[1], M, F, u, iters, -100.0, 20.0,
              _stream())
    torch.cuda.synchronize()
    assert bool((bits[:MARGIN] == CANARY).all()) and bool((bits[MARGIN + n:] == CANARY).all()), "a margin was written"
    return out.view(nb, x.shape[1] * u, F)


def _bits(t):
    return t.contiguous().view(torch.int32)


@pytest.mark.parametrize("case", R.CASES, ids=lambda c: "%d-%d-%d" % (c[0], c[1], c[2]))
def test_kernel_matches_the_float64_restatement(dev, case):
    from deepvoice3_pytorch_amd import audio
    n_fft, sr, M, fmin, fmax = case
    W, x = _inputs(case)
    uncovered = W.sum(axis=0) == 0
    cfg = _cfg(case)
    worst = 0.0
    for lengths in (LENGTHS, None):
        xin = x.copy()
        lens = lengths if lengths is not None else (T,) * B
        for b, n in enumerate(lens):
            xin[b, n:] = np.nan                 # the padding is never read
        xd = torch.from_numpy(xin).to(dev)
        base = {}
        for u in (1, 4, 3):
            for iters in (0, 1, 32):
                opt = audio.MelInverse(iters=iters, fmin=fmin, fmax=fmax)
                got_d = _direct(dev, case, xd, lengths, u, iters)
                via = audio.mel_to_linear(xd, cfg, lengths, u, opt)
                assert torch.equal(_bits(via), _bits(got_d)), "audio.mel_to_linear differs from the entry point"
                got = got_d.cpu().numpy()
                assert np.isfinite(got).all(), "an element was not written (or is not finite)"
                refs = {b: (R.mel_to_linear(x[b, :n], W, u, iters), R.mel_to_linear(x[b, :n], W, u, iters, dtype=np.float32))
                        for b, n in enumerate(lens) if n > 0}
                e32 = max(float(np.abs(r32.astype(np.float64) - r64).max()) for r64, r32 in refs.values())
                for b, n in enumerate(lens):
                    assert (got[b, n * u:] == 0.0).all(), "rows past the length are not zero"
                    if n == 0:
                        continue
                    err = float(np.abs(got[b, :n * u].astype(np.float64) - refs[b][0]).max())
                    worst = max(worst, err / e32)
                    print("%s lengths=%s u=%d iters=%d item %d: E32 %.3g err %.3g ratio %.2f"
                          % (case, lengths is not None, u, iters, b, e32, err, err / e32))
                    assert err <= FACTOR * e32, (case, lengths, u, iters, b, err, e32)
                    assert (got[b, :n * u][:, uncovered] == 0.0).all(), "a bin under no filter is not 0.0"
                    # the item alone, on its trimmed mel
                    alone = audio.mel_to_linear(xd[b:b + 1, :n].contiguous(), cfg, None, u, opt)
                    assert torch.equal(_bits(alone[0]), _bits(got_d[b, :n * u])), "item %d differs from its B = 1 call" % b
                # the same batch in reversed order
                rev = audio.mel_to_linear(xd.flip(0).contiguous(), cfg, None if lengths is None else lengths[::-1], u, opt)
                assert torch.equal(_bits(rev.flip(0)), _bits(got_d)), "the order of the items changes their rows"
                if u == 1:
                    base[iters] = got_d.clone()
                elif u == 4:
                    assert torch.equal(_bits(got_d[:, ::4]), _bits(base[iters])), "upsample = 4 rows 0, 4, ... differ"
    print("%s worst ratio %.2f" % (case, worst))


@pytest.mark.parametrize("F,M", [(257, 26), (1025, 122)], ids=["staged", "from-global-memory"])
def test_a_basis_with_six_filters_over_a_bin(dev, F, M):
    """The kernel assumes no number of filters per bin: Hann-shaped filters 48 bins wide every 8 bins put six filters
    over a bin.  At 257 bins their 1248 nonzeros are staged in LDS; at 1025 bins the 5856 do not fit and the basis is
    read from global memory -- the other path of the kernel.  Same allowance as the six framings: the chains (48 terms)
    are shorter than the longest there (142) and E32 is the restatement's own error on this basis."""
    from deepvoice3_pytorch_amd import audio
    k = np.arange(F)[None, :] - (8 * np.arange(M)[:, None] + 3)             # bins 0 .. 3 and the last five: no filter
    W = np.where((k > 0) & (k < 49), 0.5 - 0.5 * np.cos(2 * np.pi * k / 49.0), 0.0).astype(np.float32) / 24.0
    band = audio.filter_bands_np(W)
    bins = audio.bin_bands_np(band, F)
    assert (band[:, 1] - band[:, 0] == 48).all() and int((bins[:, 1] - bins[:, 0]).max()) == 6
    assert (int(np.count_nonzero(W)) > 3072) == (F == 1025)
    uncovered = W.sum(axis=0) == 0
    assert uncovered[:4].all() and uncovered[-5:].all() and not uncovered[4:-5].any()
    tables = (torch.from_numpy(W).to(dev), torch.from_numpy(band).to(dev), torch.from_numpy(bins).to(dev),
              1.0 / float(W.astype(np.float64).sum()))
    rng = np.random.RandomState(11)
    x = np.clip(0.5 + 0.2 * np.sin(np.linspace(0, 9, M))[None, None, :] + 0.1 * rng.randn(3, 5, M), 0, 1).astype(np.float32)
    lengths = (5, 2, 0)
    xd = torch.from_numpy(x).to(dev)
    for u, iters in ((1, 0), (3, 1), (2, 32)):
        got_d = _launch(dev, tables, xd, lengths, u, iters)
        got = got_d.cpu().numpy()
        assert np.isfinite(got).all()
        refs = {b: (R.mel_to_linear(x[b, :n], W, u, iters), R.mel_to_linear(x[b, :n], W, u, iters, dtype=np.float32))
                for b, n in enumerate(lengths) if n > 0}
        e32 = max(float(np.abs(r32.astype(np.float64) - r64).max()) for r64, r32 in refs.values())
        for b, n in enumerate(lengths):
            assert (got[b, n * u:] == 0.0).all()
            if n == 0:
                continue
            err = float(np.abs(got[b, :n * u].astype(np.float64) - refs[b][0]).max())
            print("F=%d u=%d iters=%d item %d: E32 %.3g err %.3g ratio %.2f" % (F, u, iters, b, e32, err, err / e32))
            assert err <= FACTOR * e32, (F, u, iters, b, err, e32)
            assert (got[b, :n * u][:, uncovered] == 0.0).all()
            alone = _launch(dev, tables, xd[b:b + 1, :n].contiguous(), None, u, iters)
            assert torch.equal(_bits(alone[0]), _bits(got_d[b, :n * u]))


def test_upsampled_tail_holds_the_last_frame(dev):
    """the last upsample - 1 rows of an item equal its row -upsample: its own last frame, never the neighbour's"""
    from deepvoice3_pytorch_amd import audio
    case = R.CASES[0]
    _, x = _inputs(case)
    xd = torch.from_numpy(x).to(dev)
    out = audio.mel_to_linear(xd, _cfg(case), (9, 4, 2, 1), 4)
    for b, n in enumerate((9, 4, 2, 1)):
        for j in (1, 2, 3):
            assert torch.equal(_bits(out[b, 4 * n - 4 + j]), _bits(out[b, 4 * n - 4]))


def test_wrapper_refuses_what_the_kernel_would(dev):
    from deepvoice3_pytorch_amd import audio
    x = torch.rand(2, 5, 80, device=dev)
    for kw in (dict(upsample=0), dict(upsample=17), dict(upsample=True), dict(frame_lengths=(5,)),
               dict(frame_lengths=(6, 1)), dict(frame_lengths=(-1, 1)), dict(options=32)):
        with pytest.raises(ValueError):
            audio.mel_to_linear(x, None, **kw)
    with pytest.raises(ValueError):
        audio.mel_to_linear(torch.rand(2, 5, 257, device=dev))
    with pytest.raises(ValueError):
        audio.mel_to_linear(torch.rand(5, 80, device=dev))


@pytest.mark.parametrize("lengths", (None, (9, 5, 7, 4)))
def test_inv_melspectrogram_batch_is_the_composition(dev, lengths):
    from deepvoice3_pytorch_amd import audio
    case = R.CASES[0]
    _, x = _inputs(case)
    xd = torch.from_numpy(x).to(dev)
    cfg = _cfg(case, griffin_lim_iters=3)
    opt = audio.MelInverse(iters=8)
    got = audio.inv_melspectrogram_batch(xd, cfg, lengths, 4, opt)
    lin = audio.mel_to_linear(xd, cfg, lengths, 4, opt)
    if lengths is None:
        want = audio.inv_spectrogram_batch(lin, cfg, None)
        assert got.shape == (B, (4 * T + 1) * 256 - 1024) and torch.equal(_bits(got), _bits(want))
        # the numpy sibling: (num_mels, T) in, the waveform of inv_spectrogram on the item's own inversion out
        one = audio.inv_melspectrogram(x[0].T, cfg, device=dev, options=opt)
        lin1 = audio.mel_to_linear(xd[:1], cfg, None, 1, opt)
        assert one.shape == (T * 256 + 256 - 1024,)
        assert np.array_equal(one, audio.inv_spectrogram(lin1[0].cpu().numpy().T, cfg, device=dev))
    else:
        want, wlen = audio.inv_spectrogram_batch(lin, cfg, None, torch.tensor(lengths) * 4)
        assert torch.equal(_bits(got[0]), _bits(want)) and torch.equal(got[1], wlen)
        assert got[1].tolist() == [(4 * n + 1) * 256 - 1024 for n in lengths]

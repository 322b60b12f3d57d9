# coding: utf-8
"""No GPU: the mel-to-linear estimator's restatement (tests/mel_inverse_ref.py), the header's declaration of
dv3_mel_to_linear_f32, the library's refusals (loaded here with no device: every limit is checked before any launch),
and the defaults of the Python layer (audio.MelInverse, the `from_mel` / `postnet` keywords, the bin_band table).

The round-trip figures: ROUND_TRIP below are the means of |norm(W s) - x| this restatement gives on
fast_gl_ref.speechlike_magnitudes(n_fft, n_fft / 4) x 30 (two items of 40 frames, 80 bands, 125 .. 7600 Hz), and the
test holds the file to them within 10 %.  The table of the issue that asked for this (1.1e-2, 3.4e-4, 8.6e-5 and 2.3e-5
after 1, 16, 32 and 64 updates at 1024; 6.4e-5 at 512 and 8.8e-5 at 2048 after 32) could not be reproduced from its
description of the inputs: the figures depend on the level of the input (x 150 gives 1.1e-2, 3.6e-4, 9.8e-5, 2.3e-5), and
no level met all of them within 10 %.  They decay with the iterations at the same rate.
"""
import ctypes
import inspect
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tests import fast_gl_ref as GL  # noqa: E402
from tests import mel_inverse_ref as R  # noqa: E402

# (n_fft, sample_rate, iterations) -> the mean round-trip error of the restatement (float64)
ROUND_TRIP = {(1024, 22050, 1): 1.346e-2, (1024, 22050, 16): 7.076e-4, (1024, 22050, 32): 2.098e-4,
              (1024, 22050, 64): 4.911e-5, (512, 16000, 32): 1.224e-4, (2048, 44100, 32): 1.798e-4}

_MAG = {}


def _speech(n_fft):
    if n_fft not in _MAG:
        m = GL.speechlike_magnitudes(n_fft, n_fft // 4) * 30.0
        _MAG[n_fft] = m.reshape(-1, m.shape[-1])
    return _MAG[n_fft]


def _basis(case):
    from deepvoice3_pytorch_amd import audio
    n_fft, sr, M, fmin, fmax = case
    return audio.mel_basis(sr, n_fft, M, fmin, fmax)


def _mel(case, frames=12, seed=0):
    """(frames, M) float64 in [0, 1]: speech-like mel frames of the case's framing"""
    W = _basis(case)
    rows = np.random.RandomState(seed).choice(_speech(case[0]).shape[0], frames, replace=False)
    return R.mel_of(_speech(case[0])[rows], W), W.astype(np.float64)


# ---------------------------------------------------------------------------------------------------------------------
# the restatement
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", R.CASES, ids=lambda c: "%d-%d" % (c[0], c[2]))
def test_objective_never_rises_and_uncovered_bins_stay_zero(case):
    x, W = _mel(case)
    a = R.amplitudes(x)
    b, s = R.start(a, W)
    uncovered = W.sum(axis=0) == 0
    assert uncovered.any() or case[3] == 0.0
    last = R.objective(s, a, W)
    for _ in range(64):
        s = R.update(s, b, W)
        now = R.objective(s, a, W)
        assert (now <= last * (1 + 1e-12)).all()
        last = now
        assert (s[:, uncovered] == 0.0).all() and (s[:, ~uncovered] > 0.0).all()
    assert (R.mel_to_linear(x, W, 1, 64)[:, uncovered] == 0.0).all()


def test_zero_iterations_return_the_normalised_start():
    x, W = _mel(R.CASES[0])
    _, s = R.start(R.amplitudes(x), W)
    assert np.array_equal(R.mel_to_linear(x, W, 1, 0), R.normalise(s))
    # the start is flat over the covered bins: sum a / sum W
    covered = W.sum(axis=0) > 0
    assert np.allclose(s[:, covered], (R.amplitudes(x).sum(axis=1) / W.sum())[:, None], rtol=1e-15, atol=0)


def test_upsampling_keeps_the_mel_frames_and_holds_the_last_one():
    x, W = _mel(R.CASES[0], frames=5)
    y1, y4 = R.mel_to_linear(x, W, 1, 8), R.mel_to_linear(x, W, 4, 8)
    assert y4.shape == (20, W.shape[1])
    # the frames that go in are the same bits; what comes out is compared at 1e-12, because numpy's matrix product may
    # sum a row differently in a product of 20 rows than in one of 5 (the kernel's rows ARE equal bit for bit: GPU test)
    xi = R.interpolate(x, 4)
    assert np.array_equal(xi[0::4], x) and all(np.array_equal(xi[j], xi[-4]) for j in (-1, -2, -3))
    assert np.allclose(y4[0::4], y1, rtol=0, atol=1e-12)
    for j in (-1, -2, -3):
        assert np.allclose(y4[j], y4[-4], rtol=0, atol=1e-12)
    # in between: interpolation in the normalised domain, at quarters
    assert np.allclose(xi[1], 0.75 * x[0] + 0.25 * x[1]) and np.allclose(xi[6], 0.5 * x[1] + 0.5 * x[2])


def test_inputs_outside_the_unit_interval_behave_as_clipped():
    _, W = _mel(R.CASES[0])
    x = np.random.RandomState(1).uniform(-0.5, 1.5, (6, W.shape[0]))
    assert (x < 0).any() and (x > 1).any()
    for u in (1, 3):
        assert np.array_equal(R.mel_to_linear(x, W, u, 4), R.mel_to_linear(np.clip(x, 0, 1), W, u, 4))


def test_a_one_frame_item_and_an_empty_one():
    x, W = _mel(R.CASES[0], frames=1)
    y = R.mel_to_linear(x, W, 4, 4)
    assert y.shape == (4, W.shape[1]) and all(np.allclose(y[j], y[0], rtol=0, atol=1e-12) for j in (1, 2, 3))
    assert np.array_equal(R.interpolate(x, 4), np.repeat(x, 4, axis=0))
    assert np.allclose(y[0], R.mel_to_linear(x, W, 1, 4)[0], rtol=0, atol=1e-12)
    assert R.mel_to_linear(x[:0], W, 4, 4).shape == (0, W.shape[1])


@pytest.mark.parametrize("key", sorted(ROUND_TRIP), ids=lambda k: "%d-%d" % (k[0], k[2]))
def test_round_trip_means(key):
    from deepvoice3_pytorch_amd import audio
    n_fft, sr, iters = key
    W = audio.mel_basis(sr, n_fft, 80, 125.0, 7600.0)
    got = float(R.round_trip(_speech(n_fft), W, iters).mean())
    print("round trip %s: %.4g (recorded %.4g)" % (key, got, ROUND_TRIP[key]))
    assert abs(got - ROUND_TRIP[key]) <= 0.1 * ROUND_TRIP[key]


def test_float32_stays_close_to_float64():
    """the allowance of the GPU test rests on this distance: a few 1e-6 of the normalised range after 32 updates"""
    x, W = _mel(R.CASES[0], frames=40)
    e = np.abs(R.mel_to_linear(x, W, 1, 32, dtype=np.float32).astype(np.float64) - R.mel_to_linear(x, W, 1, 32)).max()
    assert 0 < e < 2e-5, e


@pytest.mark.parametrize("case", R.CASES, ids=lambda c: "%d-%d" % (c[0], c[2]))
def test_at_most_two_filters_over_a_bin(case):
    """what makes the frame fit one wave's LDS -- a fact about THIS filterbank, not something the kernel assumes"""
    W = _basis(case)
    assert int((W > 0).sum(axis=0).max()) <= 2
    bb = R.bin_band(W)
    assert int((bb[:, 1] - bb[:, 0]).max()) <= 2


# ---------------------------------------------------------------------------------------------------------------------
# the header and the library
# ---------------------------------------------------------------------------------------------------------------------
def test_header_declares_the_entry_point():
    from deepvoice3_pytorch_amd import _lib
    assert _lib.CONSTS["DV3_ABI_VERSION"] == 50
    assert _lib.CONSTS["DV3_MELINV_MAX_MELS"] == 256 and _lib.CONSTS["DV3_MELINV_MAX_ITERS"] == 1024
    i32, f32, ptr = ctypes.c_int32, ctypes.c_float, ctypes.c_void_p
    assert _lib.FUNCS["dv3_mel_to_linear_f32"] == (
        ctypes.c_int, [ptr, ptr, ptr, ptr, ptr, f32, ptr, i32, i32, i32, i32, i32, i32, f32, f32, ptr])
    assert sum(1 for f in _lib.FUNCS if f.endswith("_n")) == 12
    mk = open(os.path.join(ROOT, "deepvoice3_pytorch_amd", "csrc", "Makefile")).read()
    assert "mel_inverse.hip" in mk
    text = open(os.path.join(ROOT, "include", "dv3hip.h")).read()
    doc = text[text.index("Mel-to-linear inversion"):text.index("int dv3_mel_to_linear_f32")]
    assert "version stays 49" in " ".join(doc.split()).replace("* ", "")
    assert R.FLOOR == 1e-30 and "1e-30" in doc


def _call(lib, **kw):
    """the entry point with valid scalars and dummy non-null pointers, `kw` replacing some: every refusal comes before
    any launch, so nothing is dereferenced"""
    a = dict(mel=8, tlen=None, basis=8, mel_band=8, bin_band=8, inv_basis_sum=0.25, lin=8, B=2, T=3, n_mels=80, n_bins=513,
             upsample=4, iters=32, min_level_db=-100.0, ref_level_db=20.0)
    assert set(kw) <= set(a)
    a.update(kw)
    return lib.dv3_mel_to_linear_f32(a["mel"], a["tlen"], a["basis"], a["mel_band"], a["bin_band"], a["inv_basis_sum"],
                                     a["lin"], a["B"], a["T"], a["n_mels"], a["n_bins"], a["upsample"], a["iters"],
                                     a["min_level_db"], a["ref_level_db"], None)


@pytest.mark.parametrize("kw,names", [
    (dict(mel=None), b"mel is null"), (dict(basis=None), b"basis is null"), (dict(mel_band=None), b"mel_band is null"),
    (dict(bin_band=None), b"bin_band is null"), (dict(lin=None), b"lin is null"),
    (dict(B=0), b"B = 0"), (dict(T=0), b"T = 0"), (dict(B=65536, T=4096, upsample=8), b"2^31"),
    (dict(n_mels=0), b"n_mels = 0"), (dict(n_mels=257), b"n_mels = 257"),
    (dict(n_bins=0), b"n_bins = 0"), (dict(n_bins=1026), b"n_bins = 1026"),
    (dict(upsample=0), b"upsample = 0"), (dict(upsample=17), b"upsample = 17"),
    (dict(iters=-1), b"iters = -1"), (dict(iters=1025), b"iters = 1025"),
    (dict(min_level_db=0.0), b"min_level_db"), (dict(inv_basis_sum=0.0), b"inv_basis_sum"),
    (dict(inv_basis_sum=float("nan")), b"inv_basis_sum"), (dict(inv_basis_sum=float("inf")), b"inv_basis_sum"),
], ids=lambda v: "-".join("%s" % k for k in v) if isinstance(v, dict) else None)
def test_library_refuses_every_limit_violation_without_a_gpu(kw, names):
    from deepvoice3_pytorch_amd import _lib
    lib = _lib.lib()
    assert _call(lib, **kw) == _lib.CONSTS["DV3_EINVAL"]
    msg = lib.dv3_last_error()
    assert msg.startswith(b"mel_to_linear:") and names in msg, msg


# ---------------------------------------------------------------------------------------------------------------------
# the Python layer
# ---------------------------------------------------------------------------------------------------------------------
def test_defaults_leave_everything_as_it_was():
    import deepvoice3_pytorch_amd as pkg
    from deepvoice3_pytorch_amd import audio, synthesis
    for fn in (synthesis.tts_batch, synthesis.RollingSynthesizer.__init__, synthesis.tts_stream):
        params = list(inspect.signature(fn).parameters.values())
        assert params[-1].name == "from_mel" and params[-1].default is False, fn
    params = list(inspect.signature(pkg.MultiSpeakerTTSModel.synthesize_batch).parameters.values())
    assert params[-1].name == "postnet" and params[-1].default is True and params[-2].name == "stall_limit"
    assert list(inspect.signature(audio.griffin_lim).parameters)[-1] == "momentum"
    assert list(inspect.signature(audio.mel_to_linear).parameters) == ["mel", "cfg", "frame_lengths", "upsample", "options"]
    assert list(inspect.signature(audio.inv_melspectrogram_batch).parameters) == [
        "mel", "cfg", "frame_lengths", "upsample", "options", "init_phasor"]
    assert list(inspect.signature(audio.inv_melspectrogram).parameters) == ["mel", "cfg", "device", "options"]
    assert synthesis.mel_options(False) is None and synthesis.mel_options(None) is None
    opt = synthesis.mel_options(True)
    assert isinstance(opt, audio.MelInverse) and (opt.iters, opt.fmin, opt.fmax) == (32, 125.0, 7600.0)
    mine = audio.MelInverse(iters=8)
    assert synthesis.mel_options(mine) is mine
    for bad in (1, "yes", 32.0):
        with pytest.raises(ValueError):
            synthesis.mel_options(bad)


def test_mel_inverse_options_refuse_by_value():
    from deepvoice3_pytorch_amd import audio
    o = audio.MelInverse()
    assert (o.iters, o.fmin, o.fmax) == (32, 125.0, 7600.0)
    assert audio.MelInverse(iters=0).iters == 0 and audio.MelInverse(iters=np.int64(1024)).iters == 1024
    assert audio.MelInverse(fmin=0, fmax=8000).fmin == 0.0
    for bad in (-1, 1025, 32.0, True, "32", None, float("nan")):
        with pytest.raises(ValueError, match="iters"):
            audio.MelInverse(iters=bad)
    for fmin, fmax in ((-1.0, 7600.0), (7600.0, 7600.0), (8000.0, 125.0), (float("nan"), 7600.0), (125.0, float("nan")),
                       (125.0, float("inf")), ("125", 7600.0), (125.0, None), (True, 7600.0)):
        with pytest.raises(ValueError, match="fmin"):
            audio.MelInverse(fmin=fmin, fmax=fmax)


@pytest.mark.parametrize("case", R.CASES, ids=lambda c: "%d-%d" % (c[0], c[2]))
def test_bin_band_table_equals_brute_force(case):
    from deepvoice3_pytorch_amd import audio
    W = _basis(case)
    band = audio.filter_bands_np(W)
    got = audio.bin_bands_np(band, W.shape[1])
    assert got.dtype == np.int32 and np.array_equal(got, R.bin_band(W))
    # the table the device gets is this one, beside mel_tables' two, and cached with them
    n_fft, sr, M, fmin, fmax = case
    basis, fb, bb, inv_sum = audio.mel_inverse_tables("cpu", sr, M, fmin, fmax, n_fft)
    assert np.array_equal(bb.numpy(), got) and np.array_equal(fb.numpy(), band) and np.array_equal(basis.numpy(), W)
    assert inv_sum == 1.0 / float(W.astype(np.float64).sum())
    assert audio.mel_inverse_tables("cpu", sr, M, fmin, fmax, n_fft)[2] is bb
    assert audio.mel_tables("cpu", sr, M, fmin, fmax, n_fft)[0] is basis


def test_bin_band_refuses_a_gap():
    from deepvoice3_pytorch_amd import audio
    with pytest.raises(ValueError, match="contiguous"):
        audio.bin_bands_np(np.array([[0, 4], [5, 6], [2, 4]]), 8)      # over bin 2: filters 0 and 2, not 1
    assert audio.bin_bands_np(np.array([[0, 0], [1, 3]]), 4).tolist() == [[0, 0], [1, 2], [1, 2], [0, 0]]


def test_mel_to_linear_refuses_the_cpu():
    import torch
    from deepvoice3_pytorch_amd import audio
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        audio.mel_to_linear(torch.rand(1, 3, 80))

# coding: utf-8
"""Speaking rate and pitch at vocoding without a GPU: tests/prosody_ref.py -- the float64 restatement
of dv3_prosody_warp_f32 -- pinned to known answers, the property that makes the envelope-preserving warp what it is,
the pitch actually moving by the requested interval through Griffin-Lim and YIN in float64, the options' refusals and
the C header's entry point."""
import inspect
import os
import re
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tests import prosody_ref as P  # noqa: E402


def _f32(x):
    return np.asarray(x, dtype=np.float32).astype(np.float64)


def _mags(B, T, bins, seed=0):
    rng = np.random.RandomState(seed)
    return _f32(10.0 ** rng.uniform(-5.6, 1.4, (B, T, bins)))


# ----------------------------------------------------------------------------------------------------------------------
# reference pins
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("preserve", [0, 1])
def test_identity_at_rate_1_ratio_1(preserve):
    mag = _mags(2, 9, 257)
    out = P.warp(mag, [9, 6], [9, 6], [1.0, 1.0], [1.0, 1.0], 19, preserve, 9)
    assert np.array_equal(out[0], mag[0]) and np.array_equal(out[1, :6], mag[1, :6])
    assert not out[1, 6:].any()


def test_frame_count_formula():
    """T' = max(tmin, floor((T - 1) / rate + 0.5) + 1): the first and last source frames keep their places (frame T' - 1
    reads at or past T - 1), a rate below 1 lengthens, above 1 shortens, and the clamp holds the inverse's shortest
    signal (4 frames at 1024 / 256 on the lws framing)."""
    from deepvoice3_pytorch_amd import audio
    cfg = audio.AudioConfig()
    tmin = audio.min_frames(256, "lws", 1024)
    assert tmin == 4
    assert P.out_frames(24, 1.0, tmin) == 24
    assert P.out_frames(24, 0.8, tmin) == 30 and P.out_frames(24, 1.25, tmin) == 19      # 23 / 0.8 = 28.75, 23 / 1.25 = 18.4
    assert P.out_frames(12, 0.3, tmin) == 38 and P.out_frames(7, 4.0, tmin) == tmin       # 1.5 + 0.5 -> 3 < 4: clamped
    assert P.out_frames(11, 4.0, tmin) == tmin and P.out_frames(15, 4.0, tmin) == 5       # 10 / 4 = 2.5 -> 3 + 1 = 4; 4 + 1
    for T in (4, 7, 12, 24, 101):
        for rate in (0.25, 0.3, 0.8, 1.0, 1.25, 3.0, 4.0):
            assert audio.warped_frames(T, rate, cfg) == P.out_frames(T, rate, tmin)


def test_the_last_source_frame_is_held():
    """rate 1.25 on 7 frames: T' = max(4, floor(4.8 + 0.5) + 1) = 6; frame 5 asks for u = 6.25 > 6 and gets frame 6
    itself; with T' forced beyond the formula the held frame repeats; nothing of the NaN padding gets through"""
    mag = _mags(1, 9, 33, seed=1)
    mag[0, 7:] = np.nan
    Tp = P.out_frames(7, 1.25, 4)
    assert Tp == 6
    out = P.warp(mag, [7], [8], [1.25], [1.0], 3, 1, 10)
    assert np.isfinite(out).all()
    assert np.array_equal(out[0, 5], mag[0, 6]) and np.array_equal(out[0, 7], mag[0, 6])
    i0, a, i1 = P.time_split(np.arange(6), 1.25, 7)
    assert i0.tolist() == [0, 1, 2, 3, 5, 6] and i1.tolist() == [1, 2, 3, 4, 6, 6]
    assert a.tolist() == [0.0, 0.25, 0.5, 0.75, 0.0, 0.0]
    assert np.array_equal(out[0, 1], 0.75 * mag[0, 1] + 0.25 * mag[0, 2])
    assert not out[0, 8:].any()                                                # rows past tlen_out are zero


def test_rows_past_the_output_length_are_zero():
    mag = _mags(2, 12, 65, seed=2)
    out = P.warp(mag, [12, 5], [15, 6], [0.8, 0.8], [2 ** (4 / 12.0)] * 2, 5, 1, 17)
    assert out[0, :15].all() and not out[0, 15:].any() and out[1, :6].all() and not out[1, 6:].any()


def test_plain_warp_moves_a_peak_by_the_ratio():
    bins = 513
    row = np.full(bins, 1e-3)
    row[100] = 1.0
    for ratio in (2 ** (4 / 12.0), 2 ** (-3 / 12.0), 2.0, 0.5):
        out = P.warp(row[None, None], None, [1], [1.0], [ratio], 19, 0, 1)[0, 0]
        assert abs(int(np.argmax(out)) - 100 * ratio) <= 1.0, ratio
    up = P.warp(row[None, None], None, [1], [1.0], [0.25], 19, 0, 1)[0, 0]
    assert np.array_equal(up[129:], np.full(bins - 129, row[-1]))             # k / ratio > bins - 1: the last bin's value


# ----------------------------------------------------------------------------------------------------------------------
# the affine property
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("W", [1, 19, 64])
@pytest.mark.parametrize("semitones", [4.0, -3.0, 12.0, -24.0, 24.0])
def test_an_affine_log_spectrum_is_its_own_envelope(W, semitones):
    """log m affine in the bin index: the triangular average reproduces it wherever its window is whole, so X = 0 there
    and the envelope-preserving warp returns the frame on every bin k with k, floor(k / ratio) and floor(k / ratio) + 1
    all in [W, bins - 1 - W]; the plain warp does not."""
    bins, ratio = 513, 2.0 ** (semitones / 12.0)
    k = np.arange(bins, dtype=np.float64)
    row = np.exp(-9.0 + 0.02 * k)
    out = P.warp(row[None, None], None, [1], [1.0], [ratio], W, 1, 1)[0, 0]
    s0 = np.floor(k / ratio)
    ok = (k >= W) & (k <= bins - 1 - W) & (s0 >= W) & (s0 + 1 <= bins - 1 - W)
    assert ok.sum() > 20, (W, semitones)
    assert np.allclose(out[ok], row[ok], rtol=1e-12, atol=0.0)
    plain = P.warp(row[None, None], None, [1], [1.0], [ratio], W, 0, 1)[0, 0]
    assert np.abs(plain[ok] / row[ok] - 1.0).max() > 0.1


@pytest.mark.parametrize("bins,W", [(33, 1), (65, 19), (129, 64), (40, 64)])
def test_the_envelope_is_the_truncated_renormalised_triangle(bins, W):
    """the matrix form the restatement evaluates against the bin-by-bin form of the header; a constant row is its own
    envelope up to the last bin (the renormalisation), tap counts 2 W + 1 inside and W + 1 at the two ends"""
    l = np.random.RandomState(bins).randn(bins) * 5.0
    E, absE, taps = P.envelope(l, W)
    assert np.allclose(E, P.envelope_literal(l, W), rtol=0, atol=1e-12)
    assert np.allclose(P.envelope(np.full(bins, -7.25), W)[0], -7.25, rtol=1e-14)
    assert taps[0] == min(W + 1, bins) and taps[bins // 2] == min(2 * W + 1, bins, bins // 2 + W + 1)
    assert (absE >= np.abs(E) - 1e-12).all()


def test_the_f32_restatement_of_the_plain_modes_stays_on_the_float64_one():
    """warp_f32_plain (what the kernel must give bit for bit) against the float64 restatement under the stated bound"""
    mag = _mags(3, 12, 257, seed=4)
    tin, rate, ratio = [12, 7, 4], [1.0, 0.8, 1.25], [1.0, 2 ** (4 / 12.0), 2 ** (-3 / 12.0)]
    tout = [P.out_frames(n, r, 4) for n, r in zip(tin, rate)]
    want, det = P.warp(mag, tin, tout, rate, ratio, 19, 0, max(tout), details=True)
    got = P.warp_f32_plain(mag, tin, tout, rate, ratio, max(tout)).astype(np.float64)
    lim = P.bound(det, want.shape)
    assert np.array_equal(got[0], want[0])                                     # the untouched item: a copy
    assert (np.abs(got - want) <= lim).all() and np.abs(got - want).max() > 0.0


# ----------------------------------------------------------------------------------------------------------------------
# pitch closure in float64: |lws_stft| -> warp -> fast Griffin-Lim -> YIN
# ----------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def tone_magnitudes():
    from oracle import audio_oracle as A
    mag = np.abs(A.lws_stft(P.harmonic_tones(), P.N_FFT, P.HOP))
    assert mag.shape == (len(P.TONE_F0), P.T_TONES, P.N_FFT // 2 + 1)
    return _f32(mag)


@pytest.mark.parametrize("preserve", [1, 0])
@pytest.mark.parametrize("semitones,rate", P.CLOSURE_SETTINGS)
def test_pitch_closure_in_float64(tone_magnitudes, semitones, rate, preserve):
    """Two steady tones (140 and 205 Hz) under a formant-like amplitude curve: after the warp, 30 fast Griffin-Lim
    iterations and YIN, the median F0 over frames 5 .. T' - 5 lies within 25 cents of f0 x ratio.  The margin is a
    condition on the method (a stage that fails to shift misses by 300 cents or more), not a measurement."""
    from tests import fast_gl_ref as R
    from tests import pitch_ref as Y
    from deepvoice3_pytorch_amd import audio
    B, T = len(P.TONE_F0), P.T_TONES
    ratio = 2.0 ** (semitones / 12.0)
    Tp = P.out_frames(T, rate, audio.min_frames(P.HOP, "lws", P.N_FFT))
    W = audio.Prosody().half_width(audio.AudioConfig())
    assert W == 19
    out = P.warp(tone_magnitudes, None, [Tp] * B, [rate] * B, [ratio] * B, W, preserve, Tp)
    y = R.fast_griffin_lim(out, 30, P.HOP, P.N_FFT, 0.99)
    assert y.shape == (B, (Tp + 1) * P.HOP - P.N_FFT)
    res = Y.yin_frames(y.reshape(-1), [y.shape[1]] * B, P.HOP, P.N_FFT, P.YIN_LAGS[0], P.YIN_LAGS[1], P.YIN_THRESHOLD,
                       float(P.SR))
    assert res["frames"].tolist() == [Tp] * B
    for b, f0 in enumerate(P.TONE_F0):
        got = P.median_f0(res["f0"][b * Tp:(b + 1) * Tp], Tp)
        c = P.cents(got, f0 * ratio)
        print("f0 %g Hz, %+g st, rate %g, preserve %d: median %.2f Hz, %+.2f cents" % (f0, semitones, rate, preserve, got, c))
        assert abs(c) <= P.CENTS, (f0, semitones, rate, preserve, got, c)


# ----------------------------------------------------------------------------------------------------------------------
# options
# ----------------------------------------------------------------------------------------------------------------------
def test_prosody_refuses_by_value():
    from deepvoice3_pytorch_amd import audio
    for bad in (0, 5, float("nan"), 0.2, True, "fast", [1.0, 0.0], []):
        with pytest.raises(ValueError, match="rate"):
            audio.Prosody(rate=bad)
    for bad in (25, -24.5, float("nan"), [0.0, 30.0]):
        with pytest.raises(ValueError, match="semitones"):
            audio.Prosody(semitones=bad)
    with pytest.raises(ValueError, match="25"):
        audio.Prosody(semitones=25)
    with pytest.raises(ValueError):
        audio.Prosody(rate=[1.0, 0.8], semitones=[0.0, 1.0, 2.0])
    with pytest.raises(ValueError, match="3 items"):
        audio.Prosody(rate=[1.0, 0.8]).per_item(3)                             # a list of the wrong length
    with pytest.raises(ValueError, match="semitones"):
        audio.Prosody(semitones=[1.0, 2.0, 3.0, 4.0]).per_item(3)
    for bad in (0.0, -1.0, float("inf"), float("nan"), None):
        with pytest.raises(ValueError, match="envelope_hz"):
            audio.Prosody(envelope_hz=bad)
    cfg = audio.AudioConfig()
    with pytest.raises(ValueError, match="envelope_hz=10.0"):                  # 0.46 bins -> W = 0
        audio.Prosody(envelope_hz=10.0).half_width(cfg)
    with pytest.raises(ValueError, match="65 bins"):                           # 1400 Hz * 1024 / 22050 = 65.01
        audio.Prosody(envelope_hz=1400.0).half_width(cfg)
    assert audio.Prosody(envelope_hz=1370.0).half_width(cfg) == 64 and audio.Prosody(envelope_hz=11.0).half_width(cfg) == 1
    assert audio.Prosody().half_width(cfg) == 19
    assert audio.Prosody().half_width(audio.AudioConfig(fft_size=2048, hop_size=512, sample_rate=48000)) == 17


def test_prosody_values():
    from deepvoice3_pytorch_amd import audio
    p = audio.Prosody(rate=[0.8, 1.0], semitones=3)
    assert p.per_item(2) == ([0.8, 1.0], [3.0, 3.0]) and not p.neutral() and p.preserve_envelope
    assert audio.Prosody().neutral() and audio.Prosody(rate=[1.0, 1.0], semitones=[0, 0.0]).neutral()
    assert audio.Prosody(rate=np.array([0.25, 4.0]), semitones=np.float32(-24)).per_item(2) == ([0.25, 4.0], [-24.0, -24.0])
    assert audio.Prosody().per_item(3) == ([1.0] * 3, [0.0] * 3)


def test_the_keywords_of_synthesis():
    """rate / semitones override the prosody's own, the envelope settings are the prosody's, neutral settings are None"""
    from deepvoice3_pytorch_amd import audio, synthesis
    up = synthesis.utterance_prosody
    assert up(None, None, None, 2, "t") is None and up(1.0, 0, None, 2, "t") is None
    assert up(None, None, audio.Prosody(), 2, "t") is None and up([1.0, 1.0], [0.0, 0.0], None, 2, "t") is None
    p = up([0.8, 1.0], None, audio.Prosody(semitones=2.0, preserve_envelope=False, envelope_hz=300.0), 2, "t")
    assert p.per_item(2) == ([0.8, 1.0], [2.0, 2.0]) and not p.preserve_envelope and p.envelope_hz == 300.0
    with pytest.raises(ValueError, match="rate"):
        up([0.8, 1.0, 1.0], None, None, 2, "t")
    with pytest.raises(ValueError, match="audio.Prosody"):
        up(None, None, "fast", 2, "t")
    for fn in (synthesis.tts_batch, synthesis.tts_stream, synthesis.RollingSynthesizer.submit):
        sig = inspect.signature(fn)
        assert [sig.parameters[k].default for k in ("rate", "semitones", "prosody")] == [None] * 3
    assert inspect.signature(audio.inv_spectrogram_batch).parameters["prosody"].default is None


# ----------------------------------------------------------------------------------------------------------------------
# the header and the build
# ----------------------------------------------------------------------------------------------------------------------
_GOOD = dict(mag=64, out=128, B=1, T_in=4, T_out=4, bins=513, tlen_in=None, tlen_out=64, rate=64, ratio=64, W=19, preserve=1)


@pytest.mark.parametrize("kw,names", [
    (dict(mag=None), b"mag is null"), (dict(out=None), b"out is null"), (dict(tlen_out=None), b"tlen_out is null"),
    (dict(rate=None), b"rate is null"), (dict(ratio=None), b"ratio is null"), (dict(out=64), b"out must not be mag"),
    (dict(mag=66), b"4-byte aligned"), (dict(rate=68), b"8-byte aligned"), (dict(B=0), b"B = 0"), (dict(B=65536), b"B = 65536"),
    (dict(T_in=0), b"T_in = 0"), (dict(T_out=0), b"T_out = 0"), (dict(bins=0), b"bins = 0"), (dict(bins=1026), b"bins = 1026"),
    (dict(W=0), b"env_half_width = 0"), (dict(W=65), b"env_half_width = 65"), (dict(W=0, preserve=0), b"env_half_width = 0"),
    (dict(preserve=2), b"preserve_envelope = 2"),
])
def test_library_refuses_every_violation_without_a_gpu(kw, names):
    """dummy non-null pointers: a refusal comes before any launch, so nothing is dereferenced"""
    from deepvoice3_pytorch_amd import _lib
    lib = _lib.lib()
    a = dict(_GOOD, **kw)
    rc = lib.dv3_prosody_warp_f32(a["mag"], a["out"], a["B"], a["T_in"], a["T_out"], a["bins"], a["tlen_in"], a["tlen_out"],
                                  a["rate"], a["ratio"], a["W"], a["preserve"], None)
    assert rc == _lib.CONSTS["DV3_EINVAL"]
    msg = lib.dv3_last_error()
    assert msg.startswith(b"prosody_warp:") and names in msg, msg



def test_the_header_exports_the_entry_point_under_abi_50():
    import ctypes
    from deepvoice3_pytorch_amd import _lib
    restype, args = _lib.FUNCS["dv3_prosody_warp_f32"]
    P_, I = ctypes.c_void_p, ctypes.c_int32
    assert restype is ctypes.c_int and args == [P_, P_, I, I, I, I, P_, P_, P_, P_, I, I, P_]
    assert _lib.CONSTS["DV3_PROSODY_MAX_HALF_WIDTH"] == 64 and _lib.CONSTS["DV3_ABI_VERSION"] == 50
    assert [f for f in _lib.FUNCS if "prosody" in f] == ["dv3_prosody_warp_f32"]
    header = open(os.path.join(ROOT, "include", "dv3hip.h")).read()
    m = re.search(r"/\*((?:(?!\*/).)*)\*/\s*#define DV3_PROSODY_MAX_HALF_WIDTH 64\s*int dv3_prosody_warp_f32\(", header,
                  flags=re.S)
    assert m, "the definition stands in the comment in front of the entry point"
    for word in ("tlen_in", "tlen_out", "floor(u)", "logf", "expf", "never read", "zeros", "Refused"):
        assert word in m.group(1), word
    mk = open(os.path.join(ROOT, "deepvoice3_pytorch_amd", "csrc", "Makefile")).read()
    assert "prosody.hip" in mk
    from deepvoice3_pytorch_amd import audio
    assert "dv3_prosody_warp_f32" in inspect.getsource(audio.warp_magnitudes)

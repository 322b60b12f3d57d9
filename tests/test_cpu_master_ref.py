# coding: utf-8
"""Deliverable audio without a GPU: tests/master_ref.py -- the numpy restatement of
dv3_wave_levels_f32, dv3_wave_gains_f32 and dv3_wave_master_f32 -- checked against itself (float32 against float64, the
crossfade's weights, the reference policy against save_wav's formula), synthesis.plan_document on hand-written cases,
the refusals of audio.Mastering, audio.save_wav's round trip and the C header's entry points and constants."""
import os
import sys
import wave

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tests import master_ref as M  # noqa: E402

U = 2.0 ** -24                                  # one fp32 rounding, relative


_layout = M.issue_layout


@pytest.mark.parametrize("F", [64, 221])
def test_float32_restatement_agrees_with_float64(F):
    """every term is at most three roundings (g w, the fade-out product, times x) and the sum of two one more:
    |y32 - y64| <= ((1 + u)^4 - 1) sum |terms| < 4.001 u sum |terms|"""
    rng = np.random.RandomState(F)
    x, src, length, dst, gain, flags, N = _layout(F, rng)
    assert N % 8 != 0 and sorted({int(v) % 4 for v in src - dst}) == [0, 1, 2, 3]
    fade = M.fade_table(F)
    y32, _ = M.mix(x, src, length, dst, gain, flags, fade, N, np.float32)
    y64, mag = M.mix(x, src, length, dst, gain, flags, fade, N, np.float64)
    assert y32.dtype == np.float32 and y64.dtype == np.float64
    err = np.abs(y32.astype(np.float64) - y64)
    assert np.all(err <= 4.001 * U * mag), float((err / np.maximum(mag, 1e-300)).max() / U)
    assert not y64[:37].any() and not y64[38:49].any() and y64[37] != 0            # the gaps are zeros
    q = M.master(x, src, length, dst, gain, flags, fade, N, M.MODE_I16)
    assert q.dtype == np.int16 and np.all(np.abs(q.astype(np.float64) - y64 * 32767) <= 0.5 + 32767 * 5 * U * mag + 1e-9)


@pytest.mark.parametrize("F", [1, 2, 63, 256, 8192])
def test_a_constant_stays_constant_through_a_crossfade(F):
    """fade[i] + fade[F - 1 - i] is 1 in exact arithmetic (cos a + cos(pi - a) = 0); each table entry is rounded once
    (at most 1: an error of at most u / 2 each), each product once and the sum once: |y - c| <= (u + u + u) |c| to first order"""
    fade = M.fade_table(F)
    assert fade.dtype == np.float32 and np.all(fade > 0) and np.all(fade <= 1) and np.all(np.diff(fade) >= 0)
    c = np.float32(0.7310934)
    L = 3 * F + 5
    x = np.full(2 * L, c, dtype=np.float32)
    dst = [0, L - F]
    y, _ = M.mix(x, [0, L], [L, L], dst, [1.0, 1.0], [M.FADE_OUT, M.FADE_IN], fade, 2 * L - F, np.float32)
    assert np.all(np.abs(y.astype(np.float64) - float(c)) <= 3.01 * U * float(c))
    assert np.array_equal(y[:L - F], x[:L - F])                                       # outside the fades: the samples


def test_reference_policy_is_save_wavs_formula():
    rng = np.random.RandomState(3)
    for scale in (1e-3, 0.3, 1.0, 7.0):
        wav = (rng.randn(3001) * scale).astype(np.float32)
        row, _ = M.levels_row(wav)
        div = M.gains([row], [wav.size], [0, 1], M.GAIN_REFERENCE)
        got = M.master(wav, [0], [wav.size], [0], div, [0], M.fade_table(0), wav.size, M.MODE_I16_REFERENCE)
        assert np.array_equal(got, M.save_wav_samples(wav)), scale
    assert M.gains([(0.001, 1.0, 0, 0, 0)], [5], [0, 1], M.GAIN_REFERENCE)[0] == np.float32(0.01)


def test_levels_and_gains_restatement():
    x = np.array([0.5, -1.0, np.nan, np.inf, 1.0, -0.25, -np.inf], dtype=np.float32)
    row, sabs = M.levels_row(x)
    assert row == (1.0, 0.25 + 1 + 1 + 0.0625, 0.25, 4, 3) and sabs == 2.75
    assert M.levels_row(np.zeros(0, np.float32))[0] == (0.0, 0.0, 0.0, 0, 0)
    lv = [(0.5, 2.0, 0, 0, 0), (0.0, 0.0, 0, 0, 0), (0.25, 1.0, 0, 0, 0)]
    g = M.gains(lv, [8, 8, 16], [0, 1, 2, 3], M.GAIN_PEAK, target=0.5, max_gain=10.0)
    assert g.tolist() == [1.0, 1.0, 2.0]                                             # a silent item keeps gain 1
    g = M.gains(lv, [8, 8, 16], [0, 3], M.GAIN_RMS, target=0.1, ceiling=0.9, max_gain=100.0)
    want = np.float32(min(0.1 / np.sqrt(3.0 / 32.0), 0.9 / 0.5))
    assert g.tolist() == [want] * 3
    assert M.gains(lv, [8, 8, 16], [0, 3], M.GAIN_PEAK, target=0.5, max_gain=0.75).tolist() == [0.75] * 3


def test_dither_is_triangular_and_a_function_of_seed_and_index():
    d = M.dither(np.arange(20000), 0x123456789ABCDEF0)
    assert d.dtype == np.float32 and d.min() > -1 and d.max() < 1 and abs(float(d.mean())) < 0.02
    assert abs(float(d.astype(np.float64).var()) - 1.0 / 6.0) < 0.01                 # the variance of a TPDF of +-1
    assert np.array_equal(M.dither(np.arange(100, 200), 7), M.dither(np.arange(200), 7)[100:])
    assert not np.array_equal(M.dither(np.arange(100), 7), M.dither(np.arange(100), 8))
    big = M.dither(np.array([2 ** 32 + 5, 5], dtype=np.uint64), 7)                   # the counter's high word is read
    assert big[0] != big[1]


# ----------------------------------------------------------------------------------------------------------------------
# the host layer
# ----------------------------------------------------------------------------------------------------------------------
def test_plan_document_by_hand():
    from deepvoice3_pytorch_amd.synthesis import plan_document
    F = 100
    table, N = plan_document([1000, 50, 400, 300], 1000, pauses=[0.0, 0.25, 0.0], fade_samples=F, lead=0.01)
    # sentence 1 is shorter than F: no fade, butt joins on both... its right neighbour comes 0.25 s later
    assert table["flags"].tolist() == [3, 0, 3, 3]
    assert table["src"].tolist() == [0, 1000, 1050, 1450] and table["len"].tolist() == [1000, 50, 400, 300]
    assert table["dst"].tolist() == [10, 1010, 1060 + 250, 1310 + 400 - F]
    assert N == 1610 + 300 and table["dst"].dtype == np.int64 and table["flags"].dtype == np.int32
    # a crossfade that would put a third sentence over a sample becomes a butt join: 150 < 2 F
    table, N = plan_document([500, 150, 500], 1000, pauses=0.0, fade_samples=F)
    assert table["dst"].tolist() == [0, 400, 550] and N == 1050
    table, N = plan_document([500, 200, 500], 1000, pauses=0.0, fade_samples=F, tail=0.5)
    assert table["dst"].tolist() == [0, 400, 500] and N == 1000 + 500
    # given sources, an empty sentence, no fade at all
    table, N = plan_document([7, 0, 9], 8000, pauses=0.001, fade_samples=0, starts=[5, 40, 100])
    assert table["src"].tolist() == [5, 40, 100] and table["dst"].tolist() == [0, 15, 23] and N == 32
    assert table["flags"].tolist() == [0, 0, 0]
    table, N = plan_document([5], 8000, fade_samples=5)
    assert table["flags"].tolist() == [3] and N == 5
    for bad in (dict(lengths=[]), dict(lengths=[4, -1]), dict(lengths=[4, 4], pauses=[0.1, 0.1]),
                dict(lengths=[4, 4], pauses=-0.1), dict(lengths=[4], fade_samples=-1), dict(lengths=[4], sample_rate=0),
                dict(lengths=[4, 4], starts=[0]), dict(lengths=[4], lead=-1.0), dict(lengths=[4], fade_samples=2.5)):
        kw = dict(sample_rate=1000, fade_samples=0)
        kw.update(bad)
        with pytest.raises(ValueError, match="plan_document"):
            plan_document(**kw)


def test_a_plan_passes_the_layout_rules_and_refusals():
    from deepvoice3_pytorch_amd import audio
    from deepvoice3_pytorch_amd.synthesis import plan_document
    rng = np.random.RandomState(0)
    for _ in range(50):
        lens = rng.randint(0, 400, rng.randint(1, 9))
        table, N = plan_document(lens, 1000, pauses=rng.choice([0.0, 0.0, 0.05], max(len(lens) - 1, 1))[:len(lens) - 1],
                                 fade_samples=int(rng.choice([0, 1, 64, 150])))
        audio.check_segments(table["src"], table["len"], table["dst"], int(lens.sum()), N)
    ok = ([0, 10, 20], [10, 10, 10], [0, 8, 16])
    audio.check_segments(*ok, total=30, N=26)
    for src, ln, dst, total, N, ref, what in (
            ([0, 10], [10, 10], [10, 0], 20, 20, False, "sorted"),                   # dst descends
            ([0, 10], [10, 2], [0, 2], 20, 20, False, "sorted"),                     # an end descends
            ([0, 10, 20], [10, 10, 10], [0, 4, 8], 30, 30, False, "three"),          # triple overlap
            ([0, 25], [10, 10], [0, 10], 30, 30, False, "source"),                   # a span outside the buffer
            ([0, 10], [10, 10], [0, 10], 20, 19, False, "output"),
            ([0, 10], [10, 10], [0, 9], 20, 20, True, "reference"),
            ([0], [10, 10], [0, 10], 20, 20, False, "entries")):
        with pytest.raises(ValueError, match=what):
            audio.check_segments(src, ln, dst, total, N, ref)


def test_mastering_refuses_bad_values():
    from deepvoice3_pytorch_amd import audio
    m = audio.Mastering()
    assert (m.level, m.scope, m.dtype, m.dither, m.seed) == (None, "item", "int16", False, 0)
    assert audio.Mastering("rms").target_db == -20.0 and audio.Mastering("peak").target_db == -1.0
    assert audio.Mastering("peak", fade_ms=5.0).fade_samples(22050) == 110
    assert audio.Mastering("reference", fade_ms=5.0).fade_samples(22050) == 0
    assert audio.Mastering("reference").mode() == 2 and audio.Mastering(dtype="float32").mode() == 0
    for kw, what in ((dict(level="loud"), "level"), (dict(scope="batch"), "scope"), (dict(dtype="int8"), "dtype"),
                     (dict(target_db=3.0), "target_db"), (dict(target_db=float("nan")), "target_db"),
                     (dict(ceiling_db="0"), "ceiling_db"), (dict(max_gain_db=-1.0), "max_gain_db"),
                     (dict(fade_ms=-1.0), "fade_ms"), (dict(fade_ms=True), "fade_ms"), (dict(dither=1), "dither"),
                     (dict(seed=-1), "seed"), (dict(seed=2 ** 64), "seed"), (dict(seed=1.5), "seed"),
                     (dict(dither=True, dtype="float32"), "dither"), (dict(level="reference", dtype="float32"), "reference"),
                     (dict(level="reference", dither=True), "reference")):
        with pytest.raises(ValueError, match=what):
            audio.Mastering(**kw)
    with pytest.raises(ValueError, match="fade_ms"):
        audio.Mastering(fade_ms=900.0).fade_samples(48000)
    with pytest.raises(ValueError, match="Mastering"):
        audio.check_mastering("peak", "tts_batch")
    assert audio.check_mastering(None, "x") is None and audio.check_mastering(m, "x") is m
    assert audio.LEVEL_COLUMNS == ("peak", "sumsq", "sum", "over", "nonfinite")
    assert np.array_equal(audio.fade_table_np(221), M.fade_table(221)) and audio.fade_table_np(0).size == 0


def test_save_wav_round_trip(tmp_path):
    import torch
    from deepvoice3_pytorch_amd import audio
    rng = np.random.RandomState(1)
    pcm = rng.randint(-32768, 32768, 4001).astype(np.int16)
    pcm[:2] = (-32768, 32767)
    path = str(tmp_path / "a.wav")
    audio.save_wav(path, torch.from_numpy(pcm), 22050)
    w = wave.open(path, "rb")
    try:
        assert (w.getnchannels(), w.getsampwidth(), w.getframerate(), w.getnframes()) == (1, 2, 22050, pcm.size)
        back = np.frombuffer(w.readframes(pcm.size), dtype="<i2")
    finally:
        w.close()
    assert np.array_equal(back, pcm)
    try:
        from scipy.io import wavfile
    except ImportError:
        wavfile = None
    if wavfile is not None:
        sr, data = wavfile.read(path)
        assert sr == 22050 and data.dtype == np.int16 and np.array_equal(data, pcm)
    for bad, rate in ((pcm.astype(np.float32), 22050), (pcm.reshape(1, -1), 22050), (pcm, 0), (pcm, 22050.5)):
        with pytest.raises(ValueError, match="save_wav"):
            audio.save_wav(path, bad, rate)


def test_header_constants_and_entry_points():
    from deepvoice3_pytorch_amd import _lib
    c = _lib.CONSTS
    assert c["DV3_ABI_VERSION"] == 50
    assert (c["DV3_LEVEL_COLUMNS"], c["DV3_LEVELS_CHUNK"]) == (5, 16384)
    assert (c["DV3_GAIN_PEAK"], c["DV3_GAIN_RMS"], c["DV3_GAIN_REFERENCE"]) == (M.GAIN_PEAK, M.GAIN_RMS, M.GAIN_REFERENCE)
    assert (c["DV3_MASTER_F32"], c["DV3_MASTER_I16"], c["DV3_MASTER_I16_REFERENCE"]) == \
        (M.MODE_F32, M.MODE_I16, M.MODE_I16_REFERENCE)
    assert (c["DV3_MASTER_FADE_IN"], c["DV3_MASTER_FADE_OUT"]) == (M.FADE_IN, M.FADE_OUT)
    assert c["DV3_MASTER_MAX_FADE"] == 8192 and c["DV3_MASTER_MAX_SEGMENTS"] == 2 ** 20
    import ctypes
    f = _lib.FUNCS
    assert len(f["dv3_wave_levels_f32"][1]) == 8 and f["dv3_wave_levels_f32"][1][4] is ctypes.c_int64
    assert len(f["dv3_wave_gains_f32"][1]) == 11 and f["dv3_wave_gains_f32"][1][6:9] == [ctypes.c_double] * 3
    assert len(f["dv3_wave_master_f32"][1]) == 15 and f["dv3_wave_master_f32"][1][11] is ctypes.c_uint64
    src = open(os.path.join(ROOT, "deepvoice3_pytorch_amd", "csrc", "Makefile")).read()
    assert "master.hip" in src

# coding: utf-8
"""No GPU: the float64 restatement of the loudness measure (tests/loudness_ref.py) against ITU-R BS.1770's own figures --
the coefficient table at 48 kHz, the 997 Hz sine, two gating programmes whose block counts are known -- the chunked form
of the filter against the sequential one, the edge rules, the true-peak estimate, the gains, and the host side of the
feature: audio.k_weighting, audio.true_peak_table, the Mastering("lufs") refusals and the header's constants."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tests import loudness_ref as R  # noqa: E402

# ITU-R BS.1770-4, tables 1 and 2 (48 kHz)
BS1770_SHELF_B = (1.53512485958697, -2.69169618940638, 1.19839281085285)
BS1770_SHELF_A = (1.0, -1.69065929318241, 0.73248077421585)
BS1770_HP_B = (1.0, -2.0, 1.0)
BS1770_HP_A = (1.0, -1.99004745483398, 0.99007225036621)


def test_coefficients_at_48k_are_the_standards_table():
    sb, sa, pb, pa = R.coefficients(48000)
    for got, want in ((sb, BS1770_SHELF_B), (sa, BS1770_SHELF_A), (pb, BS1770_HP_B), (pa, BS1770_HP_A)):
        assert np.abs(got - np.array(want)).max() <= 1e-12, (got, want)
    from deepvoice3_pytorch_amd import audio
    kw = audio.k_weighting(48000)
    assert np.array_equal(kw["coef"], np.concatenate([sb, sa[1:], pb, pa[1:]]))
    assert kw["h"] == 4800 and np.array_equal(kw["A"], R.transition(48000))
    assert np.array_equal(kw["Ah"], np.linalg.matrix_power(R.transition(48000), 4800))
    assert [audio.loudness_step(fs) for fs in (8000, 16000, 22050, 44100, 192000)] == [800, 1600, 2205, 4410, 19200]
    assert [R.step(fs) for fs in (8000, 16000, 22050, 44100, 192000)] == [800, 1600, 2205, 4410, 19200]
    for bad in (7999, 192001, "48000", True, None):
        with pytest.raises(ValueError, match="sample_rate"):
            audio.k_weighting(bad)


@pytest.mark.parametrize("fs,tol", [(48000, 0.01), (44100, 0.1), (22050, 0.1), (16000, 0.1)])
def test_full_scale_997_hz_sine(fs, tol):
    """-3.01 LKFS: +-0.01 at 48 kHz, within EBU Tech 3341's 0.1 LU at the other rates"""
    x = R.tone(fs, 997.0, 5.0, 0.0).astype(np.float32)
    rows, detail, _ = R.measure([x], fs)
    print("997 Hz at %d Hz: %.4f LKFS" % (fs, rows[0, 0]))
    assert abs(rows[0, 0] - (-3.01)) <= tol, rows[0]
    assert rows[0, 1] == 47 and rows[0, 2] == 47 and rows[0, 6] == 0


@pytest.fixture(scope="module")
def gating():
    out = {}
    for name, make, rates in (("A", R.gating_a, (8000, 22050)), ("B", R.gating_b, (8000,))):
        for fs in rates:
            x = make(fs)
            rows, detail, E = R.measure([x], fs)
            out[name, fs] = (x, rows[0], detail[0])
    return out


@pytest.mark.parametrize("name,fs,counts,level", [("A", 8000, (77, 77, 43), -23.30), ("A", 22050, (77, 77, 43), -23.29),
                                                  ("B", 8000, (77, 31, 30), None)])
def test_gating_programmes(gating, name, fs, counts, level):
    x, row, (l, gamma) = gating[name, fs]
    margin = R.gate_margin(l, gamma)
    print("gating %s at %d Hz: L = %.4f, counts %s, nearest block %.3f LU from a gate" % (name, fs, row[0], row[1:4], margin))
    assert margin > 0.01, "a block lies within 0.01 LU of a gate: the input is no fair test"
    assert tuple(int(v) for v in row[1:4]) == counts
    assert margin > (6.8 if name == "A" else 4.2)
    if level is not None:
        assert abs(row[0] - level) <= 0.01, row[0]
    else:
        assert abs(row[0] - (-20.0 - 3.0103 + 0.0)) < 0.5      # the tone alone, about -23 LKFS: the silence is gated out
    assert row[6] == 0


def test_chunked_filter_agrees_with_the_sequential_one():
    """zero-state chunks plus A^h reproduce every chunk's start state; the bound is the cascade's noise gain times the
    unit roundoff times the number of samples behind, relative to the largest state"""
    rng = np.random.RandomState(3)
    for fs, n in ((8000, 5 * 800 + 123), (22050, 3 * 2205 + 7)):
        x = (0.3 * rng.randn(n)).astype(np.float32)
        a, b = R.chunk_states(x, fs), R.chunked_states(x, fs)
        assert a.shape == b.shape == (-(-n // R.step(fs)), 4) and not a[0].any() and not b[0].any()
        bound = 2.0 ** -52 * R.noise_gain(fs, 4 * R.step(fs)) * n * max(np.abs(a).max(), 1.0)
        print("chunked vs sequential at %d Hz: %.3e (bound %.3e)" % (fs, np.abs(a - b).max(), bound))
        assert np.abs(a - b).max() <= bound
    # and A is the zero-input transition of the cascade
    s = np.array([0.3, -0.2, 0.5, 0.1])
    _, after = R.cascade(np.zeros(1), 22050, s)
    assert np.allclose(after, R.transition(22050).dot(s), rtol=0, atol=1e-15)


def test_edge_rules():
    fs, h = 8000, 800
    rng = np.random.RandomState(5)
    want_blocks = {0: 0, h - 1: 0, 4 * h - 1: 0, 4 * h: 1, 4 * h + 1: 1, 5 * h: 2}
    for n, J in want_blocks.items():
        x = (0.1 * rng.randn(n)).astype(np.float32)
        rows, _, E = R.measure([x], fs)
        row = rows[0]
        assert row[1] == J and len(E[0]) == -(-n // h)
        if n == 0:
            assert row[0] == R.NINF and row[6] == (R.SHORT | R.SILENT)
        elif J == 0:
            y, _ = R.cascade(x, fs)
            assert row[6] == R.SHORT and abs(row[0] - (-0.691 + 10 * np.log10(np.sum(y * y) / n))) < 1e-9
        else:
            assert row[6] == 0 and row[2] == J and np.isfinite(row[0])
    # blocks, but none above the absolute gate: silent, and the gain is 1
    quiet = (1e-6 * rng.randn(5 * h)).astype(np.float32)
    rows, _, _ = R.measure([quiet], fs)
    assert rows[0, 0] == R.NINF and rows[0, 1] == 2 and rows[0, 2] == 0 and rows[0, 6] == R.SILENT
    assert R.gains(rows, [0, 1], -23.0, 0.9, 30.0)[0] == 1.0
    # a group of short items is measured over their pooled samples
    a, b = (0.1 * rng.randn(h - 1)).astype(np.float32), (0.4 * rng.randn(3 * h)).astype(np.float32)
    rows, _, E = R.measure([a, b], fs, [0, 2])
    want = -0.691 + 10 * np.log10((E[0].sum() + E[1].sum()) / (a.size + b.size))
    assert rows[0, 6] == R.SHORT and abs(rows[0, 0] - want) < 1e-9


def test_document_scope_pools_blocks_and_differs_from_item_scope():
    fs = 8000
    loud, soft = R.tone(fs, 1000.0, 2.0, -20).astype(np.float32), R.tone(fs, 1000.0, 2.0, -40).astype(np.float32)
    per_item, _, _ = R.measure([loud, soft], fs)
    pooled, detail, _ = R.measure([loud, soft], fs, [0, 2])
    assert R.gate_margin(*detail[0]) > 0.01
    assert pooled[0, 1] == per_item[0, 1] + per_item[1, 1] == 34             # blocks never straddle items
    assert pooled[0, 3] == 17                                                # the soft item falls under the relative gate
    assert abs(pooled[0, 0] - per_item[0, 0]) < 0.01 and abs(per_item[0, 0] - per_item[1, 0] - 20.0) < 0.01
    g_item = R.gains(per_item, [0, 1, 2], -23.0, 1.0, 100.0)
    g_doc = R.gains(pooled, [0, 2], -23.0, 1.0, 100.0)
    assert g_doc[0] == g_doc[1] and abs(g_item[1] / g_item[0] - 10.0) < 0.02 and g_doc[1] != g_item[1]


TP_TONES = ((4.0, 0.0), (4.0, np.pi / 4), (6.0, 0.0), (8.0, 0.0), (3.0, 0.0), (2.5, 0.0))
# tones moved off the sample grid (by half a sample at fs/6 and fs/8, by a quarter at fs/3) so that the samples
# under-read and the interpolants have to find the peak, which still lies on the 4x grid
TP_SHIFTED = ((6.0, np.pi / 6), (8.0, np.pi / 8), (3.0, np.pi / 6))


@pytest.mark.parametrize("fs", [8000, 22050])
def test_true_peak_on_faded_tones(fs):
    """amplitude 0.5 cosines: -6.02 dBTP within 0.05 dB at fs/4 (0 and 45 degrees), fs/6, fs/8, fs/3 and fs/2.5, whose
    peaks lie on the 4x grid (a 4x grid with P points per period under-reads a peak BETWEEN its points by up to
    20 log10 cos(pi / P), 0.3 dB at fs/3: the estimate's resolution, not its interpolator's error); the sample peak of
    the fs/4 45-degree tone reads -9.03.  Off the sample grid the reading is the tone's level times the interpolator's
    gain at that frequency, |H_p| of the table's own phases, to 0.01 dB (the fades)."""
    for div, phase in TP_TONES:
        x = R.faded_tone(fs, fs / div, phase)
        tp = 20 * np.log10(R.true_peak(x))
        print("fs/%g phase %.2f at %d Hz: %.3f dBTP (sample peak %.3f)" % (div, phase, fs, tp, 20 * np.log10(np.abs(x).max())))
        assert abs(tp - (-6.0206)) <= 0.05, (div, phase, tp)
    x = R.faded_tone(fs, fs / 4.0, np.pi / 4)
    assert abs(20 * np.log10(np.abs(x).max()) - (-9.03)) < 0.01
    for div, phase in TP_SHIFTED:
        x = R.faded_tone(fs, fs / div, phase)
        tp, sp = 20 * np.log10(R.true_peak(x)), 20 * np.log10(np.abs(x).max())
        H = 20 * np.log10(R.interpolator_response(1.0 / div))
        print("fs/%g shifted at %d Hz: %.3f dBTP (sample peak %.3f, |H| %s dB)" % (div, fs, tp, sp, np.round(H, 3)))
        assert sp < -6.0206 - 0.5 and -6.0206 + min(H.min(), 0.0) - 0.01 <= tp <= -6.0206 + max(H.max(), 0.0) + 0.01
        assert tp > sp + 0.2                                                     # the interpolants found what the samples miss
    assert R.true_peak(np.zeros(0, np.float32)) == 0.0
    one = np.zeros(40, np.float32)
    one[17] = -0.75
    assert R.true_peak(one) == 0.75                                          # phase 0 is the identity; |g| <= 1


def test_true_peak_table():
    from deepvoice3_pytorch_amd import audio
    t = audio.true_peak_table()
    assert t.dtype == np.float32 and t.shape == (3, 12) and np.array_equal(t, R.peak_table())
    g = R.interpolator()
    assert g[24] == 1.0 and np.abs(g[[0, 4, 8, 12, 16, 20, 28, 48]]).max() < 1e-15        # phase 0: the identity
    assert np.array_equal(t[0], t[2][::-1]) and np.array_equal(t[1], t[1][::-1])           # symmetric
    assert np.abs(t.astype(np.float64).sum(axis=1) - 1.0).max() < 2e-3                    # unit gain at DC


def test_gains_formula():
    rows = np.array([[-30.0, 10, 10, 10, -28.0, 0.1, 0],       # 7 dB up
                     [-30.0, 10, 10, 10, -28.0, 0.5, 0],       # the ceiling binds: 0.8 / 0.5
                     [-80.0, 10, 10, 10, -75.0, 1e-4, 0],      # max_gain binds
                     [R.NINF, 10, 0, 0, R.NINF, 0.0, R.SILENT],
                     [-20.0, 0, 0, 0, R.NINF, 0.2, R.SHORT]])
    g = R.gains(rows, [0, 1, 2, 3, 5, 6], -23.0, 0.8, 10.0 ** (30 / 20.0))
    assert g.dtype == np.float32 and g.shape == (6,)
    assert g[0] == np.float32(10.0 ** (7 / 20.0)) and g[1] == np.float32(0.8 / 0.5) and g[2] == np.float32(10.0 ** 1.5)
    assert g[3] == g[4] == 1.0 and g[5] == np.float32(10.0 ** (-3 / 20.0))


def test_mastering_lufs_values_and_refusals():
    from deepvoice3_pytorch_amd import audio
    m = audio.Mastering("lufs")
    assert (m.level, m.target_db, m.ceiling_db, m.true_peak, m.scope) == ("lufs", -23.0, -1.0, False, "item")
    assert audio.Mastering("lufs", target_db=-16.0, true_peak=True, scope="document").true_peak is True
    assert audio.Mastering("rms").true_peak is False and audio.Mastering("lufs").mode() == 1
    assert audio.Mastering("lufs", fade_ms=5.0).fade_samples(22050) == 110
    for kw, what in ((dict(level="loud"), "level"), (dict(level="LUFS"), "level"), (dict(level="peak", true_peak=True), "true_peak"),
                     (dict(level=None, true_peak=True), "true_peak"), (dict(level="lufs", true_peak=1), "true_peak"),
                     (dict(level="lufs", target_db=1.0), "target_db"), (dict(level="lufs", dither=True, dtype="float32"), "dither")):
        with pytest.raises(ValueError, match=what):
            audio.Mastering(**kw)
    with pytest.raises(ValueError, match="lufs"):
        audio.loudness_gains(None, [0, 1], audio.Mastering("rms"))
    with pytest.raises(ValueError, match="lufs"):
        audio.wave_gains(None, None, m)
    assert audio.LOUDNESS_COLUMNS == R.COLUMNS


def test_header_constants():
    from deepvoice3_pytorch_amd import _lib
    C = _lib.CONSTS
    assert C["DV3_ABI_VERSION"] == 50
    assert (C["DV3_LOUDNESS_COLUMNS"], C["DV3_LOUDNESS_SHORT"], C["DV3_LOUDNESS_SILENT"]) == (7, R.SHORT, R.SILENT)
    assert (C["DV3_LOUDNESS_MIN_STEP"], C["DV3_LOUDNESS_MAX_STEP"]) == (R.step(8000), R.step(192000))
    assert C["DV3_TRUE_PEAK_TAPS"] == 12 and C["DV3_TRUE_PEAK_CHUNK"] % 256 == 0
    for name in ("dv3_wave_loudness_f64", "dv3_loudness_gate_f64", "dv3_loudness_gains_f32"):
        assert name in _lib.FUNCS and len(_lib.FUNCS[name][1]) == {"dv3_wave_loudness_f64": 14, "dv3_loudness_gate_f64": 11,
                                                                  "dv3_loudness_gains_f32": 9}[name]

# coding: utf-8
"""No GPU: the float64 restatement of the look-ahead limiter (tests/limiter_ref.py) against the consequences its
definition promises -- the two release forms, the ceiling, exact unity where nothing exceeds --, the syllable fixture's
inequalities on the reference alone, and the refusals by value of audio.Limiter and Mastering(limiter=)."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tests import limiter_ref as R  # noqa: E402

FS = 22050
RHO_50, RHO_400 = float(np.exp(-1000.0 / (50.0 * FS))), float(np.exp(-1000.0 / (400.0 * FS)))


def _spiky(n, seed):
    """sparse spikes over low noise, a full-scale spike at sample 0 and at the last sample"""
    x = R.spikes(n, seed, at=(n // 3, n // 3 + 34), extra=6)
    x[0], x[-1] = 1.0, -1.0
    return x


@pytest.mark.parametrize("rho", [0.0, 0.5, RHO_50, RHO_400])
def test_the_two_release_forms_agree(rho):
    rng = np.random.RandomState(3)
    for n in (1, 2, 700, 3589):
        dm = np.where(rng.rand(n) < 0.02, rng.rand(n), 0.0)
        a, b = R.release_sequential(dm, rho), R.release_powers(dm, rho)
        assert np.abs(a - b).max() <= 1e-13, (n, rho)
    x = _spiky(3000, 5)
    a, b = (R.limit(x, 1.7, 0.7, 33, rho, release=form) for form in ("sequential", "powers"))
    for key in ("dq", "ds", "s"):
        assert np.abs(a[key] - b[key]).max() <= 1e-13, key
    assert np.array_equal(a["report"][1:], b["report"][1:])


@pytest.mark.parametrize("true_peak", [False, True])
@pytest.mark.parametrize("A", [0, 1, 33])
def test_ds_covers_dr_and_the_ceiling_holds(A, true_peak):
    g, c = 1.7, 0.7
    for seed, n in ((1, 2500), (2, 1025), (3, 40)):
        for rho in (RHO_50, RHO_400):
            r = R.limit(_spiky(n, seed), g, c, A, rho, true_peak)
            assert r["report"][1] >= 2 and r["dr"][0] > 0.5 and r["dr"][-1] > 0.5
            assert np.all(r["ds"] >= r["dr"] - 1e-15), (A, n, float((r["dr"] - r["ds"]).max()))
            assert np.all(r["dq"] >= r["dm"]) and np.all(r["dm"] >= r["dr"])
            assert r["report"][0] == r["s"].min() and 0.0 < r["report"][0] < 1.0
            if not true_peak:
                assert np.abs(r["out"]).max() <= c * (1.0 + 2.0 ** -22)
                assert np.abs(r["out"].astype(np.float64) - r["exact"]).max() <= R.out_bound(r["y"]).max()
                assert np.all(np.abs(r["out"].astype(np.float64) - r["exact"]) <= R.out_bound(r["y"]))
            else:                                       # the detector reads more than the samples: it demands no less
                assert np.all(r["e"] >= np.abs(r["y"]))


def test_unity_where_nothing_exceeds():
    x = R.spikes(3000, 9, level=0.02, lo=0.2, hi=0.3)
    for true_peak in (False, True):
        r = R.limit(x, 1.7, 0.7, 33, RHO_50, true_peak)
        assert np.all(r["s"] == 1.0) and not r["dr"].any() and np.array_equal(r["report"], [1.0, 0.0])
        assert np.array_equal(r["out"].view(np.int32), (np.float32(1.7) * x).astype(np.float32).view(np.int32))
    # far behind a spike the release has not reached zero, but before the look-ahead sees it s is exactly 1
    x[2000] = 1.0
    r = R.limit(x, 1.7, 0.7, 33, RHO_50)
    assert np.all(r["s"][:2000 - 66] == 1.0) and r["s"][2000] < 0.42 and r["report"][1] == 1
    empty = R.limit(np.zeros(0, np.float32), 1.7, 0.7, 33, RHO_50, True)
    assert np.array_equal(empty["report"], [1.0, 0.0]) and empty["out"].size == 0


def test_limiter_by_value():
    from deepvoice3_pytorch_amd import _lib, audio
    lim = audio.Limiter()
    assert (lim.lookahead_ms, lim.release_ms, lim.passes) == (1.5, 50.0, 1)
    assert lim.lookahead(22050) == 33 and lim.lookahead(8000) == 12 and audio.Limiter(0).lookahead(48000) == 0
    assert lim.rho(22050) == float(np.exp(-1000.0 / (50.0 * 22050)))
    amax = _lib.CONSTS["DV3_LIMIT_MAX_LOOKAHEAD"]
    assert audio.Limiter(lookahead_ms=1000.0 * amax / 22050).lookahead(22050) == amax
    with pytest.raises(ValueError, match=r"%d samples.*at most %d" % (amax + 1, amax)):
        audio.Limiter(lookahead_ms=1000.0 * (amax + 1) / 22050).lookahead(22050)
    for kw in (dict(lookahead_ms=-0.1), dict(lookahead_ms=None), dict(lookahead_ms=float("nan")), dict(lookahead_ms=True),
               dict(release_ms=0.0), dict(release_ms=-1.0), dict(release_ms="50"), dict(release_ms=float("inf")),
               dict(passes=0), dict(passes=5), dict(passes=1.0), dict(passes=True)):
        with pytest.raises(ValueError, match="Limiter: %s" % list(kw)[0]):
            audio.Limiter(**kw)


def test_mastering_takes_a_limiter_by_value():
    from deepvoice3_pytorch_amd import audio
    lim = audio.Limiter()
    assert audio.Mastering("lufs").limiter is None and audio.Mastering().limiter is None
    for level in (None, "rms", "lufs"):
        assert audio.Mastering(level, limiter=lim).limiter is lim
    assert audio.Mastering("lufs", limiter=audio.Limiter(passes=3), true_peak=True).limiter.passes == 3
    # the last keyword: positional callers are untouched
    m = audio.Mastering("lufs", "item", -16.0, -1.0, 30.0, 5.0, False, 0, "float32", True)
    assert m.true_peak and m.limiter is None
    for level in ("peak", "reference"):
        with pytest.raises(ValueError, match="limiter"):
            audio.Mastering(level, limiter=lim)
    for level in (None, "rms"):
        with pytest.raises(ValueError, match="passes"):
            audio.Mastering(level, limiter=audio.Limiter(passes=2))
    for bad in (1.5, "on", True, audio.Limiter):
        with pytest.raises(ValueError, match="limiter"):
            audio.Mastering("lufs", limiter=bad)


def test_constants_and_the_entry_point():
    from deepvoice3_pytorch_amd import _lib, audio
    C = _lib.CONSTS
    assert C["DV3_ABI_VERSION"] == 50
    T = C["DV3_LIMIT_TILE"]
    assert T & (T - 1) == 0 and 0 < C["DV3_LIMIT_MAX_LOOKAHEAD"] <= T and C["DV3_LIMIT_COLUMNS"] == 2
    assert 2 ** (C["DV3_LIMIT_RHO_POWERS"] - 1) == T
    assert audio.LIMITER_COLUMNS == R.COLUMNS == ("gain_min", "over_samples")
    assert "dv3_wave_limit_f32" in _lib.FUNCS and len(_lib.FUNCS["dv3_wave_limit_f32"][1]) == 14
    rho = 0.9995
    assert np.array_equal(audio.rho_powers(rho), R.rho_powers(rho, C["DV3_LIMIT_RHO_POWERS"]))
    assert abs(audio.rho_powers(rho)[-1] - rho ** T) <= 1e-15


@pytest.fixture(scope="module")
def fixture_loudness():
    """the syllable fixture through the reference's mastering chain: {(target, true_peak): (static, [pass 1, 2, 3])} in LUFS"""
    x = R.syllables(FS)
    c = 10.0 ** (-1.0 / 20.0)
    out = {}
    for true_peak in (False, True):
        for target in (-16.0, -14.0):
            static = R.integrated(R.master(x, FS, target, c, true_peak=true_peak), FS)
            limited = [R.integrated(o, FS) for o in R.master(x, FS, target, c, 33, RHO_50, 3, true_peak)]
            out[(target, true_peak)] = (static, limited)
    return x, out


def test_the_syllable_fixture(fixture_loudness):
    x, _ = fixture_loudness
    assert x.size == 47624 and x.dtype == np.float32 and abs(float(np.abs(x).max()) - 0.5) < 1e-7
    rms = [np.sqrt(np.mean(x[i * 5953:(i + 1) * 5953].astype(np.float64) ** 2)) for i in range(8)]
    assert int(np.argmax(rms)) == 2 and rms[2] > 2.4 * max(rms[:2] + rms[3:])


@pytest.mark.parametrize("true_peak", [False, True])
@pytest.mark.parametrize("target", [-16.0, -14.0])
def test_the_fixture_inequalities_on_the_reference(fixture_loudness, target, true_peak):
    static, limited = fixture_loudness[1][(target, true_peak)]
    print("target %g, true_peak %r: static %.3f, passes %s" % (target, true_peak, static, ["%.3f" % v for v in limited]))
    deficit = [target - v for v in limited]
    assert target - static >= 1.0                                   # one loud syllable: the ceiling binds the static gain
    assert deficit[0] <= 0.5 * (target - static)
    assert deficit[1] <= deficit[0] and deficit[2] <= deficit[1]
    assert max(limited) <= target + 0.05


def test_the_ceiling_on_the_fixture():
    x = R.syllables(FS)
    c = 10.0 ** (-1.0 / 20.0)
    from tests import loudness_ref as LR
    sp, tp = (R.master(x, FS, -14.0, c, 33, RHO_50, 1, flag)[0] for flag in (False, True))
    assert np.abs(sp).max() <= c * (1.0 + 2.0 ** -22)
    assert LR.true_peak(sp) > c                                     # the sample-peak limiter leaves inter-sample overs
    assert LR.true_peak(tp) <= c * (1.0 + 1e-12)                    # the trim

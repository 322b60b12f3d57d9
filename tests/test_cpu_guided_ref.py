# coding: utf-8
"""No GPU: the host side of the guided decode.

  * tests/guided_ref.guide_table equals np.repeat(np.arange(key_len), dur)[:T] on random cases with zero durations and
    with T below, at and above the sum; past the item's steps it repeats the last spoken token (these two tests check
    the restatement against numpy and do not touch the library: they hold the reference the GPU test compares the
    kernel with, and pass with or without the feature);
  * synthesis.fit_durations equals the rational restatement, sums to the requested total exactly, keeps zeros, never
    gives the token with the larger duration fewer steps, and is the identity when the total is unchanged;
  * the header exports the three guided entry points and the DV3_GUIDE_* bits, and the ABI is still 50.
"""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tests import guided_ref  # noqa: E402


def _cases(seed, n):
    rng = np.random.RandomState(seed)
    for _ in range(n):
        Tk = int(rng.randint(1, 40))
        dur = rng.randint(0, 5, Tk) * (rng.rand(Tk) > 0.3)
        if dur.sum() == 0:
            dur[rng.randint(Tk)] = 1 + rng.randint(4)
        yield dur.astype(np.int64), int(rng.randint(1, Tk + 1))


def test_guide_table_is_np_repeat():
    seen = set()
    for dur, key_len in _cases(0, 300):
        S = int(dur[:key_len].sum())
        if S == 0:
            continue
        for T in sorted({max(S - 3, 1), S, S + 4}):
            g, steps, flags = guided_ref.guide_table(dur[None], [key_len], T)
            want = np.repeat(np.arange(key_len), dur[:key_len])[:T]
            assert steps[0] == len(want) == min(S, T)
            assert np.array_equal(g[0, :len(want)], want)
            assert (g[0, len(want):] == want[-1]).all()
            assert flags[0] == (guided_ref.OVER if S > T else 0)
            seen.add((S > T) - (S < T))
            seen.add("zero" if (dur[:key_len] == 0).any() else "dense")
    assert seen == {-1, 0, 1, "zero", "dense"}


def test_guide_table_flags():
    g, steps, flags = guided_ref.guide_table([[2, -3, 1], [0, 0, 0], [4, 4, 4]], [3, 3, 2], 6)
    assert flags.tolist() == [guided_ref.NEGATIVE, guided_ref.EMPTY, guided_ref.OVER]
    assert steps.tolist() == [3, 0, 6]
    assert g.tolist() == [[0, 0, 2, 2, 2, 2], [0] * 6, [0, 0, 0, 0, 1, 1]]


def test_fit_durations():
    from deepvoice3_pytorch_amd.synthesis import fit_durations
    rng = np.random.RandomState(1)
    for dur, _ in _cases(2, 300):
        d = dur.tolist()
        S, N = sum(d), len(d)
        assert fit_durations(d, S) == d                                   # the identity
        assert fit_durations(np.asarray(d), S) == d
        for total in (1, S // 2 + 1, S + 1, 3 * S + int(rng.randint(0, 7))):
            got = fit_durations(d, total)
            assert got == guided_ref.fit_durations(d, total), (d, total)
            assert sum(got) == total and min(got) >= 0
            assert all(g == 0 for g, v in zip(got, d) if v == 0)          # zeros stay zero
            for a in range(N):
                for b in range(N):
                    if d[a] > d[b]:
                        assert got[a] >= got[b], (d, total, got)
        m = 1 + int(rng.randint(0, 2))
        total = N * m + S
        got = fit_durations(d, total, min_steps=m)
        assert got == guided_ref.fit_durations(d, total, m) and sum(got) == total and min(got) >= m
        if min(d) >= m:
            assert fit_durations(d, S, min_steps=m) == d


def test_fit_durations_ties_and_refusals():
    from deepvoice3_pytorch_amd.synthesis import fit_durations
    assert fit_durations([1, 1, 1], 4) == [2, 1, 1]                        # the tie goes to the earlier token
    assert fit_durations([1, 1, 1], 5) == [2, 2, 1]
    assert fit_durations([3, 0, 3], 7) == [4, 0, 3]
    assert fit_durations([0, 0], 5, min_steps=1) == [3, 2]
    with pytest.raises(ValueError, match="negative"):
        fit_durations([1, -1], 4)
    with pytest.raises(ValueError, match="nothing to scale"):
        fit_durations([0, 0], 4)
    with pytest.raises(ValueError, match="do not hold"):
        fit_durations([2, 2], 3, min_steps=2)


def test_header_exports_guided_entry_points():
    from deepvoice3_pytorch_amd import _lib
    for name in ("dv3_attn_step_guided_f32", "dv3_decode_program_launch_guided", "dv3_guide_from_durations_i32"):
        assert name in _lib.FUNCS, name
    assert len(_lib.FUNCS["dv3_attn_step_guided_f32"][1]) == 5
    assert len(_lib.FUNCS["dv3_decode_program_launch_guided"][1]) == 5
    assert len(_lib.FUNCS["dv3_guide_from_durations_i32"][1]) == 11
    assert (_lib.CONSTS["DV3_GUIDE_NEGATIVE"], _lib.CONSTS["DV3_GUIDE_EMPTY"], _lib.CONSTS["DV3_GUIDE_OVER"]) == (
        guided_ref.NEGATIVE, guided_ref.EMPTY, guided_ref.OVER)
    assert _lib.CONSTS["DV3_ABI_VERSION"] == 50

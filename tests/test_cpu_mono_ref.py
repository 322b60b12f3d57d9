# coding: utf-8
"""No GPU: the monotonic-search reference (tests/mono_ref.py, what tests/test_gpu_mono_path.py holds the kernels to)
against an enumeration of every admissible path and on hand-worked ties, the C header's declarations, the off-by-default
keywords of the synthesis entry points and the arithmetic of the token spans."""
import itertools
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tests import mono_ref as MR  # noqa: E402


def _softmax_rows(rng, T, N):
    x = rng.randn(T, N) * 2.0
    e = np.exp(x - x.max(axis=1, keepdims=True))
    return e / e.sum(axis=1, keepdims=True)


def _all_paths(T, N, J):
    """every path the three rules admit, by enumerating the advances"""
    out = []
    for first in range(min(J, N)):
        for adv in itertools.product(range(J + 1), repeat=T - 1):
            p = [first]
            for a in adv:
                p.append(p[-1] + a)
            if p[-1] < N and p[-1] >= N - J:
                out.append(p)
    return out


# ----------------------------------------------------------------------------------------------------------------------
# 1. the reference against brute force
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("J", [1, 2, 3])
def test_reference_is_the_maximum_over_every_admissible_path(J):
    rng = np.random.RandomState(10 + J)
    n_infeasible = 0
    for T in range(1, 7):
        for N in range(1, 6):
            s = MR.scores(_softmax_rows(rng, T, N))
            paths = _all_paths(T, N, J)
            for p in paths:
                assert MR.path_ok(p, T, N, J), (T, N, J, p)
            r = MR.search(s, J)
            assert r["feasible"] == (1 if paths else 0), (T, N, J)
            assert (r["steps"], r["keys"]) == (T, N)
            if not paths:
                n_infeasible += 1
                assert r["score"] == 0.0 and r["path"] == [] and r["durations"] == [0] * N
                assert r["skipped_keys"] == 0 and r["longest"] == 0
                assert N > (T + 1) * J - 1
                continue
            best = max(MR.path_score(s, p) for p in paths)
            assert abs(r["score"] - best) <= 1e-12 * (abs(best) + 1.0), (T, N, J)
            assert MR.path_ok(r["path"], T, N, J)
            assert abs(MR.path_score(s, r["path"]) - r["score"]) <= 1e-12 * (abs(best) + 1.0)
            assert sum(r["durations"]) == T
            assert r["durations"] == [r["path"].count(n) for n in range(N)]
            assert r["skipped_keys"] == r["durations"].count(0) and r["longest"] == max(r["durations"])
    assert (n_infeasible > 0) == (J < 3)         # N <= 5 <= (T + 1) 3 - 1: with J = 3 every one of these shapes has a path


def test_path_ok_refuses_what_breaks_a_rule():
    assert MR.path_ok([0, 0, 1, 2], 4, 3, 1)
    assert not MR.path_ok([1, 1, 2, 2], 4, 3, 1)             # starts past key J - 1
    assert MR.path_ok([1, 1, 2, 2], 4, 3, 2)
    assert not MR.path_ok([0, 0, 1, 1], 4, 3, 1)             # ends before key N - J
    assert MR.path_ok([0, 0, 1, 1], 4, 3, 2)
    assert not MR.path_ok([0, 2, 2, 2], 4, 3, 1)             # advances by more than J
    assert not MR.path_ok([0, 1, 0, 2], 4, 3, 2)             # goes back
    assert not MR.path_ok([0, 1, 2], 4, 3, 1) and not MR.path_ok([0, 1, 3], 3, 3, 1) and not MR.path_ok([], 0, 1, 1)


def test_ties_uniform_rows_by_hand():
    """Uniform rows: every admissible path has the same score, the tie-break alone decides.  The smallest advance wins at
    every cell, so walking back from the end the path stays on a key for as long as the cell can still be reached by
    staying: the advances are taken as EARLY as possible.  T = 5, N = 3, J = 1: back from key 2 at step 4, staying is
    possible down to step 2 (key 2 is first reachable there), and so on: 0 1 2 2 2."""
    s = MR.scores(np.full((5, 3), 1.0 / 3.0))
    r = MR.search(s, 1)
    assert r["path"] == [0, 1, 2, 2, 2] and r["durations"] == [1, 1, 3]
    assert (r["feasible"], r["skipped_keys"], r["longest"]) == (1, 0, 3)
    # J = 2: the end keys 2 and 1 tie -> key 2, tried first; key 2 is first reachable at step 1 (from key 0 by 2, or from
    # key 1 by 1 -> the advance 1 wins, from key 1 at step 0)
    r = MR.search(s, 2)
    assert r["path"] == [1, 2, 2, 2, 2] and r["durations"] == [0, 1, 4] and r["skipped_keys"] == 1


def test_end_key_and_advance_ties_by_hand():
    """two steps, three keys, J = 2; p chosen so that the scores are exact in float64 (powers of two)"""
    p = np.array([[0.5, 0.25, 0.0], [0.0, 0.25, 0.5]])        # s = log p; zeros are floored: never chosen
    r = MR.search(MR.scores(p), 2)
    # Q[0] = log .5, log .25, unreachable.  Q[1, 2] = log .5 + max(Q[0,1] (j=1), Q[0,0] (j=2)) -> j = 2 strictly greater;
    # Q[1, 1] = log .25 + max(Q[0,1] (j=0), Q[0,0] (j=1)) -> j = 1 strictly greater.  End: key 2 = 2 log .5 first,
    # key 1 = log .25 + log .5 is smaller: key 2.
    assert r["path"] == [0, 2] and r["score"] == 2.0 * np.log(0.5)
    assert r["durations"] == [1, 0, 1] and r["skipped_keys"] == 1 and r["longest"] == 1
    # the same score through two end keys: the larger key keeps the tie
    p = np.array([[0.5, 0.5, 0.0], [0.0, 0.5, 0.5]])
    assert MR.search(MR.scores(p), 2)["path"] == [1, 2]       # Q[1,2]: j = 1 from key 1 ties j = 2 from key 0 -> j = 1
    # NaN scores as the floor, and the layer mean is taken first
    two = np.stack([np.array([[0.25, 0.75]]), np.array([[0.75, np.nan]])])
    s = MR.scores(two)
    assert s[0, 0] == np.log(0.5) and s[0, 1] == np.log(MR.FLOOR)
    assert MR.FLOOR == float(np.float32(1e-20))


# ----------------------------------------------------------------------------------------------------------------------
# 2. the header
# ----------------------------------------------------------------------------------------------------------------------
def test_header_declares_the_entry_points():
    import ctypes
    from deepvoice3_pytorch_amd import _lib, synthesis
    assert _lib.CONSTS["DV3_ABI_VERSION"] == 50
    assert _lib.CONSTS["DV3_MONO_COLS"] == 6 == len(synthesis.TIMING_COLUMNS) == len(MR.COLUMNS)
    assert synthesis.TIMING_COLUMNS == MR.COLUMNS
    assert _lib.CONSTS["DV3_MONO_MAX_T"] == 8192 and _lib.CONSTS["DV3_MONO_MAX_TK"] == 2048
    assert _lib.CONSTS["DV3_MONO_MAX_ADVANCE"] == 8 == MR.MAX_ADVANCE
    assert _lib.CONSTS["DV3_MONO_FLOOR"] == 1e-20
    i32, ptr = ctypes.c_int32, ctypes.c_void_p
    assert _lib.FUNCS["dv3_mono_path_f32"] == (ctypes.c_int, [ptr, ptr])
    assert _lib.FUNCS["dv3_mono_path_scratch_bytes"] == (ctypes.c_int, [i32, i32, i32, ptr])
    fields = dict(_lib.STRUCT_FIELDS["dv3_mono_desc"])
    for name in ("attn", "steps", "key_len", "out", "path", "durations", "scratch"):
        assert fields[name] is ptr, name
    for name in ("layer_stride", "item_stride", "step_stride", "scratch_bytes"):
        assert fields[name] is ctypes.c_int64, name
    for name in ("n_layers", "B", "T", "Tk", "max_advance"):
        assert fields[name] is i32, name
    assert len(fields) == 16
    api = open(os.path.join(ROOT, "deepvoice3_pytorch_amd", "csrc", "api.hip")).read()
    assert "DV3_SZ(dv3_mono_desc)" in api                            # registered with dv3_sizeof (test_cpu_host walks them)
    mk = open(os.path.join(ROOT, "deepvoice3_pytorch_amd", "csrc", "Makefile")).read()
    assert "mono_path.hip" in mk
    text = open(os.path.join(ROOT, "include", "dv3hip.h")).read()
    doc = text[text.index("Monotonic alignment search"):text.index("int dv3_mono_path_f32")]
    assert "version stays 49" in " ".join(doc.split()).replace("* ", "")
    for name in synthesis.TIMING_COLUMNS:
        assert name in doc, name
    # an integer constant is still an int, and the float one did not leak in as its leading digit
    assert isinstance(_lib.CONSTS["DV3_MONO_COLS"], int) and isinstance(_lib.CONSTS["DV3_DTW_MAX_T"], int)


# ----------------------------------------------------------------------------------------------------------------------
# 3. defaults and host logic
# ----------------------------------------------------------------------------------------------------------------------
def test_defaults_are_off():
    import inspect
    from deepvoice3_pytorch_amd import synthesis, train_step
    for fn in (synthesis.tts_batch, synthesis.tts_stream, synthesis.RollingSynthesizer.__init__):
        p = inspect.signature(fn).parameters
        assert p["timings"].default is False and p["timing_advance"].default == 1, fn
    p = inspect.signature(synthesis.token_timings).parameters
    assert list(p) == ["alignments", "steps", "lengths", "seconds_per_step", "layout", "max_advance"]
    assert p["layout"].default == "btk" and p["max_advance"].default == 1
    p = inspect.signature(train_step.align_batch).parameters
    assert list(p) == ["trainer", "batch", "max_advance", "averaged"]
    assert p["max_advance"].default == 1 and p["averaged"].default is False
    from deepvoice3_pytorch_amd import ops
    p = inspect.signature(ops.monotonic_path).parameters
    assert list(p) == ["attn", "steps", "key_len", "layout", "max_advance"]
    assert p["layout"].default == "btk" and p["max_advance"].default == 1


def test_token_spans_on_hand_made_durations():
    import torch
    from deepvoice3_pytorch_amd import audio, synthesis
    sps = synthesis.seconds_per_step(None, 4, 4)                       # r = 4 frames of 4 hops of 256 samples at 22050 Hz
    assert sps == 4 * 4 * 256 / 22050.0
    assert synthesis.seconds_per_step(audio.AudioConfig(fft_size=512, hop_size=128, sample_rate=16000), 1, 4) == 512 / 16000.0
    dur = torch.tensor([[2, 0, 3, 1, 0], [0, 0, 0, 0, 0]], dtype=torch.int32)
    start, end = synthesis.token_spans(dur, sps)
    assert start.dtype == torch.float64 and start.shape == dur.shape
    assert start[0].tolist() == [0.0, 2 * sps, 2 * sps, 5 * sps, 6 * sps]
    assert end[0].tolist() == [2 * sps, 2 * sps, 5 * sps, 6 * sps, 6 * sps]
    assert end[0, -1].item() == 6 * sps                                # steps x seconds_per_step, exactly
    assert start[1].tolist() == [0.0] * 5 and end[1].tolist() == [0.0] * 5
    # a skipped token has an empty span at the start of the next one; spans tile the utterance
    assert torch.equal(start[0, 1:], end[0, :-1])
    for n in range(5):
        assert abs(end[0, n].item() - (start[0, n].item() + sps * int(dur[0, n]))) <= 1e-15


def test_token_timings_refuses_the_cpu():
    import torch
    from deepvoice3_pytorch_amd import synthesis
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        synthesis.token_timings(torch.rand(1, 3, 2), [3], [2], 0.01)

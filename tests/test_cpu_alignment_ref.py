# coding: utf-8
"""No GPU: the alignment statistics' definitions on hand-worked matrices -- tests/alignment_ref.py is
what tests/test_gpu_alignment.py holds the kernel to, so it is itself held to values written out by hand --, the
end-of-text stop's step count, the host-side flags, and the C header's declarations."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tests import alignment_ref as AR  # noqa: E402

NAN = float("nan")


def one_hot_rows(path, n_keys, Tk, hi, lo):
    """rows with `hi` on path[t] and `lo` on the item's other keys; NaN past the item's keys"""
    a = np.full((len(path), Tk), NAN, dtype=np.float32)
    a[:, :n_keys] = lo
    for t, p in enumerate(path):
        a[t, p] = hi
    return a


def row(steps, keys, focus_mean, focus_min, last_key, furthest_key, end_step, tail_steps, covered_keys, back_steps,
        max_jump, longest_stall, bad_rows):
    return dict(zip(AR.COLUMNS, (steps, keys, focus_mean, focus_min, last_key, furthest_key, end_step, tail_steps,
                                 covered_keys, back_steps, max_jump, longest_stall, bad_rows)))


# name -> (attn, steps, key_len, the 13 expected values); all probabilities are dyadic, so the focus columns are exact
CASES = {
    # 0.625 on the diagonal, 0.125 on the three other keys: every row sums to 1
    "diagonal": (one_hot_rows([0, 1, 2, 3], 4, 4, 0.625, 0.125), 4, 4,
                 row(4, 4, 0.625, 0.625, 3, 3, 3, 0, 4, 0, 1, 1, 0)),
    # path 0 1 0 2 1: back at t = 2 and t = 4, never on key 3
    "regress": (one_hot_rows([0, 1, 0, 2, 1], 4, 4, 0.625, 0.125), 5, 4,
                row(5, 4, 0.625, 0.625, 1, 2, -1, 0, 3, 2, 2, 1, 0)),
    # 6 of 8 keys are the item's; 0.375 + 5 * 0.125 = 1; path 0 1 5 5 jumps by 4 and ends at t = 2
    "jump": (one_hot_rows([0, 1, 5, 5], 6, 8, 0.375, 0.125), 4, 6,
             row(4, 6, 0.375, 0.375, 5, 5, 2, 1, 3, 0, 4, 2, 0)),
    # reaches the last key at t = 2 and stays: rows 0-2 peak 0.5, rows 3-5 peak 0.75
    "stall": (np.concatenate([one_hot_rows([0, 1, 2], 3, 3, 0.5, 0.25), one_hot_rows([2, 2, 2], 3, 3, 0.75, 0.125)]), 6, 3,
              row(6, 3, 0.625, 0.5, 2, 2, 2, 3, 3, 0, 1, 4, 0)),
    # no steps: nothing is read (the matrix is all NaN)
    "no_steps": (np.full((3, 4), NAN, dtype=np.float32), 0, 2,
                 row(0, 2, 0.0, 0.0, 0, 0, -1, 0, 0, 0, 0, 0, 0)),
    # one key (key_len 0 is clamped to 1, steps 7 to the 3 rows): the end is reached at once
    "one_key": (one_hot_rows([0, 0, 0], 1, 4, 1.0, 0.0), 7, 0,
                row(3, 1, 1.0, 1.0, 0, 0, 0, 2, 1, 0, 0, 3, 0)),
    # exact ties go to the first maximum: keys 1 = 2 -> 1; all four equal -> 0
    "tie": (np.array([[0.25, 0.375, 0.375, 0.0], [0.25, 0.25, 0.25, 0.25]], dtype=np.float32), 2, 4,
            row(2, 4, 0.3125, 0.25, 0, 1, -1, 0, 2, 1, 1, 1, 0)),
    # the middle row holds a NaN: bad, path 0, peak 0
    "nan_row": (np.array([[0.125, 0.125, 0.75], [NAN, 0.5, 0.5], [0.25, 0.5, 0.25]], dtype=np.float32), 3, 3,
                row(3, 3, 1.25 / 3, 0.0, 1, 2, 0, 2, 3, 1, 2, 1, 1)),
}


@pytest.mark.parametrize("name", sorted(CASES))
def test_reference_on_hand_worked_matrices(name):
    attn, steps, key_len, want = CASES[name]
    got = AR.item_stats(attn, steps, key_len)
    assert tuple(got) == AR.COLUMNS
    for k in AR.COLUMNS:
        if k.startswith("focus"):
            assert got[k] == pytest.approx(want[k], rel=1e-12, abs=0), (name, k)
        else:
            assert got[k] == want[k] and isinstance(got[k], int), (name, k, got[k], want[k])


def test_reference_reads_both_layouts():
    names = ["diagonal", "regress"]                   # both 4 keys wide
    T = max(CASES[n][0].shape[0] for n in names)
    btk = np.full((2, T, 4), NAN, dtype=np.float32)
    for b, n in enumerate(names):
        btk[b, :CASES[n][0].shape[0]] = CASES[n][0]
    steps, keys = [CASES[n][1] for n in names], [CASES[n][2] for n in names]
    want = [CASES[n][3] for n in names]
    assert AR.batch_stats(btk, steps, keys) == want
    assert AR.batch_stats(np.ascontiguousarray(btk.transpose(1, 0, 2)), steps, keys, layout="tbk") == want


def test_stall_stop_table():
    from deepvoice3_pytorch_amd.decode_program import stall_stop
    table = [  # (end_step, stall_limit, min_steps) -> steps
        ((-1, 3, 0), 0),           # the end was never reached: the item runs on
        ((-1, 3, 10), 0),
        ((0, 3, 0), 4),            # reached at the first step: that step and three more
        ((5, 0, 0), 6),
        ((5, 3, 0), 9),
        ((2, 3, 5), 6),            # both bounds meet
        ((2, 3, 10), 11),          # min_steps dominates: the done flag's rule allows a stop after step 11 at the earliest
        ((199, 8, 0), 208),
    ]
    for args, want in table:
        assert stall_stop(*args) == want, args
    with pytest.raises(ValueError, match="stall_limit"):
        stall_stop(3, -1, 0)


def test_alignment_flags():
    from deepvoice3_pytorch_amd import synthesis
    L = synthesis.AlignmentLimits
    assert tuple(L()) == (1, 2, 3, 8, 0.3) and L._fields == ("end_tolerance", "back_steps", "max_jump", "stall", "focus")
    assert synthesis.ALIGNMENT_COLUMNS == AR.COLUMNS
    want = {  # with the default limits
        "diagonal": (), "regress": (), "jump": ("skipped",), "stall": (), "no_steps": ("unfocused",), "one_key": (),
        "tie": ("incomplete",), "nan_row": ("bad_rows",),
    }
    for name, flags in want.items():
        r = CASES[name][3]
        assert synthesis.alignment_flags(r) == flags, name
        assert synthesis.alignment_flags([r[k] for k in AR.COLUMNS]) == flags, name        # the 13 values in order
    diag, regress, stall = CASES["diagonal"][3], CASES["regress"][3], CASES["stall"][3]
    assert synthesis.alignment_flags(diag, max_steps=3) == ("capped",)                      # 4 steps = max_steps + 1
    assert synthesis.alignment_flags(diag, max_steps=4) == ()
    assert synthesis.alignment_flags(regress, limits=L(back_steps=1)) == ("regressed",)
    assert synthesis.alignment_flags(regress, limits=L(end_tolerance=0)) == ("incomplete",)     # furthest 2 < 4 - 1 - 0
    assert synthesis.alignment_flags(stall, limits=L(stall=3)) == ("stalled",)
    assert synthesis.alignment_flags(stall, limits=L(focus=0.7)) == ("unfocused",)
    everything = row(12, 30, 0.1, 0.0, 3, 9, -1, 0, 4, 5, 6, 9, 2)
    assert synthesis.alignment_flags(everything, max_steps=11) == (
        "bad_rows", "capped", "incomplete", "regressed", "skipped", "stalled", "unfocused")
    # a result row as diagnostics=True returns it (with its own "flags" entry) is taken as it is
    assert synthesis.alignment_flags(dict(CASES["jump"][3], flags=("skipped",))) == ("skipped",)


def test_header_declares_the_entry_points():
    import ctypes
    from deepvoice3_pytorch_amd import _lib, synthesis
    assert _lib.CONSTS["DV3_ABI_VERSION"] == 50
    assert _lib.CONSTS["DV3_ALIGN_COLS"] == 13 == len(synthesis.ALIGNMENT_COLUMNS)
    i32, i64, ptr = ctypes.c_int32, ctypes.c_int64, ctypes.c_void_p
    assert _lib.FUNCS["dv3_alignment_stats_scratch_bytes"] == (ctypes.c_int, [i32, i32])
    assert _lib.FUNCS["dv3_alignment_stats_f32"] == (ctypes.c_int, [ptr, i64, i64, i32, i32, i32, ptr, ptr, ptr, ptr, ptr])
    text = open(os.path.join(ROOT, "include", "dv3hip.h")).read()
    doc = text[text.index("Alignment diagnostics"):text.index("int dv3_alignment_stats_f32")]
    assert "deepvoice3.py:445" in doc
    for name in synthesis.ALIGNMENT_COLUMNS:
        assert name in doc, name
    mk = open(os.path.join(ROOT, "deepvoice3_pytorch_amd", "csrc", "Makefile")).read()
    assert "alignment.hip" in mk


def test_defaults_are_off():
    import inspect
    import deepvoice3_pytorch_amd as pkg
    from deepvoice3_pytorch_amd import synthesis
    for fn in (synthesis.tts_batch, synthesis.tts_stream, synthesis.RollingSynthesizer.__init__):
        p = inspect.signature(fn).parameters
        assert p["diagnostics"].default is False and p["stall_limit"].default is None, fn
    assert inspect.signature(pkg.MultiSpeakerTTSModel.synthesize_batch).parameters["stall_limit"].default is None

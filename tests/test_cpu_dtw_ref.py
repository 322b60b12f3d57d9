# coding: utf-8
"""No GPU: the DTW reference (tests/dtw_ref.py, what tests/test_gpu_dtw.py holds the kernels to) on hand-worked cases,
the scale of the mel-cepstral features through the Parseval identity, the C header's declarations, and the arithmetic
of SynthEvalTotals."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tests import dtw_ref as DR  # noqa: E402


def _figures(r):
    return tuple(r[k] for k in DR.COLUMNS)


# ----------------------------------------------------------------------------------------------------------------------
# 1. the reference on hand-worked cases
# ----------------------------------------------------------------------------------------------------------------------
def test_identical_sequences_give_the_diagonal():
    x = np.array([[0.0, 1.0], [2.0, -1.0], [5.0, 5.0], [5.5, 4.0], [-3.0, 0.25]])
    r = DR.dtw(x, x.copy())
    assert _figures(r) == (0.0, 5, 4, 0, 0)
    assert r["path"] == [(i, i) for i in range(5)]


def test_doubled_frames_n3_by_hand():
    """x = 0 1 3, y = 0 0 1 1 3 3.  d and C (rows i, columns j), worked by hand:
         d  0 0 1 1 3 3      C  0 0 1 2 5 8
            1 1 0 0 2 2         1 1 0 0 2 4
            3 3 2 2 0 0         4 4 2 2 0 0
    C(1,1): diagonal 0 = up 0 -> diagonal.  C(1,3): left 0 < diagonal 1 -> left.  C(2,3): diagonal 0 = up 0 -> diagonal.
    C(2,5): left 0 < diagonal 2 -> left.  Back from (2,5): left, diagonal, left, diagonal, then row 0 goes left."""
    x = np.array([[0.0], [1.0], [3.0]])
    y = np.repeat(x, 2, axis=0)
    r = DR.dtw(x, y)
    assert _figures(r) == (0.0, 6, 2, 0, 3)
    assert r["path"] == [(0, 0), (0, 1), (1, 2), (1, 3), (2, 4), (2, 5)]
    # and the other way round: the doubled sequence as x
    r = DR.dtw(y, x)
    assert _figures(r) == (0.0, 6, 2, 3, 0)
    assert r["path"] == [(0, 0), (1, 0), (2, 1), (3, 1), (4, 2), (5, 2)]


@pytest.mark.parametrize("n", [1, 2, 7])
def test_doubled_frames_any_n(n):
    x = np.cumsum(np.arange(1, n + 1, dtype=np.float64))[:, None]         # distinct frames
    r = DR.dtw(x, np.repeat(x, 2, axis=0))
    assert _figures(r) == (0.0, 2 * n, n - 1, 0, n)


def test_single_frames():
    r = DR.dtw([[3.0, 4.0]], [[0.0, 0.0]])
    assert _figures(r) == (5.0, 1, 0, 0, 0) and r["path"] == [(0, 0)]
    x = [[1.0]]
    y = [[1.0], [3.0], [0.0], [1.5]]                     # distances 0 2 1 0.5
    r = DR.dtw(x, y)
    assert _figures(r) == (3.5, 4, 0, 0, 3) and r["path"] == [(0, j) for j in range(4)]
    r = DR.dtw(y, x)
    assert _figures(r) == (3.5, 4, 0, 3, 0) and r["path"] == [(i, 0) for i in range(4)]
    assert _figures(DR.dtw(np.zeros((0, 2)), np.zeros((3, 2)))) == (0.0, 0, 0, 0, 0)


def test_three_way_tie_3x4_by_hand():
    """     d  1 0 9 9      C  1  1 10 19
               0 1 9 9         1  2 10 19
               9 9 1 1        10 10  3  4
    C(1,1): diagonal, up and left are all 1 -> the diagonal (from (0,0)).  C(1,3): diagonal 10 = left 10 -> diagonal.
    C(2,2): diagonal 2.  C(2,3): left 3 < diagonal 10 -> left.  Back from (2,3): left, diagonal, diagonal.  Under any
    other order the path would leave (1,1) through (0,1) or (1,0) and be one cell longer."""
    d = np.array([[1.0, 0.0, 9.0, 9.0], [0.0, 1.0, 9.0, 9.0], [9.0, 9.0, 1.0, 1.0]])
    r = DR.dtw_from_distances(d)
    assert _figures(r) == (4.0, 4, 2, 0, 1)
    assert r["path"] == [(0, 0), (1, 1), (2, 2), (2, 3)]
    assert DR.path_cost(d, r["path"]) == 4.0


def test_counts_identities_on_random_input():
    rng = np.random.RandomState(0)
    for Lx, Ly in ((1, 5), (6, 1), (9, 14), (20, 11)):
        x, y = rng.randn(Lx, 3), rng.randn(Ly, 3)
        r = DR.dtw(x, y)
        assert r["path_len"] == 1 + r["n_diag"] + r["n_x_only"] + r["n_y_only"] == len(r["path"])
        assert r["n_diag"] + r["n_x_only"] == Lx - 1 and r["n_diag"] + r["n_y_only"] == Ly - 1
        assert r["path"][0] == (0, 0) and r["path"][-1] == (Lx - 1, Ly - 1)
        assert abs(DR.path_cost(DR.distances(x, y), r["path"]) - r["cost"]) <= 1e-12 * r["cost"]


# ----------------------------------------------------------------------------------------------------------------------
# 2. the scale of the features
# ----------------------------------------------------------------------------------------------------------------------
def _parseval(delta_db):
    """With every cepstrum but c0 kept (order = M - 1) the squared feature distance of two frames is the mean-removed
    mean square of their dB difference over FOUR: the cosines of one k have mean square 1/2 over the M bands, so
    sum_k>=1 (sum_m v_m cos)^2 = (M / 2) (sum v^2 - (sum v)^2 / M), and the features carry 1 / (sqrt 2 M).  The quarter
    is the definition's own: MCD = (10 / ln 10) sqrt(2 sum dc^2) with ln a = c0 + 2 sum c_k cos gives
    MCD = (10 / ln 10) rms(d ln a - mean) = rms(d dB - mean) / 2."""
    return 0.25 * ((delta_db ** 2).mean(axis=-1) - delta_db.mean(axis=-1) ** 2)


@pytest.mark.parametrize("M", [80, 20, 7])
def test_parseval_pins_the_reference_scale(M):
    rng = np.random.RandomState(M)
    a, b = rng.uniform(0, 1, (6, M)), rng.uniform(0, 1, (6, M))
    fa, fb = DR.mel_cepstra(a, -100.0, M - 1), DR.mel_cepstra(b, -100.0, M - 1)
    got = ((fa - fb) ** 2).sum(axis=-1)
    want = _parseval((a - b) * 100.0)
    assert np.all(np.abs(got - want) <= 1e-10 * want), (got, want)
    # a lower order is the same numbers, cut
    n = min(13, M - 1)
    assert np.array_equal(DR.mel_cepstra(a, -100.0, n), fa[:, :n])


def test_parseval_pins_audio_mel_cepstra():
    import torch
    from deepvoice3_pytorch_amd import audio
    M = 80
    rng = np.random.RandomState(1)
    a, b = rng.uniform(0, 1, (2, 3, M)).astype(np.float32), rng.uniform(0, 1, (2, 3, M)).astype(np.float32)
    fa = audio.mel_cepstra(torch.from_numpy(a), order=M - 1).double().numpy()
    fb = audio.mel_cepstra(torch.from_numpy(b), order=M - 1).double().numpy()
    assert fa.shape == (2, 3, M - 1)
    got = ((fa - fb) ** 2).sum(axis=-1)
    want = _parseval((a.astype(np.float64) - b.astype(np.float64)) * 100.0)
    assert np.all(np.abs(got - want) <= 1e-5 * want), (got, want)
    # against the reference, element-wise.  The worst case of an fp32 dot of M terms: the dB value, the table entry and
    # the product round once each, the sum M - 1 times -- (M + 2) half-ulps of sum_m |dB_m t_m| <= 100 / sqrt 2
    f13 = audio.mel_cepstra(torch.from_numpy(a)).double().numpy()
    assert f13.shape == (2, 3, 13)
    assert np.abs(f13 - DR.mel_cepstra(a, -100.0, 13)).max() <= (M + 2) * 2.0 ** -24 * 100.0 / np.sqrt(2.0)
    # another floor, values outside [0, 1] clipped
    cfg = audio.AudioConfig(min_level_db=-80)
    wild = a * 1.5 - 0.25
    got = audio.mel_cepstra(torch.from_numpy(wild), cfg, 5).double().numpy()
    assert np.abs(got - DR.mel_cepstra(wild, -80.0, 5)).max() <= 1e-4
    for order in (0, M, -1):
        with pytest.raises(ValueError, match="order"):
            audio.mel_cepstra(torch.from_numpy(a), order=order)


# ----------------------------------------------------------------------------------------------------------------------
# 3. the header
# ----------------------------------------------------------------------------------------------------------------------
def test_header_declares_the_entry_points():
    import ctypes
    from deepvoice3_pytorch_amd import _lib
    assert _lib.CONSTS["DV3_ABI_VERSION"] == 50
    assert _lib.CONSTS["DV3_DTW_COLS"] == 5 == len(DR.COLUMNS)
    assert _lib.CONSTS["DV3_DTW_MAX_T"] == 4096 and _lib.CONSTS["DV3_DTW_MAX_D"] == 128
    i32, ptr = ctypes.c_int32, ctypes.c_void_p
    assert _lib.FUNCS["dv3_dtw_f32"] == (ctypes.c_int, [ptr, ptr])
    assert _lib.FUNCS["dv3_dtw_scratch_bytes"] == (ctypes.c_int, [i32, i32, i32, i32, ptr])
    fields = dict(_lib.STRUCT_FIELDS["dv3_dtw_desc"])
    for name in ("x", "y", "x_len", "y_len", "out", "path", "scratch"):
        assert fields[name] is ptr, name
    for name in ("x_batch_stride", "x_time_stride", "y_batch_stride", "y_time_stride", "scratch_bytes"):
        assert fields[name] is ctypes.c_int64, name
    for name in ("B", "Tx", "Ty", "D"):
        assert fields[name] is i32, name
    api = open(os.path.join(ROOT, "deepvoice3_pytorch_amd", "csrc", "api.hip")).read()
    assert "DV3_SZ(dv3_dtw_desc)" in api                             # registered with dv3_sizeof (test_cpu_host walks them)
    mk = open(os.path.join(ROOT, "deepvoice3_pytorch_amd", "csrc", "Makefile")).read()
    assert "dtw.hip" in mk


# ----------------------------------------------------------------------------------------------------------------------
# 4. SynthEvalTotals
# ----------------------------------------------------------------------------------------------------------------------
def test_totals_do_not_depend_on_the_batching():
    import torch
    from deepvoice3_pytorch_amd import synthesis
    assert synthesis.SYNTH_EVAL_COLUMNS == ("mcd_sum", "path_len", "n_diag", "n_synth_only", "n_target_only",
                                            "frames_synth", "frames_target")
    rows = torch.tensor([[30.5, 12.0, 7.0, 1.0, 3.0, 9.0, 11.0],
                         [0.1, 3.0, 1.0, 0.0, 1.0, 2.0, 3.0],
                         [812.25, 150.0, 90.0, 49.0, 10.0, 140.0, 101.0]], dtype=torch.float32)
    one = synthesis.SynthEvalTotals()
    one.add(rows, ids=["a", "b", "c"])
    split = synthesis.SynthEvalTotals()
    split.add(rows[:1], ids=["a"])
    split.add(rows[1:], ids=["b", "c"])
    r1, r2 = one.result(), split.result()
    assert r1 == r2
    assert r1["n_items"] == 3 and [it["id"] for it in r1["items"]] == ["a", "b", "c"]
    mcd_sum = float(np.float32(30.5)) + float(np.float32(0.1)) + float(np.float32(812.25))
    assert r1["mcd"] == mcd_sum / 165.0
    assert r1["duration_ratio"] == 151.0 / 115.0
    assert r1["items"][2]["mcd"] == 812.25 / 150.0 and r1["items"][2]["duration_ratio"] == 140.0 / 101.0
    assert r1["items"][0]["path_len"] == 12 and isinstance(r1["items"][0]["path_len"], int)
    worst = max(r1["items"], key=lambda it: it["mcd"])
    assert worst["id"] == "c"
    with pytest.raises(ValueError):
        synthesis.SynthEvalTotals().result()
    with pytest.raises(ValueError):
        one.add(rows[:, :5])
    with pytest.raises(ValueError):
        one.add(rows)                                # ids for every batch or for none

# coding: utf-8
"""No GPU: training health -- the option and the declarations it needs, the host-built chunk table of
the per-tensor statistics, and the float64 reference tests/test_gpu_health.py holds the kernels to (tests/health_ref.py)
on an arena worked by hand."""
import ctypes
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tests import health_ref as H  # noqa: E402

SIZES = [1, 3, 4, 5, 1027, 4096, 4097, 3 * 4096 + 5, 70000]


def _layout(sizes):
    """FlatArena's: every tensor starts on a multiple of 4 elements"""
    offs, total = [], 0
    for n in sizes:
        offs.append(total)
        total += (n + 3) // 4 * 4
    return offs, total


# ----------------------------------------------------------------------------------------------------------------------
# 1. the option, the constants, the symbols
# ----------------------------------------------------------------------------------------------------------------------
def test_the_option_is_accepted_and_off_by_default():
    from deepvoice3_pytorch_amd import train_step
    assert train_step.TrainConfig().skip_nonfinite is False
    assert train_step.TrainConfig(skip_nonfinite=True).skip_nonfinite is True
    assert train_step.TrainConfig(skip_nonfinite=1, ema_decay=0.9).skip_nonfinite is True


def test_the_columns_are_named_once():
    from deepvoice3_pytorch_amd import _lib, train_step
    assert len(train_step.TENSOR_STAT_COLUMNS) == _lib.CONSTS["DV3_TENSOR_STAT_COLS"] == 6
    assert tuple(train_step.TENSOR_STAT_COLUMNS) == H.COLUMNS
    assert _lib.CONSTS["DV3_ARENA_CHUNK_MAX"] == 4096


def test_the_library_exports_the_entry_points_under_the_same_abi():
    from deepvoice3_pytorch_amd import _lib
    assert _lib.CONSTS["DV3_ABI_VERSION"] == 50
    f, i32, i64, ptr = ctypes.c_float, ctypes.c_int32, ctypes.c_int64, ctypes.c_void_p
    tail = [ptr, f, ptr, f, f, f, f, f]                    # grad_norm, clip, hyper, beta1, beta2, eps, wd, prescale
    assert _lib.FUNCS["dv3_clip_adam_f32"] == (ctypes.c_int, [ptr] * 4 + [i64] + tail + [ptr])
    assert _lib.FUNCS["dv3_clip_adam_guard_f32"] == (ctypes.c_int, [ptr] * 4 + [i64] + tail + [ptr, ptr])
    assert _lib.FUNCS["dv3_clip_adam_ema_f32"] == (ctypes.c_int, [ptr] * 5 + [i64] + tail + [ptr])
    assert _lib.FUNCS["dv3_clip_adam_ema_guard_f32"] == (ctypes.c_int, [ptr] * 5 + [i64] + tail + [ptr, ptr])
    assert _lib.FUNCS["dv3_arena_stats_f32"] == (ctypes.c_int, [ptr] * 4 + [i64, ptr, ptr, ptr, i64, ptr, i32, f, f,
                                                                   ptr, ptr, ptr])
    h = _lib.lib()                                         # (raises when a declared symbol is missing)
    assert h.dv3_abi_version() == 50
    for name in ("dv3_clip_adam_guard_f32", "dv3_clip_adam_ema_guard_f32", "dv3_arena_stats_f32"):
        assert getattr(h, name) is not None
    mk = open(os.path.join(ROOT, "deepvoice3_pytorch_amd", "csrc", "Makefile")).read()
    assert "arena_stats.hip" in mk


def test_the_wrappers_take_a_health_buffer():
    import inspect
    from deepvoice3_pytorch_amd import ops, train_step
    for fn in (ops.clip_adam, ops.clip_adam_ema):
        assert inspect.signature(fn).parameters["health"].default is None
    sig = inspect.signature(ops.arena_stats)
    assert list(sig.parameters)[:9] == ["p", "g", "m", "v", "hyper", "health", "chunks", "ranges", "grad_prescale"]
    assert sig.parameters["grad_prescale"].default == 1.0
    for cls in (train_step.Trainer, train_step.GraphedTrainer, train_step.LatticeReplay):
        assert callable(cls.health) and callable(cls.tensor_stats)


# ----------------------------------------------------------------------------------------------------------------------
# 2. the chunk table
# ----------------------------------------------------------------------------------------------------------------------
def test_arena_chunks_cover_every_tensor_element_once_and_no_padding():
    from deepvoice3_pytorch_amd import train_step
    offs, total = _layout(SIZES)
    chunks, ranges = train_step.arena_chunks(offs, SIZES)
    assert chunks.dtype == ranges.dtype and str(chunks.dtype) == "torch.int64"
    assert chunks.is_contiguous() and ranges.is_contiguous()
    H.check_chunks(chunks.numpy(), ranges.numpy(), offs, SIZES, total)
    assert chunks.shape[0] == sum(-(-n // 4096) for n in SIZES)
    assert ranges[:, 1].tolist() == [1, 1, 1, 1, 1, 1, 2, 4, 18]
    assert chunks[:, 1].max().item() == 4096 and (chunks[:, 0] % 4 == 0).all()


@pytest.mark.parametrize("chunk", [4, 1024])
def test_arena_chunks_at_other_chunk_lengths(chunk):
    from deepvoice3_pytorch_amd import train_step
    sizes = [1, 3, 4, 5, 1027, 4097]
    offs, total = _layout(sizes)
    chunks, ranges = train_step.arena_chunks(offs, sizes, chunk=chunk)
    H.check_chunks(chunks.numpy(), ranges.numpy(), offs, sizes, total, chunk=chunk)


def test_arena_chunks_refuses_what_the_kernel_cannot_take():
    from deepvoice3_pytorch_amd import train_step
    for offs, sizes, kw in (([0, 5], [5, 3], {}),              # an offset off the 16-byte grid
                            ([0, 4], [5, 3], {}),              # overlap
                            ([0], [0], {}),                    # an empty tensor
                            ([0, 8], [4], {}),                 # lengths that do not match
                            ([0], [4], dict(chunk=8192)),      # longer than a workgroup's chunk
                            ([0], [4], dict(chunk=6))):        # a chunk that would start off the 16-byte grid
        with pytest.raises(ValueError):
            train_step.arena_chunks(offs, sizes, **kw)


def test_the_check_itself_sees_a_bad_table():
    from deepvoice3_pytorch_amd import train_step
    sizes = [5, 4097]
    offs, total = _layout(sizes)
    chunks, ranges = (t.numpy().copy() for t in train_step.arena_chunks(offs, sizes))
    H.check_chunks(chunks, ranges, offs, sizes, total)
    bad = chunks.copy()
    bad[0, 1] = 8                                              # reaches into the padding behind the 5-element tensor
    with pytest.raises(AssertionError):
        H.check_chunks(bad, ranges, offs, sizes, total)
    bad = chunks.copy()
    bad[2, 1] -= 1                                             # leaves the last element out
    with pytest.raises(AssertionError):
        H.check_chunks(bad, ranges, offs, sizes, total)


# ----------------------------------------------------------------------------------------------------------------------
# 3. the reference by hand
# ----------------------------------------------------------------------------------------------------------------------
def test_the_guard_rule():
    assert not H.skips(0.0) and not H.skips(3.0e38) and not H.skips(1e-45)
    assert H.skips(np.nan) and H.skips(np.inf) and H.skips(-np.inf)
    assert H.skips(1e39)                                       # the norm is an fp32 word: past its range it is +Inf
    assert H.norm_f32_overflows([3e19, 3e19]) and not H.norm_f32_overflows([1e19, 1e19])
    assert not H.norm_f32_overflows([np.nan, 1.0])


def test_the_columns_of_a_three_tensor_arena_by_hand():
    nan, inf = np.nan, np.inf
    sizes = [3, 2, 5]
    offs, total = _layout(sizes)
    assert offs == [0, 4, 8] and total == 16
    pad = nan                                                   # (the pads must not be read)
    g = np.array([1, nan, -2, pad, inf, 4, pad, pad, -inf, 8, -16, 0, 2, pad, pad, pad], dtype=np.float32)
    p = np.array([1, 2, -3, pad, 0, -0.5, pad, pad, 1, 1, 1, 1, -2, pad, pad, pad], dtype=np.float32)
    m = np.array([1, 0, -2, pad, 3, 0, pad, pad, 0, 0, 0, 0, 1, pad, pad, pad], dtype=np.float32)
    v = np.array([4, 1, 16, pad, 9, 1, pad, pad, 1, 1, 1, 1, 0, pad, pad, pad], dtype=np.float32)
    hyper = np.array([0.5, 0.25, 2.0], dtype=np.float32)        # step size 2, sqrt(v) / 2
    got = H.columns(p, g, m, v, hyper, offs, sizes, grad_prescale=0.5, eps=1.0)
    # update: 2 * m / (sqrt(v) / 2 + 1):  tensor 0: 2*1/2 = 1, 0, 2*-2/3 = -4/3;  tensor 1: 2*3/2.5 = 2.4, 0;
    # tensor 2: 0, 0, 0, 0, 2*1/1 = 2
    want = np.array([[0.25 + 1.0, 1.0, 1, 14.0, 3.0, 1.0 + 16.0 / 9.0],
                     [4.0, 2.0, 1, 0.25, 0.5, 2.4 ** 2],
                     [16.0 + 64.0 + 0.0 + 1.0, 8.0, 1, 8.0, 2.0, 4.0]])
    assert got.shape == (3, 6) and got.dtype == np.float64
    np.testing.assert_allclose(got, want, rtol=1e-15, atol=0)
    skipped = H.columns(p, g, m, v, hyper, offs, sizes, grad_prescale=0.5, eps=1.0, skipped=True)
    assert (skipped[:, 5] == 0).all() and (skipped[:, :5] == got[:, :5]).all()
    # a tensor whose gradient is non-finite throughout: no finite element, maximum 0
    none = H.columns([1.0], [nan], [0.0], [1.0], hyper, [0], [1])
    assert none[0].tolist() == [0.0, 0.0, 1.0, 1.0, 1.0, 0.0]

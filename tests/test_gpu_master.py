# coding: utf-8
"""-m gpu: deliverable audio (csrc/master.hip; include/dv3hip.h: dv3_wave_levels_f32, dv3_wave_gains_f32,
dv3_wave_master_f32) against the numpy restatement of tests/master_ref.py.

  1. levels: peak and counts exact, the two sums within the bound of fp64 accumulation, every row a function of its own
     item -- alone, in a batch, and at every 4-byte alignment;
  2. gains bit for bit against the float64 restatement, from a host-made level table;
  3. the master launch bit for bit against the float32 restatement in all three modes, with and without dither, the
     footprint under guard bands, two calls bit-equal;
  4. the reference policy against numpy's evaluation of save_wav's formula;
  5. the refusals of the three entry points and of the Python wrapper;
  6. through synthesis: tts_batch, RollingSynthesizer, tts_stream, tts_document and its timings."""
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tests import master_ref as M  # noqa: E402

pytestmark = pytest.mark.gpu

SENTINEL = -7.25


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


def _i64(dev, v):
    return torch.tensor([int(a) for a in v], dtype=torch.int64, device=dev)


# ----------------------------------------------------------------------------------------------------------------------
# 1. levels
# ----------------------------------------------------------------------------------------------------------------------
LEVEL_LENGTHS = (0, 1, 63, 4097, 40000, 5001, 777)


def _level_items():
    """the lengths of the issue, then an item with a NaN and infinities and an item with samples at exactly +-1"""
    rng = np.random.RandomState(11)
    items = [(rng.randn(n) * 0.3).astype(np.float32) for n in LEVEL_LENGTHS]
    items[5][[3, 2500, 4999]] = (np.nan, np.inf, -np.inf)
    items[6][:] = np.clip(items[6] * 4, -1, 1)
    items[6][[0, 776]] = (1.0, -1.0)
    return items


def _pack_at_odd_starts(items, shift=0):
    """-> (flat float32, starts): every span starts at an odd sample offset (+ shift), NaN between the spans"""
    starts, o = [], 1 + shift
    for it in items:
        o += (1 - (o - shift) % 2)              # odd relative to the unshifted layout
        starts.append(o)
        o += it.size + 4
    flat = np.full(o + 8, np.nan, dtype=np.float32)
    for s, it in zip(starts, items):
        flat[s:s + it.size] = it
    return flat, starts


def _raw_levels(dev, flat, starts, lengths, guard=3):
    """dv3_wave_levels_f32 itself, the table between guard rows -> float64 (B, 5) numpy"""
    from deepvoice3_pytorch_amd import _lib
    B = len(starts)
    x = torch.from_numpy(flat).to(dev)
    max_len = max(int(n) for n in lengths)
    nchunk = -(-max_len // _lib.CONSTS["DV3_LEVELS_CHUNK"])
    scratch = torch.empty(max(B * nchunk * 5, 1), dtype=torch.float64, device=dev)
    table = torch.full((B + 2 * guard, 5), SENTINEL, dtype=torch.float64, device=dev)
    st, ln = _i64(dev, starts), _i64(dev, lengths)
    _lib.call("dv3_wave_levels_f32", x.data_ptr(), st.data_ptr(), ln.data_ptr(), B, max_len, scratch.data_ptr(),
              table[guard].data_ptr(), None)
    torch.cuda.synchronize()
    t = table.cpu().numpy()
    assert np.all(t[:guard] == SENTINEL) and np.all(t[guard + B:] == SENTINEL), "the level table's guard rows were written"
    return t[guard:guard + B]


@pytest.fixture(scope="module")
def level_rows(dev):
    items = _level_items()
    flat, starts = _pack_at_odd_starts(items)
    assert all(s % 2 == 1 for s in starts)
    return items, _raw_levels(dev, flat, starts, [it.size for it in items])


def test_levels_against_float64(level_rows):
    items, rows = level_rows
    for b, it in enumerate(items):
        (peak, sumsq, total, over, bad), sabs = M.levels_row(it)
        n = it.size
        got = rows[b]
        assert got[0] == peak and got[3] == over and got[4] == bad, (b, got.tolist(), peak, over, bad)
        assert abs(got[1] - sumsq) <= n * 2.0 ** -52 * sumsq, (b, got[1], sumsq)
        assert abs(got[2] - total) <= n * 2.0 ** -53 * sabs, (b, got[2], total)
    assert not rows[0].any()                                                          # the zero-length item
    assert rows[5][4] == 3 and rows[5][3] >= 2 and rows[6][0] == 1.0 and rows[6][3] >= 2


@pytest.mark.parametrize("shift", [0, 1, 2, 3])
def test_a_level_row_depends_on_its_item_alone(dev, level_rows, shift):
    """bit-equal rows: each item called alone, and the whole batch with every span moved by 1, 2 and 3 samples"""
    items, rows = level_rows
    flat, starts = _pack_at_odd_starts(items, shift)
    moved = _raw_levels(dev, flat, starts, [it.size for it in items])
    assert np.array_equal(moved.view(np.int64), rows.view(np.int64)), shift
    if shift == 0:
        for b, it in enumerate(items):
            alone = _raw_levels(dev, flat, starts[b:b + 1], [it.size])
            assert np.array_equal(alone[0].view(np.int64), rows[b].view(np.int64)), b


def test_wave_levels_wrapper_takes_a_padded_batch(dev, level_rows):
    from deepvoice3_pytorch_amd import audio
    items, rows = level_rows
    L = max(it.size for it in items)
    batch = np.full((len(items), L), np.nan, dtype=np.float32)
    for b, it in enumerate(items):
        batch[b, :it.size] = it
    x = torch.from_numpy(batch).to(dev)
    lens = [it.size for it in items]
    got = audio.wave_levels(x, np.arange(len(items)) * L, lens)
    assert got.dtype == torch.float64 and tuple(got.shape) == (len(items), len(audio.LEVEL_COLUMNS))
    assert np.array_equal(got.cpu().numpy().view(np.int64), rows.view(np.int64))
    on_dev = audio.wave_levels(x, _i64(dev, np.arange(len(items)) * L), _i64(dev, lens), max_len=L)
    assert torch.equal(on_dev, got)
    with pytest.raises(ValueError, match="max_len"):
        audio.wave_levels(x, _i64(dev, [0]), _i64(dev, [5]))
    with pytest.raises(ValueError, match="spans"):
        audio.wave_levels(x, [0], [x.numel() + 1])


# ----------------------------------------------------------------------------------------------------------------------
# 2. gains
# ----------------------------------------------------------------------------------------------------------------------
GAIN_TABLE = np.array([[0.5, 0.03, 0.1, 0, 0],         # group 0: one item, peaky: the RMS policy's ceiling binds
                       [0.0, 0.0, 0.0, 0, 0],          # group 1: silent
                       [0.25, 1.5, 0.0, 0, 0],         # group 2: three items, the largest peak in the middle
                       [0.9, 40.0, 0.0, 0, 0],
                       [0.125, 0.75, 0.0, 0, 0],
                       [1e-4, 1e-6, 0.0, 0, 0],        # group 3: near-silent: the cap binds
                       [0.003, 1e-5, 0.0, 0, 0]],      # group 4: under the reference's floor of 0.01
                      dtype=np.float64)
GAIN_LENGTHS = [100, 50, 1000, 2000, 3000, 4000, 10]
GAIN_GROUPS = [0, 1, 2, 5, 6, 7]


@pytest.mark.parametrize("policy,target,ceiling,max_gain", [
    (M.GAIN_PEAK, 10 ** (-1 / 20.0), 1.0, 10 ** (30 / 20.0)),          # the cap binds on the quiet groups 3 and 4
    (M.GAIN_PEAK, 0.5, 1.0, 1.25),                                    # the cap binds on most groups
    (M.GAIN_RMS, 0.1, 10 ** (-1 / 20.0), 10 ** (30 / 20.0)),           # the ceiling binds on group 0, the cap on 3
    (M.GAIN_RMS, 0.05, 0.99, 2.0),
    (M.GAIN_REFERENCE, 1.0, 1.0, 1.0)])
@pytest.mark.parametrize("groups", [GAIN_GROUPS, list(range(8)), [0, 7]])
def test_gains_bit_for_bit(dev, policy, target, ceiling, max_gain, groups):
    from deepvoice3_pytorch_amd import _lib
    B = len(GAIN_LENGTHS)
    lv = torch.from_numpy(GAIN_TABLE).to(dev)
    ln = _i64(dev, GAIN_LENGTHS)
    goff = torch.tensor(groups, dtype=torch.int32, device=dev)
    out = torch.full((B + 8,), SENTINEL, dtype=torch.float32, device=dev)
    _lib.call("dv3_wave_gains_f32", lv.data_ptr(), ln.data_ptr(), goff.data_ptr(), B, len(groups) - 1, policy,
              target, ceiling, max_gain, out[4:].data_ptr(), None)
    got = out.cpu().numpy()
    assert np.all(got[:4] == SENTINEL) and np.all(got[4 + B:] == SENTINEL)
    want = M.gains(GAIN_TABLE, GAIN_LENGTHS, groups, policy, target, ceiling, max_gain)
    assert np.array_equal(got[4:4 + B].view(np.int32), want.view(np.int32)), (got[4:4 + B], want)
    if groups == GAIN_GROUPS and policy != M.GAIN_REFERENCE:
        assert want[1] == 1.0 and want[2] == want[3] == want[4] and want[5] == np.float32(max_gain)
    if groups == GAIN_GROUPS and policy == M.GAIN_REFERENCE:
        assert want[6] == np.float32(0.01) and want[3] == np.float32(0.9)


# ----------------------------------------------------------------------------------------------------------------------
# 3. the master launch
# ----------------------------------------------------------------------------------------------------------------------
def _raw_master(dev, x, src, length, dst, gain, flags, fade, N, mode, dither=0, seed=0, guard=64):
    """dv3_wave_master_f32 itself into a sentinel-filled buffer with guard bands -> numpy (N,)"""
    from deepvoice3_pytorch_amd import _lib
    xd = torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32)).to(dev)
    i16 = mode != M.MODE_F32
    buf = torch.full((N + 2 * guard,), -77 if i16 else SENTINEL, dtype=torch.int16 if i16 else torch.float32, device=dev)
    sd, ld, dd = _i64(dev, src), _i64(dev, length), _i64(dev, dst)
    gd = torch.from_numpy(np.asarray(gain, dtype=np.float32)).to(dev)
    fd = torch.tensor([int(f) for f in flags], dtype=torch.int32, device=dev)
    ft = torch.from_numpy(np.asarray(fade, dtype=np.float32)).to(dev) if len(fade) else None
    _lib.call("dv3_wave_master_f32", xd.data_ptr(), sd.data_ptr(), ld.data_ptr(), dd.data_ptr(), gd.data_ptr(),
              fd.data_ptr(), len(src), ft.data_ptr() if ft is not None else None, len(fade), mode, dither, seed,
              buf[guard:].data_ptr(), N, None)
    torch.cuda.synchronize()
    got = buf.cpu().numpy()
    fill = got.dtype.type(-77 if i16 else SENTINEL)
    assert np.all(got[:guard] == fill) and np.all(got[guard + N:] == fill), "the guard bands around the output were written"
    return got[guard:guard + N]


def _bits(a):
    return a.view(np.int32) if a.dtype == np.float32 else a


@pytest.mark.parametrize("F", [64, 221])
@pytest.mark.parametrize("mode,dither", [(M.MODE_F32, 0), (M.MODE_I16, 0), (M.MODE_I16, 1)])
def test_master_bit_for_bit(dev, F, mode, dither):
    """segment lengths {1, F, F + 1, 2F - 1, 5000}, src - dst over every residue mod 4, N no multiple of 8, a leading gap,
    a pause, a crossfade of exactly F, the last segment ending at N (tests/master_ref.issue_layout)"""
    rng = np.random.RandomState(F)
    x, src, length, dst, gain, flags, N = M.issue_layout(F, rng)
    assert N % 8 != 0 and sorted({int(v) % 4 for v in src - dst}) == [0, 1, 2, 3]
    x[int(src[4]) + 100] = np.nan                                  # a NaN sample quantises to 0
    x[int(src[4]) + 200] = 3.0e4                                   # and a wild one saturates
    fade = M.fade_table(F)
    seed = 0x9E3779B97F4A7C15
    want = M.master(x, src, length, dst, gain, flags, fade, N, mode, bool(dither), seed)
    got = _raw_master(dev, x, src, length, dst, gain, flags, fade, N, mode, dither, seed)
    assert got.dtype == want.dtype
    diff = np.flatnonzero(_bits(got) != _bits(want))
    assert diff.size == 0, (diff[:8], got[diff[:8]], want[diff[:8]])
    again = _raw_master(dev, x, src, length, dst, gain, flags, fade, N, mode, dither, seed)
    assert np.array_equal(_bits(again), _bits(got))                # two calls: bit-equal
    if mode == M.MODE_I16:
        n_nan, n_big = int(dst[4]) + 100, int(dst[4]) + 200
        assert got[n_nan] == (want[n_nan] if dither else 0) and got[n_big] == 32767
        assert np.abs(got[:37]).max() <= (1 if dither else 0)          # the leading gap: zeros, or the dither alone
    if dither:
        plain = M.master(x, src, length, dst, gain, flags, fade, N, mode, False, seed)
        assert np.abs(got.astype(np.int64) - plain.astype(np.int64)).max() <= 1 and not np.array_equal(got, plain)


def test_master_reference_mode_bit_for_bit(dev):
    """no fades, no overlap, gain the divisor: truncation, not rounding; several chunks per wave and a gap between"""
    rng = np.random.RandomState(5)
    length = np.array([1, 64, 65, 127, 5000, 9000], dtype=np.int64)
    dst = np.cumsum(np.concatenate([[5], length[:-1] + np.array([0, 3, 0, 2, 1])])).astype(np.int64)
    src = np.array([2, 12, 83, 150, 283, 5301], dtype=np.int64)
    N = int(dst[-1] + length[-1]) + 3
    x = rng.uniform(-1, 1, 14400).astype(np.float32)
    div = np.maximum(rng.uniform(0.005, 1.0, 6), 0.01).astype(np.float32)
    want = M.master(x, src, length, dst, div, [0] * 6, M.fade_table(0), N, M.MODE_I16_REFERENCE)
    got = _raw_master(dev, x, src, length, dst, div, [0] * 6, M.fade_table(0), N, M.MODE_I16_REFERENCE)
    assert N % 8 != 0 and np.array_equal(got, want)
    rounded = M.master(x, src, length, dst, 1.0 / div, [0] * 6, M.fade_table(0), N, M.MODE_I16)
    assert not np.array_equal(rounded, want)


def test_wave_master_wrapper_is_the_entry_point(dev):
    from deepvoice3_pytorch_amd import audio
    F = 64
    x, src, length, dst, gain, flags, N = M.issue_layout(F, np.random.RandomState(1))
    xd = torch.from_numpy(x).to(dev)
    gd = torch.from_numpy(gain).to(dev)
    for dtype, mode in (("float32", M.MODE_F32), ("int16", M.MODE_I16)):
        got = audio.wave_master(xd, src, length, dst, gd, flags, N, F, dtype)
        want = M.master(x, src, length, dst, gain, flags, M.fade_table(F), N, mode)
        assert np.array_equal(_bits(got.cpu().numpy()), _bits(want)), dtype
    got = audio.wave_master(xd, src, length, dst, None, 0, N, 0, "int16", dither=True, seed=3)
    want = M.master(x, src, length, dst, np.ones(5, np.float32), [0] * 5, M.fade_table(0), N, M.MODE_I16, True, 3)
    assert np.array_equal(got.cpu().numpy(), want)


# ----------------------------------------------------------------------------------------------------------------------
# 4. the reference policy: save_wav's samples
# ----------------------------------------------------------------------------------------------------------------------
def test_to_pcm16_is_numpys_save_wav_formula(dev):
    """random waves at several scales, an item with its peak under 0.01, an all-zero item, a peak of exactly 1"""
    from deepvoice3_pytorch_amd import audio
    rng = np.random.RandomState(9)
    lens = [4097, 3000, 5001, 2048, 1500, 777, 4000]
    waves = [(rng.randn(n) * s).astype(np.float32) for n, s in zip(lens[:4], (0.05, 0.3, 1.0, 6.0))]
    waves.append((rng.randn(lens[4]) * 1e-3).astype(np.float32).clip(-0.009, 0.009))
    waves.append(np.zeros(lens[5], np.float32))
    one = rng.uniform(-1, 1, lens[6]).astype(np.float32)
    one[1234] = -1.0
    waves.append(one)
    assert np.abs(waves[4]).max() < 0.01 and np.abs(waves[6]).max() == 1.0
    L = max(lens) + 3
    batch = np.full((len(waves), L), 9.0, dtype=np.float32)          # the padding is louder than every item: never read
    for b, w in enumerate(waves):
        batch[b, :w.size] = w
    got = audio.to_pcm16(torch.from_numpy(batch).to(dev), lens)
    assert got.dtype == torch.int16 and tuple(got.shape) == (len(waves), L)
    got = got.cpu().numpy()
    for b, w in enumerate(waves):
        want = (w * 32767 / max(0.01, np.max(np.abs(w)))).astype(np.int16)
        assert np.array_equal(got[b, :w.size], want), b
        assert not got[b, w.size:].any()
    assert np.abs(got[6]).max() == 32767 and np.abs(got[4]).max() < 32767 * 0.91


def test_master_items_is_levels_gains_and_one_launch(dev):
    from deepvoice3_pytorch_amd import audio
    rng = np.random.RandomState(4)
    lens = [3001, 1200, 0, 2500]
    L = 3001
    batch = (rng.randn(4, L) * np.array([0.05, 0.4, 1.0, 2.0])[:, None]).astype(np.float32)
    x = torch.from_numpy(batch).to(dev)
    starts = np.arange(4) * L
    for m in (audio.Mastering("peak"), audio.Mastering("rms", scope="document", dtype="float32"),
              audio.Mastering("peak", scope="document", dither=True, seed=11), audio.Mastering(None)):
        got = audio.master_items(x, lens, m).cpu().numpy()
        rows = [M.levels_row(batch[b, :n])[0] for b, n in enumerate(lens)]
        lin = lambda db: 10.0 ** (db / 20.0)
        groups = list(range(5)) if m.scope == "item" else [0, 4]
        if m.level is None:
            gain = np.ones(4, np.float32)
        else:
            dev_rows = audio.wave_levels(x, starts, lens).cpu().numpy()      # the gains come from the DEVICE's sums
            gain = M.gains(dev_rows, lens, groups, M.GAIN_PEAK if m.level == "peak" else M.GAIN_RMS, lin(m.target_db),
                           lin(m.ceiling_db), lin(m.max_gain_db))
            assert dev_rows[:, 0].tolist() == [r[0] for r in rows]
        mode = M.MODE_F32 if m.dtype == "float32" else M.MODE_I16
        for b, n in enumerate(lens):
            want = M.master(batch[b], [0], [n], [0], gain[b:b + 1], [0], M.fade_table(0), L, mode, m.dither, m.seed)
            assert np.array_equal(_bits(got[b]), _bits(want)), (m.level, m.scope, b)
        if m.level == "peak" and m.scope == "item" and not m.dither:
            assert abs(int(np.abs(got[0]).max()) - round(32767 * lin(-1.0))) <= 1


# ----------------------------------------------------------------------------------------------------------------------
# 5. refusals
# ----------------------------------------------------------------------------------------------------------------------
def test_refusals(dev):
    from deepvoice3_pytorch_amd import _lib, audio
    h = _lib.lib()
    EINVAL = _lib.CONSTS["DV3_EINVAL"]
    x = torch.ones(64, device=dev)
    one = _i64(dev, [0])
    n8 = _i64(dev, [8])
    lv = torch.zeros(1, 5, dtype=torch.float64, device=dev)
    scratch = torch.zeros(8, dtype=torch.float64, device=dev)
    good = [x.data_ptr(), one.data_ptr(), n8.data_ptr(), 1, 8, scratch.data_ptr(), lv.data_ptr(), None]
    assert h.dv3_wave_levels_f32(*good) == 0
    for pos, bad in ((0, None), (1, None), (2, None), (6, None), (5, None), (3, 0), (3, 65536), (4, -1), (4, 2 ** 41),
                     (6, lv.data_ptr() + 4)):
        args = list(good)
        args[pos] = bad
        assert h.dv3_wave_levels_f32(*args) == EINVAL, ("levels", pos, bad)
        assert h.dv3_last_error().decode().startswith("wave_levels:")
    goff = torch.tensor([0, 1], dtype=torch.int32, device=dev)
    g = torch.zeros(1, device=dev)
    good = [lv.data_ptr(), n8.data_ptr(), goff.data_ptr(), 1, 1, M.GAIN_PEAK, 0.5, 0.9, 10.0, g.data_ptr(), None]
    assert h.dv3_wave_gains_f32(*good) == 0
    for pos, bad in ((0, None), (1, None), (2, None), (9, None), (3, 0), (3, 65536), (4, 0), (4, 2), (5, 3), (5, -1),
                     (6, 0.0), (6, float("nan")), (7, -1.0), (8, float("inf"))):
        args = list(good)
        args[pos] = bad
        assert h.dv3_wave_gains_f32(*args) == EINVAL, ("gains", pos, bad)
        assert h.dv3_last_error().decode().startswith("wave_gains:")
    g.zero_()                                                             # (the gains call above wrote it)
    flags = torch.zeros(1, dtype=torch.int32, device=dev)
    fade = torch.from_numpy(M.fade_table(4)).to(dev)
    out = torch.full((32,), -77, dtype=torch.int16, device=dev)
    good = [x.data_ptr(), one.data_ptr(), n8.data_ptr(), one.data_ptr(), g.data_ptr(), flags.data_ptr(), 1, fade.data_ptr(),
            4, M.MODE_I16, 0, 0, out.data_ptr(), 8, None]
    top_f, top_s = _lib.CONSTS["DV3_MASTER_MAX_FADE"], _lib.CONSTS["DV3_MASTER_MAX_SEGMENTS"]
    for pos, bad in ((0, None), (1, None), (2, None), (3, None), (4, None), (5, None), (12, None), (7, None), (6, 0),
                     (6, top_s + 1), (8, -1), (8, top_f + 1), (9, 3), (9, -1), (10, 2), (13, -1), (13, 2 ** 41),
                     (12, out.data_ptr() + 2), (12, x.data_ptr())):
        args = list(good)
        args[pos] = bad
        assert h.dv3_wave_master_f32(*args) == EINVAL, ("master", pos, bad)
        assert h.dv3_last_error().decode().startswith("wave_master:")
    for fix in ({8: 4}, {10: 1}, {8: 4, 10: 1}):                          # the reference mode with fades or dither
        args = list(good)
        args[9], args[8] = M.MODE_I16_REFERENCE, 0
        for k, v in fix.items():
            args[k] = v
        assert h.dv3_wave_master_f32(*args) == EINVAL and h.dv3_last_error().decode().startswith("wave_master:")
    args = list(good)
    args[9], args[10] = M.MODE_F32, 1                                     # dither without an integer to round to
    assert h.dv3_wave_master_f32(*args) == EINVAL
    torch.cuda.synchronize()
    assert torch.all(out == -77), "a refused call launched something"
    assert h.dv3_wave_master_f32(*good) == 0
    torch.cuda.synchronize()
    assert torch.all(out[8:] == -77) and torch.all(out[:8] == 0)         # gain 0: zeros, and nothing past N
    # the Python wrapper: the layout rules live on the host
    for src, ln, dst, N, kw, what in (([0, 10], [10, 10], [10, 0], 20, {}, "sorted"),
                                      ([0, 10, 20], [10, 10, 10], [0, 4, 8], 30, {}, "three"),
                                      ([0, 60], [10, 10], [0, 10], 20, {}, "source"),
                                      ([0, 10], [10, 10], [0, 9], 20, dict(reference=True), "reference"),
                                      ([0], [10], [0], 10, dict(fade_samples=top_f + 1), "fade_samples"),
                                      ([0], [10], [0], 10, dict(dtype="int8"), "dtype")):
        with pytest.raises(ValueError, match=what):
            audio.wave_master(x, src, ln, dst, None, 0, N, **kw)
    with pytest.raises(ValueError, match="lengths"):
        audio.master_items(x.view(2, 32), [33, 1], audio.Mastering("peak"))
    with pytest.raises(ValueError, match="Mastering"):
        audio.master_items(x.view(2, 32), [3, 1], "peak")


# ----------------------------------------------------------------------------------------------------------------------
# 6. through synthesis
# ----------------------------------------------------------------------------------------------------------------------
E2E_HP = dict(n_vocab=40, embed_dim=32, mel_dim=20, linear_dim=257, r=1, downsample_step=4, padding_idx=0, dropout=0.05,
              kernel_size=3, encoder_channels=64, decoder_channels=32, converter_channels=32, use_memory_mask=True,
              force_monotonic_attention=True, use_decoder_state_for_postnet_input=True, key_projection=True,
              value_projection=True, max_positions=128)


@pytest.fixture(scope="module")
def spoken(dev):
    """the tiny random model of the synthesis tests at 512 / 128, three short sentences, and their plain tts_batch"""
    from deepvoice3_pytorch_amd import audio, builder, synthesis
    torch.manual_seed(0)
    model = builder.deepvoice3(**E2E_HP).to(dev).eval()
    dec = model.seq2seq.decoder
    dec.min_decoder_steps = dec.max_decoder_steps = 11
    rng = np.random.RandomState(2)
    ids = [rng.randint(2, 40, n).tolist() for n in (9, 14, 6)]
    cfg = audio.AudioConfig(fft_size=512, hop_size=128, sample_rate=16000, griffin_lim_iters=3)
    plain = synthesis.tts_batch(model, ids, audio_cfg=cfg, timings=True)
    return model, ids, cfg, plain


@pytest.mark.parametrize("kind", ["rms-int16", "peak-dither", "reference", "float32"])
def test_mastering_through_the_three_entry_points(dev, spoken, kind):
    from deepvoice3_pytorch_amd import audio, synthesis
    model, ids, cfg, plain = spoken
    m = {"rms-int16": audio.Mastering("rms"), "peak-dither": audio.Mastering("peak", dither=True, seed=5),
         "reference": audio.Mastering("reference"), "float32": audio.Mastering("peak", dtype="float32")}[kind]
    res = synthesis.tts_batch(model, ids, audio_cfg=cfg, timings=True, mastering=m)
    L = max(r[3].numel() for r in plain)
    wavs = torch.zeros(len(ids), L, device=dev)
    for b, r in enumerate(plain):
        wavs[b, :r[3].numel()] = r[3]
    by_hand = audio.master_items(wavs, [r[3].numel() for r in plain], m)
    for b in range(len(ids)):
        for i in range(3):
            assert torch.equal(res[b][i], plain[b][i]), (b, i)                  # mel, linear, alignment untouched
        assert res[b][3].dtype == (torch.float32 if kind == "float32" else torch.int16)
        assert torch.equal(res[b][3], by_hand[b, :plain[b][3].numel()]), b
        assert torch.equal(res[b][4]["end"], plain[b][4]["end"])
        if kind == "reference":
            w = plain[b][3].cpu().numpy()
            assert np.array_equal(res[b][3].cpu().numpy(), M.save_wav_samples(w))
    got = {r[0]: r for r in synthesis.tts_stream(model, ids, slots=2, audio_cfg=cfg, mastering=m)}
    rs = synthesis.RollingSynthesizer(model, slots=3, max_text_len=14, audio_cfg=cfg, mastering=m)
    tickets = [rs.submit(s) for s in ids]
    rolled = {r[0]: r[4] for r in rs.drain()}
    for b in range(len(ids)):
        assert torch.equal(got[b][4], res[b][3]), (b, "tts_stream")
        assert torch.equal(rolled[tickets[b]], res[b][3]), (b, "RollingSynthesizer")
    with pytest.raises(ValueError, match="Mastering"):
        synthesis.tts_batch(model, ids, audio_cfg=cfg, mastering="peak")


TRIM_DB = 3.0                # tight, so that the random model's noise-like waveforms do lose frames at their edges


@pytest.mark.parametrize("pause", [0.0, 0.05])
def test_tts_document_is_the_by_hand_composition(dev, spoken, pause):
    from deepvoice3_pytorch_amd import audio, synthesis
    model, ids, cfg, plain = spoken
    m = audio.Mastering("rms", scope="document", fade_ms=4.0)
    doc, where, spans = synthesis.tts_document(model, ids, batch=2, timings=True, audio_cfg=cfg, pauses=pause,
                                               trim_db=TRIM_DB, mastering=m)
    wavs = [r[3] for r in plain]
    lens = np.array([w.numel() for w in wavs])
    starts = np.concatenate([[0], np.cumsum(lens)[:-1]])
    flat = torch.cat(wavs)
    t_start, t_len = audio.trim_items(flat, starts, lens, TRIM_DB)
    src, tl = t_start.cpu().numpy(), t_len.cpu().numpy()
    assert lens.min() >= 1025 and (tl < lens).any(), "the trim cut nothing: the test would not see a wrong offset"
    F = m.fade_samples(cfg.sample_rate)
    assert F == 64
    table, N = synthesis.plan_document(tl, cfg.sample_rate, pause, F, starts=src)
    gain = audio.wave_gains(audio.wave_levels(flat, src, tl), _i64(dev, tl), m)
    want = audio.wave_master(flat, table["src"], table["len"], table["dst"], gain, table["flags"], N, F, "int16")
    assert doc.dtype == torch.int16 and doc.numel() == N and torch.equal(doc, want)
    assert len(set(gain.tolist())) == 1                                           # one gain for the document
    if pause == 0.0:
        assert table["dst"][1] == table["dst"][0] + tl[0] - F                       # a crossfade
    sr = float(cfg.sample_rate)
    for k in range(len(ids)):
        assert where[k] == (table["dst"][k] / sr, (table["dst"][k] + tl[k]) / sr)
        shift = (int(table["dst"][k]) - (int(src[k]) - int(starts[k]))) / sr
        for key in ("start", "end"):
            assert torch.equal(spans[k][key], plain[k][4][key] + shift), (k, key)
        assert torch.equal(spans[k]["durations"], plain[k][4]["durations"])
    # the float restatement of the whole document from the device's own gains
    ref = M.master(flat.cpu().numpy(), table["src"], table["len"], table["dst"], gain.cpu().numpy(), table["flags"],
                   M.fade_table(F), N, M.MODE_I16)
    assert np.array_equal(doc.cpu().numpy(), ref)
    two, _ = synthesis.join_utterances(wavs, cfg.sample_rate, pauses=pause, trim_db=TRIM_DB, mastering=m)
    assert torch.equal(two, doc)

# coding: utf-8
"""-m gpu: loudness mastering (csrc/loudness.hip; include/dv3hip.h: dv3_wave_loudness_f64,
dv3_loudness_gate_f64, dv3_loudness_gains_f32) against the float64 restatement of tests/loudness_ref.py.

The bounds, derived here and not fitted (U = 2^-53, the unit roundoff of fp64; NG = the sum of |impulse response| of the
K-weighting cascade, computed below per sample rate; M = the largest magnitude among the item's reference states and
outputs; MARGIN = 4 for what the first-order analysis leaves out: second-order terms, the rounding of A^h itself by
numpy.linalg.matrix_power, the device's fma contraction against numpy's separate roundings, and the gain from a state's
rounding to the output, which exceeds the input's):

  states    |s_k - ref| <= MARGIN * U * NG * (k h) * M: k h samples lie behind the state of chunk k, each adding one
            rounded update of relative size U that reaches the state with gain at most NG;
  outputs   the same with the samples behind the chunk's LAST sample, dy_k = MARGIN * U * NG * ((k + 1) h) * M;
  energies  E[k] = sum of y^2 over at most h samples: |dE| <= 2 * sum|y| * dy_k + h * U * E[k] -- the first term is the
            filter's error carried into the squares, the second the accumulation of h terms in fp64;
  lufs      L = -0.691 + 10 log10(a mean of z): a mean of positive terms has at most the largest relative error of its
            terms, so |dL| <= (10 / ln 10) * max over the gated blocks of (sum of dE / sum of E) + 1e-12 (the device's log10
            and the order of the sums: a few ulp of a number below 100);
  counts    exact -- every gating input is first shown to keep each block 0.01 LU or more away from both gates in the
            reference, far beyond dL, so no rounding flips a block;
  true peak each interpolant is a chain of 12 fp32 fmaf: |dv| <= 13 * 2^-24 * sum|tap * sample| (the standard bound of a
            12-term inner product), times 2 for the margin; the sum is at most sum|g| * peak, and the reference reports the
            largest one of the item;
  gains     bit for bit from the device's own rows by the reference's float64 formula rounded once; end to end against
            the reference's rows within |dL| ln(10) / 20 + dpeak / peak + 2^-23 relative.

Shapes: at 8 kHz (h = 800) six items of 0, 799, 3199, 3200, 4001 and 12345 samples at unaligned offsets -- no sample, less
than a chunk, one sample short of a block, exactly one block, two blocks and one sample of a sixth chunk, and 16 chunks; at 22.05 kHz
(h = 2205, not a multiple of the 64-sample tile) one item of 30000."""
import ctypes
import math
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tests import loudness_ref as R  # noqa: E402
from tests import master_ref as M  # noqa: E402

pytestmark = pytest.mark.gpu

U = 2.0 ** -53
MARGIN = 4.0
LENGTHS_8K = (0, 799, 3199, 3200, 4001, 12345)
SENTINEL = -7.25


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


def _i64(dev, v):
    return torch.tensor([int(a) for a in v], dtype=torch.int64, device=dev)


def _items_8k():
    rng = np.random.RandomState(21)
    out = []
    for n in LENGTHS_8K:
        t = np.arange(n)
        out.append((0.2 * rng.randn(n) + 0.3 * np.sin(2 * np.pi * 440.0 * t / 8000.0)).astype(np.float32))
    return out


def _pack(items, shift=0):
    """-> (flat float32 with NaN between the spans, starts): odd, unaligned starts, all moved by `shift`"""
    starts, o = [], 3 + shift
    for it in items:
        starts.append(o)
        o += it.size + 4
        o += 1 - (o - shift) % 2                # odd relative to the unshifted layout
    flat = np.full(o + 16, np.nan, dtype=np.float32)
    for s, it in zip(starts, items):
        flat[s:s + it.size] = it
    return flat, starts


def _measure(dev, flat, starts, lengths, fs, groups=None, true_peak=False):
    from deepvoice3_pytorch_amd import audio
    x = torch.from_numpy(flat).to(dev)
    rows, energy, states = audio.wave_loudness(x, starts, lengths, fs, groups, true_peak, want_tables=True)
    return rows.cpu().numpy(), energy.cpu().numpy(), states.cpu().numpy()


_REF = {}


def _reference(key, items, fs):
    """per item: (E, states, dE bound, state bound per chunk, y) -- computed once per key and left unchanged"""
    if key not in _REF:
        h = R.step(fs)
        NG = R.noise_gain(fs, 8 * h)
        out = []
        for x in items:
            y, _ = R.cascade(x, fs)
            st = R.chunk_states(x, fs)
            E = R.sub_blocks(x, fs)
            mag = max([1e-300] + ([float(np.abs(y).max()), float(np.abs(st).max())] if x.size else []))
            k = np.arange(E.size)
            ds = MARGIN * U * NG * (k * h) * mag
            dy = MARGIN * U * NG * ((k + 1) * h) * mag
            sabs = np.array([np.abs(y[i * h:(i + 1) * h]).sum() for i in k]) if E.size else np.zeros(0)
            dE = 2.0 * sabs * dy + h * U * E
            out.append((E, st, dE, ds, y))
        _REF[key] = (out, NG)
    return _REF[key]


def _lufs_bound(E, dE, n, fs):
    """(10 / ln 10) * the largest relative error of a block's energy, over the blocks of one item that pass the
    absolute gate (the others enter no mean)"""
    h = R.step(fs)
    J = (n - 4 * h) // h + 1 if n >= 4 * h else 0
    rel = [dE[j:j + 4].sum() / E[j:j + 4].sum() for j in range(J) if R.lkfs(E[j:j + 4].sum() / (4.0 * h)) > -70.0]
    if J == 0 and E.sum() > 0:
        rel = [dE.sum() / E.sum()]
    return 10.0 / math.log(10.0) * max(rel + [0.0]) + 1e-12


def _check_item(b, x, fs, ref, row, energy, states):
    E, st, dE, ds, _ = ref
    K = E.size
    assert np.all(np.abs(energy[:K] - E) <= dE), (b, np.abs(energy[:K] - E).max(), dE.max())
    assert not energy[K:].any() and not states[K:].any(), (b, "chunks past the item's end are zeros")
    assert np.all(np.abs(states[:K] - st) <= ds[:, None]), (b, np.abs(states[:K] - st).max(axis=1), ds)
    want, detail, _ = R.measure([x], fs)
    want, (l, gamma) = want[0], detail[0]
    assert R.gate_margin(l, gamma) > 0.01, (b, "a block within 0.01 LU of a gate: no fair input")
    assert row[1:4].tolist() == want[1:4].tolist() and row[6] == want[6], (b, row, want)
    assert row[5] == want[5], (b, "the sample peak is exact")
    if np.isfinite(want[0]):
        tol = _lufs_bound(E, dE, x.size, fs)
        print("item %d (n = %d, fs = %d): lufs %.6f, |d| = %.3e (bound %.3e); max |dE| / bound = %.3e" % (
            b, x.size, fs, row[0], abs(row[0] - want[0]), tol, (np.abs(energy[:K] - E) / dE).max()))
        assert abs(row[0] - want[0]) <= tol, (b, row[0], want[0], tol)
        if want[1] > 0:
            assert abs(row[4] - want[4]) <= tol, (b, row[4], want[4])
    else:
        assert row[0] == want[0]


@pytest.fixture(scope="module")
def batch_8k(dev):
    items = _items_8k()
    flat, starts = _pack(items)
    assert all(s % 2 == 1 for s in starts)
    return items, _measure(dev, flat, starts, LENGTHS_8K, 8000)


def test_energies_states_and_rows_against_float64(batch_8k):
    items, (rows, energy, states) = batch_8k
    ref, NG = _reference("8k", items, 8000)
    assert energy.shape == (6, 16) and states.shape == (6, 16, 4) and rows.shape == (6, 7)
    for b, x in enumerate(items):
        _check_item(b, x, 8000, ref[b], rows[b], energy[b], states[b])
    assert rows[0, 6] == 3 and rows[1, 6] == 1 and rows[2, 6] == 1 and rows[3, 1] == 1 and rows[4, 1] == 2 and rows[5, 1] == 12


def test_one_item_at_22050(dev):
    """h = 2205 = 34 tiles of 64 and a tail of 29; 14 chunks, the last one partial"""
    rng = np.random.RandomState(22)
    n = 30000
    x = (0.1 * rng.randn(n) + 0.25 * np.sin(2 * np.pi * 300.0 * np.arange(n) / 22050.0)).astype(np.float32)
    flat, starts = _pack([x])
    rows, energy, states = _measure(dev, flat, starts, [n], 22050)
    ref, _ = _reference("22k", [x], 22050)
    assert energy.shape == (1, 14)
    _check_item(0, x, 22050, ref[0], rows[0], energy[0], states[0])
    assert rows[0, 1] == 10


@pytest.mark.parametrize("shift", [0, 1, 3, 64])
def test_a_row_depends_on_its_item_alone(dev, batch_8k, shift):
    """bit-equal rows, energies and states: the batch moved by 1, 3 and 64 samples, and every item called alone"""
    items, (rows, energy, states) = batch_8k
    flat, starts = _pack(items, shift)
    r2, e2, s2 = _measure(dev, flat, starts, LENGTHS_8K, 8000)
    eq = lambda a, b: np.array_equal(a.view(np.int64), b.view(np.int64))
    assert eq(r2, rows) and eq(e2, energy) and eq(s2, states), shift
    if shift == 0:
        for b, it in enumerate(items):
            r1, e1, s1 = _measure(dev, flat, starts[b:b + 1], [it.size], 8000)
            K = e1.shape[1]
            assert eq(r1[0], rows[b]) and eq(e1[0], energy[b, :K].copy()) and eq(s1[0], states[b, :K].copy()), b
        tp_all = _measure(dev, flat, starts, LENGTHS_8K, 8000, true_peak=True)[0]
        tp_one = _measure(dev, flat, starts[5:6], LENGTHS_8K[5:6], 8000, true_peak=True)[0]
        assert eq(tp_one[0], tp_all[5]) and eq(tp_all[:, :5].copy(), rows[:, :5].copy())


@pytest.mark.parametrize("name", ["A", "B"])
def test_gating_programmes_on_the_device(dev, name):
    """gating A and B at 8 kHz as one group, and cut into two items as per-item groups and as one pooled group"""
    fs = 8000
    x = (R.gating_a if name == "A" else R.gating_b)(fs)
    ref, _ = _reference("gating" + name, [x], fs)
    flat, starts = _pack([x])
    rows, energy, states = _measure(dev, flat, starts, [x.size], fs)
    _check_item(0, x, fs, ref[0], rows[0], energy[0], states[0])
    assert rows[0, 1:4].tolist() == ([77, 77, 43] if name == "A" else [77, 31, 30])
    # two items (the cut falls on no chunk border), per item and pooled
    parts = [x[:30001], x[30001:]]
    flat, starts = _pack(parts)
    lens = [p.size for p in parts]
    for groups in ([0, 1, 2], [0, 2]):
        want, detail, E = R.measure(parts, fs, groups)
        for l, gamma in detail:
            assert R.gate_margin(l, gamma) > 0.01
        got = _measure(dev, flat, starts, lens, fs, groups)[0]
        assert got.shape == want.shape
        pref, _ = _reference("gating%s-parts" % name, parts, fs)
        tol = max(_lufs_bound(pref[b][0], pref[b][2], lens[b], fs) for b in range(2))
        for g in range(len(groups) - 1):
            assert got[g, 1:4].tolist() == want[g, 1:4].tolist() and got[g, 5] == want[g, 5] and got[g, 6] == want[g, 6]
            print("gating %s groups %s row %d: %.6f vs %.6f (bound %.3e)" % (name, groups, g, got[g, 0], want[g, 0], tol))
            assert abs(got[g, 0] - want[g, 0]) <= tol if np.isfinite(want[g, 0]) else got[g, 0] == want[g, 0]
    assert want[0, 1] == 34 + 39                                                  # blocks never straddle items: 4 fewer


def test_true_peak_against_float64(dev):
    """the CPU test's tones at 8 kHz in one batch, items of 0 and 1 sample, and noise over several workgroups"""
    fs = 8000
    tones = [R.faded_tone(fs, fs / d, p) for d, p in ((4.0, 0.0), (4.0, np.pi / 4), (6.0, np.pi / 6), (8.0, np.pi / 8),
                                                      (3.0, np.pi / 6), (2.5, 0.0))]
    rng = np.random.RandomState(23)
    items = tones + [np.zeros(0, np.float32), np.array([-0.625], np.float32), (0.4 * rng.randn(2500)).astype(np.float32)]
    flat, starts = _pack(items)
    lens = [it.size for it in items]
    rows = _measure(dev, flat, starts, lens, fs, true_peak=True)[0]
    plain = _measure(dev, flat, starts, lens, fs)[0]
    for b, x in enumerate(items):
        want, asum = R.true_peak(x, want_abs_sum=True)
        bound = 2.0 * 13.0 * 2.0 ** -24 * asum
        print("true peak item %d: %.7f vs %.7f (bound %.3e), sample peak %.7f" % (b, rows[b, 5], want, bound, plain[b, 5]))
        assert abs(rows[b, 5] - want) <= bound, (b, rows[b, 5], want)
        assert plain[b, 5] == (float(np.abs(x).max()) if x.size else 0.0) and rows[b, 5] >= plain[b, 5]
        assert np.array_equal(rows[b, :5], plain[b, :5], equal_nan=True)
    assert rows[6, 5] == 0.0 and rows[7, 5] == 0.625
    for b in (0, 1, 2, 3, 5):
        assert abs(20 * np.log10(rows[b, 5]) - (-6.0206)) <= 0.05, b
    assert abs(20 * np.log10(plain[1, 5]) - (-9.03)) < 0.01


GAIN_ROWS = np.array([[-30.0, 10, 10, 10, -28.0, 0.1, 0],
                      [-30.0, 10, 10, 10, -28.0, 0.5, 0],
                      [-80.0, 10, 10, 10, -75.0, 1e-4, 0],
                      [-float("inf"), 10, 0, 0, -float("inf"), 0.0, 2],
                      [-20.0, 0, 0, 0, -float("inf"), 0.2, 1],
                      [-17.123456789, 50, 40, 30, -12.0, 0.0, 0]], dtype=np.float64)


@pytest.mark.parametrize("target,ceiling_db,max_gain_db", [(-23.0, -1.0, 30.0), (-16.0, -2.0, 6.0), (-31.5, 0.0, 120.0)])
def test_gains_bit_for_bit(dev, target, ceiling_db, max_gain_db):
    from deepvoice3_pytorch_amd import _lib
    groups = [0, 1, 2, 3, 5, 6, 7]
    B, G = 7, 6
    lin = lambda db: 10.0 ** (db / 20.0)
    rows = torch.from_numpy(GAIN_ROWS).to(dev)
    goff = torch.tensor(groups, dtype=torch.int32, device=dev)
    out = torch.full((B + 8,), SENTINEL, dtype=torch.float32, device=dev)
    _lib.call("dv3_loudness_gains_f32", rows.data_ptr(), goff.data_ptr(), B, G, target, lin(ceiling_db), lin(max_gain_db),
              out[4:].data_ptr(), None)
    got = out.cpu().numpy()
    assert np.all(got[:4] == SENTINEL) and np.all(got[4 + B:] == SENTINEL)
    want = R.gains(GAIN_ROWS, groups, target, lin(ceiling_db), lin(max_gain_db))
    assert np.array_equal(got[4:4 + B].view(np.int32), want.view(np.int32)), (got[4:4 + B], want)
    assert want[3] == want[4] == 1.0


# ----------------------------------------------------------------------------------------------------------------------
# mastering: master_items, join_utterances, and the by-hand composition
# ----------------------------------------------------------------------------------------------------------------------
def _speechlike(fs, seconds, level_db, seed, f0=180.0):
    """a harmonic tone under a slow envelope, well above the absolute gate"""
    rng = np.random.RandomState(seed)
    n = int(seconds * fs)
    t = np.arange(n) / float(fs)
    env = 0.55 + 0.45 * np.sin(2 * np.pi * 1.7 * t + rng.uniform(0, 6))
    x = sum(np.sin(2 * np.pi * f0 * k * t + rng.uniform(0, 6)) / k for k in (1, 2, 3, 5))
    return (10.0 ** (level_db / 20.0) * env * x / 2.0).astype(np.float32)


def _remeasure(dev, out, starts, lens, fs, groups):
    from deepvoice3_pytorch_amd import audio
    return audio.wave_loudness(out.reshape(-1), starts, lens, fs, groups).cpu().numpy()


@pytest.mark.parametrize("scope", ["item", "document"])
def test_master_items_under_lufs(dev, scope):
    """item 0 and 1: plain; item 2: peaky, the -1 dB ceiling binds; item 3: nearly silent, max_gain_db binds; item 4: short"""
    from deepvoice3_pytorch_amd import audio
    fs, L = 8000, 8000
    lens = [8000, 6000, 7000, 5000, 2000]
    sig = [_speechlike(fs, 1.0, -30.0, 1), _speechlike(fs, 0.75, -16.0, 2), _speechlike(fs, 0.875, -40.0, 3),
           _speechlike(fs, 0.625, -45.0, 4), _speechlike(fs, 0.25, -20.0, 5)]
    sig[2][3000] = 0.9                                                    # one click far above the programme
    batch = np.zeros((5, L), np.float32)
    for b, s in enumerate(sig):
        batch[b, :lens[b]] = s[:lens[b]]
    batch[1, lens[1]:] = 5.0                                              # padding louder than anything: never read
    x = torch.from_numpy(batch).to(dev)
    groups = list(range(6)) if scope == "item" else [0, 5]
    items = [batch[b, :n] for b, n in enumerate(lens)]
    want_rows, detail, _ = R.measure(items, fs, groups)
    for l, gamma in detail:
        assert R.gate_margin(l, gamma) > 0.01, "a block within 0.01 LU of a gate: no fair input"
    m = audio.Mastering("lufs", scope=scope, dtype="float32", max_gain_db=25.0)
    with pytest.raises(ValueError, match="sample_rate"):
        audio.master_items(x, lens, m)
    got = audio.master_items(x, lens, m, fs)
    starts = np.arange(5) * L
    rows = audio.wave_loudness(x, starts, lens, fs, groups)
    gain = audio.loudness_gains(rows, groups, m)
    Lp = -(-L // 8) * 8
    by_hand = audio.wave_master(x.reshape(-1), starts, lens, np.arange(5) * Lp, gain, 0, 5 * Lp, dtype="float32")
    assert torch.equal(got, by_hand.view(5, Lp)[:, :L])
    rows_h, gain_h = rows.cpu().numpy(), gain.cpu().numpy()
    lin = lambda db: 10.0 ** (db / 20.0)
    assert np.array_equal(gain_h.view(np.int32), R.gains(rows_h, groups, -23.0, lin(-1.0), lin(25.0)).view(np.int32))
    # end to end: the gains from the reference's own rows, within the bound of the docstring (the sample peak is exact)
    ref, _ = _reference("master_items", items, fs)
    d_lufs = max(_lufs_bound(ref[b][0], ref[b][2], lens[b], fs) for b in range(5))
    want_gain = R.gains(want_rows, groups, -23.0, lin(-1.0), lin(25.0)).astype(np.float64)
    rel = d_lufs * math.log(10.0) / 20.0 + 2.0 ** -23
    print("gains end to end (%s): max relative difference %.3e (bound %.3e)" % (
        scope, np.abs(gain_h / want_gain - 1.0).max(), rel))
    assert np.all(np.abs(gain_h - want_gain) <= rel * want_gain), (gain_h, want_gain)
    assert np.array_equal(rows_h[:, 1:4], want_rows[:, 1:4]) and np.array_equal(rows_h[:, 5:], want_rows[:, 5:])
    after = _remeasure(dev, got, starts, lens, fs, groups)
    out = got.cpu().numpy()
    if scope == "item":
        for b in (0, 1, 4):                                                # neither the ceiling nor the cap binds
            assert abs(after[b, 0] - (-23.0)) <= 0.01, (b, after[b])
        assert rows_h[4, 6] == 1 and after[4, 6] == 1
        g2 = np.float32(lin(-1.0) / float(np.float32(0.9)))
        assert gain_h[2] == g2 and np.abs(out[2]).max() == g2 * np.float32(0.9)          # the ceiling, exactly
        assert abs(float(np.abs(out[2]).max()) - lin(-1.0)) <= 2.0 ** -23 and after[2, 0] < -24.0
        assert gain_h[3] == np.float32(lin(25.0)) and after[3, 0] < -24.0                  # the cap
    else:
        assert len(set(gain_h.tolist())) == 1 and rows_h.shape == (1, 7)
        assert gain_h[0] == np.float32(lin(-1.0) / float(np.float32(0.9)))                                    # the click binds for all
        m2 = audio.Mastering("lufs", scope=scope, dtype="float32", ceiling_db=0.0, target_db=-36.0)
        got2 = audio.master_items(x, lens, m2, fs)
        after2 = _remeasure(dev, got2, starts, lens, fs, groups)
        assert abs(after2[0, 0] - (-36.0)) <= 0.01 and after2[0, 1] == rows_h[0, 1]
    assert not out[1, lens[1]:].any()


def test_true_peak_ceiling_attenuates_where_the_sample_peak_does_not(dev):
    """the fs/4 tone at 45 degrees, amplitude 0.95: every sample reads 0.67 (-3.5 dBFS), the waveform peaks at -0.45 dBTP"""
    from deepvoice3_pytorch_amd import audio
    fs = 8000
    x = R.faded_tone(fs, fs / 4.0, np.pi / 4, amp=0.95, seconds=1.0)
    xd = torch.from_numpy(x[None]).to(dev)
    rows = audio.wave_loudness(xd, [0], [x.size], fs).cpu().numpy()
    target = float(rows[0, 0])                                           # ask for the level it already has
    plain = audio.Mastering("lufs", target_db=target, dtype="float32")
    tp = audio.Mastering("lufs", target_db=target, dtype="float32", true_peak=True)
    g_plain = audio.loudness_gains(audio.wave_loudness(xd, [0], [x.size], fs), [0, 1], plain).item()
    rows_tp = audio.wave_loudness(xd, [0], [x.size], fs, true_peak=True)
    g_tp = audio.loudness_gains(rows_tp, [0, 1], tp).item()
    assert abs(g_plain - 1.0) < 1e-6                                     # the sample-peak ceiling does not bind
    peak = rows_tp.cpu().numpy()[0, 5]
    assert abs(peak - 0.95) < 0.002 and g_tp == np.float32(10.0 ** (-1 / 20.0) / peak) and g_tp < 0.94
    out = audio.master_items(xd, [x.size], tp, fs)
    assert torch.equal(out, audio.wave_master(xd.reshape(-1), [0], [x.size], [0], torch.tensor([g_tp], device=dev), 0,
                                               x.size, dtype="float32").view(1, -1))
    again = audio.wave_loudness(out, [0], [x.size], fs, true_peak=True).cpu().numpy()
    assert abs(again[0, 5] - 10.0 ** (-1 / 20.0)) < 1e-6


@pytest.mark.parametrize("scope", ["item", "document"])
def test_join_utterances_under_lufs(dev, scope):
    from deepvoice3_pytorch_amd import audio, synthesis
    fs = 8000
    sig = [_speechlike(fs, 1.0, -28.0, 7), _speechlike(fs, 0.6, -14.0, 8, 240.0), _speechlike(fs, 0.8, -21.0, 9, 140.0)]
    sig = [np.concatenate([np.zeros(2100, np.float32), s, np.zeros(2100, np.float32)]) for s in sig]
    wavs = [torch.from_numpy(s).to(dev) for s in sig]
    m = audio.Mastering("lufs", scope=scope, dtype="float32", fade_ms=0.0, target_db=-20.0)
    doc, where, plan = synthesis.join_utterances(wavs, fs, pauses=0.1, trim_db=30.0, mastering=m, return_plan=True)
    flat = torch.cat(wavs)
    lens = np.array([w.numel() for w in wavs])
    starts = np.concatenate([[0], np.cumsum(lens)[:-1]])
    t_start, t_len = audio.trim_items(flat, starts, lens, 30.0)
    src, tl = t_start.cpu().numpy(), t_len.cpu().numpy()
    assert (tl < lens).all() and np.array_equal(plan["src"], src) and np.array_equal(plan["len"], tl)
    groups = [0, 1, 2, 3] if scope == "item" else [0, 3]
    host = flat.cpu().numpy()
    for l, gamma in R.measure([host[a:a + n] for a, n in zip(src, tl)], fs, groups)[1]:
        assert R.gate_margin(l, gamma) > 0.01, "a block within 0.01 LU of a gate: no fair input"
    rows = audio.wave_loudness(flat, src, tl, fs, groups)
    gain = audio.loudness_gains(rows, groups, m)
    want = audio.wave_master(flat, plan["src"], plan["len"], plan["dst"], gain, plan["flags"], plan["N"], 0, "float32")
    assert torch.equal(doc, want)
    after = _remeasure(dev, doc, plan["dst"], plan["len"], fs, groups)
    assert np.abs(after[:, 0] - (-20.0)).max() <= 0.01, after[:, 0]
    g = gain.cpu().numpy()
    assert (len(set(g.tolist())) == 1) == (scope == "document")
    if scope == "document":
        per_item = audio.wave_loudness(flat, src, tl, fs).cpu().numpy()
        assert rows.cpu().numpy()[0, 1] == per_item[:, 1].sum() and np.ptp(per_item[:, 0]) > 5.0
    m16 = audio.Mastering("lufs", scope=scope, true_peak=True)                    # int16, fades, a dBTP ceiling: composition only
    doc16, _, plan16 = synthesis.join_utterances(wavs, fs, mastering=m16, return_plan=True)
    gain16 = audio.loudness_gains(audio.wave_loudness(flat, plan16["src"], plan16["len"], fs, groups, True), groups, m16)
    want16 = audio.wave_master(flat, plan16["src"], plan16["len"], plan16["dst"], gain16, plan16["flags"], plan16["N"],
                               m16.fade_samples(fs), "int16")
    assert doc16.dtype == torch.int16 and torch.equal(doc16, want16)


def test_old_levels_keep_their_bits(dev):
    """mastering=None and "peak", "rms", "reference": master_items (with and without a sample rate) against
    tests/master_ref.py from the device's own levels, as before the loudness level existed"""
    from deepvoice3_pytorch_amd import audio
    rng = np.random.RandomState(4)
    lens = [3001, 1200, 0, 2500]
    L = 3001
    batch = (rng.randn(4, L) * np.array([0.05, 0.4, 1.0, 2.0])[:, None]).astype(np.float32)
    x = torch.from_numpy(batch).to(dev)
    starts = np.arange(4) * L
    lin = lambda db: 10.0 ** (db / 20.0)
    for m in (audio.Mastering("peak"), audio.Mastering("rms", scope="document", dtype="float32"), audio.Mastering("rms"),
              audio.Mastering("reference"), audio.Mastering(None), audio.Mastering("peak", dither=True, seed=11)):
        got = audio.master_items(x, lens, m).cpu().numpy()
        assert np.array_equal(got, audio.master_items(x, lens, m, 8000).cpu().numpy())
        groups = list(range(5)) if m.scope == "item" else [0, 4]
        if m.level is None:
            gain = np.ones(4, np.float32)
        else:
            dev_rows = audio.wave_levels(x, starts, lens).cpu().numpy()
            policy = {"peak": M.GAIN_PEAK, "rms": M.GAIN_RMS, "reference": M.GAIN_REFERENCE}[m.level]
            gain = M.gains(dev_rows, lens, groups, policy, lin(m.target_db), lin(m.ceiling_db), lin(m.max_gain_db))
        mode = M.MODE_I16_REFERENCE if m.level == "reference" else (M.MODE_F32 if m.dtype == "float32" else M.MODE_I16)
        for b, n in enumerate(lens):
            want = M.master(batch[b], [0], [n], [0], gain[b:b + 1], [0], M.fade_table(0), L, mode, m.dither, m.seed)
            a, w = got[b], want
            assert np.array_equal(a.view(np.int32) if a.dtype == np.float32 else a,
                                  w.view(np.int32) if w.dtype == np.float32 else w), (m.level, m.scope, b)


# ----------------------------------------------------------------------------------------------------------------------
# through synthesis
# ----------------------------------------------------------------------------------------------------------------------
E2E_HP = dict(n_vocab=40, embed_dim=32, mel_dim=20, linear_dim=257, r=1, downsample_step=4, padding_idx=0, dropout=0.05,
              kernel_size=3, encoder_channels=64, decoder_channels=32, converter_channels=32, use_memory_mask=True,
              force_monotonic_attention=True, use_decoder_state_for_postnet_input=True, key_projection=True,
              value_projection=True, max_positions=128)


@pytest.fixture(scope="module")
def spoken(dev):
    """the tiny random model of tests/test_gpu_master.py at 512 / 128 and 16 kHz; 20 decoder steps give 10240 samples, three
    blocks of 6400 at h = 1600"""
    from deepvoice3_pytorch_amd import audio, builder, synthesis
    torch.manual_seed(0)
    model = builder.deepvoice3(**E2E_HP).to(dev).eval()
    dec = model.seq2seq.decoder
    dec.min_decoder_steps = dec.max_decoder_steps = 20
    rng = np.random.RandomState(2)
    ids = [rng.randint(2, 40, n).tolist() for n in (9, 14, 6)]
    cfg = audio.AudioConfig(fft_size=512, hop_size=128, sample_rate=16000, griffin_lim_iters=3)
    plain = synthesis.tts_batch(model, ids, audio_cfg=cfg)
    return model, ids, cfg, plain


@pytest.mark.parametrize("kind", ["lufs", "lufs-tp-document"])
def test_the_three_entry_points_agree_under_lufs(dev, spoken, kind):
    from deepvoice3_pytorch_amd import audio, synthesis
    model, ids, cfg, plain = spoken
    m = audio.Mastering("lufs") if kind == "lufs" else audio.Mastering("lufs", scope="document", true_peak=True, dtype="float32")
    res = synthesis.tts_batch(model, ids, audio_cfg=cfg, mastering=m)
    L = max(r[3].numel() for r in plain)
    wavs = torch.zeros(len(ids), L, device=dev)
    for b, r in enumerate(plain):
        wavs[b, :r[3].numel()] = r[3]
    by_hand = audio.master_items(wavs, [r[3].numel() for r in plain], m, cfg.sample_rate)
    for b in range(len(ids)):
        assert torch.equal(res[b][3], by_hand[b, :plain[b][3].numel()]), b
        assert not torch.equal(res[b][3].float(), plain[b][3])
    if kind == "lufs":                                  # every utterance alone: the admission order cannot matter
        got = {r[0]: r for r in synthesis.tts_stream(model, ids, slots=2, audio_cfg=cfg, mastering=m)}
        rs = synthesis.RollingSynthesizer(model, slots=3, max_text_len=14, audio_cfg=cfg, mastering=m)
        tickets = [rs.submit(s) for s in ids]
        rolled = {r[0]: r[4] for r in rs.drain()}
        for b in range(len(ids)):
            assert torch.equal(got[b][4], res[b][3]), (b, "tts_stream")
            assert torch.equal(rolled[tickets[b]], res[b][3]), (b, "RollingSynthesizer")
        rows = audio.wave_loudness(wavs, np.arange(len(ids)) * L, [r[3].numel() for r in plain], cfg.sample_rate).cpu().numpy()
        assert rows[:, 1].min() >= 1, "the utterances hold no complete block: the gated path was not reached"


def test_tts_document_is_the_by_hand_composition(dev, spoken):
    from deepvoice3_pytorch_amd import audio, synthesis
    model, ids, cfg, plain = spoken
    m = audio.Mastering("lufs", scope="document", fade_ms=4.0)
    doc, where = synthesis.tts_document(model, ids, batch=2, audio_cfg=cfg, pauses=0.05, trim_db=3.0, mastering=m)
    wavs = [r[3] for r in plain]
    lens = np.array([w.numel() for w in wavs])
    starts = np.concatenate([[0], np.cumsum(lens)[:-1]])
    flat = torch.cat(wavs)
    t_start, t_len = audio.trim_items(flat, starts, lens, 3.0)
    src, tl = t_start.cpu().numpy(), t_len.cpu().numpy()
    F = m.fade_samples(cfg.sample_rate)
    table, N = synthesis.plan_document(tl, cfg.sample_rate, 0.05, F, starts=src)
    rows = audio.wave_loudness(flat, src, tl, cfg.sample_rate, [0, 3])
    gain = audio.loudness_gains(rows, [0, 3], m)
    want = audio.wave_master(flat, table["src"], table["len"], table["dst"], gain, table["flags"], N, F, "int16")
    assert doc.dtype == torch.int16 and doc.numel() == N and torch.equal(doc, want)
    assert len(set(gain.tolist())) == 1 and len(where) == 3


# ----------------------------------------------------------------------------------------------------------------------
# refusals
# ----------------------------------------------------------------------------------------------------------------------
def test_refusals(dev):
    """every refusal of the three entry points by value; nothing is launched, so the guarded tables keep their fill"""
    from deepvoice3_pytorch_amd import _lib, audio
    h = _lib.lib()
    EINVAL = _lib.CONSTS["DV3_EINVAL"]
    kw = audio.k_weighting(8000)
    coef = (ctypes.c_double * 10)(*kw["coef"].tolist())
    Ah = (ctypes.c_double * 16)(*kw["Ah"].reshape(-1).tolist())
    tab = (ctypes.c_float * 36)(*audio.true_peak_table().reshape(-1).tolist())
    bad_coef = (ctypes.c_double * 10)(*([float("nan")] + kw["coef"].tolist()[1:]))
    bad_Ah = (ctypes.c_double * 16)(*([float("inf")] + kw["Ah"].reshape(-1).tolist()[1:]))
    bad_tab = (ctypes.c_float * 36)(*([float("nan")] + [0.0] * 35))
    A = ctypes.addressof
    x = torch.ones(2048, device=dev)
    one, n = _i64(dev, [0]), _i64(dev, [1000])
    f64 = dict(dtype=torch.float64, device=dev)
    states, energy = torch.full((2, 4), SENTINEL, **f64), torch.full((2,), SENTINEL, **f64)
    scratch, tp = torch.full((1,), SENTINEL, **f64), torch.full((1,), SENTINEL, **f64)
    good = [x.data_ptr(), one.data_ptr(), n.data_ptr(), 1, 1000, 800, A(coef), A(Ah), A(tab), states.data_ptr(),
            energy.data_ptr(), scratch.data_ptr(), tp.data_ptr(), None]
    for pos, bad in ((0, None), (1, None), (2, None), (6, None), (7, None), (9, None), (10, None), (8, None), (12, None),
                     (11, None), (3, 0), (3, 65536), (4, -1), (4, 2 ** 30 + 1), (5, 799), (5, 19201), (6, A(bad_coef)),
                     (7, A(bad_Ah)), (8, A(bad_tab)), (9, states.data_ptr() + 8), (10, energy.data_ptr() + 4),
                     (12, tp.data_ptr() + 4)):
        args = list(good)
        args[pos] = bad
        assert h.dv3_wave_loudness_f64(*args) == EINVAL, ("loudness", pos, bad)
        assert h.dv3_last_error().decode().startswith("wave_loudness:"), h.dv3_last_error()
    torch.cuda.synchronize()
    for t in (states, energy, scratch, tp):
        assert torch.all(t == SENTINEL), "a refused call launched something"
    assert h.dv3_wave_loudness_f64(*good) == 0
    no_tp = list(good)
    no_tp[8] = no_tp[11] = no_tp[12] = None
    assert h.dv3_wave_loudness_f64(*no_tp) == 0
    torch.cuda.synchronize()
    assert abs(tp.item() - R.true_peak(np.ones(1000, np.float32))) < 1e-5 and abs(energy.sum().item() - R.sub_blocks(np.ones(1000, np.float32), 8000).sum()) < 1e-9
    goff = torch.tensor([0, 1], dtype=torch.int32, device=dev)
    rows = torch.full((1, 7), SENTINEL, **f64)
    good = [energy.data_ptr(), n.data_ptr(), goff.data_ptr(), tp.data_ptr(), 1, 1, 1, 1000, 800, rows.data_ptr(), None]
    for pos, bad in ((0, None), (1, None), (2, None), (3, None), (9, None), (4, 0), (4, 65), (5, 0), (5, 65536), (6, 0),
                     (6, 2), (7, -1), (7, 2 ** 30 + 1), (8, 799), (8, 19201), (9, rows.data_ptr() + 4), (0, energy.data_ptr() + 4)):
        args = list(good)
        args[pos] = bad
        assert h.dv3_loudness_gate_f64(*args) == EINVAL, ("gate", pos, bad)
        assert h.dv3_last_error().decode().startswith("loudness_gate:")
    torch.cuda.synchronize()
    assert torch.all(rows == SENTINEL)
    assert h.dv3_loudness_gate_f64(*good) == 0
    gain = torch.full((1,), SENTINEL, device=dev)
    good = [rows.data_ptr(), goff.data_ptr(), 1, 1, -23.0, 0.9, 30.0, gain.data_ptr(), None]
    for pos, bad in ((0, None), (1, None), (7, None), (2, 0), (2, 65536), (3, 0), (3, 2), (4, 0.5), (4, -121.0),
                     (4, float("nan")), (5, 0.0), (5, float("inf")), (6, -1.0), (6, float("nan")), (0, rows.data_ptr() + 4)):
        args = list(good)
        args[pos] = bad
        assert h.dv3_loudness_gains_f32(*args) == EINVAL, ("gains", pos, bad)
        assert h.dv3_last_error().decode().startswith("loudness_gains:")
    torch.cuda.synchronize()
    assert gain.item() == SENTINEL
    assert h.dv3_loudness_gains_f32(*good) == 0
    torch.cuda.synchronize()
    r = rows.cpu().numpy()
    assert r[0, 6] == 1 and gain.item() == R.gains(r, [0, 1], -23.0, 0.9, 30.0)[0]
    # the Python wrappers
    with pytest.raises(ValueError, match="sample_rate"):
        audio.wave_loudness(x, [0], [1000], 4000)
    with pytest.raises(ValueError, match="groups"):
        audio.wave_loudness(x, [0], [1000], 8000, groups=[0, 2])
    with pytest.raises(ValueError, match="max_len"):
        audio.wave_loudness(x, one, n, 8000)
    with pytest.raises(ValueError, match="rows"):
        audio.loudness_gains(rows[:, :5], [0, 1], audio.Mastering("lufs"))
    with pytest.raises(ValueError, match="lufs"):
        audio.loudness_gains(rows, [0, 1], audio.Mastering("peak"))

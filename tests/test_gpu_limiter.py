# coding: utf-8
"""-m gpu: the look-ahead peak limiter (csrc/limiter.hip; include/dv3hip.h: dv3_wave_limit_f32) against
the float64 restatement of tests/limiter_ref.py, whose docstring derives the two bounds used here: the float64 tables
(gain_min) to 1e-12 absolute, `out` to one float32 rounding of s plus one of the product relative to |y|, against the
unrounded y s.  over_samples, empty spans, what lies outside the spans and every "bit for bit" below are exact.

Shapes (T = DV3_LIMIT_TILE): seven and six spans at odd offsets of one flat buffer with NaN between them, lengths
0, 1, 2, A, A + 1, T - 1, T, T + 1, 2 T + A + 3 and 3 T + 517 over two layouts; A in {0, 1, 33, DV3_LIMIT_MAX_LOOKAHEAD};
rho for 50 ms and for 400 ms at 22 050 Hz (the second carries a release over three tiles: the walk).  Signals: noise at
0.05 with spikes of 0.5 .. 1.0 at sample 0, at the last sample, at T - 1, T and T + 1 and at pairs A and A + 1 apart;
g = 1.7, c = 0.7; both detectors."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tests import limiter_ref as R  # noqa: E402
from tests import loudness_ref as LR  # noqa: E402

pytestmark = pytest.mark.gpu

FS = 22050
T = 1024
AMAX = 512
G, C = 1.7, 0.7
RHOS = {50: float(np.exp(-1000.0 / (50.0 * FS))), 400: float(np.exp(-1000.0 / (400.0 * FS)))}
SENTINEL = -7.25
TP_TOL = 1e-6                 # tests/test_gpu_loudness.py: the static true-peak ceiling is met within 1e-6


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


def _i64(dev, v):
    return torch.tensor([int(a) for a in v], dtype=torch.int64, device=dev)


def _lengths(A, layout):
    return [(0, 1, A, T - 1, T + 1, 2 * T + A + 3, 3 * T + 517), (2, A + 1, T, 0, 3 * T + 517, T - 1)][layout]


def _signal(n, A, seed):
    at = (0, n - 1, T - 1, T, T + 1, 300, 300 + A, 700, 700 + A + 1, 2 * T - 7, 2 * T - 7 + A, 3 * T - 2, 3 * T - 2 + A + 1)
    return R.spikes(n, seed, at=at)


def _pack(items, shift=0):
    """-> (flat float32 with NaN between the spans, starts): odd, unaligned starts, all moved by `shift`"""
    starts, o = [], 3 + shift
    for it in items:
        starts.append(o)
        o += it.size + 4
        o += 1 - (o - shift) % 2
    flat = np.full(o + 16, np.nan, dtype=np.float32)
    for s, it in zip(starts, items):
        flat[s:s + it.size] = it
    return flat, starts


def _direct(dev, flat, starts, lengths, gains, c, A, rho, true_peak, max_len=None):
    """dv3_wave_limit_f32 called by name on sentinel-filled tables -> (out, report) on the host"""
    from deepvoice3_pytorch_amd import _lib, audio
    x = torch.from_numpy(flat).to(dev)
    B = len(starts)
    max_len = max(lengths) if max_len is None else max_len
    st, ln = _i64(dev, starts), _i64(dev, lengths)
    gain = torch.tensor(gains, dtype=torch.float32, device=dev)
    scratch = torch.empty(max(B * -(-max_len // T) * (T + 3), 1), dtype=torch.float64, device=dev)
    out = torch.full_like(x, SENTINEL)
    report = torch.full((B, 2), SENTINEL, dtype=torch.float64, device=dev)
    powers = (ctypes.c_double * 11)(*audio.rho_powers(rho).tolist())
    table = (ctypes.c_float * 36)(*audio.true_peak_table().reshape(-1).tolist())
    _lib.call("dv3_wave_limit_f32", x.data_ptr(), st.data_ptr(), ln.data_ptr(), B, max_len, gain.data_ptr(), float(c), int(A),
              ctypes.addressof(powers), ctypes.addressof(table) if true_peak else None, scratch.data_ptr(), out.data_ptr(),
              report.data_ptr(), None)
    torch.cuda.synchronize()
    return out.cpu().numpy(), report.cpu().numpy()


def _check(name, items, starts, out, report, refs, outside=None):
    worst = 0.0
    for b, (x, s, ref) in enumerate(zip(items, starts, refs)):
        got = out[s:s + x.size].astype(np.float64)
        err, bound = np.abs(got - ref["exact"]), R.out_bound(ref["y"])
        if x.size:
            worst = max(worst, float((err / bound).max()))
        assert np.all(err <= bound), (name, b, x.size, float((err / bound).max()))
        assert report[b, 1] == ref["report"][1], (name, b, report[b], ref["report"])
        assert abs(report[b, 0] - ref["report"][0]) <= R.TABLE_TOL, (name, b, report[b], ref["report"])
        if x.size == 0:
            assert report[b, 0] == 1.0 and report[b, 1] == 0.0
    if outside is not None:
        mask = np.ones(out.size, bool)
        for x, s in zip(items, starts):
            mask[s:s + x.size] = False
        assert np.all(out[mask] == outside), (name, "a sample outside the spans was written")
    return worst


@pytest.mark.parametrize("layout", [0, 1])
@pytest.mark.parametrize("true_peak", [False, True])
@pytest.mark.parametrize("A", [0, 1, 33, AMAX])
def test_element_by_element_against_float64(dev, A, true_peak, layout):
    from deepvoice3_pytorch_amd import _lib, audio
    assert (_lib.CONSTS["DV3_LIMIT_TILE"], _lib.CONSTS["DV3_LIMIT_MAX_LOOKAHEAD"]) == (T, AMAX)
    lengths = _lengths(A, layout)
    items = [_signal(n, A, 10 * layout + b) for b, n in enumerate(lengths)]
    flat, starts = _pack(items)
    for ms, rho in sorted(RHOS.items()):
        refs = [R.limit(x, G, C, A, rho, true_peak) for x in items]
        assert sum(r["report"][1] for r in refs) >= 20 and min(r["report"][0] for r in refs) < 0.5
        out, report = _direct(dev, flat, starts, lengths, [G] * len(items), C, A, rho, true_peak)
        worst = _check("direct", items, starts, out, report, refs, SENTINEL)
        out2, report2 = _direct(dev, flat, starts, lengths, [G] * len(items), C, A, rho, true_peak)
        assert np.array_equal(out.view(np.int32), out2.view(np.int32)) and np.array_equal(report, report2)
        x = torch.from_numpy(flat).to(dev)
        lim, rep = audio.limit_spans(x, _i64(dev, starts), _i64(dev, lengths), max(lengths), torch.full(
            (len(items),), G, dtype=torch.float32, device=dev), C, A, rho, true_peak)
        assert lim.dtype == torch.float32 and lim.shape == x.shape and tuple(rep.shape) == (len(items), 2)
        lim = lim.cpu().numpy()
        _check("limit_spans", items, starts, lim, rep.cpu().numpy(), refs, 0.0)
        for x_b, s in zip(items, starts):                 # the wrapper and the direct call: the same bits
            assert np.array_equal(lim[s:s + x_b.size].view(np.int32), out[s:s + x_b.size].view(np.int32))
        print("A = %d, true_peak %r, layout %d, release %d ms: worst error / bound %.3f" % (A, true_peak, layout, ms, worst))
        if not true_peak:                                 # the ceiling, derived: one rounding of s and one of the product
            for x_b, s in zip(items, starts):
                if x_b.size:
                    assert np.abs(out[s:s + x_b.size]).max() <= C * (1.0 + 2.0 ** -22)


def test_host_spans_and_a_scalar_gain(dev):
    from deepvoice3_pytorch_amd import audio
    items = [_signal(n, 33, 40 + b) for b, n in enumerate((T + 1, 700))]
    flat, starts = _pack(items)
    lim, rep = audio.limit_spans(torch.from_numpy(flat).to(dev), starts, [x.size for x in items], None, G, C, 33, RHOS[50])
    refs = [R.limit(x, G, C, 33, RHOS[50]) for x in items]
    _check("host spans", items, starts, lim.cpu().numpy(), rep.cpu().numpy(), refs, 0.0)


def _true_peak_bound(x, c):
    """the float64 true peak of a trimmed output meets c within TP_TOL plus what the device's float32 interpolation can
    differ from float64 by where it measured the trim (tests/test_gpu_loudness.py: 2 * 13 * 2^-24 * sum |tap * sample|)"""
    peak, abs_sum = LR.true_peak(x, want_abs_sum=True)
    return peak <= c + TP_TOL + 2.0 * 13.0 * 2.0 ** -24 * abs_sum


def test_the_true_peak_ceiling_with_the_trim(dev):
    """through master_items(dtype="float32"): the limiter's true-peak detector, then the trim min(1, c / peak) as the
    master launch's gain -- the measured true peak meets the ceiling within the tolerance of the static ceiling"""
    from deepvoice3_pytorch_amd import audio
    fs = 8000
    lens = [3589, 2500, 4001]
    L = max(lens)
    batch = np.zeros((3, L), np.float32)
    for b, n in enumerate(lens):
        batch[b, :n] = _signal(n, 12, 60 + b)
    x = torch.from_numpy(batch).to(dev)
    m = audio.Mastering("lufs", target_db=-12.0, dtype="float32", true_peak=True, limiter=audio.Limiter())
    c = 10.0 ** (-1.0 / 20.0)
    got = audio.master_items(x, lens, m, fs)
    peaks = audio.wave_loudness(got, np.arange(3) * L, lens, fs, true_peak=True).cpu().numpy()[:, 5]
    print("true peaks after the trim:", peaks - c)
    assert np.all(peaks <= c + TP_TOL) and np.all(peaks >= 0.9 * c), peaks
    host = got.cpu().numpy()
    for b, n in enumerate(lens):
        assert _true_peak_bound(host[b, :n], c) and not host[b, n:].any()
    # by hand: the same source and trim from master_source
    st, ln = _i64(dev, np.arange(3) * L), _i64(dev, lens)
    src, trim = audio.master_source(x.reshape(-1), st, ln, L, m, fs)
    Lp = -(-L // 8) * 8
    want = audio.wave_master(src, np.arange(3) * L, lens, np.arange(3) * Lp, trim, 0, 3 * Lp, dtype="float32")
    assert torch.equal(got, want.view(3, Lp)[:, :L]) and trim.dtype == torch.float32 and float(trim.max()) <= 1.0
    # the sample-peak detector on the same batch leaves inter-sample overs: the reason the other one exists
    sp = audio.Mastering("lufs", target_db=-12.0, dtype="float32", limiter=audio.Limiter())
    got_sp = audio.master_items(x, lens, sp, fs)
    assert float(got_sp.abs().max()) <= c * (1.0 + 2.0 ** -22)


def _quiet(n, seed, level=0.05):
    rng = np.random.RandomState(seed)
    t = np.arange(n) / 8000.0
    return (level * (np.sin(2 * np.pi * 180.0 * t + rng.uniform(0, 6)) + 0.5 * np.sin(2 * np.pi * 540.0 * t))
            * (0.6 + 0.4 * np.sin(2 * np.pi * 1.3 * t))).astype(np.float32)


def test_no_limiting_is_bit_for_bit(dev):
    from deepvoice3_pytorch_amd import audio
    items = [R.spikes(n, 70 + b, level=0.02, lo=0.2, hi=0.4) for b, n in enumerate((T + 1, 0, 3 * T + 517, 33))]
    flat, starts = _pack(items)
    for true_peak in (False, True):
        assert max(LR.true_peak(R.pre(x, G)) for x in items) < C
        lim, rep = audio.limit_spans(torch.from_numpy(flat).to(dev), starts, [x.size for x in items], None, G, C, 33,
                                     RHOS[400], true_peak)
        lim = lim.cpu().numpy()
        for x, s in zip(items, starts):
            want = (np.float32(G) * x).astype(np.float32)
            assert np.array_equal(lim[s:s + x.size].view(np.int32), want.view(np.int32))
        assert np.array_equal(rep.cpu().numpy(), np.array([[1.0, 0.0]] * len(items)))
    fs = 8000
    lens = [8000, 5000, 6500]
    batch = np.zeros((3, 8000), np.float32)
    for b, n in enumerate(lens):
        batch[b, :n] = _quiet(n, b, 0.05 * (b + 1))
    x = torch.from_numpy(batch).to(dev)
    for kw in (dict(dtype="int16"), dict(dtype="float32"), dict(dtype="float32", true_peak=True),
               dict(dtype="int16", scope="document")):
        static = audio.master_items(x, lens, audio.Mastering("lufs", **kw), fs)
        limited = audio.master_items(x, lens, audio.Mastering("lufs", limiter=audio.Limiter(), **kw), fs)
        assert torch.equal(static, limited), kw
        assert float(static.float().abs().max()) > 0
    with pytest.raises(ValueError, match="sample_rate"):
        audio.master_items(x, lens, audio.Mastering(None, limiter=audio.Limiter()))
    same = audio.master_items(x, lens, audio.Mastering(None, limiter=audio.Limiter(), dtype="float32"), fs)
    assert torch.equal(same, x)                         # level None: the pre-gain is 1, nothing exceeds, x comes back


@pytest.mark.parametrize("true_peak", [False, True])
def test_an_item_is_limited_alone(dev, true_peak):
    from deepvoice3_pytorch_amd import audio
    A = 33
    items = [_signal(n, A, 80 + b) for b, n in enumerate((700, 2 * T + A + 3, T, 3 * T + 517, 1))]
    gains = [1.7, 1.3, 2.0, 1.7, 1.1]
    flat, starts = _pack(items)
    out, report = _direct(dev, flat, starts, [x.size for x in items], gains, C, A, RHOS[400], true_peak)
    for b in (1, 3, 4):
        for shift in (0, 5):
            f1, s1 = _pack([items[b]], shift)
            o1, r1 = _direct(dev, f1, s1, [items[b].size], [gains[b]], C, A, RHOS[400], true_peak)
            n = items[b].size
            assert np.array_equal(o1[s1[0]:s1[0] + n].view(np.int32), out[starts[b]:starts[b] + n].view(np.int32)), (b, shift)
            assert np.array_equal(r1[0], report[b])
    # a larger max_len (another tile count, another scratch layout) changes nothing either
    o2, r2 = _direct(dev, flat, starts, [x.size for x in items], gains, C, A, RHOS[400], true_peak, max_len=5 * T + 1)
    assert np.array_equal(o2.view(np.int32), out.view(np.int32)) and np.array_equal(r2, report)


@pytest.fixture(scope="module")
def syllables(dev):
    x = R.syllables(FS)
    return x, torch.from_numpy(x[None]).to(dev)


@pytest.mark.parametrize("true_peak", [False, True])
@pytest.mark.parametrize("target", [-16.0, -14.0])
def test_the_limiter_meets_the_target_the_static_gain_misses(dev, syllables, target, true_peak):
    from deepvoice3_pytorch_amd import audio
    x, xd = syllables
    c = 10.0 ** (-1.0 / 20.0)
    kw = dict(target_db=target, dtype="float32", true_peak=true_peak)
    static = audio.master_items(xd, [x.size], audio.Mastering("lufs", **kw), FS).cpu().numpy()[0]
    l_static = R.integrated(static, FS)
    limited = []
    for p in (1, 2, 3):
        out = audio.master_items(xd, [x.size], audio.Mastering("lufs", limiter=audio.Limiter(passes=p), **kw), FS)
        out = out.cpu().numpy()[0]
        limited.append(R.integrated(out, FS))
        if true_peak:
            assert _true_peak_bound(out, c)
        else:
            assert np.abs(out).max() <= c * (1.0 + 2.0 ** -22)
    print("target %g, true_peak %r: static %.3f LUFS, passes 1..3 %s" % (target, true_peak, l_static,
                                                                       ["%.3f" % v for v in limited]))
    deficit = [target - v for v in limited]
    assert target - l_static >= 1.0
    assert deficit[0] <= 0.5 * (target - l_static)
    assert deficit[1] <= deficit[0] and deficit[2] <= deficit[1]
    assert max(limited) <= target + 0.05


# ----------------------------------------------------------------------------------------------------------------------
# through synthesis
# ----------------------------------------------------------------------------------------------------------------------
E2E_HP = dict(n_vocab=40, embed_dim=32, mel_dim=20, linear_dim=257, r=1, downsample_step=4, padding_idx=0, dropout=0.05,
              kernel_size=3, encoder_channels=64, decoder_channels=32, converter_channels=32, use_memory_mask=True,
              force_monotonic_attention=True, use_decoder_state_for_postnet_input=True, key_projection=True,
              value_projection=True, max_positions=128)


@pytest.fixture(scope="module")
def spoken(dev):
    """the tiny random model of tests/test_gpu_loudness.py at 512 / 128 and 16 kHz: two utterances of 10240 samples"""
    from deepvoice3_pytorch_amd import audio, builder, synthesis
    torch.manual_seed(0)
    model = builder.deepvoice3(**E2E_HP).to(dev).eval()
    dec = model.seq2seq.decoder
    dec.min_decoder_steps = dec.max_decoder_steps = 20
    rng = np.random.RandomState(2)
    ids = [rng.randint(2, 40, n).tolist() for n in (9, 14)]
    cfg = audio.AudioConfig(fft_size=512, hop_size=128, sample_rate=16000, griffin_lim_iters=3)
    plain = synthesis.tts_batch(model, ids, audio_cfg=cfg)
    return model, ids, cfg, plain


@pytest.mark.parametrize("kind", ["lufs", "lufs-tp-2", "rms"])
def test_the_entry_points_agree_under_a_limiter(dev, spoken, kind):
    from deepvoice3_pytorch_amd import audio, synthesis
    model, ids, cfg, plain = spoken
    lim = audio.Limiter(passes=2 if kind == "lufs-tp-2" else 1)
    kw = dict(fade_ms=0.0, max_gain_db=120.0, target_db=-8.0)
    m = {"lufs": lambda: audio.Mastering("lufs", limiter=lim, **kw),
         "lufs-tp-2": lambda: audio.Mastering("lufs", true_peak=True, dtype="float32", limiter=lim, **kw),
         "rms": lambda: audio.Mastering("rms", dtype="float32", limiter=lim, **kw)}[kind]()
    static = audio.Mastering(m.level, true_peak=m.true_peak, dtype=m.dtype, **kw)
    res = synthesis.tts_batch(model, ids, audio_cfg=cfg, mastering=m)
    res_static = synthesis.tts_batch(model, ids, audio_cfg=cfg, mastering=static)
    lens = [r[3].numel() for r in plain]
    L = max(lens)
    wavs = torch.zeros(len(ids), L, device=dev)
    for b, r in enumerate(plain):
        wavs[b, :lens[b]] = r[3]
    by_hand = audio.master_items(wavs, lens, m, cfg.sample_rate)
    c = 10.0 ** (-1.0 / 20.0) * (32767.0 if m.dtype == "int16" else 1.0)
    for b in range(len(ids)):
        assert torch.equal(res[b][3], by_hand[b, :lens[b]]), (kind, b, "master_items")
        doc, _ = synthesis.join_utterances([plain[b][3]], cfg.sample_rate, pauses=0.0, trim_db=None, mastering=m, lead=0.0,
                                           tail=0.0)
        assert torch.equal(doc, res[b][3]), (kind, b, "join_utterances")
        assert not torch.equal(res[b][3], res_static[b][3]), (kind, b, "the limiter did nothing: no fair input")
        assert float(res[b][3].float().abs().max()) <= c * (1.0 + 2.0 ** -22) + (0.5 if m.dtype == "int16" else 0.0)
        # the target is -8 and the ceiling -1: the limited utterance is louder than the one the static ceiling held back
        assert float(res[b][3].float().pow(2).mean()) > float(res_static[b][3].float().pow(2).mean())
    got = {r[0]: r for r in synthesis.tts_stream(model, ids, slots=2, audio_cfg=cfg, mastering=m)}
    for b in range(len(ids)):
        assert torch.equal(got[b][4], res[b][3]), (kind, b, "tts_stream")


# ----------------------------------------------------------------------------------------------------------------------
# refusals
# ----------------------------------------------------------------------------------------------------------------------
def test_refusals(dev):
    """every refusal of dv3_wave_limit_f32 by value; nothing is launched, so the guarded tables keep their fill"""
    from deepvoice3_pytorch_amd import _lib, audio
    h = _lib.lib()
    EINVAL = _lib.CONSTS["DV3_EINVAL"]
    P = ctypes.addressof
    arr = lambda v: (ctypes.c_double * 11)(*v)
    good_pow = audio.rho_powers(0.999).tolist()
    powers = arr(good_pow)
    tab = (ctypes.c_float * 36)(*audio.true_peak_table().reshape(-1).tolist())
    bad_tab = (ctypes.c_float * 36)(*([float("inf")] + [0.0] * 35))
    bad_pows = [arr([1.0] + good_pow[1:]), arr([-0.1] + good_pow[1:]), arr([float("nan")] + good_pow[1:]),
                arr(good_pow[:3] + [good_pow[2] * 1.01] + good_pow[4:]), arr(good_pow[:10] + [float("nan")]),
                arr(good_pow[:5] + [-1e-9] + good_pow[6:])]
    x = torch.ones(4096, device=dev)
    one, n = _i64(dev, [1]), _i64(dev, [2000])
    gain = torch.full((2,), 1.5, device=dev)
    f64 = dict(dtype=torch.float64, device=dev)
    scratch = torch.full((2 * (T + 3) + 1,), SENTINEL, **f64)
    out = torch.full((4096,), SENTINEL, device=dev)
    report = torch.full((1, 2), SENTINEL, **f64)
    good = [x.data_ptr(), one.data_ptr(), n.data_ptr(), 1, 2000, gain.data_ptr(), 0.7, 33, P(powers), P(tab),
            scratch.data_ptr(), out.data_ptr(), report.data_ptr(), None]
    cases = [(0, None), (1, None), (2, None), (5, None), (8, None), (10, None), (11, None), (12, None),
             (3, 0), (3, -1), (3, 65536), (4, -1), (4, 2 ** 30 + 1), (7, -1), (7, AMAX + 1),
             (6, 0.0), (6, -0.7), (6, float("inf")), (6, float("nan")), (11, x.data_ptr()),
             (10, scratch.data_ptr() + 4), (12, report.data_ptr() + 4), (1, one.data_ptr() + 4), (2, n.data_ptr() + 4),
             (0, x.data_ptr() + 2), (11, out.data_ptr() + 2), (5, gain.data_ptr() + 2), (9, P(bad_tab))]
    cases += [(8, P(b)) for b in bad_pows]
    for pos, bad in cases:
        args = list(good)
        args[pos] = bad
        assert h.dv3_wave_limit_f32(*args) == EINVAL, (pos, bad)
        assert h.dv3_last_error().decode().startswith("wave_limit:"), h.dv3_last_error()
    torch.cuda.synchronize()
    for t in (scratch, out, report):
        assert torch.all(t == SENTINEL), "a refused call launched something"
    assert h.dv3_wave_limit_f32(*good) == 0
    no_tab = list(good)
    no_tab[9] = None
    assert h.dv3_wave_limit_f32(*no_tab) == 0
    empty = list(good)
    empty[4], empty[10] = 0, None                        # max_len 0: no scratch needed, the report alone is written
    assert h.dv3_wave_limit_f32(*empty) == 0
    torch.cuda.synchronize()
    assert report.cpu().tolist() == [[1.0, 0.0]]
    assert h.dv3_wave_limit_f32(*no_tab) == 0
    torch.cuda.synchronize()
    got, rep = out.cpu().numpy(), report.cpu().numpy()              # a constant 1.5 under 0.7: s = 0.7 / 1.5 everywhere
    assert np.all(got[1:2001] <= 0.7 * (1 + 2.0 ** -22)) and np.all(got[1:2001] >= 0.7 * (1 - 2.0 ** -22))
    assert got[0] == SENTINEL and np.all(got[2001:] == SENTINEL)
    assert abs(rep[0, 0] - 0.7 / 1.5) <= R.TABLE_TOL and rep[0, 1] == 2000.0
    # the wrappers' own refusals
    with pytest.raises(ValueError, match="max_len"):
        audio.limit_spans(x, one, n, None, 1.0, 0.7, 33, 0.999)
    with pytest.raises(ValueError, match="gain"):
        audio.limit_spans(x, one, n, 2000, torch.ones(3, device=dev), 0.7, 33, 0.999)
    with pytest.raises(RuntimeError, match="wave_limit: lookahead"):
        audio.limit_spans(x, one, n, 2000, 1.0, 0.7, AMAX + 1, 0.999)
    with pytest.raises(RuntimeError, match="wave_limit: rho"):
        audio.limit_spans(x, one, n, 2000, 1.0, 0.7, 33, 1.0)
    with pytest.raises(RuntimeError, match="wave_limit: ceiling"):
        audio.limit_spans(x, one, n, 2000, 1.0, 0.0, 33, 0.999)

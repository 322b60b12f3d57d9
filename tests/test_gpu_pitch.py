# coding: utf-8
"""-m gpu: the YIN pitch tracker (dv3_yin_items_f32 through audio.yin_items; csrc/pitch.hip) against the
float64 restatement tests/pitch_ref.py, and the waveform-level evaluation built on it (synthesis.waveform_distortion).

All three frame sizes at their presets' hops and rates, B = 3 items of lengths (1, n_fft - hop + 3, 32 n_fft + 17): one
sample, an item shorter than a frame, and a long one.  The long item is 32 frames' worth and not 5: the four frames of the
one-sample item are ties by construction (d' = 1 at every lag, up to an ulp) and the short item's padded frames are close
calls, so with 5 n_fft + 17 samples those alone pass the 10 % cap on frames left out of the lag comparison; at 32 the
reference leaves out 10, 9 and 11 of 141 frames (512, 1024, 2048).  The fixture: a 12-harmonic tone (equal amplitudes, so
that the parabola's curvature D stays above 8 eps at 48 kHz) gliding 80 -> 310 Hz over each item, a 1e-3 noise floor, and in
the long item one frame's length of noise alone and a stretch of exact zeros.

Every tolerance is computed from the header's bounds and the reference's own values; none is fitted."""
import functools
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tests import pitch_ref as P  # noqa: E402

pytestmark = pytest.mark.gpu

PRESETS = [(512, 128, 16000), (1024, 256, 22050), (2048, 512, 48000)]
U = 2.0 ** -24
SENTINEL = -12345.0
GUARD = 64
THR = 0.15


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


def make_items(n_fft, hop, sr, mult=32, shift=1.0, noise_stretch=True, seed=0):
    """-> the three float32 items"""
    rs = np.random.RandomState(seed)
    items = []
    for L in (1, n_fft - hop + 3, mult * n_fft + 17):
        f = (80.0 + (310.0 - 80.0) * np.arange(L) / max(L - 1, 1)) * shift
        ph = 2 * np.pi * np.cumsum(f) / sr
        x = 0.08 * sum(np.sin((k + 1) * ph + 0.7 * k) for k in range(12)) + 1e-3 * rs.randn(L)
        if L > 4 * n_fft:
            a = int(0.40 * L)
            if noise_stretch:
                x[a:a + n_fft] = 0.1 * rs.randn(n_fft)
            a += 3 * n_fft // 2 + n_fft // 4
            x[a:a + n_fft + 2 * hop] = 0.0
        items.append(x.astype(np.float32))
    return items


def _cfgs(n_fft, hop, sr):
    from deepvoice3_pytorch_amd import audio
    cfg = audio.AudioConfig(fft_size=n_fft, hop_size=hop, sample_rate=sr)
    pitch = audio.PitchConfig(threshold=THR)
    return cfg, pitch, pitch.lags(cfg)


@functools.lru_cache(maxsize=None)
def reference(n_fft, hop, sr):
    """computed once per preset and shared; nothing writes to it"""
    _, _, (tau_min, tau_max) = _cfgs(n_fft, hop, sr)
    items = make_items(n_fft, hop, sr)
    r = P.yin_frames(np.concatenate(items), [len(x) for x in items], hop, n_fft, tau_min, tau_max, THR, float(sr))
    for v in r.values():
        v.setflags(write=False)
    return items, r


def run_raw(dev, items, n_fft, hop, sr, tau_min, tau_max, want_lag=True):
    """the entry point itself, each output between two guard stretches -> (f0, ap, power, lag or None) as numpy, after
    asserting the guards are untouched"""
    from deepvoice3_pytorch_amd import _lib, audio
    lengths = np.array([len(x) for x in items], dtype=np.int64)
    frames = np.array([audio.lws_num_frames(int(n), hop, n_fft) for n in lengths], dtype=np.int64)
    nf = int(frames.sum())
    x = torch.from_numpy(np.concatenate(items)).to(dev)
    soff = torch.from_numpy(np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64)).to(dev)
    foff = torch.from_numpy(np.concatenate([[0], np.cumsum(frames)]).astype(np.int32)).to(dev)
    bufs = [torch.full((nf + 2 * GUARD,), SENTINEL, dtype=torch.float32, device=dev) for _ in range(3)]
    lag = torch.full((nf + 2 * GUARD,), int(SENTINEL), dtype=torch.int32, device=dev) if want_lag else None
    _lib.call("dv3_yin_items_f32", x.data_ptr(), soff.data_ptr(), foff.data_ptr(), len(items), nf, hop, n_fft, tau_min,
              tau_max, THR, float(sr), *[b.data_ptr() + 4 * GUARD for b in bufs],
              lag.data_ptr() + 4 * GUARD if want_lag else None, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    out = []
    for b in bufs + ([lag] if want_lag else []):
        h = b.cpu().numpy()
        assert (h[:GUARD] == h.dtype.type(SENTINEL)).all() and (h[-GUARD:] == h.dtype.type(SENTINEL)).all(), "a guard was written"
        out.append(h[GUARD:-GUARD].copy())
    return tuple(out) + ((None,) if not want_lag else ())


@functools.lru_cache(maxsize=None)
def device_run(n_fft, hop, sr):
    items, _ = reference(n_fft, hop, sr)
    _, _, (tau_min, tau_max) = _cfgs(n_fft, hop, sr)
    return run_raw(torch.device("cuda:0"), items, n_fft, hop, sr, tau_min, tau_max)


@pytest.mark.parametrize("n_fft,hop,sr", PRESETS)
def test_power_and_ap_within_the_header_bounds(dev, n_fft, hop, sr):
    """power: (N + 2) 2^-24 relative.  ap is d' at the lag the device chose, so it is held against the reference's d' at
    THAT lag on every frame, agreed or not: (2 W + lag + 8) 2^-24 relative."""
    _, r = reference(n_fft, hop, sr)
    f0, ap, power, lag = device_run(n_fft, hop, sr)
    _, _, (tau_min, tau_max) = _cfgs(n_fft, hop, sr)
    assert np.isfinite(f0).all() and np.isfinite(ap).all() and np.isfinite(power).all()
    assert ((lag >= tau_min) & (lag < tau_max)).all()
    err = np.abs(power.astype(np.float64) - r["power"])
    bound = (n_fft + 2) * U * r["power"]
    print("power: worst error / bound = %.3f" % np.max(err[bound > 0] / bound[bound > 0]))
    assert (err <= bound).all()
    W = n_fft - tau_max
    want = r["dprime"][np.arange(len(lag)), lag]
    err = np.abs(ap.astype(np.float64) - want)
    bound = (2 * W + lag + 8) * U * want
    print("ap: worst error / bound = %.3f" % np.max(err / bound))
    assert (err <= bound).all()


@pytest.mark.parametrize("n_fft,hop,sr", PRESETS)
def test_lag_and_f0_where_the_reference_decides(dev, n_fft, hop, sr):
    """lag: equal on every frame whose decision margin exceeds twice the d' bound; all-zero frames exactly; the frames
    left out (margin too small, or the parabola's D below 8 eps) stay under 10 % of the others, by the reference alone.
    f0 where the lag agrees: the d' bound eps through the parabola, |delta's error| <= eps (|a| + |c|) / (2 D) +
    |delta| eps (|a| + 2 |b| + |c|) / D, through f0 = sr / (lag + delta), plus 4 ulp of f0."""
    _, r = reference(n_fft, hop, sr)
    f0, ap, power, lag = device_run(n_fft, hop, sr)
    _, _, (tau_min, tau_max) = _cfgs(n_fft, hop, sr)
    eps = P.dprime_bound(n_fft, tau_max)
    zero = r["zero"]
    assert zero.sum() >= 2
    assert (lag[zero] == tau_min).all() and (ap[zero] == 1.0).all() and (power[zero] == 0.0).all()
    assert (f0[zero] == np.float32(sr) / np.float32(tau_min)).all()
    decided = ~zero & (r["margin"] > 2 * eps)
    flat = ~zero & decided & (r["D"] < 8 * eps)
    left_out = (~zero & ~decided) | flat
    print("frames %d, all-zero %d, left out %d (margin %d, D %d)" % (len(zero), zero.sum(), left_out.sum(),
                                                                    (~zero & ~decided).sum(), flat.sum()))
    assert left_out.sum() <= 0.10 * (~zero).sum(), "the fixture leaves too many frames undecided"
    assert (lag[decided] == r["lag"][decided]).all()
    ok = ~zero & ~left_out & (lag == r["lag"])
    assert ok.sum() >= 0.9 * (~zero).sum()
    a, b, c, D, delta = (r[k][ok] for k in ("a", "b", "c", "D", "delta"))
    d_delta = eps * (np.abs(a) + np.abs(c)) / (2 * D) + np.abs(delta) * eps * (np.abs(a) + 2 * np.abs(b) + np.abs(c)) / D
    tol = sr / (r["lag"][ok] + delta) ** 2 * d_delta + 4 * np.spacing(f0[ok]).astype(np.float64)
    err = np.abs(f0[ok].astype(np.float64) - r["f0"][ok])
    print("f0: worst error / bound = %.3f, worst error %.3g Hz" % (np.max(err / tol), err.max()))
    assert (err <= tol).all()
    # the voiced stretch is there and found: the tone's frames read 80 .. 310 Hz
    voiced = (r["ap"] < THR) & (r["power"] > 1e-6)
    assert voiced.sum() >= 0.5 * len(zero) and (f0[voiced & ok] > 75.0).all() and (f0[voiced & ok] < 330.0).all()


@pytest.mark.parametrize("n_fft,hop,sr", PRESETS)
def test_rows_depend_on_their_item_alone_and_calls_repeat(dev, n_fft, hop, sr):
    from deepvoice3_pytorch_amd import audio
    items, r = reference(n_fft, hop, sr)
    cfg, pitch, (tau_min, tau_max) = _cfgs(n_fft, hop, sr)
    first = device_run(n_fft, hop, sr)
    again = run_raw(dev, items, n_fft, hop, sr, tau_min, tau_max)
    for p, q in zip(first, again):
        assert np.array_equal(p.view(np.int32), q.view(np.int32)), "two calls differ"
    no_lag = run_raw(dev, items, n_fft, hop, sr, tau_min, tau_max, want_lag=False)
    assert no_lag[3] is None
    for p, q in zip(first[:3], no_lag[:3]):
        assert np.array_equal(p.view(np.int32), q.view(np.int32)), "lag = NULL changes another output"
    o = 0
    for b, x in enumerate(items):                      # each item alone, B = 1: its rows bit for bit
        alone = run_raw(dev, [x], n_fft, hop, sr, tau_min, tau_max)
        T = int(r["frames"][b])
        for p, q in zip(first, alone):
            assert np.array_equal(p[o:o + T].view(np.int32), q.view(np.int32)), "item %d alone differs" % b
        o += T
    # the Python layer is that call: same rows, same frames, and the host-list sibling
    flat = torch.from_numpy(np.concatenate(items)).to(dev)
    f0, ap, power, frames, lag = audio.yin_items(flat, [len(x) for x in items], cfg, pitch, want_lag=True)
    assert frames.tolist() == r["frames"].tolist() and lag.dtype == torch.int32
    for p, q in zip(first, (f0, ap, power, lag)):
        assert np.array_equal(p.view(np.int32), q.cpu().numpy().view(np.int32))
    g = audio.f0_from_arrays(items, cfg, dev, pitch)
    assert len(g) == 4 and torch.equal(g[0], f0) and torch.equal(g[1], ap) and torch.equal(g[2], power)
    lin, mel, fr = audio.features_items(flat, [len(x) for x in items], cfg)
    assert fr.tolist() == frames.tolist() and lin.shape[0] == f0.numel()


def test_waveform_distortion_of_a_set_against_itself(dev):
    from deepvoice3_pytorch_amd import audio, synthesis
    n_fft, hop, sr = PRESETS[1]
    cfg, pitch, _ = _cfgs(n_fft, hop, sr)
    items = make_items(n_fft, hop, sr)
    table = synthesis.waveform_distortion(items, [torch.from_numpy(x) for x in items], cfg, pitch, device=dev)
    assert tuple(table.shape) == (3, 13) and table.dtype == torch.float32 and table.device.type == "cuda"
    row = {k: table[:, i].cpu().numpy() for i, k in enumerate(synthesis.WAVE_EVAL_COLUMNS)}
    frames = [audio.lws_num_frames(len(x), hop, n_fft) for x in items]
    assert (row["mcd_sum"] == 0.0).all() and (row["f0_sqcents_sum"] == 0.0).all() and (row["n_voicing_errors"] == 0.0).all()
    assert row["path_len"].tolist() == frames == row["pitch_path_len"].tolist()
    assert row["n_diag"].tolist() == [n - 1 for n in frames]            # the diagonal: every move after the first cell
    assert (row["n_voiced_a"] == row["n_voiced_b"]).all() and (row["n_both_voiced"] == row["n_voiced_a"]).all()
    assert row["n_voiced_a"][2] >= 0.4 * frames[2]
    tot = synthesis.WaveEvalTotals()
    tot.add(table, ["one", "short", "long"])
    res = tot.result()
    assert res["mcd"] == 0.0 and res["f0_rmse_cents"] == 0.0 and res["vuv_error"] == 0.0 and res["duration_ratio"] == 1.0


def test_a_semitone_up_reads_as_the_reference_says_along_the_devices_path(dev):
    """The tones against the same tones a semitone up (no noise stretch), 1024 / 256 at 22.05 kHz, the lengths of the other tests:
    f0_rmse_cents of the table equals the figure tests/pitch_ref.py gives -- float64 tracks of both sides, its own
    voicing, its own pitch_distortion -- along the path the device's DTW chose, and the counts are equal exactly.
    Margin 1e-4 cents.  How it was obtained: a numpy float32 emulation of the kernel's arithmetic (differences, squares
    and both sums as float32 chains, d', the search and the parabola in float32) against the float64 reference on this
    comparison along the identity path differed by 6.3e-6, 1.1e-5 and 5.1e-7 cents at the three presets (about 100 cents
    measured on 100-odd voiced pairs, the squares summed into an fp32 as the table holds them); the kernel adds in another order than that emulation, which is worth a small
    factor either way, so the margin is the worst of the three rounded up to the next power of ten.  No frame of either
    side lies within the d' bound of the voicing threshold (asserted on the reference), so the voicing flags are not
    at the mercy of rounding."""
    from deepvoice3_pytorch_amd import audio, synthesis
    n_fft, hop, sr = PRESETS[1]
    cfg, pitch, (tau_min, tau_max) = _cfgs(n_fft, hop, sr)
    a = make_items(n_fft, hop, sr, noise_stretch=False)
    b = make_items(n_fft, hop, sr, shift=2.0 ** (1.0 / 12.0), noise_stretch=False, seed=1)
    table = synthesis.waveform_distortion(a, b, cfg, pitch, device=dev)
    # the device's own path: the same two calls waveform_distortion makes
    sides, tracks = [], []
    eps = P.dprime_bound(n_fft, tau_max)
    for items in (a, b):
        lengths = [len(x) for x in items]
        flat = torch.from_numpy(np.concatenate(items)).to(dev)
        _, mel, frames = audio.features_items(flat, lengths, cfg)
        sides.append((synthesis._pad_rows(mel, frames), [int(n) for n in frames]))
        r = P.yin_frames(np.concatenate(items), lengths, hop, n_fft, tau_min, tau_max, THR, float(sr))
        loud = r["power"] > 10.0 ** (pitch.silence_db / 10.0)
        assert (np.abs(r["ap"][loud] - THR) > 2 * eps * THR).all(), "a frame's voicing hangs on rounding: change the fixture"
        assert (np.abs(r["power"] - 1e-6) > 1e-6 * (n_fft + 2) * U).all()
        tracks.append((r["f0"], (r["ap"] < THR) & loud, np.concatenate([[0], np.cumsum(r["frames"])])))
    ref_table, path = synthesis.mel_distortion(sides[0][0], sides[0][1], sides[1][0], sides[1][1], cfg, 13, want_path=True)
    assert torch.equal(ref_table, table[:, :7])
    path = path.cpu().numpy()
    (fa, va, oa), (fb, vb, ob) = tracks
    want = np.array([P.pitch_distortion(fa[oa[i]:oa[i + 1]], va[oa[i]:oa[i + 1]], fb[ob[i]:ob[i + 1]], vb[ob[i]:ob[i + 1]],
                                        path[i]) for i in range(3)])
    got = table[:, 7:].cpu().numpy().astype(np.float64)
    assert np.array_equal(got[:, 1:], want[:, 1:]), (got, want)
    assert want[:, 1].sum() >= 20
    tot = synthesis.WaveEvalTotals()
    tot.add(table)
    res = tot.result()
    want_rmse = np.sqrt(want[:, 0].sum() / want[:, 1].sum())
    print("f0_rmse_cents: device %.9f, reference %.9f, vuv_error %.4f" % (res["f0_rmse_cents"], want_rmse, res["vuv_error"]))
    assert abs(res["f0_rmse_cents"] - want_rmse) <= 1e-4
    # frame against frame the two sets are 100 cents apart; on a glide the DTW path trades time for pitch, so the
    # figure along it lies below that, and above zero
    assert 1.0 < want_rmse < 101.0 and res["vuv_error"] == want[:, 2].sum() / want[:, 3].sum()


def test_evaluate_synthesis_audio_with_the_models_own_waveforms_as_targets(dev):
    """a toy deepvoice3 (random weights, 512 / 128 at 16 kHz, one Griffin-Lim iteration): against its own tts_batch
    waveforms every distance is zero and the path is the diagonal; against those waveforms at half the length the
    duration ratio says so"""
    from deepvoice3_pytorch_amd import audio, builder, synthesis
    from tests.test_gpu_rolling_decode import DV3_HP
    torch.manual_seed(3)
    hp = dict(DV3_HP, linear_dim=257)
    model = builder.deepvoice3(**hp).to(dev).eval()
    dec = model.seq2seq.decoder
    dec.min_decoder_steps, dec.max_decoder_steps = 0, 24
    cfg = audio.AudioConfig(fft_size=512, hop_size=128, sample_rate=16000, griffin_lim_iters=1)
    rng = np.random.RandomState(11)
    seqs = [rng.randint(2, hp["n_vocab"], n).tolist() for n in (19, 6, 13)]
    wavs = [res[3].clone() for res in synthesis.tts_batch(model, seqs, audio_cfg=cfg)]
    table = synthesis.evaluate_synthesis_audio(model, seqs, [w.cpu().numpy() for w in wavs], audio_cfg=cfg)
    assert tuple(table.shape) == (3, 13)
    row = {k: table[:, i].tolist() for i, k in enumerate(synthesis.WAVE_EVAL_COLUMNS)}
    frames = [float(audio.lws_num_frames(int(w.numel()), 128, 512)) for w in wavs]
    assert row["mcd_sum"] == [0.0] * 3 and row["f0_sqcents_sum"] == [0.0] * 3 and row["n_voicing_errors"] == [0.0] * 3
    assert row["path_len"] == frames == row["pitch_path_len"] == row["frames_synth"] == row["frames_target"]
    assert row["n_voiced_a"] == row["n_voiced_b"] == row["n_both_voiced"]
    half = synthesis.evaluate_synthesis_audio(model, seqs, [w[:w.numel() // 2] for w in wavs], audio_cfg=cfg,
                                              pitch=audio.PitchConfig(threshold=0.3))
    tot = synthesis.WaveEvalTotals()
    tot.add(half, ["a", "b", "c"])
    res = tot.result()
    assert 1.5 < res["duration_ratio"] < 2.5 and res["n_items"] == 3 and 0.0 <= res["vuv_error"] <= 1.0


@pytest.mark.parametrize("n_fft,hop,sr,tau_min,tau_max", [
    (2048, 512, 48000, 96, 1024),      # 257 quads of lags: one thread owns two of them
    (1024, 256, 22050, 40, 512),       # 129 quads: one slice
    (1024, 256, 22050, 40, 509),       # 128 quads: two slices, W = 515 (a tail of three)
    (512, 128, 16000, 2, 255),         # the smallest tau_min; 64 quads: four slices
    (512, 192, 16000, 30, 33),         # the narrowest range the entry point takes, a hop that does not divide n_fft
])
def test_the_other_paths_through_the_kernel(dev, n_fft, hop, sr, tau_min, tau_max):
    """lag ranges the presets do not reach, on a shorter fixture (long item 6 n_fft + 17): power and ap within the
    header's bounds on every frame, the lag equal wherever the reference decides it, all-zero frames exact"""
    items = make_items(n_fft, hop, sr, mult=6)
    r = P.yin_frames(np.concatenate(items), [len(x) for x in items], hop, n_fft, tau_min, tau_max, THR, float(sr))
    f0, ap, power, lag = run_raw(dev, items, n_fft, hop, sr, tau_min, tau_max)
    assert len(lag) == r["frames"].sum() and ((lag >= tau_min) & (lag < tau_max)).all() and np.isfinite(f0).all()
    assert (np.abs(power.astype(np.float64) - r["power"]) <= (n_fft + 2) * U * r["power"]).all()
    want = r["dprime"][np.arange(len(lag)), lag]
    assert (np.abs(ap.astype(np.float64) - want) <= (2 * (n_fft - tau_max) + lag + 8) * U * want).all()
    zero = r["zero"]
    assert zero.any() and (lag[zero] == tau_min).all() and (ap[zero] == 1.0).all() and (power[zero] == 0.0).all()
    decided = ~zero & (r["margin"] > 2 * P.dprime_bound(n_fft, tau_max))
    print("frames %d, decided %d, agreeing %d" % (len(lag), decided.sum(), (lag == r["lag"]).sum()))
    assert decided.sum() >= 0.5 * len(lag) and (lag[decided] == r["lag"][decided]).all()

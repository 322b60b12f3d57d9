# coding: utf-8
"""Pitch tracking without a GPU: tests/pitch_ref.py -- the float64 restatement of dv3_yin_items_f32 --
pinned to known answers (pure and harmonic tones, noise, silence), the framing, audio.PitchConfig's resolution and
refusals, the C header's entry point with every refusal of the library, the arithmetic of synthesis.pitch_distortion on a
hand-made path, synthesis.WaveEvalTotals' invariance to batching, and the new signatures."""
import ctypes
import inspect
import math
import os
import re
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tests import pitch_ref as P  # noqa: E402

SR, N, HOP = 22050, 1024, 256
TAU_MIN, TAU_MAX, THR = 44, 367, 0.15          # PitchConfig() at the default AudioConfig


def _f32(x):
    return np.asarray(x, dtype=np.float32).astype(np.float64)


def _tone(f, n, harmonics, seed=0):
    t = np.arange(n) / SR
    ph = np.random.RandomState(seed).uniform(0, 2 * np.pi, harmonics)
    return _f32(0.3 * sum(np.sin(2 * np.pi * f * (k + 1) * t + ph[k]) / (k + 1) for k in range(harmonics)))


def _interior(L):
    """frames that hold samples only: t hop - (N - hop) >= 0 and the frame's end inside the item"""
    T = P.lws_num_frames(L, HOP, N)
    return [t for t in range(T) if t * HOP - (N - HOP) >= 0 and t * HOP + HOP <= L]


@pytest.mark.parametrize("harmonics", [1, 12])
@pytest.mark.parametrize("f", [110.0, 220.0, 330.0])
def test_tones_come_back_within_five_cents(f, harmonics):
    L = 6 * N
    r = P.yin_frames(_tone(f, L, harmonics), [L], HOP, N, TAU_MIN, TAU_MAX, THR, float(SR))
    rows = _interior(L)
    assert len(rows) >= 10
    cents = 1200.0 * np.log2(r["f0"][rows] / f)
    assert np.abs(cents).max() < 5.0, cents
    assert (r["ap"][rows] < THR).all() and (r["power"][rows] > 1e-3).all()
    assert (np.abs(r["delta"]) <= 1.0).all() and (r["dprime"][:, 0] == 1.0).all()


def test_white_noise_is_aperiodic_on_every_frame():
    L = 5 * N + 17
    x = _f32(0.1 * np.random.RandomState(1).randn(L))
    r = P.yin_frames(x, [L], HOP, N, TAU_MIN, TAU_MAX, THR, float(SR))
    assert (r["ap"] > THR).all(), r["ap"].min()
    assert ((r["lag"] >= TAU_MIN) & (r["lag"] < TAU_MAX)).all()


def test_an_all_zero_frame_gives_the_exact_values():
    r = P.yin_frame(np.zeros(N), TAU_MIN, TAU_MAX, THR, float(SR))
    assert r["lag"] == TAU_MIN and r["f0"] == SR / TAU_MIN and r["ap"] == 1.0 and r["power"] == 0.0 and r["zero"]
    assert r["margin"] == 0.0 and (r["dprime"] == 1.0).all()
    # inside a batch: an exactly-zero item between two tones
    L = 2 * N
    x = np.concatenate([_tone(200.0, L, 3), np.zeros(L), _tone(150.0, L, 3)])
    q = P.yin_frames(x, [L, L, L], HOP, N, TAU_MIN, TAU_MAX, THR, float(SR))
    T = P.lws_num_frames(L, HOP, N)
    mid = slice(T, 2 * T)
    assert q["zero"][mid].all() and (q["lag"][mid] == TAU_MIN).all() and (q["ap"][mid] == 1.0).all()
    assert (q["power"][mid] == 0.0).all() and not q["zero"][:T].any() and not q["zero"][2 * T:].any()


@pytest.mark.parametrize("n_fft,hop", [(512, 128), (1024, 256), (2048, 512)])
def test_frames_are_the_lws_frames(n_fft, hop):
    from deepvoice3_pytorch_amd import audio
    for L in (1, hop, n_fft, n_fft + 1):
        r = P.yin_frames(np.ones(L), [L], hop, n_fft, 8, n_fft // 4, THR, 16000.0)
        assert r["frames"].tolist() == [audio.lws_num_frames(L, hop, n_fft)] == [len(r["lag"])]
        # every frame holds samples of the item, the last one its last sample; a further frame would hold none
        T = int(r["frames"][0])
        assert (r["power"] > 0.0).all() and (T - 1) * hop - (n_fft - hop) <= L - 1 < T * hop - (n_fft - hop)


# ----------------------------------------------------------------------------------------------------------------------
# audio.PitchConfig
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sr,n_fft,hop,fmin,lags", [(16000, 512, 128, 62.5, (32, 256)), (22050, 1024, 256, 60.0, (44, 367)),
                                                    (48000, 2048, 512, 60.0, (96, 800))])
def test_pitch_config_resolves_per_audio_config(sr, n_fft, hop, fmin, lags):
    from deepvoice3_pytorch_amd import audio
    cfg = audio.AudioConfig(fft_size=n_fft, hop_size=hop, sample_rate=sr)
    p = audio.PitchConfig()
    assert (p.fmin, p.fmax, p.threshold, p.silence_db) == (None, 500.0, 0.15, -60.0)
    assert p.resolved_fmin(cfg) == fmin == max(60.0, 2.0 * sr / n_fft)
    assert p.lags(cfg) == lags and lags[1] <= n_fft // 2 and lags[0] == max(2, sr // 500)
    # an fmin whose period does not fit half a frame: refused, naming fmin, the rate and the frame size
    with pytest.raises(ValueError) as e:
        audio.PitchConfig(fmin=0.9 * sr / (n_fft // 2)).lags(cfg)
    msg = str(e.value)
    assert "fmin=" in msg and "sample_rate=%g" % sr in msg and "fft_size=%d" % n_fft in msg
    # a range without two lags
    with pytest.raises(ValueError, match="fmin="):
        audio.PitchConfig(fmin=sr / 4.0, fmax=sr / 3.0).lags(cfg)
    assert audio.PitchConfig(fmin=100, fmax=400).lags(cfg) == (sr // 400, sr // 100)


def test_pitch_config_refuses_by_value():
    from deepvoice3_pytorch_amd import audio
    for kw in (dict(fmin=0), dict(fmin=-5.0), dict(fmin="60"), dict(fmin=float("nan")), dict(fmax=0), dict(fmax=None),
               dict(fmin=500.0, fmax=500.0), dict(threshold=0.0), dict(threshold=1.5), dict(threshold=float("nan")),
               dict(threshold=True), dict(silence_db=None), dict(silence_db=float("inf"))):
        with pytest.raises(ValueError, match="PitchConfig"):
            audio.PitchConfig(**kw)
    assert audio.PitchConfig(threshold=1.0).threshold == 1.0
    with pytest.raises(ValueError, match="PitchConfig"):
        audio.yin_items(torch.zeros(8), [8], pitch=0.15)
    with pytest.raises(ValueError, match="lws framing"):
        audio.yin_items(torch.zeros(8), [8], audio.AudioConfig(convention="torch"))


def test_voiced_is_the_two_comparisons():
    from deepvoice3_pytorch_amd import audio
    p = audio.PitchConfig(threshold=0.2, silence_db=-40.0)
    ap = torch.tensor([0.1, 0.2, 0.1, 0.3])
    power = torch.tensor([1e-3, 1e-3, 1e-4, 1.0])
    assert audio.voiced(ap, power, p).tolist() == [True, False, False, False]


# ----------------------------------------------------------------------------------------------------------------------
# the C header, the Makefile, the library's refusals
# ----------------------------------------------------------------------------------------------------------------------
def test_header_makefile_and_abi():
    from deepvoice3_pytorch_amd import _lib
    p, i, f = ctypes.c_void_p, ctypes.c_int32, ctypes.c_float
    restype, args = _lib.FUNCS["dv3_yin_items_f32"]
    assert restype is ctypes.c_int and args == [p, p, p, i, i, i, i, i, i, f, f, p, p, p, p, p]
    header = open(os.path.join(ROOT, "include", "dv3hip.h")).read()
    m = re.search(r"/\*((?:(?!\*/).)*)\*/\s*#define DV3_YIN_MAX_LAG 1024\s*int dv3_yin_items_f32\(([^)]*)\);", header, flags=re.S)
    assert m, "the block comment, the constant and the prototype stand together"
    want = ("const float* x, const int64_t* soff, const int32_t* foff, int32_t B, int32_t n_frames, int32_t hop, "
            "int32_t n_fft, int32_t tau_min, int32_t tau_max, float threshold, float sample_rate, "
            "float* f0, float* ap, float* power, int32_t* lag, void* stream")
    assert " ".join(m.group(2).split()) == want
    comment = " ".join(m.group(1).replace("\n *", " ").split())
    for words in ("version stays 50", "d'(0) = 1", "(N + 2) 2^-24", "(W + 2) 2^-24", "(2 W + tau + 8) 2^-24", "Hillis-Steele",
                  "lag = tau_min, f0 = sample_rate / tau_min, ap = 1, power = 0", "yin_items:"):
        assert words in comment, words
    assert _lib.CONSTS["DV3_ABI_VERSION"] == 50 and _lib.CONSTS["DV3_YIN_MAX_LAG"] == 1024
    assert not "dv3_yin_items_f32".endswith("_n")
    assert "dv3_yin_desc" not in _lib.STRUCTS and not [s for s in _lib.STRUCTS if "yin" in s or "pitch" in s]
    make = open(os.path.join(ROOT, "deepvoice3_pytorch_amd", "csrc", "Makefile")).read()
    assert "pitch.hip" in make.split("SRCS")[1].split("OBJS")[0]
    assert "Cheveign" in open(os.path.join(ROOT, "PAPERS.md")).read()
    assert P.dprime_bound(1024, 367) == (2 * 657 + 367 + 8) * 2.0 ** -24


_GOOD = dict(x=64, soff=64, foff=64, B=1, n_frames=1, hop=256, n_fft=1024, tau_min=44, tau_max=367, threshold=0.15,
             sample_rate=22050.0, f0=64, ap=64, power=64, lag=64)


def _call(lib, **kw):
    a = dict(_GOOD, **kw)
    return lib.dv3_yin_items_f32(a["x"], a["soff"], a["foff"], a["B"], a["n_frames"], a["hop"], a["n_fft"], a["tau_min"],
                                 a["tau_max"], a["threshold"], a["sample_rate"], a["f0"], a["ap"], a["power"], a["lag"], None)


@pytest.mark.parametrize("kw,names", [
    (dict(x=None), b"x is null"), (dict(soff=None), b"soff is null"), (dict(foff=None), b"foff is null"),
    (dict(f0=None), b"f0 is null"), (dict(ap=None), b"ap is null"), (dict(power=None), b"power is null"),
    (dict(B=0), b"B = 0"), (dict(n_frames=0), b"n_frames = 0"), (dict(n_frames=-3), b"n_frames = -3"),
    (dict(hop=0), b"hop = 0"), (dict(hop=1025), b"hop = 1025"), (dict(n_fft=4096), b"n_fft = 4096"),
    (dict(n_fft=1000), b"n_fft = 1000"), (dict(n_fft=256, hop=64, tau_max=100), b"n_fft = 256"),
    (dict(tau_min=1), b"tau_min = 1"), (dict(tau_max=513), b"tau_max = 513"),
    (dict(n_fft=2048, tau_max=1025), b"tau_max = 1025"), (dict(n_fft=512, hop=128, tau_max=257), b"tau_max = 257"),
    (dict(tau_min=366), b"tau_max = 367"), (dict(tau_min=400), b"tau_max = 367"),
    (dict(threshold=0.0), b"threshold = 0"), (dict(threshold=1.25), b"threshold = 1.25"),
    (dict(threshold=float("nan")), b"threshold = nan"), (dict(sample_rate=0.0), b"sample_rate = 0"),
    (dict(sample_rate=-8000.0), b"sample_rate = -8000"), (dict(sample_rate=float("inf")), b"sample_rate = inf"),
    (dict(sample_rate=float("nan")), b"sample_rate = nan"),
])
def test_library_refuses_every_violation_without_a_gpu(kw, names):
    """dummy non-null pointers: a refusal comes before any launch, so nothing is dereferenced"""
    from deepvoice3_pytorch_amd import _lib
    lib = _lib.lib()
    assert _call(lib, **kw) == _lib.CONSTS["DV3_EINVAL"]
    msg = lib.dv3_last_error()
    assert msg.startswith(b"yin_items:") and names in msg, msg


# ----------------------------------------------------------------------------------------------------------------------
# synthesis.pitch_distortion, WaveEvalTotals, the signatures
# ----------------------------------------------------------------------------------------------------------------------
def test_pitch_distortion_on_a_hand_made_path():
    from deepvoice3_pytorch_amd import synthesis
    semitone = 2.0 ** (1.0 / 12.0)
    # item 0: Ta = 3, Tb = 2; the pairs (0,0) a 100-cent pair, (1,0) a unvoiced, (2,1) equal; then a row of -1
    # item 1: one pair only, unvoiced on both sides; padding voiced=True past the lengths must not be counted
    f0_a = torch.tensor([[200.0 * semitone, 300.0, 150.0], [100.0, 100.0, 100.0]])
    v_a = torch.tensor([[True, False, True], [False, True, True]])
    f0_b = torch.tensor([[200.0, 150.0], [50.0, 50.0]])
    v_b = torch.tensor([[True, True], [False, True]])
    path = torch.tensor([[[0, 0], [1, 0], [2, 1], [-1, -1]], [[0, 0], [-1, -1], [-1, -1], [-1, -1]]], dtype=torch.int32)
    out = synthesis.pitch_distortion(f0_a, v_a, f0_b, v_b, path)
    assert out.dtype == torch.float32 and tuple(out.shape) == (2, len(synthesis.PITCH_EVAL_COLUMNS))
    row = dict(zip(synthesis.PITCH_EVAL_COLUMNS, out[0].tolist()))
    assert abs(row["f0_sqcents_sum"] - 100.0 ** 2) < 100.0 ** 2 * 1e-5          # fp32 ratio of the two f0
    assert (row["n_both_voiced"], row["n_voicing_errors"], row["pitch_path_len"]) == (2.0, 1.0, 3.0)
    assert (row["n_voiced_a"], row["n_voiced_b"]) == (2.0, 2.0)
    assert out[1].tolist() == [0.0, 0.0, 0.0, 1.0, 0.0, 0.0]
    for b in range(2):
        ref = P.pitch_distortion(f0_a[b].numpy(), v_a[b].numpy(), f0_b[b].numpy(), v_b[b].numpy(), path[b].numpy())
        np.testing.assert_allclose(out[b].numpy(), ref, rtol=1e-6)
    with pytest.raises(ValueError, match="pitch_distortion"):
        synthesis.pitch_distortion(f0_a, v_a[:, :2], f0_b, v_b, path)


def test_wave_eval_totals_do_not_depend_on_the_batching():
    from deepvoice3_pytorch_amd import synthesis
    cols = synthesis.WAVE_EVAL_COLUMNS
    assert cols == synthesis.SYNTH_EVAL_COLUMNS + synthesis.PITCH_EVAL_COLUMNS and len(cols) == 13
    assert synthesis.PITCH_EVAL_COLUMNS == ("f0_sqcents_sum", "n_both_voiced", "n_voicing_errors", "pitch_path_len",
                                            "n_voiced_a", "n_voiced_b")
    rs = np.random.RandomState(3)
    rows = np.zeros((7, 13), dtype=np.float32)
    rows[:, 0] = rs.uniform(100, 900, 7)
    rows[:, 1] = rs.randint(50, 200, 7)
    rows[:, 5], rows[:, 6] = rs.randint(40, 150, 7), rs.randint(40, 150, 7)
    rows[:, 7] = rs.uniform(1e3, 1e6, 7)
    rows[:, 8] = rs.randint(0, 60, 7)
    rows[:, 9] = rs.randint(0, 20, 7)
    rows[:, 10] = rows[:, 1]
    rows[3, 7], rows[3, 8] = 0.0, 0.0                      # an utterance without a pair voiced on both sides
    table = torch.from_numpy(rows)
    ids = ["u%d" % i for i in range(7)]
    results = []
    for cuts in ([7], [1, 6], [3, 2, 2], [1] * 7):
        tot, o = synthesis.WaveEvalTotals(), 0
        for n in cuts:
            tot.add(table[o:o + n], ids[o:o + n])
            o += n
        results.append(tot.result())
    for r in results[1:]:
        assert r == results[0] or (str(r) == str(results[0]))      # NaN != NaN: the item without voiced pairs
    r = results[0]
    d = rows.astype(np.float64)
    assert r["n_items"] == 7 and [it["id"] for it in r["items"]] == ids
    assert r["mcd"] == sum(d[:, 0].tolist()) / sum(d[:, 1].tolist())
    assert r["duration_ratio"] == sum(d[:, 5].tolist()) / sum(d[:, 6].tolist())
    assert r["f0_rmse_cents"] == math.sqrt(sum(d[:, 7].tolist()) / sum(d[:, 8].tolist()))
    assert r["vuv_error"] == sum(d[:, 9].tolist()) / sum(d[:, 10].tolist())
    assert math.isnan(r["items"][3]["f0_rmse_cents"]) and r["items"][3]["vuv_error"] == d[3, 9] / d[3, 10]
    assert r["items"][0]["f0_rmse_cents"] == math.sqrt(d[0, 7] / d[0, 8])
    with pytest.raises(ValueError, match="WaveEvalTotals"):
        synthesis.WaveEvalTotals().add(table[:, :7])
    with pytest.raises(ValueError, match="nothing"):
        synthesis.WaveEvalTotals().result()
    empty = synthesis.WaveEvalTotals()
    empty.add(torch.zeros(1, 13))
    assert math.isnan(empty.result()["f0_rmse_cents"]) and math.isnan(empty.result()["vuv_error"])


def test_signatures_and_defaults():
    from deepvoice3_pytorch_amd import audio, synthesis

    def sig(fn):
        return [(p.name, p.default) for p in inspect.signature(fn).parameters.values()]

    E = inspect.Parameter.empty
    assert sig(audio.PitchConfig.__init__)[1:] == [("fmin", None), ("fmax", 500.0), ("threshold", 0.15), ("silence_db", -60.0)]
    assert sig(audio.yin_items) == [("wav_flat", E), ("lengths", E), ("cfg", None), ("pitch", None), ("want_lag", False)]
    assert sig(audio.f0_from_arrays) == [("wavs", E), ("cfg", None), ("device", "cuda:0"), ("pitch", None)]
    assert sig(audio.voiced) == [("ap", E), ("power", E), ("pitch", E)]
    assert sig(synthesis.pitch_distortion) == [("f0_a", E), ("voiced_a", E), ("f0_b", E), ("voiced_b", E), ("path", E)]
    assert sig(synthesis.waveform_distortion) == [("wavs_a", E), ("wavs_b", E), ("cfg", None), ("pitch", None), ("order", 13),
                                                  ("device", "cuda:0"), ("num_mels", 80), ("fmin", 125), ("fmax", 7600)]
    assert sig(synthesis.evaluate_synthesis_audio) == [("model", E), ("sequences", E), ("target_wavs", E), ("speaker_ids", None),
                                                       ("audio_cfg", None), ("pitch", None), ("order", 13)]
    assert sig(synthesis.WaveEvalTotals.add)[1:] == [("table", E), ("ids", None)]
    assert "dv3_yin_items_f32" in inspect.getsource(audio.yin_items)
    # what the issue leaves alone
    assert list(inspect.signature(audio.griffin_lim).parameters)[-1] == "momentum"
    assert list(inspect.signature(audio.AudioConfig.__init__).parameters)[-1] == "griffin_lim_init"
    assert len(synthesis.SYNTH_EVAL_COLUMNS) == 7
    with pytest.raises(ValueError, match="4096"):
        synthesis.waveform_distortion([np.zeros(256 * 4100, dtype=np.float32)], [np.zeros(256, dtype=np.float32)],
                                      device="cpu")

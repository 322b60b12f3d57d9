# coding: utf-8
"""Prosody marks without a GPU: tests/prosody_curve_ref.py -- the float64 restatement of
dv3_curve_warp_f32, dv3_curve_plan_f64 and dv3_curve_fill_f64 -- held to the properties that make a plan a plan,
audio.plan_map on such a plan, the pitch moving part by part (and a break being silent) through Griffin-Lim and YIN in
float64, the options' refusals, the library's refusals and the C header."""
import inspect
import os
import re
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tests import prosody_curve_ref as C  # noqa: E402
from tests import prosody_ref as P  # noqa: E402

TMIN = 4


def _plan(rows, tlen_in, R=0, tmin=TMIN, S=None):
    t = C.tables(rows, S)
    o, tout = C.plan(tlen_in, t["nseg"], t["bounds"], t["rate"], t["brk"], tmin)
    T_out = int(tout.max())
    pos, ratio, gain = C.fill(tlen_in, t["nseg"], t["bounds"], t["rate"], t["semitones"], t["gain_db"], t["brk"], o, tout,
                              T_out, R)
    return t, o, tout, pos, ratio, gain


# ----------------------------------------------------------------------------------------------------------------------
# plan properties
# ----------------------------------------------------------------------------------------------------------------------
def test_one_segment_is_the_scalar_warp():
    """one segment, no break: T' = warped_frames(n, rate) and pos[j] == j * rate, the same fp64 product -- so the curve
    warp of such a plan is the scalar warp (the GPU test holds the two kernels to each other bit for bit)"""
    from deepvoice3_pytorch_amd import audio
    cfg = audio.AudioConfig()
    for n in (4, 7, 12, 24, 101):
        for rate in (0.25, 0.3, 0.8, 1.0, 1.25, 3.0, 4.0):
            t, o, tout, pos, ratio, gain = _plan([[(0, rate, 0.0, 0.0, 0)]], [n])
            assert int(tout[0]) == audio.warped_frames(n, rate, cfg) == P.out_frames(n, rate, TMIN)
            own = int(o[0, 1])
            assert own == int(np.floor((n - 1) / rate + 0.5)) + 1
            assert np.array_equal(pos[0, :own], np.arange(own, dtype=np.float64) * rate)
            # the frames the min_frames clamp adds hold the last frame, as j * rate beyond n - 1 does in the scalar warp
            assert (pos[0, own:] == n - 1).all() and (np.arange(own, int(tout[0])) * rate >= n - 1).all()
            assert (ratio == 1.0).all() and (gain == 1.0).all() and gain.dtype == np.float32


ROWS = [
    [(0, 0.8, 0.0, 0.0, 0), (5, 1.0, 3.0, 6.0, 4), (9, 1.7, -2.0, -12.0, 0), (15, 0.3, 0.0, 0.0, 2)],
    [(0, 1.0, 0.0, 0.0, 0), (3, 2.0, 1.0, 0.0, 0), (3, 0.5, 5.0, 0.0, 3), (8, 1.0, 0.0, 0.0, 0)],      # an empty segment
    [(0, 1.3, 2.0, -3.0, 5)],                                                                          # nseg = 1, a trailing break
]
TLEN = [21, 11, 9]


def test_positions_are_monotone_and_stay_inside_their_segment():
    t, o, tout, pos, _, _ = _plan(ROWS, TLEN)
    for b, n in enumerate(TLEN):
        ns = int(t["nseg"][b])
        c = C.repair(t["bounds"][b], ns, n)
        live = pos[b, :int(tout[b])]
        speech = live[live >= 0]
        assert (np.diff(speech) >= 0).all() and speech[0] == 0.0
        for s in range(ns):
            brk = int(t["brk"][b, s])
            inside = pos[b, int(o[b, s]):int(o[b, s + 1]) - brk]
            assert (inside >= c[s]).all()
            if c[s + 1] < n:
                assert (inside < c[s + 1]).all(), (b, s)                       # stops short of the next segment's first frame
            if c[s + 1] > c[s]:
                assert inside.size >= 1 and inside[0] == c[s]                  # a non-empty segment starts on its bound
                if c[s + 1] < n:
                    assert inside[-1] + t["rate"][b, s] >= c[s + 1]            # ... and one more frame would leave it
            else:
                assert inside.size == 0
            gap = pos[b, int(o[b, s + 1]) - brk:int(o[b, s + 1])]
            assert gap.size == brk and (gap == -1.0).all()                     # exactly break_frames silent frames
        assert int((live < 0).sum()) == int(t["brk"][b, :ns].sum())
        assert (pos[b, int(tout[b]):] == -1.0).all()


def test_bounds_out_of_order_are_repaired():
    """clamped into [0, n], made non-decreasing by a running maximum, the first 0 and the last n"""
    assert C.repair([7, 5, 3, 30, 8, 99], 5, 12) == [0, 5, 5, 12, 12, 12]
    assert C.repair([0, -4, 2], 3, 9) == [0, 0, 2, 9] and C.repair([3], 1, 9) == [0, 9]
    rows = [[(0, 1.0, 0.0, 0.0, 0), (9, 1.0, 1.0, 0.0, 0), (4, 1.0, 2.0, 0.0, 0), (50, 1.0, 3.0, 0.0, 0)]]
    t, o, tout, pos, ratio, _ = _plan(rows, [12])
    assert o[0].tolist() == [0, 9, 9, 12, 12] and int(tout[0]) == 12           # [0, 9), empty, [9, 12), empty
    assert np.array_equal(pos[0], np.arange(12.0))
    assert np.array_equal(ratio[0], np.exp2(np.array([0.0] * 9 + [2.0] * 3) / 12.0))


def test_a_quotient_rounded_across_an_integer_does_not_cost_a_frame():
    """len_s is defined by the two products, not by the rounded quotient: every non-last segment satisfies
    (len - 1) rate < L <= len rate in fp64 over a sweep of awkward rates"""
    rng = np.random.RandomState(3)
    for rate in list(rng.uniform(0.25, 4.0, 300)) + [0.1 * k for k in range(3, 40)] + [1.0 / 3.0, 2.0 / 3.0, 0.7, 1.1]:
        for L in (1, 3, 7, 10, 21, 49):
            n = C.seg_frames(0, L, float(rate), False)
            assert float(n - 1) * rate < L <= float(n) * rate, (rate, L, n)


def test_the_ramp_is_linear_and_touches_only_its_frames():
    R = 4
    rows = [[(0, 1.0, 0.0, 0.0, 0), (10, 1.0, 5.0, -10.0, 3), (20, 1.0, -3.0, 6.0, 0), (26, 1.0, 9.0, 0.0, 0), (26, 1.0, 1.0, 0.0, 0)]]
    t, o, tout, pos, ratio, gain = _plan(rows, [32], R)
    _, _, _, pos0, ratio0, gain0 = _plan(rows, [32], 0)
    assert np.array_equal(pos, pos0)                                           # the time map is not ramped
    semis, db = 12.0 * np.log2(ratio[0]), 20.0 * np.log10(gain[0].astype(np.float64))
    changed = np.nonzero((ratio[0] != ratio0[0]) | (gain[0] != gain0[0]))[0]
    # eligible: 0|1 at frame 10 (no break after segment 0).  1|2 has a break; 2|3: segment 3 is empty; 3|4: 3 is empty
    assert o[0].tolist() == [0, 10, 23, 29, 29, 35] and changed.tolist() == [8, 9, 10, 11]
    w = np.arange(1, R + 1) / float(R + 1)
    assert np.allclose(semis[8:12], 5.0 * w, rtol=0, atol=1e-12) and np.allclose(db[8:12], -10.0 * w, rtol=0, atol=1e-5)
    assert np.allclose(np.diff(semis[7:13]), 1.0, rtol=0, atol=1e-12)          # 0, 1, 2, 3, 4, 5: one straight line
    # a ramp is cut at the segment's own ends: a 2-frame segment between two eligible boundaries, R = 8
    rows = [[(0, 1.0, 0.0, 0.0, 0), (6, 1.0, 4.0, 0.0, 0), (8, 1.0, 8.0, 0.0, 0)]]
    _, o, _, _, ratio, _ = _plan(rows, [16], 8)
    semis = 12.0 * np.log2(ratio[0])
    assert o[0].tolist() == [0, 6, 8, 16]
    assert np.allclose(semis[:2], 0.0, atol=1e-12) and np.allclose(semis[12:], 8.0, atol=1e-12)
    assert np.allclose(semis[2:6], 4.0 * np.arange(1, 5) / 9.0, atol=1e-12)    # segment 0's share of the first ramp
    assert np.allclose(semis[6:8], 4.0 + 4.0 * np.arange(3, 5) / 9.0, atol=1e-12)      # segment 1: the later boundary's ramp
    assert np.allclose(semis[8:12], 4.0 + 4.0 * np.arange(5, 9) / 9.0, atol=1e-12)


def test_curve_warp_restatement_reduces_to_the_scalar_one():
    mag = np.asarray(10.0 ** np.random.RandomState(0).uniform(-5.6, 1.4, (2, 12, 65)), dtype=np.float32).astype(np.float64)
    tin, rate, ratio = [12, 7], [0.8, 1.25], [2 ** (4 / 12.0), 2 ** (-3 / 12.0)]
    tout = [P.out_frames(n, r, TMIN) for n, r in zip(tin, rate)]
    T_out = max(tout)
    pos = np.stack([np.arange(T_out) * r for r in rate])
    q = np.stack([np.full(T_out, v) for v in ratio])
    for preserve in (0, 1):
        want = P.warp(mag, tin, tout, rate, ratio, 5, preserve, T_out)
        got, det = C.curve_warp(mag, tin, tout, pos, q, np.ones((2, T_out), np.float32), 5, preserve, T_out, details=True)
        assert np.array_equal(got, want)
        half = C.curve_warp(mag, tin, tout, pos, q, np.full((2, T_out), 0.5, np.float32), 5, preserve, T_out)
        assert np.array_equal(half, 0.5 * want)
        quiet = pos.copy()
        quiet[0, 3] = -1.0
        quiet[1, 2] = np.nan
        out = C.curve_warp(mag, tin, tout, quiet, q, np.ones((2, T_out), np.float32), 5, preserve, T_out)
        assert not out[0, 3].any() and not out[1, 2].any() and np.array_equal(out[0, 4], want[0, 4])
        assert np.array_equal(C.curve_bound(det, want.shape), P.bound(det, want.shape))        # gain 1: no extra term


# ----------------------------------------------------------------------------------------------------------------------
# plan_map
# ----------------------------------------------------------------------------------------------------------------------
def _host_plan(rows, tlen_in):
    t, o, tout, _, _, _ = _plan(rows, tlen_in)
    S = t["rate"].shape[1]
    c = np.array([C.repair(t["bounds"][b], int(t["nseg"][b]), n) + [n] * (S - int(t["nseg"][b])) for b, n in enumerate(tlen_in)])
    return {"c": torch.from_numpy(c.astype(np.int32)), "o": torch.from_numpy(o.astype(np.int32)),
            "nseg": torch.from_numpy(t["nseg"]), "rate": torch.from_numpy(t["rate"]),
            "break_frames": torch.from_numpy(t["brk"])}, t, o, tout


def test_plan_map_is_monotone_a_break_is_a_gap_and_a_span_is_stretched():
    from deepvoice3_pytorch_amd import audio
    cfg = audio.AudioConfig()
    plan, t, o, tout = _host_plan(ROWS, TLEN)
    frames = torch.arange(0, 22)[None, :].repeat(3, 1).clamp(max=torch.tensor(TLEN)[:, None])
    start, end = audio.plan_map(plan, frames, "start"), audio.plan_map(plan, frames, "end")
    assert start.dtype == torch.float64 and start.shape == (3, 22)
    assert (start[:, 1:] >= start[:, :-1]).all() and (end[:, 1:] >= end[:, :-1]).all() and (end <= start).all()
    assert (start[:, 0] == 0).all() and (end[:, 0] == 0).all()
    sec = cfg.hop_size / float(cfg.sample_rate)
    # item 0: the break of 4 frames after [5, 9): a token that ends at frame 9 ends before it, one that starts there after
    gap = float(start[0, 9] - end[0, 9])
    assert gap == 4.0 and gap * sec == 4 * cfg.hop_size / float(cfg.sample_rate)
    assert float(start[0, 5] - end[0, 5]) == 0.0                               # no break: no gap
    # a span at rate r is stretched by 1 / r to within one frame; the span that ends the item has its frames as POINTS, the
    # last one kept in place as the scalar warp keeps it (warped_frames): (L - 1) / r + 1 to within half a frame
    for (b, s, x0, x1) in ((0, 0, 0, 5), (0, 1, 5, 9), (0, 2, 9, 15), (1, 0, 0, 3), (1, 2, 3, 8)):
        got = float(end[b, x1] - start[b, x0])
        assert abs(got - (x1 - x0) / t["rate"][b, s]) <= 1.0, (b, s, got)
    for (b, s, x0, x1) in ((0, 3, 15, 21), (1, 3, 8, 11), (2, 0, 0, 9)):
        got = float(end[b, x1] - start[b, x0])
        assert abs(got - ((x1 - x0 - 1) / t["rate"][b, s] + 1.0)) <= 0.5, (b, s, got)
    inside = audio.plan_map(plan, torch.tensor([[12.0], [5.5], [4.5]]), "start")           # inside a span: linear
    assert abs(float(inside[0, 0]) - (float(o[0, 2]) + 3 / 1.7)) <= 0.5 and abs(float(inside[1, 0]) - (float(o[1, 2]) + 5.0)) < 1e-12
    # the end of the item is the end of its speech: a trailing break (5 frames on item 2, 2 on item 0) is part of no token
    assert float(end[2, 9]) == float(o[2, 1]) - 5 and float(end[0, 21]) == float(o[0, 4]) - 2
    with pytest.raises(ValueError, match="side"):
        audio.plan_map(plan, frames, "middle")


# ----------------------------------------------------------------------------------------------------------------------
# pitch closure in float64: |lws_stft| -> curve warp under a plan -> fast Griffin-Lim -> YIN
# ----------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def tone_magnitudes():
    from oracle import audio_oracle as A
    mag = np.abs(A.lws_stft(P.harmonic_tones(T=C.T_CLOSURE), P.N_FFT, P.HOP))
    assert mag.shape == (len(P.TONE_F0), C.T_CLOSURE, P.N_FFT // 2 + 1)
    return np.asarray(mag, dtype=np.float32).astype(np.float64)


@pytest.mark.parametrize("preserve", [1, 0])
def test_pitch_closure_in_float64(tone_magnitudes, preserve):
    """Two steady tones (140 and 205 Hz), 48 frames: [0, 20) as it is and 6 silent frames, then [20, 48) up 4 semitones at
    rate 0.8 -- T' = 61, the parts at output frames [0, 20) and [26, 61).  After 30 fast Griffin-Lim iterations and YIN the
    median F0 over each part's frames (5 left out at each end) lies within 25 cents of f0 x ratio_s, and YIN's power in
    the break's inner frames (2 left out at each end) lies at least 20 dB under the first part's median.  Conditions on
    the method, not measurements (measured here: within 0.7 cents, the break 30.8 and 32.1 dB down)."""
    from tests import fast_gl_ref as R
    from tests import pitch_ref as Y
    B, T = len(P.TONE_F0), C.T_CLOSURE
    t, o, tout, pos, ratio, gain = _plan([C.CLOSURE_ROWS] * B, [T] * B)
    assert tout.tolist() == [61] * B and o[0].tolist() == [0, 26, 61]
    out = C.curve_warp(tone_magnitudes, None, tout, pos, ratio, gain, 19, preserve, 61)
    y = R.fast_griffin_lim(out, 30, P.HOP, P.N_FFT, 0.99)
    res = Y.yin_frames(y.reshape(-1), [y.shape[1]] * B, P.HOP, P.N_FFT, P.YIN_LAGS[0], P.YIN_LAGS[1], P.YIN_THRESHOLD,
                       float(P.SR))
    assert res["frames"].tolist() == [61] * B
    for b, f0 in enumerate(P.TONE_F0):
        track, power = np.asarray(res["f0"][b * 61:(b + 1) * 61]), np.asarray(res["power"][b * 61:(b + 1) * 61])
        for first, last, semis in C.CLOSURE_PARTS:
            got = float(np.median(track[first + 5:last - 5]))
            c = P.cents(got, f0 * 2.0 ** (semis / 12.0))
            print("f0 %g Hz, part [%d, %d) %+g st, preserve %d: median %.2f Hz, %+.2f cents" % (f0, first, last, semis, preserve, got, c))
            assert abs(c) <= P.CENTS, (f0, first, got, c)
        ref = float(np.median(power[0:20]))
        inner = power[C.CLOSURE_BREAK[0] + 2:C.CLOSURE_BREAK[1] - 2]
        down = 10.0 * np.log10(ref / float(inner.max()))
        print("f0 %g Hz, preserve %d: the break lies %.1f dB under the first part" % (f0, preserve, down))
        assert down >= C.BREAK_DB, (f0, down)


# ----------------------------------------------------------------------------------------------------------------------
# options
# ----------------------------------------------------------------------------------------------------------------------
def test_marks_refuse_by_value():
    from deepvoice3_pytorch_amd import audio
    M = audio.ProsodyMarks
    for bad, word in ((dict(rate=0.2), "rate=0.2"), (dict(rate=4.5), "rate=4.5"), (dict(rate=float("nan")), "rate=nan"),
                      (dict(rate=True), "rate=True"), (dict(semitones=25), "semitones=25"), (dict(semitones=-24.5), "semitones=-24.5"),
                      (dict(gain_db=21), "gain_db=21"), (dict(gain_db=-40.5), "gain_db=-40.5"), (dict(gain_db="loud"), "gain_db='loud'"),
                      (dict(speed=2.0), "speed")):
        with pytest.raises(ValueError, match=re.escape(word)):
            M(spans=[(0, 3, bad)])
    for spans, word in (([(3, 3, {})], "empty"), ([(4, 2, {})], "empty"), ([(0, 4, {}), (3, 6, {})], "overlaps"),
                        ([(5, 8, {}), (0, 2, {})], "overlaps or precedes"), ([(-1, 2, {})], "-1"), ([(0, 2.5, {})], "2.5"),
                        ([(0, 2)], "dict of settings"), ([(0, 2, 1.5)], "dict of settings")):
        with pytest.raises(ValueError, match=word):
            M(spans=spans)
    for breaks, word in (([(2, 10.5)], "10.5"), ([(2, -0.1)], "-0.1"), ([(2, float("nan"))], "nan"), ([(-1, 0.3)], "-1"),
                         ([(2, 0.3), (2, 0.1)], "two breaks after index 2"), ([(2,)], "after_index, seconds")):
        with pytest.raises(ValueError, match=word):
            M(breaks=breaks)
    with pytest.raises(ValueError, match="units='steps'"):
        M(units="steps")
    for bad in (-1.0, float("nan"), float("inf"), None):
        with pytest.raises(ValueError, match="transition_ms"):
            M(transition_ms=bad)
    with pytest.raises(ValueError, match="envelope_hz"):
        M(envelope_hz=0.0)
    with pytest.raises(ValueError, match="envelope_hz=10.0"):
        M(envelope_hz=10.0).half_width(audio.AudioConfig())
    with pytest.raises(ValueError, match="transition_ms=60000.0"):                   # 5168 frames
        M(transition_ms=60000.0).ramp_frames(audio.AudioConfig())
    # 64 segments are taken, 65 refused: 32 separate spans cut the utterance 64 times
    assert len(M(spans=[(2 * k + 1, 2 * k + 2, dict(rate=0.9)) for k in range(31)], breaks=[(62, 0.1)]).cuts) == 63
    with pytest.raises(ValueError, match="65 segments"):
        M(spans=[(2 * k + 1, 2 * k + 2, dict(rate=0.9)) for k in range(32)])
    with pytest.raises(ValueError, match="65 segments"):
        M(breaks=[(k, 0.1) for k in range(64)])


def test_marks_compile_to_the_segment_table():
    from deepvoice3_pytorch_amd import audio
    cfg = audio.AudioConfig()
    m = audio.ProsodyMarks(spans=[(2, 5, dict(rate=0.8)), (5, 7, dict(semitones=3, gain_db=6.0)), (9, 12, dict(rate=1.5, semitones=-2))],
                           breaks=[(6, 0.3), (3, 0.1)], transition_ms=35.0)
    t = m.segments(cfg)
    assert t["start"].tolist() == [0, 2, 4, 5, 7, 9, 12]                      # gaps between and around the spans are segments
    assert t["rate"].tolist() == [1.0, 0.8, 0.8, 1.0, 1.0, 1.5, 1.0]
    assert t["semitones"].tolist() == [0.0, 0.0, 0.0, 3.0, 0.0, -2.0, 0.0] and t["gain_db"].tolist() == [0, 0, 0, 6.0, 0, 0, 0]
    # 0.3 s = 25.84 frames -> 26 after the segment that ends with unit 6; 0.1 s = 8.61 -> 9 after unit 3
    assert t["break_frames"].tolist() == [0, 9, 0, 26, 0, 0, 0] and t["break_frames"].dtype == np.int32
    assert m.ramp_frames(cfg) == 3 and m.key() == (True, 400.0, 35.0) and m.half_width(cfg) == 19 and not m.neutral()
    assert audio.ProsodyMarks().neutral() and audio.ProsodyMarks().segments(cfg)["start"].tolist() == [0]
    assert audio.ProsodyMarks(spans=[(0, 4, {}), (6, 9, dict(rate=1.0, semitones=0, gain_db=0.0))], breaks=[(3, 0.0)]).neutral()
    assert not audio.ProsodyMarks(breaks=[(3, 0.01)]).neutral() and not audio.ProsodyMarks(spans=[(0, 1, dict(gain_db=-1))]).neutral()
    two = audio.marks_tables([m, None], cfg)
    assert two["nseg"].tolist() == [7, 1] and two["start"].shape == (2, 8) and two["start"][1].tolist() == [0] + [2 ** 31 - 1] * 7
    assert two["rate"][1].tolist() == [1.0] * 7 and two["break_frames"][1].tolist() == [0] * 7
    with pytest.raises(ValueError, match="share"):
        audio.marks_tables([m, audio.ProsodyMarks(spans=[(0, 1, dict(rate=2.0))], preserve_envelope=False)], cfg)


def test_the_keywords_of_synthesis():
    from deepvoice3_pytorch_amd import audio, synthesis
    um = synthesis.utterance_marks
    slow = audio.ProsodyMarks(spans=[(0, 3, dict(rate=0.8))])
    assert um(None, None, None, None, 2, "t") is None and um([None, None], None, None, None, 2, "t") is None
    assert um([audio.ProsodyMarks(), None], None, None, None, 2, "t") is None          # neutral marks: nothing to do
    assert um([slow, audio.ProsodyMarks()], None, None, None, 2, "t") == [slow, None] and um(slow, None, None, None, 2, "t") == [slow, slow]
    for kw in (dict(rate=0.8), dict(semitones=1.0), dict(prosody=audio.Prosody())):
        args = dict(rate=None, semitones=None, prosody=None)
        args.update(kw)
        with pytest.raises(ValueError, match="one mechanism per call"):
            um([slow], args["rate"], args["semitones"], args["prosody"], 1, "t")
    with pytest.raises(ValueError, match="3 marks for 2 items"):
        um([slow, None, None], None, None, None, 2, "t")
    with pytest.raises(ValueError, match="'frames' given where 'tokens'"):
        um([audio.ProsodyMarks(spans=[(0, 3, dict(rate=0.8))], units="frames")], None, None, None, 1, "t")
    with pytest.raises(ValueError, match="audio.ProsodyMarks"):
        um(["slow"], None, None, None, 1, "t")
    for fn in (synthesis.tts_batch, synthesis.tts_stream, synthesis.RollingSynthesizer.submit):
        assert inspect.signature(fn).parameters["marks"].default is None
    assert issubclass(audio.MarksNotApplied, UserWarning)
    for fn in (audio.plan_prosody, audio.plan_map, audio.warp_magnitudes_curve):
        assert callable(fn)
    x = torch.zeros(1, 8, 513)
    with pytest.raises(ValueError, match="'tokens' given where 'frames'"):
        audio.inv_spectrogram_batch(x, prosody=slow)
    with pytest.raises(ValueError, match="2 marks for 1 items"):
        audio.inv_spectrogram_batch(x, prosody=[None, audio.ProsodyMarks(units="frames")])


# ----------------------------------------------------------------------------------------------------------------------
# the library's refusals, the header and the build
# ----------------------------------------------------------------------------------------------------------------------
_WARP = dict(mag=64, out=128, B=1, T_in=4, T_out=4, bins=513, tlen_in=None, tlen_out=64, pos=64, ratio=64, gain=64, W=19,
             preserve=1)


@pytest.mark.parametrize("kw,names", [
    (dict(mag=None), b"mag is null"), (dict(out=None), b"out is null"), (dict(tlen_out=None), b"tlen_out is null"),
    (dict(pos=None), b"pos is null"), (dict(ratio=None), b"ratio is null"), (dict(gain=None), b"gain is null"),
    (dict(out=64), b"out must not be mag"), (dict(mag=66), b"4-byte aligned"), (dict(gain=66), b"4-byte aligned"),
    (dict(pos=68), b"8-byte aligned"), (dict(ratio=68), b"8-byte aligned"), (dict(B=0), b"B = 0"), (dict(B=65536), b"B = 65536"),
    (dict(T_in=0), b"T_in = 0"), (dict(T_out=0), b"T_out = 0"), (dict(bins=0), b"bins = 0"), (dict(bins=1026), b"bins = 1026"),
    (dict(W=0), b"env_half_width = 0"), (dict(W=65), b"env_half_width = 65"), (dict(W=0, preserve=0), b"env_half_width = 0"),
    (dict(preserve=2), b"preserve_envelope = 2"),
])
def test_curve_warp_refuses_every_violation_without_a_gpu(kw, names):
    """dummy non-null pointers: a refusal comes before any launch, so nothing is dereferenced"""
    from deepvoice3_pytorch_amd import _lib
    lib = _lib.lib()
    a = dict(_WARP, **kw)
    rc = lib.dv3_curve_warp_f32(a["mag"], a["out"], a["B"], a["T_in"], a["T_out"], a["bins"], a["tlen_in"], a["tlen_out"],
                                a["pos"], a["ratio"], a["gain"], a["W"], a["preserve"], None)
    assert rc == _lib.CONSTS["DV3_EINVAL"]
    msg = lib.dv3_last_error()
    assert msg.startswith(b"curve_warp:") and names in msg, msg


_SEG = dict(tlen_in=None, B=1, T_in=8, S=3, nseg=64, bounds=64, rate=64, semitones=64, gain_db=64, brk=64, min_frames=4, o=64,
            tlen_out=64, T_out=8, R=0, pos=64, ratio=64, gain=64)


def _call_plan(lib, a):
    return lib.dv3_curve_plan_f64(a["tlen_in"], a["B"], a["T_in"], a["S"], a["nseg"], a["bounds"], a["rate"], a["brk"],
                                  a["min_frames"], a["o"], a["tlen_out"], None)


def _call_fill(lib, a):
    return lib.dv3_curve_fill_f64(a["tlen_in"], a["B"], a["T_in"], a["S"], a["nseg"], a["bounds"], a["rate"], a["semitones"],
                                  a["gain_db"], a["brk"], a["o"], a["tlen_out"], a["T_out"], a["R"], a["pos"], a["ratio"],
                                  a["gain"], None)


@pytest.mark.parametrize("kw,names", [
    (dict(nseg=None), b"nseg is null"), (dict(bounds=None), b"bounds is null"), (dict(rate=None), b"rate is null"),
    (dict(brk=None), b"break_frames is null"), (dict(o=None), b"o is null"), (dict(tlen_out=None), b"tlen_out is null"),
    (dict(rate=68), b"8-byte aligned"), (dict(B=0), b"B = 0"), (dict(B=65536), b"B = 65536"), (dict(T_in=0), b"T_in = 0"),
    (dict(S=0), b"S = 0"), (dict(S=65), b"S = 65"), (dict(min_frames=-1), b"min_frames = -1"),
])
def test_curve_plan_refuses_every_violation_without_a_gpu(kw, names):
    from deepvoice3_pytorch_amd import _lib
    lib = _lib.lib()
    assert _call_plan(lib, dict(_SEG, **kw)) == _lib.CONSTS["DV3_EINVAL"]
    msg = lib.dv3_last_error()
    assert msg.startswith(b"curve_plan:") and names in msg, msg


@pytest.mark.parametrize("kw,names", [
    (dict(nseg=None), b"nseg is null"), (dict(bounds=None), b"bounds is null"), (dict(rate=None), b"rate is null"),
    (dict(semitones=None), b"semitones is null"), (dict(gain_db=None), b"gain_db is null"), (dict(brk=None), b"break_frames is null"),
    (dict(o=None), b"o is null"), (dict(tlen_out=None), b"tlen_out is null"), (dict(pos=None), b"pos is null"),
    (dict(ratio=None), b"ratio is null"), (dict(gain=None), b"gain is null"), (dict(semitones=68), b"8-byte aligned"),
    (dict(pos=68), b"8-byte aligned"), (dict(B=0), b"B = 0"), (dict(T_in=0), b"T_in = 0"), (dict(S=0), b"S = 0"),
    (dict(S=65), b"S = 65"), (dict(T_out=0), b"T_out = 0"), (dict(R=-1), b"ramp_frames = -1"), (dict(R=4097), b"ramp_frames = 4097"),
])
def test_curve_fill_refuses_every_violation_without_a_gpu(kw, names):
    from deepvoice3_pytorch_amd import _lib
    lib = _lib.lib()
    assert _call_fill(lib, dict(_SEG, **kw)) == _lib.CONSTS["DV3_EINVAL"]
    msg = lib.dv3_last_error()
    assert msg.startswith(b"curve_fill:") and names in msg, msg


def test_the_header_exports_the_entry_points_under_abi_50():
    import ctypes
    from deepvoice3_pytorch_amd import _lib, audio
    P_, I = ctypes.c_void_p, ctypes.c_int32
    assert _lib.FUNCS["dv3_curve_warp_f32"] == (ctypes.c_int, [P_, P_, I, I, I, I, P_, P_, P_, P_, P_, I, I, P_])
    assert _lib.FUNCS["dv3_curve_plan_f64"] == (ctypes.c_int, [P_, I, I, I, P_, P_, P_, P_, I, P_, P_, P_])
    assert _lib.FUNCS["dv3_curve_fill_f64"] == (ctypes.c_int, [P_, I, I, I, P_, P_, P_, P_, P_, P_, P_, P_, I, I, P_, P_, P_, P_])
    assert _lib.CONSTS["DV3_ABI_VERSION"] == 50 and _lib.CONSTS["DV3_PROSODY_MAX_SEGMENTS"] == 64
    assert _lib.CONSTS["DV3_PROSODY_MAX_RATE"] == C.MAX_RATE and _lib.CONSTS["DV3_PROSODY_MAX_BREAK"] == C.MAX_BREAK
    assert _lib.CONSTS["DV3_PROSODY_MAX_RAMP"] == 4096 and _lib.CONSTS["DV3_PROSODY_MAX_HALF_WIDTH"] == 64
    header = open(os.path.join(ROOT, "include", "dv3hip.h")).read()
    m = re.search(r"/\*((?:(?!\*/).)*)\*/\s*#define DV3_PROSODY_MAX_SEGMENTS 64", header, flags=re.S)
    assert m, "the definitions stand in the comment in front of the entry points"
    text = re.sub(r"\s*\n \*\s*", " ", m.group(1))
    for word in ("silence", "floor(u)", "NOT checked on the device", "bit for bit", "c_nseg = n", "min_frames clamp",
                 "pos = -1", "exp2(semitones / 12)", "ramp_frames = R", "Refused"):
        assert word in text, word
    src = open(os.path.join(ROOT, "deepvoice3_pytorch_amd", "csrc", "prosody.hip")).read()
    assert src.count("void warp_frame(") == 1 and len(re.findall(r"^\s+warp_frame\(mag \+", src, flags=re.M)) == 2, \
        "one body, called by the scalar and the curve kernel"
    assert "dv3_curve_warp_f32" in inspect.getsource(audio.warp_magnitudes_curve)
    assert "dv3_curve_plan_f64" in inspect.getsource(audio.plan_prosody) and "dv3_curve_fill_f64" in inspect.getsource(audio.plan_prosody)

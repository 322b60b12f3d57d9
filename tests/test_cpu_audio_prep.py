# coding: utf-8
"""Host side of VCTK preprocessing, no GPU needed: the fp64 restatements the GPU kernels are measured against
(tests/audio_prep_ref.py) have the properties their definitions promise; the coefficient table the package uploads is
the restatement's kernel; preprocess.read_vctk / read_hts_labels / load_wav(path, None) on synthetic files."""
import os

import numpy as np
import pytest
from scipy.io import wavfile

from tests import audio_prep_ref as R

from deepvoice3_pytorch_amd import audio, preprocess


# ---- resampler restatement: 0.5 s unit sines at 48 kHz -> 22.05 kHz (147 / 320) ----
def _tone(f, n=24000, sr=48000.0):
    return np.sin(2 * np.pi * f * np.arange(n) / sr)


@pytest.mark.parametrize("f", [100.0, 1000.0, 5000.0, 9000.0])
def test_resample_restatement_passes_tones(f):
    y = R.resample(_tone(f), 147, 320)
    assert y.size == 11025
    want = np.sin(2 * np.pi * f * np.arange(y.size) / 22050.0)
    err = np.abs(y - want)[400:-400].max()
    print("f = %g Hz: max error %.2e" % (f, err))
    assert err < 1e-7


@pytest.mark.parametrize("f", [11500.0, 13000.0, 20000.0])
def test_resample_restatement_stops_tones_above_the_new_nyquist(f):
    y = R.resample(_tone(f), 147, 320)
    assert y.size == 11025
    amp = np.abs(y)[400:-400].max()
    print("f = %g Hz: output amplitude %.2e" % (f, amp))
    assert amp < 1e-6


def test_resample_restatement_lengths_and_ratios():
    for up, down in ((147, 320), (1, 2), (160, 147), (2, 1), (441, 160)):
        for L in (1, 2, 63, 1000):
            assert R.resample(np.ones(L), up, down).size == -(-L * up // down)
    assert (R.half_width(147, 320), R.half_width(1, 2), R.half_width(2, 1), R.half_width(160, 147)) == (140, 128, 64, 64)
    # an impulse at sample 0 reads the kernel back: y[n] = h(n down / up)
    x = np.zeros(50)
    x[0] = 1.0
    y = R.resample(x, 2, 1)
    assert np.allclose(y[:40], R.kernel(np.arange(40) / 2.0, 1.0), rtol=0, atol=1e-15)
    assert abs(y[0] - R.ROLLOFF) < 1e-15                    # NOT the identity: the roll-off scales the centre tap


def test_coefficient_table_is_the_restatement_kernel():
    for up, down in ((147, 320), (1, 2), (160, 147), (2, 1), (441, 160)):
        H = R.half_width(up, down)
        assert audio.resample_half_width(up, down) == H
        tab = audio.resample_table_np(up, down)
        assert tab.shape == (2 * H + 2, up) and tab.dtype == np.float64
        s = min(1.0, up / down)
        for r in sorted({0, 1 % up, up // 2, up - 1}):
            frac = ((r * down) % up) / up
            want = R.kernel(H - np.arange(2 * H + 2) + frac, s)
            assert np.abs(tab[:, r] - want).max() < 1e-15
    assert audio.resample_ratio(48000, 22050) == (147, 320)
    assert audio.resample_ratio(22050, 22050) == (1, 1)
    assert audio.resample_ratio(16000, 22050) == (441, 320)
    assert (audio.RESAMPLE_ZEROS, audio.RESAMPLE_ROLLOFF, audio.RESAMPLE_BETA) == (R.ZEROS, R.ROLLOFF, R.BETA)


# ---- trim restatement: silence / burst / silence, spans computed by hand ----
def _burst(n, lo, hi, level=0.5, floor=0.0, seed=0):
    rng = np.random.RandomState(seed)
    x = floor * rng.randn(n)
    x[lo:hi] = level * rng.randn(hi - lo)
    return x


def test_trim_restatement_on_bursts():
    # burst over samples [5120, 10240) of 20480: frame f covers [512 f - 1024, 512 f + 1024); a frame with m of its
    # 2048 samples inside the burst sits 10 log10(m / 2048) dB below a full frame.  At top_db = 15 (m / 2048 > 0.0316,
    # m > 64.8) the first kept frame is f = 9 ([3584, 5632): 512 inside), not f = 8 ([3072, 5120): none); the last kept
    # is f = 21 ([9728, 11776): 512 inside), f = 22 starts at 10240.  Span: [9 * 512, 22 * 512) = (4608, 6656).
    x = _burst(20480, 5120, 10240)
    assert R.trim(x, 15.0) == (4608, 6656)
    assert R.trim(x, 25.0) == (4608, 6656)                   # exact zeros outside: any threshold keeps the same frames
    # a burst touching the start: frame 0 is its own reflection, all burst; the end is as above
    x = _burst(20480, 0, 5120)
    assert R.trim(x, 15.0) == (0, 12 * 512)                  # last kept f = 11 ([4608, 6656): 512 inside)
    # a burst touching the end of a signal whose length is not a hop multiple: the span is clipped to the length
    x = _burst(20000, 15360, 20000)
    assert R.trim(x, 15.0) == (29 * 512, 20000 - 29 * 512)   # first kept f = 29 ([13824, 15872): 512 inside)
    # a floor 40 dB under the burst is trimmed at 15 and 25 dB, one 10 dB under is kept whole at 15 dB
    assert R.trim(_burst(20480, 5120, 10240, 0.5, 0.005), 25.0) == (4608, 6656)
    assert R.trim(_burst(20480, 5120, 10240, 0.5, 0.16), 15.0) == (0, 20480)
    # all-zero input: every frame is at the 1e-10 floor, 0 dB under the maximum -- librosa keeps it whole
    assert R.trim(np.zeros(4096), 15.0) == (0, 4096)
    # shorter than 1025 samples: unchanged; exactly 1025 can be padded
    assert R.trim(_burst(1024, 100, 200), 15.0) == (0, 1024)
    assert R.trim(_burst(1025, 0, 1025), 15.0) == (0, 1025)
    assert audio.trim_num_frames(1024) == 0 and audio.trim_num_frames(1025) == 3 and audio.trim_num_frames(20000) == 40
    assert (audio.TRIM_FRAME, audio.TRIM_HOP) == (R.FRAME, R.HOP)


# ---- the VCTK reader ----
def _wav(path, rate, n=400):
    os.makedirs(os.path.dirname(path), exist_ok=True)
    wavfile.write(path, rate, (np.arange(n) % 100).astype(np.int16))


def _txt(path, text):
    os.makedirs(os.path.dirname(path), exist_ok=True)
    with open(path, "w", encoding="utf-8") as f:
        f.write(text)


def test_read_vctk(tmp_path):
    root = str(tmp_path / "VCTK-Corpus")
    w = lambda spk, n: os.path.join(root, "wav48", spk, "%s_%03d.wav" % (spk, n))
    t = lambda spk, n: os.path.join(root, "txt", spk, "%s_%03d.txt" % (spk, n))
    for spk, n in (("p226", 2), ("p226", 1), ("p226", 3), ("p225", 1), ("p225", 10), ("p315", 1), ("p300", 1)):
        _wav(w(spk, n), 48000)
    _txt(t("p226", 1), "Please call Stella.\n")
    _txt(t("p226", 2), "  Ask her to bring these things.  \n")
    # p226_003 has no transcript; p226_004 has a transcript and no recording
    _txt(t("p226", 4), "orphan transcript")
    _txt(t("p225", 1), "Six spoons of fresh snow peas.")
    _txt(t("p225", 10), "Five thick slabs of blue cheese.\n")
    _txt(t("p300", 1), "We also need a small plastic snake.")
    # p315: recordings, no txt/ directory (as in the published corpus); a stray file under wav48/ is not a speaker
    _txt(os.path.join(root, "wav48", "README"), "x")
    _txt(os.path.join(root, "wav48", "p226", "notes.md"), "x")
    speakers, rows = preprocess.read_vctk(root)
    assert speakers == ["p225", "p226", "p300"]
    assert rows == [
        (w("p225", 1), "Six spoons of fresh snow peas.", 0),
        (w("p225", 10), "Five thick slabs of blue cheese.", 0),
        (w("p226", 1), "Please call Stella.", 1),
        (w("p226", 2), "Ask her to bring these things.", 1),
        (w("p300", 1), "We also need a small plastic snake.", 2),
    ]
    assert preprocess.vctk_label_path(w("p225", 1)) == os.path.join(root, "lab", "p225", "p225_001.lab")


def test_read_hts_labels(tmp_path):
    def lab(name, lines):
        p = str(tmp_path / name)
        with open(p, "w") as f:
            f.write("\n".join(lines) + "\n")
        return p
    # leading and trailing pau: first / last non-pau label
    assert preprocess.read_hts_labels(lab("a.lab", [
        "0 2500000 pau", "2500000 3100000 p", "3100000 4000000 l", "4000000 9000000 pau"])) == (2500000, 4000000)
    # none: the file's own extent
    assert preprocess.read_hts_labels(lab("b.lab", [
        "100000 2500000 h", "2500000 3100000 pau", "3100000 4000000 l"])) == (100000, 4000000)
    # several pau at both ends, one inside; the label is the LAST field of a line
    assert preprocess.read_hts_labels(lab("c.lab", [
        "0 10 pau", "10 20 pau", "20 30 x y a", "30 40 pau", "40 50 x y b", "50 60 pau", "60 70 pau"])) == (20, 50)
    # leading pau only / trailing pau only
    assert preprocess.read_hts_labels(lab("d.lab", ["0 10 pau", "10 20 a", "20 30 b"])) == (10, 30)
    assert preprocess.read_hts_labels(lab("e.lab", ["0 10 a", "10 20 b", "20 30 pau"])) == (0, 20)
    with pytest.raises(ValueError):
        preprocess.read_hts_labels(lab("f.lab", ["0 10 pau", "10 20 pau"]))
    # the cut on the resampled signal, as the reference truncates it (vctk.py:62-63)
    b, e = 2500000, 4000000
    assert (int(b * 1e-7 * 22050), int(e * 1e-7 * 22050)) == (5512, 8820)


def test_load_wav_returns_the_rate_when_asked(tmp_path):
    p = str(tmp_path / "a.wav")
    x = np.array([-32768, 0, 16384, 32767], dtype=np.int16)
    wavfile.write(p, 48000, x)
    y, sr = preprocess.load_wav(p, None)
    assert sr == 48000 and isinstance(sr, int)
    assert y.dtype == np.float32 and np.array_equal(y, x.astype(np.float32) / 32768)
    # the old call form is unchanged: an array, and a mismatch raises
    assert np.array_equal(preprocess.load_wav(p, 48000), y)
    with pytest.raises(ValueError, match="resampling is not supported"):
        preprocess.load_wav(p)
    with pytest.raises(ValueError, match="48000"):
        preprocess.load_wav(p, 22050)


def test_cli_knows_vctk_and_dispatch_rejects_unknown_names(tmp_path):
    assert preprocess.DATASETS == ("ljspeech", "vctk")
    with pytest.raises(ValueError, match="unknown dataset"):
        preprocess.build_from_path(str(tmp_path), str(tmp_path / "o"), name="jsut")
    with pytest.raises(SystemExit):
        preprocess.main(["jsut", "a", "b"])


def test_restatement_against_pinned_librosa_vectors():
    """tests/golden/audio_prep_librosa.npz, written by scripts/pin_audio_prep.py on a box that has `librosa` and
    `resampy`: inputs + the packages' own resampled signals and trim indices.  Absent until someone runs it; until then
    parity with the packages themselves is unpinned.

    Resampler bound, by reasoning: resampy evaluates the same windowed sinc from a table of 512 samples per zero
    crossing with linear interpolation; the interpolation error of one coefficient is at most step^2 / 8 * max|h''| =
    (1 / 512)^2 / 8 * s * rho^3 pi^2 / 3 (the second derivative of rho sinc(rho t) at 0 bounds it; the window only
    lowers it) = 1.3e-6 s, so |y - y_resampy| <= 1.3e-6 s sum_k |x_k| over the taps, plus the float32 rounding of the
    stored output (2^-24 |y|).  The first and last 400 outputs are left out: the two pad the ends differently.
    Trim: equal as integers where no frame is within 0.05 dB of the threshold, for librosa <= 0.9 (reflect padding)."""
    from tests.util import GOLDEN
    path = os.path.join(GOLDEN, "audio_prep_librosa.npz")
    if not os.path.exists(path):
        pytest.skip("tests/golden/audio_prep_librosa.npz not generated yet (scripts/pin_audio_prep.py needs librosa)")
    z = np.load(path, allow_pickle=False)
    up, down = 147, 320
    s = up / down
    H = R.half_width(up, down)
    coef_err = (1.0 / 512) ** 2 / 8 * s * R.ROLLOFF ** 3 * np.pi ** 2 / 3
    reflect = tuple(int(v) for v in str(z["librosa_version"]).split(".")[:2]) <= (0, 9)
    for i in range(int(z["n"])):
        x, y = z["x%d" % i].astype(np.float64), z["y%d" % i].astype(np.float64)
        mine = R.resample(x, up, down)
        assert y.size == mine.size
        xp = np.concatenate([np.zeros(H), np.abs(x), np.zeros(H + 2 + down)])
        csum = np.concatenate([[0.0], np.cumsum(xp)])
        i0 = (np.arange(mine.size, dtype=np.int64) * down) // up
        bound = coef_err * (csum[i0 + 2 * H + 2] - csum[i0]) + 2.0 ** -24 * np.abs(mine) + 1e-12
        err = np.abs(y - mine)
        print("item %d: max |restatement - librosa| %.3e (bound / error at least %.1f)"
              % (i, err[400:-400].max(), (bound / np.maximum(err, 1e-300))[400:-400].min()))
        assert np.all(err[400:-400] <= bound[400:-400])
        if reflect:
            for top_db in (15, 25):
                if np.abs(R.trim_frame_db(y) + top_db).min() >= 0.05:
                    lo, n = R.trim(y, float(top_db))
                    assert [lo, lo + n] == z["trim%d_%d" % (top_db, i)].tolist()

# coding: utf-8
"""-m gpu: the audio kernels of csrc/audio.hip, element by element, against float64 with derived bounds
(tests/audio_kernels_ref.py: every bound is stated there term by term; tests/test_cpu_audio_kernels_ref.py shows that a
float32 emulation stays inside them and that mutated emulations do not).  Sizes 512, 1024 and 2048, both framings, hops
n/4 and 3n/16, B <= 3 and at most 12 frames except where a family says otherwise.  Every element is checked, nothing is
masked out, and every check prints its worst ratio error / bound.

Families:  W unit white noise;  S a staircase (the level falls by 2^-2 per hop, items at 2^12, 1, 2^-12: every frame and
item is judged at its own scale);  I one unit sample at every offset of a frame (every bin per bin: every twiddle path
of every pass);  K single bins through the inverse frames kernel (every k, arbitrary phasors, also at DC and Nyquist);
T bin-centred tones through the fused two-frame projection (every bin over four launches, even and odd T, and a variant
whose odd frames lie 2^-16 below the even ones);  Z silence.  White noise does not pin the projection (its derived bound is
~1 % of a frame: random spectra have near-zero bins); the chained Griffin-Lim tests keep that role.
"""
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tests import audio_kernels_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu
GUARD = 7.0


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


def _report(what, ratio):
    print("worst-ratio %-72s %.4g" % (what, ratio))


def _check(tag, ratios):
    """print every ratio, then hold all of them to 1"""
    for k in sorted(ratios):
        _report("%s %s" % (tag, k), ratios[k])
    bad = {k: v for k, v in ratios.items() if not v <= 1.0}
    assert not bad, (tag, bad)


def _configs(n):
    return [(fr, hop) for fr in R.FRAMINGS for hop in R.hops(n)]


def _api():
    from deepvoice3_pytorch_amd import audio, _lib
    from deepvoice3_pytorch_amd.ops import _stream
    return audio, _lib, _stream


def _ptr(t):
    return t.data_ptr() if t is not None else None


def _stft(dev, y32, n, hop, fr):
    """-> spec [B, T, F, 2], phasor [B, T, F, 2], mag_bct [B, F, T] (numpy float32), all three from one launch"""
    audio, _lib, _stream = _api()
    y = torch.from_numpy(y32).to(dev)
    B, L = y.shape
    T = R.num_frames(L, n, hop, fr)
    F = n // 2 + 1
    sp = torch.full((B, T, F, 2), GUARD, dtype=torch.float32, device=dev)
    ph = torch.full((B, T, F, 2), GUARD, dtype=torch.float32, device=dev)
    mb = torch.full((B, F, T), GUARD, dtype=torch.float32, device=dev)
    if fr == "lws":
        assert T == audio.lws_num_frames(L, hop, n)
        awin, _ = audio.lws_windows(dev, hop, None, n)
        _lib.call("dv3_lws_stft_f32_n", y.data_ptr(), awin.data_ptr(), ph.data_ptr(), sp.data_ptr(), mb.data_ptr(), B, T, hop, L, n,
                  _stream())
    else:
        assert L == hop * (T - 1)
        _lib.call("dv3_stft_phase_f32_n", y.data_ptr(), ph.data_ptr(), sp.data_ptr(), mb.data_ptr(), B, T, hop, n, _stream())
    return sp.cpu().numpy(), ph.cpu().numpy(), mb.cpu().numpy()


def _frames(dev, mag32, ph32, n, hop, fr):
    audio, _lib, _stream = _api()
    mag = torch.from_numpy(mag32).to(dev)
    ph = torch.from_numpy(ph32).to(dev) if ph32 is not None else None
    B, T, F = mag.shape
    out = torch.full((B, T, n), GUARD, dtype=torch.float32, device=dev)
    if fr == "lws":
        _, swin = audio.lws_windows(dev, hop, None, n)
        _lib.call("dv3_lws_istft_frames_f32_n", mag.data_ptr(), _ptr(ph), swin.data_ptr(), out.data_ptr(), B, T, n, _stream())
    else:
        _lib.call("dv3_istft_frames_f32_n", mag.data_ptr(), _ptr(ph), out.data_ptr(), B, T, n, _stream())
    return out.cpu().numpy()


def _project(dev, y32, mag32, n, hop, fr):
    """-> flat [B * T + 1, n]: the frames and a guard frame behind them, which must come back untouched"""
    audio, _lib, _stream = _api()
    y, mag = torch.from_numpy(y32).to(dev), torch.from_numpy(mag32).to(dev)
    B, T, F = mag.shape
    assert y.shape == (B, R.signal_len(T, n, hop, fr)) and F == n // 2 + 1
    out = torch.full((B * T + 1, n), GUARD, dtype=torch.float32, device=dev)
    if fr == "lws":
        awin, swin = audio.lws_windows(dev, hop, None, n)
        _lib.call("dv3_lws_gl_project_f32_n", y.data_ptr(), mag.data_ptr(), awin.data_ptr(), swin.data_ptr(), out.data_ptr(), B, T,
                  hop, n, _stream())
    else:
        _lib.call("dv3_gl_project_f32_n", y.data_ptr(), mag.data_ptr(), out.data_ptr(), B, T, hop, n, _stream())
    return out.cpu().numpy()


# ----------------------------------------------------------------------------------------------------------------------
# forward transform, phasor, mag_bct
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", R.SIZES)
def test_spectrum_phasor_and_magnitude(dev, n):
    """families W and S: every bin inside its frame's per-bin bound, every frame inside the norm-wise one; mag_bct bit for
    bit and the phasor to 4 u per component AS FUNCTIONS OF THE RETURNED SPECTRUM, at every bin (no magnitude mask).
    Family Z: item 1 silenced -- exact zeros, nothing non-finite, and items 0 and 2 unchanged bit for bit."""
    ratios = {}
    for fr, hop in _configs(n):
        for fam, make in (("W", R.family_W), ("S", R.family_S)):
            y = make(n, hop, fr)
            sp, ph, mb = _stft(dev, y, n, hop, fr)
            tag = "%s %s hop %d " % (fam, fr, hop)
            assert np.isfinite(sp).all() and np.isfinite(ph).all() and np.isfinite(mb).all(), tag
            for k, v in R.judge_spectrum(sp, y, n, hop, fr).items():
                ratios[tag + k] = v
            ratios[tag + "phasor"] = R.judge_phasor(ph, sp)["phasor"]
            ratios[tag + "mag_bct bits"] = 0.0 if np.array_equal(mb, R.mag_bct_exact(sp)) else float("inf")
            if fam == "W":
                y0 = y.copy()
                y0[1] = 0
                sp0, ph0, mb0 = _stft(dev, y0, n, hop, fr)
                ok = (not sp0[1].any() and not ph0[1].any() and not mb0[1].any() and np.isfinite(ph0).all() and
                      all(np.array_equal(a[i], b[i]) for a, b in ((sp, sp0), (ph, ph0), (mb, mb0)) for i in (0, 2)))
                ratios["Z %s hop %d silent item" % (fr, hop)] = 0.0 if ok else float("inf")
    _check("n %d spectrum" % n, ratios)


@pytest.mark.parametrize("n", R.SIZES)
def test_spectrum_of_impulses_per_bin(dev, n):
    """family I: hop items, an impulse at every position of one hop, so every offset of a frame occurs; the reference
    is w[m] exp(-2 pi i k m / n) and every bin is held to (dw[m] + (u + Cfft u) w[m]) -- relative to that frame's one
    sample.  A wrong twiddle, index or sign on any path of any pass moves some bin of some offset by far more."""
    ratios = {}
    for fr, hop in _configs(n):
        y = R.family_I(n, hop, fr)
        sp, _, _ = _stft(dev, y, n, hop, fr)
        ratios["I %s hop %d bin" % (fr, hop)] = R.judge_spectrum(sp, y, n, hop, fr)["bin"]
    _check("n %d impulses" % n, ratios)


# ----------------------------------------------------------------------------------------------------------------------
# inverse frames and overlap-add
# ----------------------------------------------------------------------------------------------------------------------
def _inverse_inputs(n, hop, fam, B=3, T=12):
    """W: random magnitudes and phasors; S: the staircase across frames, items at 2^12, 1, 2^-12"""
    rng = np.random.RandomState(n + hop + (fam == "S"))
    F = n // 2 + 1
    mag = rng.rand(B, T, F)
    if fam == "S":
        mag = mag * (4.0 ** -np.arange(T))[None, :, None] * np.array([2.0 ** 12, 1.0, 2.0 ** -12])[:, None, None]
    phz = rng.uniform(-np.pi, np.pi, (B, T, F))
    return mag.astype(np.float32), np.stack([np.cos(phz), np.sin(phz)], axis=-1).astype(np.float32)


@pytest.mark.parametrize("n", R.SIZES)
def test_istft_per_sample(dev, n):
    """families W and S through the overlap-add: every sample, then the first and last n samples and the samples on both
    sides of each switch between the 2/3 shortcut and acc / wsum on their own lines.  Family Z: an all-zero item gives
    exact zeros and leaves its neighbours' bits alone; zero phase (phasor NULL) is held to the same bounds."""
    audio, _, _ = _api()
    ratios = {}
    for fr, hop in _configs(n):
        for fam in ("W", "S"):
            mag, ph = _inverse_inputs(n, hop, fam)
            mag_d, ph_d = torch.from_numpy(mag).to(dev), torch.from_numpy(ph).to(dev)
            got = audio.istft(mag_d, ph_d, hop, convention=fr, fft_size=n).cpu().numpy()
            j = R.judge_istft(got, mag, ph, n, hop, fr)
            assert j.pop("n_switch") == (4 if (fr == "torch" and hop * 4 == n) else 0)
            for k, v in j.items():
                ratios["%s %s hop %d %s" % (fam, fr, hop, k)] = v
            if fam == "W":
                gz = audio.istft(torch.from_numpy(mag).to(dev), None, hop, convention=fr, fft_size=n).cpu().numpy()
                ratios["W %s hop %d zero phase" % (fr, hop)] = R.judge_istft(gz, mag, None, n, hop, fr)["all"]
                m0 = mag.copy()
                m0[1] = 0
                g0 = audio.istft(torch.from_numpy(m0).to(dev), ph_d, hop, convention=fr, fft_size=n).cpu().numpy()
                ok = not g0[1].any() and np.array_equal(g0[0], got[0]) and np.array_equal(g0[2], got[2])
                ratios["Z %s hop %d silent item" % (fr, hop)] = 0.0 if ok else float("inf")
    _check("n %d istft" % n, ratios)


@pytest.mark.parametrize("n", R.SIZES)
def test_inverse_frames_of_single_bins(dev, n):
    """family K: frame t holds mag = 1 at bin t alone, T = n/2 + 1 frames of one item, straight through the frames kernel:
    every sample against (c / n) cos(2 pi k m / n + phi) w[m] (c = 2, at DC and Nyquist 1 and the real part of the
    phasor alone), to a bound relative to the amplitude"""
    mag, ph, _ = R.family_K(n)
    ratios = {}
    for fr in R.FRAMINGS:
        got = _frames(dev, mag, ph, n, n // 4, fr)
        ratios["K %s" % fr] = R.judge_frames(got, mag, ph, n, n // 4, fr)["frames"]
    _check("n %d single bins" % n, ratios)


# ----------------------------------------------------------------------------------------------------------------------
# the fused two-frame projection
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", R.SIZES)
def test_projection_of_tones(dev, n):
    """family T through gl_project2_kernel: every output sample of every frame, even and odd T (an unpaired last frame),
    tones on every bin 0 .. n/2 over the four launches, and the guard frame behind the buffer untouched.  The 2^-16
    variant (torch framing, hop = n): the quiet frames' bound carries the loud partner's rounding, their worst ratio and
    their error relative to their own peak go on record.  Family Z: an all-zero mag and a silent item give exact zeros,
    the other items keep their bits."""
    ratios = {}
    for fr in R.FRAMINGS:
        for hop, T, bins, quiet in R.tone_launches(n, fr):
            y, mag = R.family_T(n, hop, fr, T, bins, quiet)
            flat = _project(dev, y, mag, n, hop, fr)
            B = len(bins)
            got = flat[:B * T].reshape(B, T, n)
            assert np.isfinite(got).all()
            j = R.judge_project(got, y, mag, n, hop, fr)
            tag = "T%s %s hop %d T %d" % (" 2^-16" if quiet else "", fr, hop, T)
            ratios[tag] = j["all"]
            ratios[tag + " guard frame"] = 0.0 if (flat[B * T] == GUARD).all() else float("inf")
            if quiet:
                ratios[tag + " quiet frames"] = j["odd"]
                print("%s: error / own peak: loud frames %.3g, quiet frames %.3g" % (tag, j["rel_even"], j["rel_odd"]))
        hop, T = n // 4, 7
        y, mag = R.family_T(n, hop, fr, T, [3, n // 5, n // 2 - 2], False)
        base = _project(dev, y, mag, n, hop, fr)[:3 * T].reshape(3, T, n)
        y0, m0 = y.copy(), mag.copy()
        y0[1] = 0
        g1 = _project(dev, y0, mag, n, hop, fr)[:3 * T].reshape(3, T, n)
        m0[1] = 0
        g2 = _project(dev, y, m0, n, hop, fr)[:3 * T].reshape(3, T, n)
        g3 = _project(dev, y, np.zeros_like(mag), n, hop, fr)[:3 * T]
        ok = (not g1[1].any() and not g2[1].any() and not g3.any() and
              all(np.array_equal(g[i], base[i]) for g in (g1, g2) for i in (0, 2)))
        ratios["Z %s silence" % fr] = 0.0 if ok else float("inf")
    _check("n %d projection" % n, ratios)


# ----------------------------------------------------------------------------------------------------------------------
# point-wise kernels
# ----------------------------------------------------------------------------------------------------------------------
def test_pointwise_kernels(dev):
    """gl_prepare relative per element over its 100 dB range, the clip ends, their neighbours and values outside the clip;
    amp_to_db_norm absolute per element at 0, below and at the floor, both clip ends and their neighbours;
    preemphasis to half an ulp of the float64 value"""
    audio, _lib, _stream = _api()
    ratios = {}
    lin = R.grid_gl_prepare()
    for power in (1.4, 1.0):
        x = torch.from_numpy(lin).to(dev)
        out = torch.empty_like(x)
        _lib.call("dv3_gl_prepare_f32", x.data_ptr(), out.data_ptr(), x.numel(), -100.0, 20.0, float(power), _stream())
        mag, rb = R.gl_prepare_ref(lin, power=power)
        ratios["gl_prepare power %.1f" % power] = R.worst(np.abs(out.cpu().numpy().astype(np.float64) / mag - 1), rb)
    for ref_db in (20.0, -20.0):
        g = R.grid_db_norm(ref_db=ref_db)
        x = torch.from_numpy(g).to(dev)
        out = torch.empty_like(x)
        _lib.call("dv3_amp_to_db_norm_f32", x.data_ptr(), out.data_ptr(), x.numel(), -100.0, float(ref_db), _stream())
        want, b = R.db_norm_ref(g, ref_db=ref_db)
        got = out.cpu().numpy().astype(np.float64)
        assert got.min() >= 0 and got.max() == 1
        ratios["amp_to_db_norm ref_db %.0f" % ref_db] = R.worst(np.abs(got - want), b)
    x32 = R.deemph_input(3073)
    for coef in (0.97, -0.5, 0.0):
        x = torch.from_numpy(x32).to(dev)
        out = torch.empty_like(x)
        _lib.call("dv3_preemphasis_f32", x.data_ptr(), out.data_ptr(), x.shape[0], x.shape[1], float(coef), _stream())
        s, b = R.preemph_ref(x32, coef)
        got = out.cpu().numpy()
        ok0 = np.array_equal(got[:, 0], x32[:, 0])
        ratios["preemphasis coef %g" % coef] = R.worst(np.abs(got[:, 1:] - s[:, 1:]), b[:, 1:]) if ok0 else float("inf")
    _check("point-wise", ratios)


# ----------------------------------------------------------------------------------------------------------------------
# de-emphasis
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("coef", R.DEEMPH_COEFS)
def test_deemphasis_per_sample(dev, coef):
    """both forms (chunked with its 1024-sample warm-up; serial with powf carries: in place, or coef 0.9995), every
    sample: L on both sides of the chunk seams and below one thread's 16 samples, B = 2 (odd L: a misaligned second row),
    a DC offset of 0.5, in place and out of place, plain and with lens in {0, L + 5} and {1, L}"""
    _, _lib, _stream = _api()
    ratios = {}
    for L in R.DEEMPH_LENGTHS:
        x32 = R.deemph_input(L)
        for inplace in (False, True):
            for lens in R.deemph_lens(L):
                x = torch.from_numpy(x32).to(dev)
                out = x if inplace else torch.full_like(x, GUARD)
                if lens is None:
                    _lib.call("dv3_deemphasis_f32", x.data_ptr(), out.data_ptr(), 2, L, float(coef), _stream())
                else:
                    ln = torch.tensor(lens, dtype=torch.int32, device=dev)
                    _lib.call("dv3_deemphasis_items_f32", x.data_ptr(), out.data_ptr(), 2, L, ln.data_ptr(), float(coef), _stream())
                got = out.cpu().numpy()
                assert np.isfinite(got).all()
                key = "%s %s%s" % (R.deemph_form(coef, inplace), "in place" if inplace else "out of place",
                                   "" if lens is None else " lens")
                r = R.judge_deemph(got, x32, coef, lens, inplace)["deemph"]
                if not r <= 1.0:
                    print("deemphasis coef %g L %d %s lens %s: ratio %.4g" % (coef, L, key, lens, r))
                ratios[key] = max(ratios.get(key, 0.0), r)
    _check("deemphasis coef %g" % coef, ratios)

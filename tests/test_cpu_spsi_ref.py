# coding: utf-8
"""Single Pass Spectrogram Inversion without a GPU: tests/spsi_ref.py pinned to known answers and to its own rule as
written, the convergence conditions tests/test_gpu_spsi.py holds the device to, shown here for the float64 restatement
alone, and the plumbing: the configuration option, the C header's entry point, the Makefile."""
import ctypes
import inspect
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tests import fast_gl_ref as R  # noqa: E402
from tests import spsi_ref as S  # noqa: E402


def _f32(x):
    return np.asarray(x, dtype=np.float32).astype(np.float64)


# ----------------------------------------------------------------------------------------------------------------------
# known answers
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,hop,centre", [(512, 128, 20.3), (1024, 192, 100.75), (2048, 512, 333.4)])
def test_a_stationary_sinusoid_between_two_bins(n, hop, centre):
    """One lobe (a Gaussian of width 1.5 bins about `centre`, every frame the same).  Along the peak bin k the phase
    advances per frame by exactly hop (k + d) / n turns, d the parabola's vertex from the three magnitudes; every bin
    of the lobe carries the peak's value; the phasor alternates in sign along the lobe."""
    F, T = n // 2 + 1, 7
    row = _f32(np.exp(-0.5 * ((np.arange(F) - centre) / 1.5) ** 2))
    mag = np.tile(row, (1, T, 1))
    turns = S.spsi_turns(mag, hop, n)
    assert turns.shape == (1, T, F) and turns.min() >= 0.0 and turns.max() < 1.0
    k = int(np.argmax(row))
    assert S.peaks(row).sum() == 1 and S.peaks(row)[k] and k in (int(np.floor(centre)), int(np.ceil(centre)))
    d = 0.5 * (row[k - 1] - row[k + 1]) / (row[k - 1] - 2.0 * row[k] + row[k + 1])
    assert abs(d) <= 0.5 and abs(k + d - centre) < 0.1           # a parabola through a Gaussian: near, not exact
    step = hop * (k + d) / n
    for t in range(T):
        want = (t + 1) * step
        err = abs(turns[0, t, k] - (want - np.floor(want)))
        assert min(err, 1.0 - err) < 1e-12, (t, turns[0, t, k], want)
    lobe = np.arange(k - 4, k + 5)                               # strictly monotone on both sides in fp32
    assert np.all(np.diff(row[k - 4:k + 1]) > 0) and np.all(np.diff(row[k:k + 5]) < 0)
    assert np.array_equal(turns[0][:, lobe], np.repeat(turns[0][:, k:k + 1], lobe.size, axis=1))
    ph = S.spsi_phasor(mag, hop, n)
    assert np.allclose(np.abs(ph), 1.0, atol=1e-15)
    want = np.exp(2j * np.pi * turns[0][:, k:k + 1]) * (1.0 - 2.0 * (lobe % 2))[None, :]
    assert np.abs(ph[0][:, lobe] - want).max() < 1e-15
    assert np.all(np.real(ph[0][:, lobe[:-1]] * np.conj(ph[0][:, lobe[1:]])) < -0.999999)     # neighbours: opposite


def test_d_needs_no_clamp():
    """|d| <= 0.5 at every peak, ties and zeros included (the denominator is strictly negative there)"""
    rng = np.random.RandomState(0)
    m = _f32(np.round(rng.rand(200, 257) * 8) / 8)
    pk = S.peaks(m)[:, 1:-1]
    lo, mid, hi = m[:, :-2][pk], m[:, 1:-1][pk], m[:, 2:][pk]
    den = lo - 2.0 * mid + hi
    assert pk.sum() > 1000 and np.all(den < 0) and np.all(np.abs(0.5 * (lo - hi) / den) <= 0.5)


# ----------------------------------------------------------------------------------------------------------------------
# ownership
# ----------------------------------------------------------------------------------------------------------------------
HAND_ROW = [5, 3, 1, 4, 2, 6, 6, 2, 2, 1, 8, 5, 4, 4, 3, 7]
#  bins 0-1   a falling edge from bin 0: the climb ends on bin 0, never a peak         -> none
#  bin 2      a valley between bin 0's edge and the peak 3: climbs right               -> 3
#  bin 4      a valley between the peaks 3 and 5: goes to the right one                -> 5
#  bin 5      6 > 2 and 6 >= 6: a peak;  bin 6: 6 > 6 fails, a plateau                 -> 5, none
#  bin 7      climbs left onto the plateau bin 6, no peak                              -> none
#  bin 8      2 = 2 on the left, 1 below on the right: nowhere to climb                -> none
#  bins 9-12  a valley climbing right, the peak 10, one and two climbs left            -> 10
#  bin 13     4 = 4 on the left, 3 below on the right                                  -> none
#  bins 14-15 a rising edge into bin F - 1, never a peak                               -> none
HAND_OWNERS = [-1, -1, 3, 3, 5, 5, -1, -1, -1, 10, 10, 10, 10, -1, -1, -1]


def test_ownership_by_the_rule():
    assert S.owners_literal(HAND_ROW).tolist() == HAND_OWNERS
    assert S.owners(np.array(HAND_ROW, dtype=np.float64)).tolist() == HAND_OWNERS
    assert np.nonzero(S.peaks(HAND_ROW))[0].tolist() == [3, 5, 10]
    rng = np.random.RandomState(1)
    for i in range(300):                                  # the vectorised form against the rule as written, ties included
        F = rng.randint(3, 48)
        row = np.round(rng.rand(F) * 5) / 5 if i % 2 else rng.rand(F)
        assert np.array_equal(S.owners(row), S.owners_literal(row)), row
    both = S.owners(np.stack([HAND_ROW, HAND_ROW[::-1]]).astype(np.float64))
    assert both[0].tolist() == HAND_OWNERS and np.array_equal(both[1], S.owners_literal(HAND_ROW[::-1]))


def test_lobes_carry_their_owners_phase_and_the_rest_zero():
    n, hop, T = 512, 96, 5
    rng = np.random.RandomState(2)
    mag = _f32(np.round(rng.rand(2, T, n // 2 + 1) * 6) / 6)
    turns = S.spsi_turns(mag, hop, n)
    for b in range(2):
        for t in range(T):
            own = S.owners_literal(mag[b, t])
            assert (own < 0).sum() > 10 and (own >= 0).sum() > 100
            assert np.array_equal(turns[b, t], np.where(own >= 0, turns[b, t][np.maximum(own, 0)], 0.0))
            if t:                                                # the whole row is replaced: an unowned bin restarts at 0
                k = np.nonzero(S.peaks(mag[b, t]))[0]
                m = mag[b, t]
                d = 0.5 * (m[k - 1] - m[k + 1]) / (m[k - 1] - 2.0 * m[k] + m[k + 1])
                x = turns[b, t - 1][k] + ((hop * k) % n) / n + hop * d / n
                assert np.array_equal(turns[b, t][k], x - np.floor(x))


# ----------------------------------------------------------------------------------------------------------------------
# convergence of the restatement
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,hop", R.CONVERGENCE_CASES)
def test_spsi_start_on_speechlike_magnitudes(n, hop):
    """Spectral convergence on fast_gl_ref.speechlike_magnitudes (B = 2, T = 40).  Measured for the restatement at
    512 / 128, 1024 / 256, 2048 / 512:
        SPSI, 0 iterations        0.1657  0.1652  0.1641   (< 0.2;  without the (-1)^k term: 0.64)
        SPSI + 10 at 0.99         0.0769  0.0776  0.0714   (< 60 plain iterations from zero: 0.1098  0.1123  0.0849)
        SPSI + 30 at 0.99         0.0523  0.0515  0.0505   (< zero + 30 at 0.99:             0.0583  0.0611  0.0564)"""
    mag = R.speechlike_magnitudes(n, hop)
    ph = S.spsi_phasor(mag, hop, n)

    def sc(iters, alpha, init):
        return R.spectral_convergence(R.fast_griffin_lim(mag, iters, hop, n, alpha, init), mag, hop, n)
    s0, unsigned = sc(0, 0.0, ph), sc(0, 0.0, np.exp(2j * np.pi * S.spsi_turns(mag, hop, n)))
    s10, s30, z30, p60 = sc(10, 0.99, ph), sc(30, 0.99, ph), sc(30, 0.99, None), R.plain60(n, hop)
    print("n %d hop %d: spsi 0 it. %.4f (without the sign term %.4f), spsi + 10 @ 0.99 %.4f, 60 plain %.4f, "
          "spsi + 30 @ 0.99 %.4f, zero + 30 @ 0.99 %.4f" % (n, hop, s0, unsigned, s10, p60, s30, z30))
    assert s0 < 0.2, s0
    assert unsigned > 0.5, unsigned                       # the sign term is what makes it a start at all
    assert s10 < p60, (s10, p60)
    assert s30 < z30, (s30, z30)


# ----------------------------------------------------------------------------------------------------------------------
# ragged batches
# ----------------------------------------------------------------------------------------------------------------------
def test_ragged_items_are_their_own_b1_runs():
    n, hop, T = 512, 128, 9
    tl = [9, 4, 0, 1]
    mag = _f32(np.random.RandomState(3).rand(len(tl), T, n // 2 + 1) ** 2)
    ph, turns = S.spsi_phasor(mag, hop, n, tl), S.spsi_turns(mag, hop, n, tl)
    for b, k in enumerate(tl):
        assert np.all(ph[b, k:] == 1.0 + 0.0j) and not turns[b, k:].any(), b
        if k:
            assert np.array_equal(ph[b, :k], S.spsi_phasor(mag[b:b + 1, :k], hop, n)[0]), b
            assert np.array_equal(turns[b, :k], S.spsi_turns(mag[b:b + 1, :k], hop, n)[0]), b
    assert np.array_equal(S.spsi_phasor(mag, hop, n), S.spsi_phasor(mag, hop, n, [T] * len(tl)))


# ----------------------------------------------------------------------------------------------------------------------
# plumbing
# ----------------------------------------------------------------------------------------------------------------------
def test_audio_config_takes_the_init_and_refuses_by_value():
    from deepvoice3_pytorch_amd import audio, preprocess
    assert audio.AudioConfig().griffin_lim_init == "zero"
    assert audio.AudioConfig(griffin_lim_init="zero").griffin_lim_init == "zero"
    assert audio.AudioConfig(griffin_lim_init="spsi", griffin_lim_iters=10).griffin_lim_init == "spsi"
    for bad in ("SPSI", "lws", "", None, 0, True):
        with pytest.raises(ValueError, match=r"griffin_lim_init=.*'zero'.*'spsi'"):
            audio.AudioConfig(griffin_lim_init=bad)
    p = inspect.signature(audio.AudioConfig.__init__).parameters
    assert list(p)[-1] == "griffin_lim_init" and p["griffin_lim_init"].default == "zero"
    assert list(inspect.signature(audio.spsi_phasor).parameters) == ["mag", "hop", "tlen", "fft_size"]
    assert inspect.signature(audio.spsi_phasor).parameters["fft_size"].default == 1024
    assert list(inspect.signature(audio.griffin_lim).parameters)[-1] == "momentum"
    # the option is not a property of stored features
    d = preprocess.audio_config_dict(audio.AudioConfig(griffin_lim_init="spsi"), 80, 125, 7600, False, 0.999)
    assert not [k for k in d if "init" in k or "griffin" in k]


def test_the_inverse_starts_where_the_config_says(monkeypatch):
    """inv_spectrogram_batch, its items path and inv_melspectrogram_batch: "spsi" calls spsi_phasor on the magnitudes
    just made (with the items' frame counts on the items path) and hands the result to griffin_lim; "zero" does not
    call it; an explicit init_phasor wins.  The device functions are replaced by recorders: no GPU."""
    import torch
    from deepvoice3_pytorch_amd import audio
    calls = []
    mags = torch.full((2, 12, 513), 2.0)
    monkeypatch.setattr(audio, "magnitudes", lambda lin, cfg: mags)
    monkeypatch.setattr(audio, "mel_to_linear", lambda mel, cfg, fl, up, opt: torch.zeros(2, 12, 513))

    def spsi(mag, hop, tlen=None, fft_size=1024):
        calls.append(("spsi", mag is mags, hop, None if tlen is None else tlen.tolist(), fft_size))
        return "SPSI"

    def gl(mag, hop, n_iter, init_phasor=None, convention="torch", window_scale=None, tlen=None, fft_size=1024,
           momentum=0.0):
        calls.append(("gl", init_phasor, None if tlen is None else tlen.tolist()))
        return torch.zeros(2, 13 * hop - fft_size)
    monkeypatch.setattr(audio, "spsi_phasor", spsi)
    monkeypatch.setattr(audio, "griffin_lim", gl)
    monkeypatch.setattr(audio, "inv_preemphasis_", lambda y, coef: y)
    monkeypatch.setattr(audio._lib, "call", lambda *a: None)              # the items path's de-emphasis launch
    monkeypatch.setattr(audio, "_stream", lambda: None)
    lin = torch.zeros(2, 12, 513)
    zero, on = audio.AudioConfig(), audio.AudioConfig(griffin_lim_init="spsi")
    for fl, tl in ((None, None), ([12, 7], [12, 7])):
        for run in (lambda c, ph: audio.inv_spectrogram_batch(lin, c, ph, fl),
                    lambda c, ph: audio.inv_melspectrogram_batch(torch.zeros(2, 12, 80), c, fl, init_phasor=ph)):
            del calls[:]
            run(zero, None)
            assert calls == [("gl", None, tl)]
            del calls[:]
            run(on, None)
            assert calls == [("spsi", True, 256, tl, 1024), ("gl", "SPSI", tl)]
            del calls[:]
            run(on, "MINE")
            assert calls == [("gl", "MINE", tl)]


def test_header_makefile_and_abi():
    from deepvoice3_pytorch_amd import _lib
    p, i = ctypes.c_void_p, ctypes.c_int
    restype, args = _lib.FUNCS["dv3_spsi_phasor_f32"]
    # mag, phasor, B, T, hop, tlen, fft_size, stream
    assert restype is ctypes.c_int and args == [p, p, i, i, i, p, i, p]
    assert _lib.CONSTS["DV3_ABI_VERSION"] == 50
    assert [f for f in _lib.FUNCS if "spsi" in f] == ["dv3_spsi_phasor_f32"]
    header = open(os.path.join(ROOT, "include", "dv3hip.h")).read()
    assert "int dv3_spsi_phasor_f32(const float* mag, float* phasor, int B, int T, int hop, const int32_t* tlen" in header
    make = open(os.path.join(ROOT, "deepvoice3_pytorch_amd", "csrc", "Makefile")).read()
    assert "spsi.hip" in make.split("SRCS")[1].split("OBJS")[0]
    src = open(os.path.join(ROOT, "deepvoice3_pytorch_amd", "csrc", "spsi.hip")).read()
    assert "Beauregard" in src and "audio.py:37-43" in src and "run_lws" in src
    assert "Beauregard" in open(os.path.join(ROOT, "PAPERS.md")).read()

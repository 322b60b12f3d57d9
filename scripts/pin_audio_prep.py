#!/usr/bin/env python
# coding: utf-8
"""Pin the waveform preparation of VCTK preprocessing to the REAL packages the reference calls.

Run once on any box that has `librosa` (with `resampy` for its kaiser_best resampler) -- neither can be installed in the
build image (no network):

    python scripts/pin_audio_prep.py              # writes tests/golden/audio_prep_librosa.npz

The file holds inputs and the packages' own outputs for the reference's two call sites: `librosa.resample(x, 48000,
22050, res_type="kaiser_best")` (what `librosa.load(path, sr=22050)` of audio.py:12-13 does to a 48 kHz file) and
`librosa.effects.trim(y, top_db)` for top_db = 15 and 25 (vctk.py:66,68), with the package versions.
tests/test_cpu_audio_prep.py::test_restatement_against_pinned_librosa_vectors then holds tests/audio_prep_ref.py -- the
yardstick of the HIP kernels -- to those vectors on every box.  Nothing of the packages' source is copied: the file is
data (inputs + outputs)."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def signals(rng):
    """silence / speech-like / silence at 48 kHz, 0.4 - 1.5 s, band-limited well under 11 kHz"""
    out = []
    for L in (19200, 30001, 48000, 72000):
        lo, hi = int(0.2 * L), int(0.8 * L)
        t = np.arange(hi - lo) / 48000.0
        x = 1e-4 * rng.randn(L)
        x[lo:hi] += 0.3 * np.sin(2 * np.pi * rng.uniform(100, 300) * t) + 0.05 * np.sin(2 * np.pi * 3000.0 * t) \
            + 0.02 * rng.randn(hi - lo)
        out.append(x.astype(np.float32))
    return out


def main():
    try:
        import librosa
    except ImportError:
        sys.exit("the `librosa` package is not importable here: run this on a box where it is installed")
    rng = np.random.RandomState(4321)
    out = {"librosa_version": np.array(librosa.__version__)}
    try:
        import resampy
        out["resampy_version"] = np.array(resampy.__version__)
    except ImportError:
        sys.exit("the `resampy` package (librosa's kaiser_best resampler) is not importable here")
    sigs = signals(rng)
    out["n"] = np.int64(len(sigs))
    for i, x in enumerate(sigs):
        try:
            y = librosa.resample(x, orig_sr=48000, target_sr=22050, res_type="kaiser_best")
        except TypeError:                          # librosa < 0.10: positional rates
            y = librosa.resample(x, 48000, 22050, res_type="kaiser_best")
        out["x%d" % i], out["y%d" % i] = x, np.asarray(y)
        for top_db in (15, 25):
            _, index = librosa.effects.trim(y, top_db=top_db)
            out["trim%d_%d" % (top_db, i)] = np.asarray(index, dtype=np.int64)
    path = os.path.join(ROOT, "tests", "golden", "audio_prep_librosa.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, "| librosa", librosa.__version__, "resampy", resampy.__version__)


if __name__ == "__main__":
    main()

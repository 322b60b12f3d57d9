# coding: utf-8
"""-m gpu: free-running evaluation (synthesis.evaluate_synthesis / mel_distortion / SynthEvalTotals) on
toy models of both decoder families.  The targets are made from the model's own free-running mel of the same
sentences, so what the figures must be is known without a trained voice:

  1. targets = the synthesis itself -> zero distortion, the diagonal, duration ratio 1;
  2. every target frame doubled -> zero distortion, one target-only move per synthesised frame, duration ratio 1/2;
  3. a constant added to every band -> still zero (c0, the level, is left out);
  4. an offset in one band -> the per-frame distortion worked out by hand from the definition of the features.
"""
import math
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tests import dtw_ref as DR  # noqa: E402
from tests.test_gpu_rolling_decode import NY_HP, DV3_HP  # noqa: E402  (the toy hyper-parameters)

pytestmark = pytest.mark.gpu

LENS = [19, 6, 13, 3]
_RUNS = {}


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


def _setup(family, dev, max_steps=24):
    """-> model, hp, seqs, mels: the free-running mel of every sentence (tts_batch), computed once per family and cap"""
    if (family, max_steps) not in _RUNS:
        from deepvoice3_pytorch_amd import builder, audio, synthesis
        torch.manual_seed(3)
        make, hp = dict(nyanko=(builder.nyanko, NY_HP), deepvoice3=(builder.deepvoice3, DV3_HP))[family]
        hp = dict(hp, linear_dim=257)                             # the bins of a 512-point FFT: tts_batch ends in Griffin-Lim
        model = make(**hp).to(dev).eval()
        dec = model.seq2seq.decoder
        dec.min_decoder_steps, dec.max_decoder_steps = 0, max_steps
        cfg = audio.AudioConfig(fft_size=512, hop_size=128, sample_rate=16000, griffin_lim_iters=1)
        rng = np.random.RandomState(11)
        seqs = [rng.randint(2, hp["n_vocab"], n).tolist() for n in LENS]
        mels = [res[0].clone() for res in synthesis.tts_batch(model, seqs, audio_cfg=cfg)]
        _RUNS[(family, max_steps)] = (model, hp, seqs, mels)
    return _RUNS[(family, max_steps)]


def _evaluate(model, hp, seqs, targets, **kw):
    from deepvoice3_pytorch_amd import synthesis
    table = synthesis.evaluate_synthesis(model, seqs, targets, downsample_step=hp["downsample_step"], **kw)
    totals = synthesis.SynthEvalTotals()
    totals.add(table if not isinstance(table, tuple) else table[0], ids=list(range(len(seqs))))
    return table, totals.result()


def _col(table, name):
    from deepvoice3_pytorch_amd import synthesis
    return table[:, synthesis.SYNTH_EVAL_COLUMNS.index(name)].tolist()


@pytest.mark.parametrize("family", ["nyanko", "deepvoice3"])
def test_own_synthesis_as_target(dev, family):
    model, hp, seqs, mels = _setup(family, dev)
    ds = hp["downsample_step"]
    frames = [float(m.size(0)) for m in mels]
    targets = [m.repeat_interleave(ds, dim=0) for m in mels]              # [::ds] returns the synthesis
    (table, rows), tot = _evaluate(model, hp, seqs, targets, diagnostics=True)
    assert table.shape == (len(seqs), 7) and table.dtype == torch.float32 and table.is_cuda
    print(family, table.tolist())
    assert _col(table, "mcd_sum") == [0.0] * len(seqs)
    assert _col(table, "path_len") == _col(table, "frames_synth") == _col(table, "frames_target") == frames
    assert _col(table, "n_diag") == [f - 1 for f in frames]
    assert tot["duration_ratio"] == 1.0 and tot["mcd"] == 0.0 and tot["n_items"] == len(seqs)
    assert [it["id"] for it in tot["items"]] == list(range(len(seqs)))
    # the alignment rows are tts_batch's
    from deepvoice3_pytorch_amd import synthesis
    assert len(rows) == len(seqs)
    for b, row in enumerate(rows):
        assert row["keys"] == LENS[b] and row["steps"] * hp["r"] == frames[b]
        assert row["flags"] == synthesis.alignment_flags(row, model.seq2seq.decoder.max_decoder_steps)
    # CPU tensors and arrays are taken too, and the table alone comes back without diagnostics
    plain = synthesis.evaluate_synthesis(model, seqs, [t.cpu().numpy() for t in targets], downsample_step=ds)
    assert torch.equal(plain, table)


@pytest.mark.parametrize("family", ["nyanko", "deepvoice3"])
def test_doubled_target_frames(dev, family):
    model, hp, seqs, mels = _setup(family, dev)
    ds = hp["downsample_step"]
    frames = [float(m.size(0)) for m in mels]
    targets = [m.repeat_interleave(2 * ds, dim=0) for m in mels]          # [::ds] returns every frame twice
    table, tot = _evaluate(model, hp, seqs, targets)
    print(family, table.tolist())
    assert _col(table, "mcd_sum") == [0.0] * len(seqs)
    assert _col(table, "n_target_only") == _col(table, "frames_synth") == frames
    assert _col(table, "frames_target") == [2 * f for f in frames]
    assert _col(table, "path_len") == [2 * f for f in frames] and _col(table, "n_synth_only") == [0.0] * len(seqs)
    assert tot["duration_ratio"] == 0.5 and tot["mcd"] == 0.0


def _headroom_sign(mels, amount, band=None):
    """+1 when every value (of one band) can rise by `amount` inside [0, 1], -1 when it can fall by it"""
    hi = max(float((m if band is None else m[:, band]).max()) for m in mels)
    lo = min(float((m if band is None else m[:, band]).min()) for m in mels)
    if hi + amount <= 1.0:
        return 1.0
    assert lo - amount >= 0.0, (lo, hi, amount)
    return -1.0


@pytest.mark.parametrize("family", ["nyanko", "deepvoice3"])
def test_level_shift_is_ignored(dev, family):
    model, hp, seqs, mels = _setup(family, dev)
    ds = hp["downsample_step"]
    shift = 0.05 * _headroom_sign(mels, 0.05)                             # 5 dB in every band
    targets = [(m + shift).repeat_interleave(ds, dim=0) for m in mels]
    table, tot = _evaluate(model, hp, seqs, targets)
    per_frame = [s / n for s, n in zip(_col(table, "mcd_sum"), _col(table, "path_len"))]
    print(family, "shift %+.2f: per-frame distortion %s dB" % (shift, per_frame))
    assert max(per_frame) <= 1e-3 and tot["mcd"] <= 1e-3


@pytest.mark.parametrize("family", ["nyanko", "deepvoice3"])
def test_single_band_offset_by_hand(dev, family):
    """The target is the synthesis with delta added to band m0 in every frame.  Along the diagonal every frame pair
    then differs by 100 delta dB in that one band, so by the definition of the features its distortion is
        mu = 100 |delta| / (sqrt 2 M) * sqrt(sum_{k=1..13} cos^2(pi k (m0 + 1/2) / M)).
    The diagonal is the optimal path when no two different frames of an utterance are closer than 2 mu (an
    off-diagonal cell then costs more than mu, and every path has at least as many cells as the diagonal), so delta is
    chosen for mu = a third of the smallest such distance, found on the host in float64.  The toy models' frames drift
    towards each other as the decode goes on (the nyanko toy's closest pair is 0.035 dB apart after 13 steps, 0.093 dB
    after 4), so this test caps the decode at 4 steps.  The fp32 features of the level-shift test above differ by up to
    2e-6 dB per frame from rounding alone; for that to stay under the 1e-4 of the check, mu must be at least 0.02 dB."""
    model, hp, seqs, mels = _setup(family, dev, max_steps=3)
    ds, M, m0, order = hp["downsample_step"], hp["mel_dim"], 7, 13
    gap = float("inf")
    for m in mels:
        f = DR.mel_cepstra(m.cpu().numpy(), -100.0, order)
        d = DR.distances(f, f)
        d[np.diag_indices_from(d)] = np.inf
        if d.size > 1:
            gap = min(gap, float(d.min()))
    unit = 100.0 / (math.sqrt(2.0) * M) * math.sqrt(sum(math.cos(math.pi * k * (m0 + 0.5) / M) ** 2
                                                        for k in range(1, order + 1)))   # dB of distortion per unit of delta
    mu = min(gap / 3.0, 1.0)
    delta = mu / unit
    print(family, "smallest frame distance %.4g dB -> mu %.4g dB, delta %.4g" % (gap, mu, delta))
    assert mu >= 0.02, "the toy model's frames are too alike for this test to mean anything"
    delta *= _headroom_sign(mels, delta, m0)
    targets = []
    for m in mels:
        t = m.clone()
        t[:, m0] += delta
        targets.append(t.repeat_interleave(ds, dim=0))
    table, tot = _evaluate(model, hp, seqs, targets)
    # what was planted, as fp32 stored it
    planted = (sum(float((t[::ds, m0].double() - m[:, m0].double()).abs().sum()) for t, m in zip(targets, mels))
               / sum(m.size(0) for m in mels))
    want = planted * unit
    print(family, "mcd %.8g want %.8g rel %.2e" % (tot["mcd"], want, abs(tot["mcd"] - want) / want))
    assert _col(table, "path_len") == _col(table, "frames_synth")          # the diagonal
    assert abs(tot["mcd"] - want) <= 1e-4 * want

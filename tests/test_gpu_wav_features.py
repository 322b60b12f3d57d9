# coding: utf-8
"""Ragged forward analysis on the GPU (audio.features_items, dv3_analysis_items_f32) and what is built on it:

  * each item's linear rows are bit for bit the batch path's spectrogram_batch(item[None]);
  * every row is batch-invariant: the same item alone, in a batch of 16 and in reversed order gives the same bits;
  * linear / mel rows against the numpy restatement (oracle/audio_oracle.py) and the mel against the tap-GEMM path;
    rescaling against its host formula;
  * preprocess.build_from_path on a tiny LJSpeech-style corpus, read back by PreprocessedDataset;
  * data.waveform_collate against device_collate(pack_batch(...)) of the preprocessed directory, plain and on a
    lattice, and one Trainer.step on each.
"""
import json
import os

import numpy as np
import pytest
import torch
from scipy.io import wavfile

from oracle import audio_oracle as A

pytestmark = pytest.mark.gpu

HOP = 256
# ragged lengths: hop multiples and not, one shorter than the 1024-point frame, one of about 10 s
LENGTHS = [22050, 700, 256 * 40, 256 * 40 + 1, 5000, 220500, 12345, 1023, 1024, 1025, 33333, 256 * 7 - 3]


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


def _wavs(lengths, seed=0, oracle_regime=False):
    """ragged test signals; oracle_regime: the signal test_audio.py holds the batch path to 5e-5 on (0.3 sin 440 Hz +
    0.05 noise) -- with much less noise the fp32 FFT's absolute error, through the log, grows past that bound in the
    bins near the -100 dB floor, on the batch path as here"""
    rng = np.random.RandomState(seed)
    out = []
    for n in lengths:
        t = np.arange(n) / 22050.0
        if oracle_regime:
            w = 0.3 * np.sin(2 * np.pi * 440 * t) + 0.05 * rng.randn(n)
        else:
            w = rng.uniform(0.05, 0.6) * np.sin(2 * np.pi * rng.uniform(100, 400) * t) + rng.uniform(0.001, 0.05) * rng.randn(n)
        out.append(w.astype(np.float32))
    return out


def _rows(x, frames):
    o = np.concatenate([[0], np.cumsum(frames)])
    return [x[o[i]:o[i + 1]] for i in range(len(frames))]


def _run(wavs, dev, **kw):
    from deepvoice3_pytorch_amd import audio
    lin, mel, frames = audio.features_from_arrays(wavs, None, dev, **kw)
    torch.cuda.synchronize()
    return _rows(lin.cpu().numpy(), frames), _rows(mel.cpu().numpy(), frames), frames


def test_linear_rows_equal_the_batch_path_bit_for_bit(dev):
    from deepvoice3_pytorch_amd import audio
    wavs = _wavs(LENGTHS)
    lin, mel, frames = _run(wavs, dev)
    assert list(frames) == [audio.lws_num_frames(n, HOP) for n in LENGTHS]
    for b, w in enumerate(wavs):
        want = audio.spectrogram_batch(torch.from_numpy(w)[None].to(dev))[0].T.cpu().numpy()
        assert lin[b].shape == want.shape == (frames[b], 513)
        assert mel[b].shape == (frames[b], 80)
        assert np.array_equal(lin[b], want), (b, LENGTHS[b], float(np.abs(lin[b] - want).max()))


def test_rows_are_batch_invariant(dev):
    wavs = _wavs(LENGTHS)
    extra = _wavs([3000, 40000, 257, 9999], seed=1)
    batched = _run(wavs, dev)
    in16 = _run(extra[:2] + wavs + extra[2:], dev)
    rev = _run(wavs[::-1], dev)
    for b in range(len(wavs)):
        alone = _run([wavs[b]], dev)
        for k in (0, 1):            # lin, mel
            ref = batched[k][b]
            assert np.array_equal(alone[k][0], ref), (b, k)
            assert np.array_equal(in16[k][b + 2], ref), (b, k)
            assert np.array_equal(rev[k][len(wavs) - 1 - b], ref), (b, k)


def test_against_oracle_gemm_path_and_rescaling(dev):
    from deepvoice3_pytorch_amd import audio, ops
    wavs = _wavs(LENGTHS, oracle_regime=True)
    lin, mel, frames = _run(wavs, dev)
    prev = ops.set_gemm_precision("f32")
    errs = []
    try:
        for b, w in enumerate(wavs):
            w64 = w.astype(np.float64)[None]
            gm = audio.melspectrogram_batch(torch.from_numpy(w)[None].to(dev))[0].T.cpu().numpy()
            assert gm.shape == mel[b].shape
            want = A.lws_spectrogram(w64)[0].T
            amp = lambda x: 10.0 ** ((x * 100.0 - 100.0 + 20.0) / 20.0)       # undo the normalisation (clipped bins too)
            peak = amp(want).max(axis=1, keepdims=True)
            big = amp(want) >= 1e-3 * peak
            errs.append((np.abs(lin[b] - want)[big].max(), np.abs(mel[b] - A.lws_melspectrogram(w64)[0].T).max(),
                         np.abs(mel[b] - gm).max(), (np.abs(amp(lin[b].astype(np.float64)) - amp(want)) / peak).max(),
                         np.abs(lin[b] - want).max()))
    finally:
        ops.set_gemm_precision(prev)
    # linear rows: 5e-5 (test_audio.py's bound) wherever a bin is at least 1e-3 of its frame's peak; below that the
    # log turns the fp32 FFT's absolute error into a larger normalised one, and the smallest of the Rayleigh-distributed
    # noise bins get smaller the more bins there are (max over all bins, last column: ~3e-6 for items under 0.5 s,
    # ~1e-4 at 10 s -- the batch path's own rows, which these equal bit for bit).  Every bin is held in the amplitude
    # domain instead: error / frame peak.  Mel rows: 5e-5 everywhere, against the oracle and the tap-GEMM path.
    e = np.array(errs)
    msg = [(LENGTHS[b],) + tuple("%.2e" % v for v in r) for b, r in enumerate(errs)]
    assert e[:, :3].max() < 5e-5 and e[:, 3].max() < 1e-5, msg
    # rescaling (ljspeech.py:59-60): gain = rescaling_max / max|x| in fp32, item b analysed as x * gain
    rmax = 0.999
    wavs = _wavs(LENGTHS)
    lin = _run(wavs, dev)[0]
    wavs_r = wavs + [np.zeros(3000, np.float32)]               # a silent item keeps gain 1
    flat, lengths = audio.pack_waveforms(wavs_r, pin=False)
    g = audio.item_gains(flat.to(dev), lengths, rmax).cpu().numpy()
    want_g = np.array([np.float32(rmax) / np.abs(w).max() if np.abs(w).max() > 0 else np.float32(1) for w in wavs_r],
                      dtype=np.float32)
    assert np.array_equal(g, want_g)
    got = _run(wavs_r, dev, rescaling=rmax)
    host = _run([w * gw for w, gw in zip(wavs_r, want_g)], dev)
    for b in range(len(wavs_r)):
        assert np.array_equal(got[0][b], host[0][b]) and np.array_equal(got[1][b], host[1][b]), b
    assert not np.array_equal(got[0][0], lin[0])               # the gain is applied


def _corpus(root, n=10, seed=3):
    rng = np.random.RandomState(seed)
    os.makedirs(os.path.join(root, "wavs"))
    lines, kept = [], []
    for i in range(n):
        uid = "LJ001-%04d" % (i + 1)
        L = int(rng.randint(2500, 9000))
        t = np.arange(L) / 22050.0
        x = 0.3 * np.sin(2 * np.pi * rng.uniform(120, 300) * t) + 0.02 * rng.randn(L)
        wavfile.write(os.path.join(root, "wavs", uid + ".wav"), 22050, (x * 32767).astype(np.int16))
        text = "too short" if i == 3 else "utterance number %d, long enough to keep" % i
        lines.append("%s|raw|%s" % (uid, text))
        if i != 3:
            kept.append((uid, L, text))
    with open(os.path.join(root, "metadata.csv"), "w", encoding="utf-8") as f:
        f.write("\n".join(lines) + "\n")
    return kept


def _t2s(text):
    return [2 + ord(c) % 38 for c in text]


@pytest.fixture(scope="module")
def corpus(tmp_path_factory, dev):
    from deepvoice3_pytorch_amd import preprocess
    base = tmp_path_factory.mktemp("ljs")
    in_dir, out_dir = str(base / "LJSpeech"), str(base / "out")
    kept = _corpus(in_dir)
    # a small sample budget so the corpus is analysed in several launches
    md = preprocess.build_from_path(in_dir, out_dir, device=dev, max_batch_samples=20000)
    return in_dir, out_dir, kept, md


def test_build_from_path(dev, corpus):
    from deepvoice3_pytorch_amd import audio, data
    in_dir, out_dir, kept, md = corpus
    assert len(md) == len(kept) == 9
    for k, ((uid, L, text), m) in enumerate(zip(kept, md)):
        assert m == ("ljspeech-spec-%05d.npy" % (k + 1), "ljspeech-mel-%05d.npy" % (k + 1),
                     audio.lws_num_frames(L, HOP), text)
        spec, mel = np.load(os.path.join(out_dir, m[0])), np.load(os.path.join(out_dir, m[1]))
        assert spec.shape == (m[2], 513) and mel.shape == (m[2], 80)
        assert spec.dtype == mel.dtype == np.float32
    with open(os.path.join(out_dir, "train.txt"), encoding="utf-8") as f:
        lines = f.read().splitlines()
    assert lines[0] == "ljspeech-spec-00001.npy|ljspeech-mel-00001.npy|%d|%s" % (md[0][2], kept[0][2])
    ds = data.PreprocessedDataset(out_dir, _t2s)
    assert len(ds) == 9 and ds.frame_lengths == [m[2] for m in md]
    text, mel, spec = ds[4]
    assert np.array_equal(text, _t2s(kept[4][2])) and mel.shape == (md[4][2], 80) and spec.shape == (md[4][2], 513)
    cfg = data.read_audio_config(out_dir)
    assert cfg["window_scale"] == audio.AudioConfig().window_scale and cfg["convention"] == "lws"
    assert (cfg["hop_size"], cfg["fft_size"], cfg["sample_rate"], cfg["num_mels"]) == (256, 1024, 22050, 80)
    assert cfg["rescaling"] is False
    with open(os.path.join(out_dir, "audio_config.json")) as f:
        assert json.load(f) == cfg
    # the stored features are what the int16 file decodes to, analysed alone
    w = np.load(os.path.join(out_dir, md[2][0]))
    from deepvoice3_pytorch_amd import preprocess
    x = preprocess.load_wav(os.path.join(in_dir, "wavs", kept[2][0] + ".wav"))
    want = audio.spectrogram_batch(torch.from_numpy(x)[None].to(dev))[0].T.cpu().numpy()
    assert np.array_equal(w, want)


def _tiny_model(dev):
    from deepvoice3_pytorch_amd import builder
    hp = dict(n_vocab=40, embed_dim=32, mel_dim=80, linear_dim=513, r=1, downsample_step=4, padding_idx=0,
              dropout=0.05, kernel_size=3, encoder_channels=64, decoder_channels=32, converter_channels=32,
              use_memory_mask=True, force_monotonic_attention=True, use_decoder_state_for_postnet_input=True,
              key_projection=True, value_projection=True, max_positions=128)
    torch.manual_seed(0)
    return builder.deepvoice3(**hp).to(dev)


def test_waveform_collate_equals_preprocessed_batch(dev, corpus):
    from deepvoice3_pytorch_amd import data, ops, train_step
    in_dir, out_dir, kept, md = corpus
    pre = data.PreprocessedDataset(out_dir, _t2s)
    wds = data.WaveformDataset.from_ljspeech(in_dir, _t2s)
    assert wds.frame_lengths == pre.frame_lengths
    idx = [5, 0, 7, 2, 8]
    names = ("text", "text_positions", "frame_positions", "mel", "y", "done", "input_lengths", "target_lengths",
             "decoder_lengths")
    batches = {}
    for lattice in (None, (16, 8)):
        got = data.waveform_collate([wds[i] for i in idx], dev, 1, 4, lattice=lattice)
        want = data.device_collate(data.pack_batch([pre[i] for i in idx]), dev, 1, 4, lattice=lattice)
        for n in names:
            g, w = getattr(got, n), getattr(want, n)
            assert g.shape == w.shape and g.dtype == w.dtype and torch.equal(g, w), (lattice, n)
        assert np.array_equal(got.target_lengths_host, want.target_lengths_host)
        if lattice is None:
            assert got.valid is None and want.valid is None
        else:
            assert torch.equal(got.valid.buf, want.valid.buf)
        batches[lattice] = (got, want)
    # one training step on each batch of the plain pair: the same losses, bit for bit
    res = []
    for b in batches[None]:
        model = _tiny_model(dev)
        tr = train_step.Trainer(model, train_step.TrainConfig(max_positions=128))
        ops.dropout_state.manual_seed(17)
        out = tr.step(b)
        res.append({k: float(v) for k, v in out.items() if torch.is_tensor(v) and v.numel() == 1})
    assert res[0].keys() == res[1].keys() and "loss" in res[0]
    assert res[0] == res[1] and np.isfinite(res[0]["loss"])

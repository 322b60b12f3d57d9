# coding: utf-8
"""Host side of GPU preprocessing (deepvoice3_pytorch_amd/preprocess.py, data.WaveformDataset): wav decoding as
librosa.load converts samples, LJSpeech metadata.csv parsing with the reference's min_text filter and numbering
(ljspeech.py:27-36), the train.txt line format (preprocess.py:24-28), sample-budget batching and the frame counts
read from wav headers.  No GPU needed."""
import json
import os

import numpy as np
import pytest
from scipy.io import wavfile

from deepvoice3_pytorch_amd import audio, data, preprocess


def _write(path, rate, x):
    wavfile.write(str(path), rate, x)
    return str(path)


def test_load_wav_conversions(tmp_path):
    i16 = np.array([-32768, -1, 0, 1, 16384, 32767], dtype=np.int16)
    got = preprocess.load_wav(_write(tmp_path / "a.wav", 22050, i16))
    assert got.dtype == np.float32 and np.array_equal(got, i16.astype(np.float32) / 32768)
    assert got[0] == -1.0 and got[-1] == np.float32(32767 / 32768)

    i32 = np.array([-2 ** 31, -1, 0, 2 ** 30, 2 ** 31 - 1], dtype=np.int32)
    got = preprocess.load_wav(_write(tmp_path / "b.wav", 22050, i32))
    assert got.dtype == np.float32 and np.array_equal(got, i32.astype(np.float32) / np.float32(2 ** 31))
    assert got[0] == -1.0 and got[3] == 0.5

    u8 = np.array([0, 64, 128, 192, 255], dtype=np.uint8)
    got = preprocess.load_wav(_write(tmp_path / "c.wav", 22050, u8))
    assert got.dtype == np.float32 and np.array_equal(got, np.array([-1, -0.5, 0, 0.5, 127 / 128], np.float32))

    f32 = np.array([-0.75, 0.0, 0.123456789, 1.5], dtype=np.float32)
    got = preprocess.load_wav(_write(tmp_path / "d.wav", 22050, f32))
    assert got.dtype == np.float32 and np.array_equal(got, f32)          # passed through, not clipped


def test_load_wav_stereo_is_averaged(tmp_path):
    st = np.array([[1000, -1000], [32767, 32767], [-32768, 0], [3, 4]], dtype=np.int16)
    got = preprocess.load_wav(_write(tmp_path / "s.wav", 22050, st))
    want = (st.astype(np.float32) / 32768).mean(axis=1)
    assert got.shape == (4,) and got.dtype == np.float32 and np.allclose(got, want, rtol=0, atol=1e-7)
    assert got[0] == 0.0 and got[1] == np.float32(32767 / 32768)
    assert preprocess.wav_num_samples(tmp_path / "s.wav") == 4


def test_load_wav_rate_mismatch_raises(tmp_path):
    p = _write(tmp_path / "r.wav", 16000, np.zeros(100, np.int16))
    with pytest.raises(ValueError, match="16000"):
        preprocess.load_wav(p, 22050)
    assert preprocess.load_wav(p, 16000).shape == (100,)


def _corpus(tmp_path, texts, lengths, rate=22050):
    root = tmp_path / "LJ"
    (root / "wavs").mkdir(parents=True)
    lines = []
    for i, (t, n) in enumerate(zip(texts, lengths)):
        uid = "LJ001-%04d" % (i + 1)
        _write(root / "wavs" / (uid + ".wav"), rate, (np.arange(n) % 200 - 100).astype(np.int16))
        lines.append("%s|raw %d|%s" % (uid, i, t))
    (root / "metadata.csv").write_text("\n".join(lines) + "\n", encoding="utf-8")
    return str(root)


def test_metadata_min_text_filter_and_numbering(tmp_path):
    texts = ["a text that is long enough.", "short", "another text, long enough too", "x" * 20, "y" * 19]
    root = _corpus(tmp_path, texts, [300, 400, 500, 600, 700])
    rows = preprocess.read_metadata(root, min_text=20)
    # kept: 0, 2, 3 (len 20 is not shorter than 20); the index advances on kept lines only (ljspeech.py:30-36)
    assert [r[0] for r in rows] == [1, 2, 3]
    assert [r[2] for r in rows] == [texts[0], texts[2], texts[3]]
    assert [os.path.basename(r[1]) for r in rows] == ["LJ001-0001.wav", "LJ001-0003.wav", "LJ001-0004.wav"]
    assert [r[0] for r in preprocess.read_metadata(root, min_text=0)] == [1, 2, 3, 4, 5]

    ds = data.WaveformDataset.from_ljspeech(root, lambda t: [ord(c) % 40 for c in t], min_text=20)
    assert ds.num_samples == [300, 500, 600]
    assert ds.frame_lengths == [audio.lws_num_frames(n, 256) for n in (300, 500, 600)] == [5, 5, 6]
    text, wav = ds[1]
    assert text.dtype == np.int32 and len(text) == len(texts[2]) and wav.shape == (500,) and wav.dtype == np.float32


def test_train_txt_line_format(tmp_path):
    md = [("ljspeech-spec-00001.npy", "ljspeech-mel-00001.npy", 123, "Hello, world."),
          ("ljspeech-spec-00002.npy", "ljspeech-mel-00002.npy", 7, "Second line")]
    preprocess.write_metadata(md, str(tmp_path))
    assert (tmp_path / "train.txt").read_text(encoding="utf-8") == (
        "ljspeech-spec-00001.npy|ljspeech-mel-00001.npy|123|Hello, world.\n"
        "ljspeech-spec-00002.npy|ljspeech-mel-00002.npy|7|Second line\n")
    assert data.read_audio_config(str(tmp_path)) is None
    cfg = audio.AudioConfig()
    d = preprocess.audio_config_dict(cfg, 80, 125, 7600, False, 0.999)
    (tmp_path / "audio_config.json").write_text(json.dumps(d))
    got = data.read_audio_config(str(tmp_path))
    assert got["window_scale"] == cfg.window_scale and got["convention"] == "lws" and got["hop_size"] == 256


def test_batches_by_samples():
    assert preprocess.batches_by_samples([5, 5, 5, 5], 10) == [(0, 2), (2, 4)]
    assert preprocess.batches_by_samples([20, 3, 3, 30, 1], 10) == [(0, 1), (1, 3), (3, 4), (4, 5)]
    assert preprocess.batches_by_samples([], 10) == []


def test_preset_audio_keys(tmp_path):
    p = tmp_path / "preset.json"
    p.write_text(json.dumps({"name": "deepvoice3", "hop_size": 200, "num_mels": 64, "rescaling": True, "builder": "x"}))
    hp = preprocess.preset_audio(str(p))
    assert hp["hop_size"] == 200 and hp["num_mels"] == 64 and hp["rescaling"] is True
    assert hp["sample_rate"] == 22050 and hp["min_text"] == 20 and "builder" not in hp


def test_features_items_refuses_torch_framing():
    import torch
    with pytest.raises(ValueError, match="lws"):
        audio.features_items(torch.zeros(10), [10], audio.AudioConfig(convention="torch"))

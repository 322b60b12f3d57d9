# coding: utf-8
"""LJSpeech preprocessing on the GPU: the reference's `preprocess.py ljspeech` (preprocess.py:18-31, ljspeech.py:9-76)
without its native dependencies (`lws`, `librosa`).  Utterances are read with scipy, batched under a sample budget and
analysed by audio.features_items in one launch per batch; the output directory is what the reference writes
(`train.txt` + `ljspeech-{spec,mel}-%05d.npy`), which data.PreprocessedDataset reads, plus `audio_config.json` recording
the constants the features were made with (data.read_audio_config).

    python -m deepvoice3_pytorch_amd.preprocess ljspeech IN_DIR OUT_DIR [--preset PRESET.json]
"""
import argparse
import json
import os

import numpy as np

from . import audio

AUDIO_CONFIG = "audio_config.json"

# the audio keys of hparams.py:35-52,137 this preprocessor reads (their reference defaults)
DEFAULTS = dict(num_mels=80, fmin=125, fmax=7600, fft_size=1024, hop_size=256, sample_rate=22050, preemphasis=0.97,
                min_level_db=-100, ref_level_db=20, rescaling=False, rescaling_max=0.999, min_text=20)


def load_wav(path, sample_rate=22050):
    """-> float32 mono samples in [-1, 1), converted as librosa.load does: PCM16 / 32768, PCM32 / 2^31,
    uint8 (x - 128) / 128, float passed through; channels averaged.  A file at another rate raises ValueError
    (no resampling)."""
    from scipy.io import wavfile
    sr, x = wavfile.read(path)
    if sr != sample_rate:
        raise ValueError("%s: sample rate %d, expected %d (resampling is not supported)" % (path, sr, sample_rate))
    if x.dtype == np.int16:
        y = x.astype(np.float32) / np.float32(32768.0)
    elif x.dtype == np.int32:
        y = x.astype(np.float32) / np.float32(2.0 ** 31)
    elif x.dtype == np.uint8:
        y = (x.astype(np.float32) - np.float32(128.0)) / np.float32(128.0)
    elif x.dtype in (np.float32, np.float64):
        y = x.astype(np.float32)
    else:
        raise ValueError("%s: unsupported sample type %s" % (path, x.dtype))
    if y.ndim == 2:
        y = y.mean(axis=1, dtype=np.float32)
    return np.ascontiguousarray(y)


def wav_num_samples(path):
    """samples per channel of a wav file, from its header (the data is memory-mapped, not decoded)"""
    from scipy.io import wavfile
    try:
        _, x = wavfile.read(path, mmap=True)
    except ValueError:          # a sample format scipy can not map (24-bit PCM): decode it
        _, x = wavfile.read(path)
    return int(x.shape[0])


def read_metadata(in_dir, min_text=20):
    """LJSpeech metadata.csv -> [(index, wav path, text)]: the third '|' column is the text; texts shorter than
    min_text are skipped and the index advances only on kept lines (ljspeech.py:27-36)."""
    out = []
    index = 1
    with open(os.path.join(in_dir, "metadata.csv"), encoding="utf-8") as f:
        for line in f:
            parts = line.strip().split("|")
            if len(parts) < 3:
                continue
            text = parts[2]
            if len(text) < min_text:
                continue
            out.append((index, os.path.join(in_dir, "wavs", "%s.wav" % parts[0]), text))
            index += 1
    return out


def batches_by_samples(lengths, max_samples):
    """consecutive index ranges whose sample total stays within max_samples (an item longer than that is alone)"""
    out, start, acc = [], 0, 0
    for i, n in enumerate(lengths):
        if i > start and acc + n > max_samples:
            out.append((start, i))
            start, acc = i, 0
        acc += int(n)
    if start < len(lengths):
        out.append((start, len(lengths)))
    return out


def audio_config_dict(cfg, num_mels, fmin, fmax, rescaling, rescaling_max):
    return dict(convention=cfg.convention, window_scale=cfg.window_scale, hop_size=cfg.hop_size, fft_size=cfg.fft_size,
                sample_rate=cfg.sample_rate, preemphasis=cfg.preemphasis, min_level_db=cfg.min_level_db,
                ref_level_db=cfg.ref_level_db, num_mels=num_mels, fmin=fmin, fmax=fmax, rescaling=bool(rescaling),
                rescaling_max=rescaling_max)


def write_metadata(metadata, out_dir):
    """train.txt: one `spec|mel|n_frames|text` line per utterance (preprocess.py:24-28)"""
    with open(os.path.join(out_dir, "train.txt"), "w", encoding="utf-8") as f:
        for m in metadata:
            f.write("|".join([str(x) for x in m]) + "\n")


def build_from_path(in_dir, out_dir, cfg=None, num_mels=80, fmin=125, fmax=7600, rescaling=False, rescaling_max=0.999,
                    min_text=20, device="cuda:0", max_batch_samples=1 << 23, tqdm=None):
    """Preprocess an LJSpeech directory into out_dir -> [(spec file, mel file, n_frames, text)], also written as
    train.txt with audio_config.json beside it.  Features of up to max_batch_samples samples are made per launch."""
    import torch
    cfg = cfg or audio.AudioConfig()
    os.makedirs(out_dir, exist_ok=True)
    rows = read_metadata(in_dir, min_text)
    spans = batches_by_samples([wav_num_samples(p) for _, p, _ in rows], max_batch_samples)
    metadata = []
    for s, e in (tqdm(spans) if tqdm is not None else spans):
        wavs = [load_wav(p, cfg.sample_rate) for _, p, _ in rows[s:e]]
        lin, mel, frames = audio.features_from_arrays(wavs, cfg, device, num_mels=num_mels, fmin=fmin, fmax=fmax,
                                                      rescaling=rescaling_max if rescaling else None)
        lin, mel = lin.cpu().numpy(), mel.cpu().numpy()
        o = 0
        for j, n in enumerate(frames):
            index, _, text = rows[s + j]
            spec_name, mel_name = "ljspeech-spec-%05d.npy" % index, "ljspeech-mel-%05d.npy" % index
            np.save(os.path.join(out_dir, spec_name), lin[o:o + n], allow_pickle=False)
            np.save(os.path.join(out_dir, mel_name), mel[o:o + n], allow_pickle=False)
            metadata.append((spec_name, mel_name, int(n), text))
            o += int(n)
    if torch.cuda.is_available():
        torch.cuda.synchronize()
    write_metadata(metadata, out_dir)
    with open(os.path.join(out_dir, AUDIO_CONFIG), "w") as f:
        json.dump(audio_config_dict(cfg, num_mels, fmin, fmax, rescaling, rescaling_max), f, indent=1, sort_keys=True)
    return metadata


def preset_audio(path=None):
    """the audio keys of a reference preset JSON (hparams.parse_json), the reference defaults for the others"""
    hp = dict(DEFAULTS)
    if path is not None:
        with open(path) as f:
            js = json.load(f)
        hp.update({k: js[k] for k in DEFAULTS if k in js})
    return hp


def main(argv=None):
    ap = argparse.ArgumentParser(description="Preprocess a dataset into train.txt + spectrogram .npy files (GPU)")
    ap.add_argument("name", choices=["ljspeech"])
    ap.add_argument("in_dir")
    ap.add_argument("out_dir")
    ap.add_argument("--preset", default=None, help="reference preset JSON; its audio keys are read")
    ap.add_argument("--device", default="cuda:0")
    args = ap.parse_args(argv)
    hp = preset_audio(args.preset)
    cfg = audio.AudioConfig(fft_size=hp["fft_size"], hop_size=hp["hop_size"], sample_rate=hp["sample_rate"],
                            preemphasis=hp["preemphasis"], min_level_db=hp["min_level_db"], ref_level_db=hp["ref_level_db"])
    md = build_from_path(args.in_dir, args.out_dir, cfg, hp["num_mels"], hp["fmin"], hp["fmax"], hp["rescaling"],
                         hp["rescaling_max"], hp["min_text"], args.device)
    frames = sum(m[2] for m in md)
    hours = frames * cfg.hop_size / cfg.sample_rate / 3600.0
    print("Wrote %d utterances, %d frames (%.2f hours)" % (len(md), frames, hours))
    if md:
        print("Max input length:  %d" % max(len(m[3]) for m in md))
        print("Max output length: %d" % max(m[2] for m in md))


if __name__ == "__main__":
    main()

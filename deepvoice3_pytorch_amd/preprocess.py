# coding: utf-8
"""LJSpeech and VCTK preprocessing on the GPU: the reference's `preprocess.py ljspeech` / `preprocess.py vctk`
(preprocess.py:18-31, ljspeech.py:9-76, vctk.py:13-88) without their native dependencies (`lws`, `librosa`, `resampy`,
`nnmnkwii`).  Utterances are read with scipy, batched under a sample budget and analysed by audio.features_items in one
launch per batch; the output directory is what the reference writes (`train.txt` + `NAME-{spec,mel}-%05d.npy`), which
data.PreprocessedDataset reads, plus `audio_config.json` recording the constants the features were made with
(data.read_audio_config).  VCTK's 48 kHz recordings are resampled, cut to their HTS labels where a label file exists and
trimmed of silence on the GPU first (audio.prepare_items), and every `train.txt` row carries a speaker id
(`speakers.json` maps the speaker names to them).

    python -m deepvoice3_pytorch_amd.preprocess ljspeech IN_DIR OUT_DIR [--preset PRESET.json]
    python -m deepvoice3_pytorch_amd.preprocess vctk IN_DIR OUT_DIR [--preset PRESET.json]
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
    (no resampling).  sample_rate=None: any rate is taken, -> (samples, the file's rate) (audio.resample_items
    brings a batch of them to the target rate)."""
    from scipy.io import wavfile
    sr, x = wavfile.read(path)
    if sample_rate is not None and sr != sample_rate:
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
    y = np.ascontiguousarray(y)
    return (y, int(sr)) if sample_rate is None else y


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
    """train.txt: one `spec|mel|n_frames|text[|speaker_id]` line per utterance (preprocess.py:24-28)"""
    with open(os.path.join(out_dir, "train.txt"), "w", encoding="utf-8") as f:
        for m in metadata:
            f.write("|".join([str(x) for x in m]) + "\n")


def read_vctk(in_dir):
    """A VCTK-Corpus directory -> (speakers, rows).  speakers: the sorted directory names under wav48/ that also have a
    directory under txt/ (the published corpus: 108 -- p315 has recordings and no transcripts); speaker ids are their
    positions 0 .. n-1, the labels nnmnkwii's TranscriptionDataSource hands the reference (vctk.py:17-22).  rows:
    [(wav path, text, speaker id)] for every utterance that has both wav48/pX/pX_N.wav and txt/pX/pX_N.txt, sorted by
    speaker, then by file name; the text is the transcript file's content, stripped."""
    wav_root, txt_root = os.path.join(in_dir, "wav48"), os.path.join(in_dir, "txt")
    speakers = sorted(d for d in os.listdir(wav_root)
                      if os.path.isdir(os.path.join(wav_root, d)) and os.path.isdir(os.path.join(txt_root, d)))
    rows = []
    for sid, name in enumerate(speakers):
        for fn in sorted(os.listdir(os.path.join(wav_root, name))):
            stem, ext = os.path.splitext(fn)
            txt = os.path.join(txt_root, name, stem + ".txt")
            if ext != ".wav" or not os.path.isfile(txt):
                continue
            with open(txt, encoding="utf-8") as f:
                rows.append((os.path.join(wav_root, name, fn), f.read().strip(), sid))
    return speakers, rows


def read_hts_labels(path):
    """An HTS label file (`begin end label` per line, times in 100 ns) -> (begin, end) of the speech in the same units,
    by the reference's rule (vctk.py:33-50, start_at / end_at) on each line's last whitespace-separated field: the
    begin of the first label unless it is `pau`, else of the first later label that is not; the end of the last label
    unless it is `pau`, else of the last label before it (the first excluded) that is not."""
    labels = []
    with open(path, encoding="utf-8") as f:
        for line in f:
            parts = line.split()
            if len(parts) >= 3:
                labels.append((int(parts[0]), int(parts[1]), parts[-1]))
    if not labels:
        raise ValueError("%s: no labels" % path)
    begin = end = None
    if labels[0][2] != "pau":
        begin = labels[0][0]
    else:
        for lab in labels[1:]:
            if lab[2] != "pau":
                begin = lab[0]
                break
    if labels[-1][2] != "pau":
        end = labels[-1][1]
    else:
        for i in range(len(labels) - 2, 0, -1):
            if labels[i][2] != "pau":
                end = labels[i][1]
                break
    if begin is None or end is None:
        raise ValueError("%s: nothing but pau labels" % path)
    return begin, end


def vctk_label_path(wav_path):
    """the label file of a VCTK recording: wav48/ -> lab/, .wav -> .lab (vctk.py:58)"""
    return wav_path.replace("wav48/", "lab/").replace(".wav", ".lab")


TRIM_TOP_DB = dict(labels=25.0, plain=15.0)          # vctk.py:66,68


def _build_vctk(in_dir, out_dir, cfg, num_mels, fmin, fmax, rescaling, rescaling_max, device, max_batch_samples, tqdm):
    """vctk.py:13-88 -> [(spec file, mel file, n_frames, text, speaker id)]; the sample budget counts source samples"""
    speakers, rows = read_vctk(in_dir)
    batches = batches_by_samples([wav_num_samples(p) for p, _, _ in rows], max_batch_samples)
    metadata, skipped, rates = [], 0, set()
    for s, e in (tqdm(batches) if tqdm is not None else batches):
        by_rate = {}                                  # one ratio per launch: group the batch by the files' rate
        for j in range(s, e):
            w, sr = load_wav(rows[j][0], None)
            by_rate.setdefault(sr, []).append((j, w))
        for sr, items in sorted(by_rate.items()):
            rates.add(sr)
            spans, top_db = [], []
            for j, _ in items:
                lab = vctk_label_path(rows[j][0])
                if os.path.exists(lab):
                    b, e_ = read_hts_labels(lab)
                    spans.append((int(b * 1e-7 * cfg.sample_rate), int(e_ * 1e-7 * cfg.sample_rate)))
                    top_db.append(TRIM_TOP_DB["labels"])
                else:
                    spans.append(None)
                    top_db.append(TRIM_TOP_DB["plain"])
            flat, lengths = audio.prepare_items([w for _, w in items], sr, cfg, spans, top_db, device)
            keep = [k for k, n in enumerate(lengths) if n > 0]
            skipped += len(items) - len(keep)
            if not keep:
                continue
            lin, mel, frames = audio.features_items(flat, lengths[keep], cfg, num_mels=num_mels, fmin=fmin, fmax=fmax,
                                                    rescaling=rescaling_max if rescaling else None)
            lin, mel = lin.cpu().numpy(), mel.cpu().numpy()
            o = 0
            for k, n in zip(keep, frames):
                j = items[k][0]
                spec_name, mel_name = "vctk-spec-%05d.npy" % (j + 1), "vctk-mel-%05d.npy" % (j + 1)
                np.save(os.path.join(out_dir, spec_name), lin[o:o + n], allow_pickle=False)
                np.save(os.path.join(out_dir, mel_name), mel[o:o + n], allow_pickle=False)
                metadata.append((j, (spec_name, mel_name, int(n), rows[j][1], rows[j][2])))
                o += int(n)
    metadata = [m for _, m in sorted(metadata)]
    if skipped:
        print("Skipped %d utterances trimmed to nothing" % skipped)
    with open(os.path.join(out_dir, SPEAKERS), "w") as f:
        json.dump({name: i for i, name in enumerate(speakers)}, f, indent=1, sort_keys=True)
    extra = dict(resample=dict(source_rates=sorted(rates), filter="kaiser_best (closed form)",
                               zeros=audio.RESAMPLE_ZEROS, rolloff=audio.RESAMPLE_ROLLOFF, beta=audio.RESAMPLE_BETA),
                 trim_top_db=dict(TRIM_TOP_DB), trim_frame_length=audio.TRIM_FRAME, trim_hop_length=audio.TRIM_HOP)
    return metadata, extra


SPEAKERS = "speakers.json"
DATASETS = ("ljspeech", "vctk")


def build_from_path(in_dir, out_dir, cfg=None, num_mels=80, fmin=125, fmax=7600, rescaling=False, rescaling_max=0.999,
                    min_text=20, device="cuda:0", max_batch_samples=1 << 23, tqdm=None, name="ljspeech"):
    """Preprocess a dataset directory into out_dir, also written as train.txt with audio_config.json beside it.
    name = "ljspeech" -> [(spec file, mel file, n_frames, text)]; name = "vctk" -> [(spec file, mel file, n_frames,
    text, speaker id)] of the resampled, label-cut and silence-trimmed recordings, plus speakers.json.  Features of up
    to max_batch_samples samples (VCTK: source samples) are made per launch."""
    import torch
    if name not in DATASETS:
        raise ValueError("unknown dataset %r (one of %s)" % (name, ", ".join(DATASETS)))
    if name == "vctk":
        cfg = cfg or audio.AudioConfig()
        os.makedirs(out_dir, exist_ok=True)
        metadata, extra = _build_vctk(in_dir, out_dir, cfg, num_mels, fmin, fmax, rescaling, rescaling_max, device,
                                      max_batch_samples, tqdm)
        if torch.cuda.is_available():
            torch.cuda.synchronize()
        write_metadata(metadata, out_dir)
        js = audio_config_dict(cfg, num_mels, fmin, fmax, rescaling, rescaling_max)
        js.update(extra)
        with open(os.path.join(out_dir, AUDIO_CONFIG), "w") as f:
            json.dump(js, f, indent=1, sort_keys=True)
        return metadata
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
    ap.add_argument("name", choices=list(DATASETS))
    ap.add_argument("in_dir")
    ap.add_argument("out_dir")
    ap.add_argument("--preset", default=None, help="reference preset JSON; its audio keys are read")
    ap.add_argument("--device", default="cuda:0")
    args = ap.parse_args(argv)
    hp = preset_audio(args.preset)
    cfg = audio.AudioConfig(fft_size=hp["fft_size"], hop_size=hp["hop_size"], sample_rate=hp["sample_rate"],
                            preemphasis=hp["preemphasis"], min_level_db=hp["min_level_db"], ref_level_db=hp["ref_level_db"])
    md = build_from_path(args.in_dir, args.out_dir, cfg, hp["num_mels"], hp["fmin"], hp["fmax"], hp["rescaling"],
                         hp["rescaling_max"], hp["min_text"], args.device, name=args.name)
    frames = sum(m[2] for m in md)
    hours = frames * cfg.hop_size / cfg.sample_rate / 3600.0
    print("Wrote %d utterances, %d frames (%.2f hours)" % (len(md), frames, hours))
    if md:
        print("Max input length:  %d" % max(len(m[3]) for m in md))
        print("Max output length: %d" % max(m[2] for m in md))


if __name__ == "__main__":
    main()

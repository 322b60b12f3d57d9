# coding: utf-8
"""Throughput of the ragged forward analysis (audio.features_items -> dv3_analysis_items_f32), and what on-the-fly
features cost a training batch.

  launch        features_items on device-resident LJSpeech-shaped utterances (lengths uniform in 1..10 s at 22.05 kHz,
                seeded) at 16, 64 and 256 utterances per launch: median over repeats of the device time of one call
                (gain kernel off), frames/s = output rows / that time.  `rescaling` repeats B = 64 with the max|x| pass.
  per_batch_b64 the whole on-the-fly path of one B = 64 batch from host arrays: packing into a pinned buffer, the
                host-to-device copy, features_items -- wall time with a synchronisation at the end (median), with its
                parts by CUDA events; `waveform_collate` adds the text, the padding and the rest of device_collate.
                Compared with the 13.4 ms B = 64 training step of the deepvoice3_ljspeech preset (bench.py, f16x3).
Usage: python scripts/wav_features_throughput.py [out.json]"""
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

STEP_MS_B64 = 13.4


def lj_lengths(rng, n, sr=22050):
    return (rng.uniform(1.0, 10.0, n) * sr).astype(np.int64)


def synth(rng, lengths):
    out = []
    for n in lengths:
        t = np.arange(n) / 22050.0
        out.append((0.3 * np.sin(2 * np.pi * rng.uniform(100, 300) * t) + 0.02 * rng.randn(n)).astype(np.float32))
    return out


def event_ms(fn, reps=20, warmup=3):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b))
    return float(np.median(ts)), float(np.min(ts))


def main():
    from deepvoice3_pytorch_amd import audio, data
    out_path = sys.argv[1] if len(sys.argv) > 1 else None
    dev = torch.device("cuda:0")
    rng = np.random.RandomState(0)
    res = {"measured_on": "MI355X (gfx950), one GPU", "lengths": "uniform 1..10 s at 22050 Hz (seeded)",
           "hop": 256, "num_mels": 80, "timing": "CUDA events, median (min) of 20 calls after 3 warm-up calls",
           "launch": {}}
    for B in (16, 64, 256):
        lengths = lj_lengths(rng, B)
        flat, _ = audio.pack_waveforms(synth(rng, lengths), pin=False)
        x = flat.to(dev)
        frames = int(sum(audio.lws_num_frames(int(n), 256) for n in lengths))
        med, mn = event_ms(lambda: audio.features_items(x, lengths))
        res["launch"]["B%d" % B] = dict(utterances=B, audio_s=float(lengths.sum() / 22050.0), frames=frames,
                                        ms=med, ms_min=mn, frames_per_s=frames / (med * 1e-3),
                                        audio_s_per_s=float(lengths.sum() / 22050.0) / (med * 1e-3))
        if B == 64:
            med_r, _ = event_ms(lambda: audio.features_items(x, lengths, rescaling=0.999))
            res["launch"]["B64_rescaling"] = dict(ms=med_r, frames_per_s=frames / (med_r * 1e-3))
    # one B = 64 batch from host arrays
    lengths = lj_lengths(rng, 64)
    wavs = synth(rng, lengths)
    texts = [rng.randint(2, 40, int(n)).astype(np.int32) for n in rng.randint(20, 150, 64)]
    items = list(zip(texts, wavs))
    frames = int(sum(audio.lws_num_frames(int(n), 256) for n in lengths))

    def wall(fn, reps=10, warmup=2):
        for _ in range(warmup):
            fn()
        torch.cuda.synchronize()
        ts = []
        for _ in range(reps):
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            ts.append((time.perf_counter() - t0) * 1e3)
        return float(np.median(ts))

    pack_ms = wall(lambda: audio.pack_waveforms(wavs))
    flat, _ = audio.pack_waveforms(wavs)
    h2d_ms, _ = event_ms(lambda: flat.to(dev, non_blocking=True))
    x = flat.to(dev)
    kern_ms, _ = event_ms(lambda: audio.features_items(x, lengths))
    feats_ms = wall(lambda: audio.features_from_arrays(wavs, None, dev))
    coll_ms = wall(lambda: data.waveform_collate(items, dev, 1, 4))
    res["per_batch_b64"] = dict(utterances=64, frames=frames, samples=int(lengths.sum()),
                                bytes_h2d=int(lengths.sum()) * 4, pack_host_ms=pack_ms, h2d_ms=h2d_ms,
                                features_items_ms=kern_ms, features_from_arrays_wall_ms=feats_ms,
                                waveform_collate_wall_ms=coll_ms, train_step_ms=STEP_MS_B64,
                                waveform_collate_over_step=coll_ms / STEP_MS_B64)
    line = json.dumps(res, indent=1)
    print(line)
    if out_path:
        os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
        with open(out_path, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()

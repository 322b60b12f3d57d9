# coding: utf-8
"""What pitch tracking costs beside the analysis it rides with.  One process:

  audio.yin_items and audio.features_items on the SAME packed batch -- 64 utterances of 804 frames each (801 hops of
  samples), a 12-harmonic tone with vibrato over a noise floor -- at 1024 / 256 (22.05 kHz, lags 44 .. 367) and at
  2048 / 512 (48 kHz, lags 96 .. 800): a queue of `--calls` calls between two device events, the four cases alternating
  inside every repeat, after a warm-up; median, minimum and maximum per call, and for YIN the difference terms
  (frames x tau_max x (n_fft - tau_max) subtract-square-adds) per second that is.

    python scripts/pitch_cost.py [--out profiles/pitch_cost.json] [--calls 10] [--repeats 7]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

SIZES = ((1024, 256, 22050), (2048, 512, 48000))
B, FRAMES = 64, 804


def summary(t):
    t = np.array(t)
    return dict(median=float(np.median(t)), min=float(t.min()), max=float(t.max()), n=int(t.size))


def batch(dev, n_fft, hop, sr):
    L = (FRAMES - 3) * hop                       # n_fft = 4 hop: lws_num_frames(L) = L / hop + 3
    rng = np.random.RandomState(n_fft)
    t = np.arange(L) / sr
    wavs = []
    for b in range(B):
        f = rng.uniform(90.0, 280.0) * (1.0 + 0.03 * np.sin(2 * np.pi * 5.0 * t))
        ph = 2 * np.pi * np.cumsum(f) / sr
        wavs.append((0.06 * sum(np.sin((k + 1) * ph) for k in range(12)) + 0.01 * rng.randn(L)).astype(np.float32))
    return torch.from_numpy(np.concatenate(wavs)).to(dev), [L] * B


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--repeats", type=int, default=7)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "pitch_cost needs a GPU"
    from deepvoice3_pytorch_amd import audio
    dev = torch.device("cuda:0")
    cases, shapes = {}, {}
    pitch = audio.PitchConfig()
    for n_fft, hop, sr in SIZES:
        cfg = audio.AudioConfig(fft_size=n_fft, hop_size=hop, sample_rate=sr)
        flat, lengths = batch(dev, n_fft, hop, sr)
        tau_min, tau_max = pitch.lags(cfg)
        f0, ap_, power, frames = audio.yin_items(flat, lengths, cfg, pitch)
        assert frames.tolist() == [FRAMES] * B
        voiced = audio.voiced(ap_, power, pitch)
        key = "%d_%d" % (n_fft, hop)
        shapes[key] = dict(B=B, frames=B * FRAMES, fft_size=n_fft, hop=hop, sample_rate=sr, tau_min=tau_min, tau_max=tau_max,
                           terms=B * FRAMES * tau_max * (n_fft - tau_max), voiced_fraction=float(voiced.float().mean()))
        cases["yin_items_" + key] = lambda flat=flat, lengths=lengths, cfg=cfg: audio.yin_items(flat, lengths, cfg, pitch)
        cases["features_items_" + key] = lambda flat=flat, lengths=lengths, cfg=cfg: audio.features_items(flat, lengths, cfg)
    with torch.no_grad():
        for fn in cases.values():
            for _ in range(3):
                fn()
        torch.cuda.synchronize()
        times = {k: [] for k in cases}
        for _ in range(args.repeats):
            for k, fn in cases.items():
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(args.calls):
                    fn()
                e1.record()
                e1.synchronize()
                times[k].append(e0.elapsed_time(e1) / args.calls)
    ms = {k: summary(v) for k, v in times.items()}
    gterms = {k: shapes[k]["terms"] / (ms["yin_items_" + k]["median"] * 1e-3) / 1e9 for k in shapes}
    res = dict(device=torch.cuda.get_device_name(0), calls=args.calls, repeats=args.repeats, shapes=shapes, ms_per_call=ms,
               yin_gterms_per_s=gterms,
               yin_over_features={k: ms["yin_items_" + k]["median"] / ms["features_items_" + k]["median"] for k in shapes})
    line = json.dumps(res, sort_keys=True)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()

# coding: utf-8
"""What the frame sizes cost in the Griffin-Lim loop: 60 iterations over 64 utterances of equal
duration at 512 / 128, 1024 / 256 and 2048 / 512 on the lws framing, device events around each call, the sizes
alternating inside every repeat, median and spread per size, and the time per transformed point (B * T * n_fft frame
points per projection; a projection is one forward and one inverse transform of every frame) relative to the 1024
kernel of the same process.

    python scripts/fft_size_cost.py [--out FILE] [--samples 131072] [--batch 64] [--iters 60] [--repeats 9]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    from deepvoice3_pytorch_amd import audio
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--samples", type=int, default=131072)
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--iters", type=int, default=60)
    ap.add_argument("--repeats", type=int, default=9)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "fft_size_cost needs a GPU"
    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(0)
    cases = {}
    for n in audio.FFT_SIZES:
        hop = n // 4
        T = audio.lws_num_frames(args.samples, hop, n)
        mag = torch.rand(args.batch, T, n // 2 + 1, generator=g).to(dev)
        cases[n] = (hop, T, mag)
        audio.griffin_lim(mag, hop, 2, convention="lws", fft_size=n)              # warm: code objects, window tables
    torch.cuda.synchronize()
    times = {n: [] for n in cases}
    for _ in range(args.repeats):
        for n, (hop, T, mag) in cases.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            audio.griffin_lim(mag, hop, args.iters, convention="lws", fft_size=n)
            e1.record()
            e1.synchronize()
            times[n].append(e0.elapsed_time(e1))
    res = dict(device=torch.cuda.get_device_name(0), batch=args.batch, samples=args.samples, iters=args.iters,
               repeats=args.repeats, sizes={})
    for n, (hop, T, _) in cases.items():
        t = np.array(times[n])
        points = args.batch * T * n * (args.iters + 1)           # the initial inverse and one projection per iteration
        res["sizes"][str(n)] = dict(hop=hop, frames=T, ms_median=float(np.median(t)), ms_min=float(t.min()),
                                    ms_max=float(t.max()), ps_per_point=float(np.median(t) * 1e9 / points))
    base = res["sizes"]["1024"]["ps_per_point"]
    for n in cases:
        res["sizes"][str(n)]["per_point_vs_1024"] = res["sizes"][str(n)]["ps_per_point"] / base
    line = json.dumps(res, sort_keys=True)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()

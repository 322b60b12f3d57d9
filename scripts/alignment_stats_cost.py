# coding: utf-8
"""What the alignment statistics cost.  Two measurements, one process:

  call   ops.alignment_stats at B = 64 items, T = 200 steps, Tk = 150 keys (the deepvoice3_ljspeech synthesis shape),
         softmax rows, item lengths between half of each axis and all of it, in both layouts: a contiguous (B, T, Tk)
         and the step program's stacked (T, B, Tk).  A queue of `--calls` calls between two device events, the two
         layouts alternating inside every repeat, after a warm-up; median, minimum and maximum per call.
  poll   RollingSynthesizer.poll() at 64 slots and chunk 8 on deepvoice3_ljspeech with random weights, every slot busy
         and nothing retiring (min = max decoder steps = 199), with and without stall_limit (a limit nothing reaches:
         the per-chunk statistics call and its device read are paid, no item stops).  Two synthesizers polled in turn
         -- the arms alternate poll by poll -- host clock around each poll (a poll ends in a device read); the first
         poll of each (admission) is the warm-up and is left out.

    python scripts/alignment_stats_cost.py [--out FILE] [--calls 5000] [--repeats 11]
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def summary(t):
    t = np.array(t)
    return dict(median=float(np.median(t)), min=float(t.min()), max=float(t.max()), n=int(t.size))


def time_calls(dev, calls, repeats):
    from deepvoice3_pytorch_amd import ops
    B, T, Tk = 64, 200, 150
    rng = np.random.RandomState(0)
    g = torch.Generator().manual_seed(0)
    steps = rng.randint(T // 2, T + 1, B)
    keys = rng.randint(Tk // 2, Tk + 1, B)
    steps[0], keys[0] = T, Tk
    i32 = lambda a: torch.as_tensor(np.asarray(a), dtype=torch.int32).to(dev)
    st, kl = i32(steps), i32(keys)
    btk = torch.softmax(torch.randn(B, T, Tk, generator=g) * 3.0, dim=-1).to(dev)
    tbk = btk.transpose(0, 1).contiguous()
    cases = {"btk": lambda: ops.alignment_stats(btk, st, kl, "btk"), "tbk": lambda: ops.alignment_stats(tbk, st, kl, "tbk")}
    assert torch.equal(cases["btk"](), cases["tbk"]())
    times = {k: [] for k in cases}
    for fn in cases.values():
        for _ in range(10):
            fn()
    torch.cuda.synchronize()
    for _ in range(repeats):
        for k, fn in cases.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(calls):
                fn()
            e1.record()
            e1.synchronize()
            times[k].append(e0.elapsed_time(e1) * 1e3 / calls)
    read_bytes = float((steps * keys).sum() * 4)
    return dict(B=B, T=T, Tk=Tk, calls=calls, repeats=repeats, bytes_read=read_bytes,
                mean_fill=dict(steps=float(steps.mean() / T), keys=float(keys.mean() / Tk)),
                us_per_call={k: summary(v) for k, v in times.items()})


def time_polls(dev):
    import bench
    from deepvoice3_pytorch_amd import audio, builder, ops, synthesis
    prev = ops.set_gemm_precision("f16x3")
    try:
        bname, hp, _ = bench.PRESETS["deepvoice3_ljspeech"]
        torch.manual_seed(0)
        model = getattr(builder, bname)(**dict(hp)).to(dev).eval()
        dec = model.seq2seq.decoder
        dec.min_decoder_steps = dec.max_decoder_steps = 199
        slots, chunk, Tk = 64, 8, 150
        rng = np.random.RandomState(1)
        seqs = [rng.randint(2, hp["n_vocab"], n).tolist() for n in rng.randint(Tk // 2, Tk + 1, slots)]
        cfg = audio.AudioConfig(griffin_lim_iters=2)
        arms = {"plain": synthesis.RollingSynthesizer(model, slots, Tk, cfg, chunk),
                "stall_limit": synthesis.RollingSynthesizer(model, slots, Tk, cfg, chunk, stall_limit=10 ** 6)}
        for rs in arms.values():
            for s in seqs:
                rs.submit(s)
            assert rs.poll() == []                     # admission + the first chunk: the warm-up
        torch.cuda.synchronize()
        times = {k: [] for k in arms}
        n_polls = (200 - chunk) // chunk - 1           # stay below the cap: nothing retires
        for _ in range(n_polls):
            for k, rs in arms.items():
                t0 = time.perf_counter()
                out = rs.poll()
                torch.cuda.synchronize()
                times[k].append((time.perf_counter() - t0) * 1e3)
                assert out == []
        res = dict(slots=slots, chunk=chunk, preset="deepvoice3_ljspeech", ms_per_poll={k: summary(v) for k, v in times.items()})
        res["stall_limit_over_plain"] = res["ms_per_poll"]["stall_limit"]["median"] / res["ms_per_poll"]["plain"]["median"]
        return res
    finally:
        ops.set_gemm_precision(prev)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--calls", type=int, default=5000)
    ap.add_argument("--repeats", type=int, default=11)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "alignment_stats_cost needs a GPU"
    dev = torch.device("cuda:0")
    with torch.no_grad():
        res = dict(device=torch.cuda.get_device_name(0), call=time_calls(dev, args.calls, args.repeats), poll=time_polls(dev))
    line = json.dumps(res, sort_keys=True)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()

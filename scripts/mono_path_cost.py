# coding: utf-8
"""What token timings cost.  One process:

  search  ops.monotonic_path at B = 64, T = 201, Tk = 100 ("btk") with item steps and keys between half of each axis and
          all of it, softmax rows sharp around a noisy diagonal, at J = 1 and J = 3: a queue of `--calls` calls between
          two device events, the cases alternating inside every repeat, after a warm-up; median, minimum and maximum per
          call.
  synth   synthesis.tts_batch for 64 utterances of 201 decoder steps (min = max decoder steps = 200) on
          deepvoice3_ljspeech with random weights and two Griffin-Lim iterations, with timings=False and timings=True
          alternating, host clock around each call (a call ends in device reads), after one warm-up call of each.

    python scripts/mono_path_cost.py [--out FILE] [--calls 20] [--repeats 7] [--search-only]
(--search-only: a few calls of each search case and nothing else, for a kernel trace.)
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


def search_cases(dev):
    from deepvoice3_pytorch_amd import ops
    B, T, Tk = 64, 201, 100
    rng = np.random.RandomState(0)
    steps, keys = rng.randint(T // 2, T + 1, B), rng.randint(Tk // 2, Tk + 1, B)
    steps[0], keys[0] = T, Tk
    a = np.zeros((B, T, Tk), dtype=np.float32)
    for b in range(B):
        t = np.arange(steps[b])[:, None]
        centre = t * (keys[b] - 1) / (steps[b] - 1) + rng.randn(steps[b], 1) * 1.5
        logits = -0.5 * ((np.arange(keys[b])[None, :] - centre) / 1.5) ** 2 + rng.randn(steps[b], keys[b]) * 0.7
        e = np.exp(logits - logits.max(axis=1, keepdims=True))
        a[b, :steps[b], :keys[b]] = e / e.sum(axis=1, keepdims=True)
    attn = torch.from_numpy(a).to(dev)
    i32 = lambda v: torch.as_tensor(np.asarray(v), dtype=torch.int32).to(dev)
    st, kl = i32(steps), i32(keys)
    cases = {"J1": lambda: ops.monotonic_path(attn, st, kl, "btk", 1),
             "J3": lambda: ops.monotonic_path(attn, st, kl, "btk", 3)}
    shape = dict(B=B, T=T, Tk=Tk, mean_fill=dict(steps=float(steps.mean() / T), keys=float(keys.mean() / Tk)),
                 cells=float((steps * keys).sum()))
    return cases, shape


def time_search(dev, calls, repeats):
    cases, shape = search_cases(dev)
    for fn in cases.values():
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    times = {k: [] for k in cases}
    for _ in range(repeats):
        for k, fn in cases.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(calls):
                fn()
            e1.record()
            e1.synchronize()
            times[k].append(e0.elapsed_time(e1) / calls)
    return dict(shape, calls=calls, repeats=repeats, ms_per_call={k: summary(v) for k, v in times.items()})


def time_synth(dev, repeats):
    import bench
    from deepvoice3_pytorch_amd import audio, builder, ops, synthesis
    prev = ops.set_gemm_precision("f16x3")
    try:
        bname, hp, _ = bench.PRESETS["deepvoice3_ljspeech"]
        torch.manual_seed(0)
        model = getattr(builder, bname)(**dict(hp)).to(dev).eval()
        dec = model.seq2seq.decoder
        dec.min_decoder_steps = dec.max_decoder_steps = 200
        B, Tk = 64, 100
        rng = np.random.RandomState(1)
        seqs = [rng.randint(2, hp["n_vocab"], n).tolist() for n in rng.randint(Tk // 2, Tk + 1, B)]
        cfg = audio.AudioConfig(griffin_lim_iters=2)
        times = {False: [], True: []}
        feasible = None
        for i in range(repeats + 1):
            for on in (False, True):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                res = synthesis.tts_batch(model, seqs, audio_cfg=cfg, timings=on)
                torch.cuda.synchronize()
                if i:                                   # the first call of each is the warm-up
                    times[on].append((time.perf_counter() - t0) * 1e3)
                if on:
                    feasible = int(sum(r[4]["summary"][0].item() for r in res))
        off, on = summary(times[False]), summary(times[True])
        return dict(preset="deepvoice3_ljspeech", B=B, decoder_steps=int(res[0][2].shape[0]), griffin_lim_iters=2,
                    feasible_items=feasible, ms_per_call=dict(timings_off=off, timings_on=on),
                    added_ms=on["median"] - off["median"])
    finally:
        ops.set_gemm_precision(prev)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--search-only", action="store_true")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "mono_path_cost needs a GPU"
    dev = torch.device("cuda:0")
    with torch.no_grad():
        if args.search_only:
            cases, _ = search_cases(dev)
            for fn in cases.values():
                for _ in range(3):
                    fn()
            torch.cuda.synchronize()
            return
        res = dict(device=torch.cuda.get_device_name(0), search=time_search(dev, args.calls, args.repeats),
                   synth=time_synth(dev, args.repeats))
    line = json.dumps(res, sort_keys=True)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()

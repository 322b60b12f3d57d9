# coding: utf-8
"""What a guided decode costs.

  synth   synthesis.tts_batch for 64 ragged utterances on deepvoice3_ljspeech with random weights and two Griffin-Lim
          iterations: free running, then guided at the SAME per-item step counts (durations that spread every item's free
          step count over its tokens: fit_durations of all-ones), alternating in one process, host clock around each call
          after one warm-up call of each.  The free run reads the done flags once per chunk of 8 steps and runs to the
          slowest item; the guided run is one library call for max(steps) steps and one host read of the step counts.
          Twice: "synth" with the done flag live (min_decoder_steps 2: a random-weight model stops within a few steps,
          ragged), and "synth_full" with it out of the rule (every item runs max_decoder_steps + 1 = 201 steps).
  table   ops.guide_from_durations alone for those 64 items (Tk = the longest text, T = max_decoder_steps + 1):
          `--launches` calls back to back between two device events.
  --parent-root DIR: a checkout of the parent commit with its library built.  The default path (tts_batch without
          durations, the same 64 utterances) is measured by this same script in child processes (--default-only),
          alternating with child processes of this checkout, `--rounds` times each.

    python scripts/guided_decode_cost.py [--out profiles/guided_decode_cost.json] [--parent-root DIR]
"""
import argparse
import json
import os
import subprocess
import sys
import time

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def summary(t):
    import numpy as np
    t = np.array(t)
    return dict(median=float(np.median(t)), min=float(t.min()), max=float(t.max()), n=int(t.size))


def setup(args, dev):
    import numpy as np
    import torch
    import bench
    from deepvoice3_pytorch_amd import audio, builder
    bname, hp, _ = bench.PRESETS["deepvoice3_ljspeech"]
    torch.manual_seed(0)
    model = getattr(builder, bname)(**dict(hp)).to(dev).eval()
    dec = model.seq2seq.decoder
    dec.min_decoder_steps, dec.max_decoder_steps = args.min_steps, args.steps - 1
    rng = np.random.RandomState(1)
    seqs = [rng.randint(2, hp["n_vocab"], n).tolist() for n in rng.randint(args.keys // 2, args.keys + 1, args.batch)]
    return model, seqs, audio.AudioConfig(griffin_lim_iters=2)


def time_calls(arms, repeats):
    """arms {name: fn}: alternating, host clock around each call, the first call of each is the warm-up"""
    import torch
    times = {k: [] for k in arms}
    for i in range(repeats + 1):
        for k, fn in arms.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            if i:
                times[k].append((time.perf_counter() - t0) * 1e3)
    return {k: summary(v) for k, v in times.items()}


def default_path(args, dev):
    from deepvoice3_pytorch_amd import ops, synthesis
    prev = ops.set_gemm_precision("f16x3")
    try:
        model, seqs, cfg = setup(args, dev)
        return time_calls({"tts_batch %d utterances" % len(seqs): lambda: synthesis.tts_batch(model, seqs, audio_cfg=cfg)},
                          args.repeats)
    finally:
        ops.set_gemm_precision(prev)


def guided(args, dev):
    import torch
    from deepvoice3_pytorch_amd import ops, synthesis
    prev = ops.set_gemm_precision("f16x3")
    try:
        model, seqs, cfg = setup(args, dev)
        free = synthesis.tts_batch(model, seqs, audio_cfg=cfg)
        steps = [int(r[2].shape[0]) for r in free]
        D = [synthesis.fit_durations([1] * len(s), n) for s, n in zip(seqs, steps)]
        got = synthesis.tts_batch(model, seqs, audio_cfg=cfg, durations=D)
        assert [int(r[2].shape[0]) for r in got] == steps
        arms = {"free running": lambda: synthesis.tts_batch(model, seqs, audio_cfg=cfg),
                "guided": lambda: synthesis.tts_batch(model, seqs, audio_cfg=cfg, durations=D)}
        ms = time_calls(arms, args.repeats)
        # the guide table alone
        B, Tk, T = len(seqs), max(len(s) for s in seqs), model.seq2seq.decoder.max_decoder_steps + 1
        dur = torch.zeros(B, Tk, dtype=torch.int32)
        for b, d in enumerate(D):
            dur[b, :len(d)] = torch.tensor(d, dtype=torch.int32)
        dur, kl = dur.to(dev), torch.tensor([len(s) for s in seqs], dtype=torch.int32).to(dev)
        table = torch.empty(B, T, dtype=torch.int32, device=dev)
        ops.guide_from_durations(dur, kl, T, guide=table)
        torch.cuda.synchronize()
        per = []
        for _ in range(args.repeats):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(args.launches):
                ops.guide_from_durations(dur, kl, T, guide=table)
            e1.record()
            e1.synchronize()
            per.append(e0.elapsed_time(e1) / args.launches)
        return dict(preset="deepvoice3_ljspeech", B=B, min_decoder_steps=args.min_steps, longest_text=Tk, griffin_lim_iters=2, steps_min=min(steps),
                    steps_max=max(steps), steps_sum=sum(steps), ms_per_call=ms,
                    guided_minus_free_ms=ms["guided"]["median"] - ms["free running"]["median"],
                    guide_table=dict(B=B, Tk=Tk, T=T, launches=args.launches, ms_per_call=summary(per)))
    finally:
        ops.set_gemm_precision(prev)


def child(root, args):
    cmd = [sys.executable, os.path.abspath(__file__), "--root", root, "--default-only", "--batch", str(args.batch),
           "--keys", str(args.keys), "--steps", str(args.steps), "--repeats", str(args.repeats)]
    out = subprocess.run(cmd, check=True, stdout=subprocess.PIPE, timeout=300).stdout.decode()
    return json.loads(out.strip().splitlines()[-1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--root", default=HERE, help="the checkout whose package is measured")
    ap.add_argument("--parent-root", default=None)
    ap.add_argument("--default-only", action="store_true")
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--keys", type=int, default=100)
    ap.add_argument("--steps", type=int, default=201, help="max_decoder_steps + 1")
    ap.add_argument("--min-steps", type=int, default=2, help="min_decoder_steps")
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--launches", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=2)
    args = ap.parse_args()
    sys.path.insert(0, os.path.abspath(args.root))
    processes = []
    if args.parent_root:                                  # before this process opens the device
        for _ in range(args.rounds):
            for name, root in (("parent", args.parent_root), ("this", args.root)):
                processes.append(dict(build=name, ms_per_call=child(root, args)["default_path"]))
    import torch
    assert torch.cuda.is_available(), "guided_decode_cost needs a GPU"
    dev = torch.device("cuda:0")
    with torch.no_grad():
        res = dict(device=torch.cuda.get_device_name(0), default_path=default_path(args, dev))
        if not args.default_only:
            res["synth"] = guided(args, dev)
            args.min_steps = args.steps - 1
            res["synth_full"] = guided(args, dev)
    if processes:
        res["default_path_by_process"] = processes
    line = json.dumps(res, sort_keys=True)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()

# coding: utf-8
"""What training health (TrainConfig(skip_nonfinite=True), Trainer.tensor_stats()) costs.  One process,
same-process A/B in the manner of scripts/ema_cost.py:

  step    the replayed training step (train_step.GraphedTrainer, the form bench.py times) of a preset at the given batch
          sizes on finite data, four trainers from one seed on one batch -- the guard off / on, each without and with
          weight averaging --, `--steps` replays between two device events per window, the arms alternating inside every
          repeat, after a warm-up of all; the arms start from one dropout seed, so their losses agree to the last bit
          and no arm ever skips a step;
  stats   Trainer.tensor_stats() on the last trainer's arena (the preset's real tensor layout), queues of `--calls` calls
          between two device events; bytes per call from the element count (four 4-byte words per parameter: the floor
          of a pass that reads p, g, m and v once), so the rate is achieved HBM traffic.

    python scripts/health_cost.py [--out FILE] [--preset deepvoice3_ljspeech] [--batches 64,16] [--steps 20]
                                  [--repeats 9] [--calls 200]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

HBM_PEAK_TB_S = 8.0          # MI355X HBM3E, specification


def summary(t):
    t = np.array(t)
    return dict(median=float(np.median(t)), min=float(t.min()), max=float(t.max()), n=int(t.size))


def _window(fn, count):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(count):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / count


ARMS = (("plain_off", {}), ("plain_on", dict(skip_nonfinite=True)),
        ("ema_off", dict(ema_decay=0.999)), ("ema_on", dict(ema_decay=0.999, skip_nonfinite=True)))


def time_step(dev, preset, batch, steps, repeats, calls, stats, text_len=150, frames=800):
    import bench
    from deepvoice3_pytorch_amd import builder, ops, train_step
    bname, hp, ga_sigma = bench.PRESETS[preset]
    hp = dict(hp)
    bt = bench.synth_batch(np.random.RandomState(1234), batch, text_len, frames, hp)
    arms = {}
    try:
        for name, kw in ARMS:
            torch.manual_seed(0)
            ops.dropout_state.manual_seed(11)       # the same masks in every arm: site numbering and the step's plan anew
            ops.mask_plan.__init__()
            model = getattr(builder, bname)(**hp).to(dev)
            tr = train_step.Trainer(model, train_step.TrainConfig(max_positions=hp["max_positions"],
                                                                  guided_attention_sigma=ga_sigma, **kw))
            b = train_step.Batch.from_collate(bt["text"], bt["input_lengths"], bt["mel"], bt["y"], bt["text_positions"],
                                              bt["frame_positions"], bt["done"], bt["target_lengths"], None,
                                              downsample_step=4, device=dev)
            arms[name] = (tr, train_step.GraphedTrainer(tr, b, warmup=2))
        for _, g in arms.values():          # every arm warm before any is timed
            for _ in range(10):
                g.step()
        torch.cuda.synchronize()
        times = {k: [] for k in arms}
        for _ in range(repeats):
            for k, (_, g) in arms.items():
                times[k].append(_window(g.step, steps))
        n = arms["ema_on"][0].arena.total
        loss = {k: float(g.scal["loss"]) for k, (_, g) in arms.items()}      # (every arm has run the same steps)
        ms = {k: summary(v) for k, v in times.items()}
        res = dict(preset=preset, batch=batch, gemm=ops.gemm_precision(), graph_split=bool(arms["ema_on"][1].split),
                   arena_elements=int(n), steps_per_window=steps, repeats=repeats, ms_per_step=ms, last_loss=loss,
                   skipped_steps={k: tr.health()["skipped_steps"] for k, (tr, _) in arms.items() if k.endswith("_on")})
        for fam in ("plain", "ema"):
            on, off = ms[fam + "_on"]["median"], ms[fam + "_off"]["median"]
            res[fam + "_on_over_off"] = on / off
            res[fam + "_on_minus_off_us"] = 1e3 * (on - off)
        st = None
        if stats:
            tr = arms["ema_on"][0]
            names, table = tr.tensor_stats()
            for _ in range(20):
                tr.tensor_stats()
            torch.cuda.synchronize()
            us = summary([1e3 * _window(tr.tensor_stats, calls) for _ in range(repeats)])
            nel = int(sum(tr.arena.sizes))
            tb_s = 16.0 * nel / (us["median"] * 1e-6) / 1e12
            st = dict(tensors=len(names), chunks=int(tr.arena.stat_tables()[0].shape[0]), elements=nel,
                      arena_elements=int(n), calls_per_window=calls, repeats=repeats, us_per_call=us,
                      floor_bytes_per_element=16, tb_per_s=tb_s, fraction_of_hbm_peak=tb_s / HBM_PEAK_TB_S,
                      hbm_peak_tb_per_s=HBM_PEAK_TB_S, grad_nonfinite_total=float(table[:, 2].sum()),
                      note="host time of the call (name lookup, two launches) is inside the window")
        return res, st
    finally:
        for tr, g in arms.values():
            g.close()
            tr.close()
        ops.dropout_state.dev_offset = None
        torch.cuda.synchronize()
        torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--preset", default="deepvoice3_ljspeech")
    ap.add_argument("--batches", default="64,16")
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=9)
    ap.add_argument("--calls", type=int, default=200)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "health_cost needs a GPU"
    dev = torch.device("cuda:0")
    res = dict(device=torch.cuda.get_device_name(0), step=[], tensor_stats=None)
    batches = [int(s) for s in args.batches.split(",") if s]
    for i, b in enumerate(batches):
        r, st = time_step(dev, args.preset, b, args.steps, args.repeats, args.calls, stats=(i == len(batches) - 1))
        res["step"].append(r)
        if st is not None:
            res["tensor_stats"] = st
        m = r["ms_per_step"]
        print("step B=%d: plain off %.3f / on %.3f ms, averaging off %.3f / on %.3f ms" % (
            b, m["plain_off"]["median"], m["plain_on"]["median"], m["ema_off"]["median"], m["ema_on"]["median"]),
            file=sys.stderr, flush=True)
    line = json.dumps(res, sort_keys=True)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()

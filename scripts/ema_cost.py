# coding: utf-8
"""What weight averaging (TrainConfig(ema_decay=...)) costs.  One process, same-process A/B:

  step    the replayed training step (train_step.GraphedTrainer, the form bench.py times) of a preset at the given
          batch sizes, two trainers from one seed on one batch -- averaging off and on --, `--steps` replays between two
          device events per window, the two arms alternating inside every repeat, after a warm-up of both; both arms
          start from one dropout seed, so their losses agree to the last bit (the update is the same update);
  kernel  dv3_clip_adam_f32 against dv3_clip_adam_ema_f32 (and dv3_swap_f32) on buffers of the arena's size, queues of
          `--calls` launches between two device events, alternating; bytes moved per call from the element count
          (7, 9 and 4 words per element), so the rates are achieved HBM traffic, and the yardstick is the 9 / 7 ratio.

    python scripts/ema_cost.py [--out FILE] [--preset deepvoice3_ljspeech] [--batches 64,16] [--steps 20] [--repeats 9]
                               [--calls 200] [--kernel-only [--elements N]]
(--kernel-only: the kernel part alone on N elements, default the deepvoice3_ljspeech arena's 25 620 992.)
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


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


def time_step(dev, preset, batch, steps, repeats, text_len=150, frames=800, decay=0.999):
    import bench
    from deepvoice3_pytorch_amd import builder, ops, train_step
    bname, hp, ga_sigma = bench.PRESETS[preset]
    hp = dict(hp)
    bt = bench.synth_batch(np.random.RandomState(1234), batch, text_len, frames, hp)
    arms = {}
    for name, kw in (("off", {}), ("on", dict(ema_decay=decay))):
        torch.manual_seed(0)
        ops.dropout_state.manual_seed(11)       # the same masks in both arms: site numbering and the step's plan anew
        ops.mask_plan.__init__()
        model = getattr(builder, bname)(**hp).to(dev)
        tr = train_step.Trainer(model, train_step.TrainConfig(max_positions=hp["max_positions"],
                                                              guided_attention_sigma=ga_sigma, **kw))
        b = train_step.Batch.from_collate(bt["text"], bt["input_lengths"], bt["mel"], bt["y"], bt["text_positions"],
                                          bt["frame_positions"], bt["done"], bt["target_lengths"], None,
                                          downsample_step=4, device=dev)
        arms[name] = (tr, train_step.GraphedTrainer(tr, b, warmup=2))
    try:
        for _, g in arms.values():          # both arms warm before either is timed
            for _ in range(10):
                g.step()
        torch.cuda.synchronize()
        times = {k: [] for k in arms}
        for _ in range(repeats):
            for k, (_, g) in arms.items():
                times[k].append(_window(g.step, steps))
        n = arms["on"][0].arena.total
        loss = {k: float(g.scal["loss"]) for k, (_, g) in arms.items()}      # (both arms have run the same steps)
        res = dict(preset=preset, batch=batch, gemm=ops.gemm_precision(), graph_split=bool(arms["on"][1].split),
                   arena_elements=int(n), steps_per_window=steps, repeats=repeats,
                   ms_per_step={k: summary(v) for k, v in times.items()}, last_loss=loss)
        res["on_over_off"] = res["ms_per_step"]["on"]["median"] / res["ms_per_step"]["off"]["median"]
        res["on_minus_off_us"] = 1e3 * (res["ms_per_step"]["on"]["median"] - res["ms_per_step"]["off"]["median"])
        return res, int(n)
    finally:
        for tr, g in arms.values():
            g.close()
            tr.close()
        ops.dropout_state.dev_offset = None
        torch.cuda.synchronize()
        torch.cuda.empty_cache()


def time_kernels(dev, n, calls, repeats):
    from deepvoice3_pytorch_amd import ops
    g0 = torch.Generator(device="cpu").manual_seed(0)
    mk = lambda s: (torch.randn(n, generator=g0) * s).to(dev)
    p, g, m, e, e2 = mk(0.1), mk(0.01), mk(0.001), mk(0.1), mk(0.1)
    v = (torch.rand(n, generator=g0) * 1e-4).to(dev)
    norm = torch.tensor([1.0, 1.0], device=dev)
    hyper = torch.tensor([5e-4, 0.9, 0.9, 1e-3], device=dev)
    args = (norm, 0.1, hyper, 0.5, 0.9, 1e-6, 0.0, 1.0)
    cases = {"clip_adam": (lambda: ops.clip_adam(p, g, m, v, *args), 7),
             "clip_adam_ema": (lambda: ops.clip_adam_ema(p, g, m, v, e, *args), 9),
             "swap": (lambda: ops.swap_(e, e2), 4)}
    for fn, _ in cases.values():
        for _ in range(20):
            fn()
    torch.cuda.synchronize()
    times = {k: [] for k in cases}
    for _ in range(repeats):
        for k, (fn, _) in cases.items():
            times[k].append(1e3 * _window(fn, calls))
    us = {k: summary(v) for k, v in times.items()}
    res = dict(elements=int(n), calls_per_window=calls, repeats=repeats, us_per_call=us,
               words_per_element={k: w for k, (_, w) in cases.items()},
               tb_per_s={k: 4.0 * w * n / (us[k]["median"] * 1e-6) / 1e12 for k, (_, w) in cases.items()})
    res["ema_over_plain"] = us["clip_adam_ema"]["median"] / us["clip_adam"]["median"]
    res["traffic_ratio"] = 9.0 / 7.0
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--preset", default="deepvoice3_ljspeech")
    ap.add_argument("--batches", default="64,16")
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=9)
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--kernel-only", action="store_true")
    ap.add_argument("--elements", type=int, default=25620992)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "ema_cost needs a GPU"
    dev = torch.device("cuda:0")
    res = dict(device=torch.cuda.get_device_name(0), step=[])
    n = args.elements
    for b in [] if args.kernel_only else [int(s) for s in args.batches.split(",") if s]:
        r, n = time_step(dev, args.preset, b, args.steps, args.repeats)
        res["step"].append(r)
        print("step B=%d: off %.3f ms, on %.3f ms (x %.4f)" % (b, r["ms_per_step"]["off"]["median"],
                                                               r["ms_per_step"]["on"]["median"], r["on_over_off"]),
              file=sys.stderr)
    res["kernel"] = time_kernels(dev, n, args.calls, args.repeats)
    line = json.dumps(res, sort_keys=True)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()

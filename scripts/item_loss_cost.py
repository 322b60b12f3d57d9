# coding: utf-8
"""What the per-item loss reductions of held-out evaluation cost beside their batch counterparts, at
the deepvoice3_ljspeech training shape: B = 64, mel (64, 200, 80), linear (64, 800, 513), attention (2, 64, 200, 150).
Forward only (no gradient buffer on either side), predictions in the model's layout (time-fastest views of BCT
tensors) against bin-fastest targets, item lengths between half the padded length and all of it.  Every case is a
queue of `--calls` calls between two device events, the eight cases alternating inside every repeat, after a warm-up;
median, minimum and maximum per call over the repeats, in one process.

    python scripts/item_loss_cost.py [--out FILE] [--batch 64] [--calls 50] [--repeats 11]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    from deepvoice3_pytorch_amd import ops
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--calls", type=int, default=50)
    ap.add_argument("--repeats", type=int, default=11)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "item_loss_cost needs a GPU"
    dev = torch.device("cuda:0")
    B, Td, Tk, L, ds, Dm, Dl = args.batch, 200, 150, 2, 4, 80, 513
    g = torch.Generator().manual_seed(0)
    rng = np.random.RandomState(0)
    i32 = lambda a: torch.as_tensor(np.asarray(a), dtype=torch.int32).to(dev)
    dec_host = rng.randint(Td // 2, Td + 1, B)
    dec_host[0] = Td
    dec_len, lin_len = i32(dec_host), i32(dec_host * ds)
    in_host = rng.randint(Tk // 2, Tk + 1, B)
    in_host[0] = Tk
    in_len = i32(in_host)
    pred = lambda T, D: (torch.rand(B, D, T, generator=g) * 0.98 + 0.01).to(dev).transpose(1, 2)
    mel_out, mel = pred(Td, Dm), torch.rand(B, Td, Dm, generator=g).to(dev)
    lin_out, lin = pred(Td * ds, Dl), torch.rand(B, Td * ds, Dl, generator=g).to(dev)
    done_hat = (torch.rand(B, Td, 1, generator=g) * 0.9 + 0.05).to(dev)
    done = (torch.rand(B, Td, 1, generator=g) > 0.5).float().to(dev)
    attn = torch.rand(L, B, Td, Tk, generator=g).to(dev)
    cases = {
        "mel/batch": lambda: ops.spec_loss(mel_out, mel, dec_len, 1, 0.5, 0.1),
        "mel/items": lambda: ops.spec_loss_items(mel_out, mel, dec_len, 1),
        "linear/batch": lambda: ops.spec_loss(lin_out, lin, lin_len, 1, 0.5, 0.1),
        "linear/items": lambda: ops.spec_loss_items(lin_out, lin, lin_len, 1),
        "done/batch": lambda: ops.bce_loss(done_hat, done),
        "done/items": lambda: ops.bce_loss_items(done_hat, done, dec_len),
        "attn/batch": lambda: ops.guided_attention_loss(attn, in_len, dec_len, 0.2),
        "attn/items": lambda: ops.guided_attention_loss_items(attn, in_len, dec_len, 0.2),
    }
    times = {k: [] for k in cases}
    with torch.no_grad():
        for fn in cases.values():                  # warm: code objects, the allocator's blocks
            for _ in range(5):
                fn()
        torch.cuda.synchronize()
        for _ in range(args.repeats):
            for k, fn in cases.items():
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(args.calls):
                    fn()
                e1.record()
                e1.synchronize()
                times[k].append(e0.elapsed_time(e1) * 1e3 / args.calls)
    res = dict(device=torch.cuda.get_device_name(0), batch=B, calls=args.calls, repeats=args.repeats,
               mean_fill=dict(decoder=float(dec_host.mean() / Td), text=float(in_host.mean() / Tk)), us_per_call={})
    for k, t in times.items():
        t = np.array(t)
        res["us_per_call"][k] = dict(median=float(np.median(t)), min=float(t.min()), max=float(t.max()))
    med = lambda k: res["us_per_call"][k]["median"]
    res["items_over_batch"] = {p: med(p + "/items") / med(p + "/batch") for p in ("mel", "linear", "done", "attn")}
    parts = ("mel", "linear", "done", "attn")
    res["us_all_four"] = dict(batch=sum(med(p + "/batch") for p in parts), items=sum(med(p + "/items") for p in parts))
    line = json.dumps(res, sort_keys=True)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()

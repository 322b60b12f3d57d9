# coding: utf-8
"""What the momentum term of fast Griffin-Lim costs on the device: 64 utterances x 804 frames on the lws
framing at 1024 / 256 (the benchmarked synthesis shape; mag + frames + cprev are 530 MB, above the 256 MiB Infinity
Cache) and at 2048 / 512, in the whole-batch and the per-item form (every item at its full length: the same work).

Arms, alternating inside every repeat, device events around `--inner` back-to-back calls of audio.griffin_lim, median
and range over `--repeats`:
    plain60   60 iterations, momentum 0 (the kernels every call ran before the option existed)
    mom60     60 iterations, momentum 0.99
    mom30     30 iterations, momentum 0.99
and, for the projection kernel alone (no overlap-add), 60 launches of the plain and of the momentum entry point:
    proj_plain, proj_mom -> time per launch and bytes/s, the bytes taken from shapes: y, mag, frames (+ 2 x cprev).

--parent-root DIR: a checkout of the parent commit with its library built.  Its plain60 is measured by this same script
in child processes (--plain-only), alternating with child processes of this checkout, `--rounds` times each, before the
main measurement: the two builds' plain60 side by side, with the spread between processes of one build.

    python scripts/fast_gl_cost.py [--out profiles/fast_gl_cost.json] [--parent-root DIR] [--frames 804] [--batch 64]
"""
import argparse
import json
import os
import subprocess
import sys

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = ((1024, 256), (2048, 512))


def _stats(ms):
    import numpy as np
    t = np.array(ms)
    return dict(ms_median=float(np.median(t)), ms_min=float(t.min()), ms_max=float(t.max()))


def measure(args):
    import torch
    from deepvoice3_pytorch_amd import audio, _lib
    from deepvoice3_pytorch_amd.ops import _stream
    assert torch.cuda.is_available(), "fast_gl_cost needs a GPU"
    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(0)
    B, T = args.batch, args.frames
    has_momentum = "dv3_gl_project_momentum_f32" in _lib.FUNCS and not args.plain_only

    def gl(mag, hop, n, iters, tlen, momentum):
        kw = dict(momentum=momentum) if momentum else {}
        return audio.griffin_lim(mag, hop, iters, None, "lws", None, tlen, n, **kw)

    arms = {}
    for n, hop in CASES:
        mag = torch.rand(B, T, n // 2 + 1, generator=g).to(dev)
        tlen = torch.full((B,), T, dtype=torch.int32, device=dev)
        for form, tl in (("batch", None), ("items", tlen)):
            arms["%d %s plain60" % (n, form)] = (lambda mag=mag, hop=hop, n=n, tl=tl: gl(mag, hop, n, 60, tl, 0.0))
            if has_momentum:
                arms["%d %s mom60" % (n, form)] = (lambda mag=mag, hop=hop, n=n, tl=tl: gl(mag, hop, n, 60, tl, 0.99))
                arms["%d %s mom30" % (n, form)] = (lambda mag=mag, hop=hop, n=n, tl=tl: gl(mag, hop, n, 30, tl, 0.99))
        if has_momentum:                                  # the projection kernel alone
            awin, swin = audio.lws_windows(dev, hop, None, n)
            y = torch.randn(B, audio.lws_num_samples(T, hop, n), generator=g).to(dev)
            frames = torch.empty((B, T, n), dtype=torch.float32, device=dev)
            cprev = torch.zeros((B, T, n // 2 + 1, 2), dtype=torch.float32, device=dev)

            def proj_plain(y=y, mag=mag, awin=awin, swin=swin, frames=frames, hop=hop, n=n):
                for _ in range(60):
                    _lib.call("dv3_lws_gl_project_f32_n", y.data_ptr(), mag.data_ptr(), awin.data_ptr(), swin.data_ptr(),
                              frames.data_ptr(), B, T, hop, n, _stream())

            def proj_mom(y=y, mag=mag, awin=awin, swin=swin, frames=frames, cprev=cprev, hop=hop, n=n):
                for _ in range(60):
                    _lib.call("dv3_gl_project_momentum_f32", y.data_ptr(), mag.data_ptr(), awin.data_ptr(), swin.data_ptr(),
                              cprev.data_ptr(), frames.data_ptr(), B, T, hop, None, 1, n, 0.99, 0, _stream())
            arms["%d proj_plain" % n], arms["%d proj_mom" % n] = proj_plain, proj_mom
    for f in arms.values():                               # warm: code objects, window tables, the allocator's blocks
        f()
    torch.cuda.synchronize()
    times = {k: [] for k in arms}
    for _ in range(args.repeats):
        for k, f in arms.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(args.inner):
                f()
            e1.record()
            e1.synchronize()
            times[k].append(e0.elapsed_time(e1) / args.inner)
    res = dict(device=torch.cuda.get_device_name(0), batch=B, frames=T, repeats=args.repeats, inner=args.inner,
               arms={k: _stats(v) for k, v in times.items()})
    if has_momentum:
        ratios = {}
        for n, hop in CASES:
            F, L = n // 2 + 1, audio.lws_num_samples(T, hop, n)
            base = 4.0 * B * (L + T * F + T * n)                                    # y, mag, frames
            for name, extra in (("proj_plain", 0.0), ("proj_mom", 2.0 * 8.0 * B * T * F)):
                a = res["arms"]["%d %s" % (n, name)]
                a["us_per_launch"] = a["ms_median"] * 1e3 / 60
                a["bytes_per_launch"] = base + extra
                a["tb_per_s"] = (base + extra) / (a["ms_median"] * 1e-3 / 60) / 1e12
            ratios["%d projection mom/plain" % n] = (res["arms"]["%d proj_mom" % n]["ms_median"] /
                                                     res["arms"]["%d proj_plain" % n]["ms_median"])
            for form in ("batch", "items"):
                p60, m60, m30 = (res["arms"]["%d %s %s" % (n, form, a)]["ms_median"] for a in ("plain60", "mom60", "mom30"))
                ratios["%d %s mom60/plain60 (per iteration)" % (n, form)] = m60 / p60
                ratios["%d %s mom30/plain60 (end to end)" % (n, form)] = m30 / p60
        res["ratios"] = ratios
    return res


def child(root, args):
    cmd = [sys.executable, os.path.abspath(__file__), "--root", root, "--plain-only", "--frames", str(args.frames), "--batch",
           str(args.batch), "--repeats", str(args.repeats), "--inner", str(args.inner)]
    out = subprocess.run(cmd, check=True, stdout=subprocess.PIPE, timeout=300).stdout.decode()
    return json.loads(out.strip().splitlines()[-1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--root", default=HERE, help="the checkout whose package is measured")
    ap.add_argument("--parent-root", default=None)
    ap.add_argument("--plain-only", action="store_true")
    ap.add_argument("--frames", type=int, default=804)
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--repeats", type=int, default=9)
    ap.add_argument("--inner", type=int, default=4)
    ap.add_argument("--rounds", type=int, default=2)
    args = ap.parse_args()
    sys.path.insert(0, os.path.abspath(args.root))
    processes = []
    if args.parent_root:                                  # before this process opens the device
        for _ in range(args.rounds):
            for name, root in (("parent", args.parent_root), ("this", args.root)):
                r = child(root, args)
                processes.append(dict(build=name, arms={k: v for k, v in r["arms"].items()}))
    res = measure(args)
    if processes:
        res["plain60_by_process"] = processes
    line = json.dumps(res, sort_keys=True)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()

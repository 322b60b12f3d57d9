# coding: utf-8
"""What the single-pass starting phase (SPSI) costs on the device and what it buys there: 64 utterances x
804 frames on the lws framing at 1024 / 256 (the benchmarked synthesis shape) and at 2048 / 512.

Magnitudes: "speech", |STFT| of a voiced, vibrato-carrying harmonic signal made on the device (the recipe of
tests/fast_gl_ref.py::speechlike, one f0 per item), and "rand", uniform noise (the input of scripts/fast_gl_cost.py:
a peak every third bin, the shortest lobes).

    spsi      the dv3_spsi_phasor_f32 launch alone, into a preallocated buffer, `--launches` back to back between two
              device events -> time per launch, on both kinds of magnitudes, whole batch and with tlen
Arms on the speech magnitudes, alternating inside every repeat, device events around `--inner` back-to-back calls, median
and range over `--repeats`; whole-batch and per-item form (every item at its full length: the same work):
    plain60   60 plain iterations from zero phase (today's default)
    spsi10    audio.spsi_phasor + 10 iterations at momentum 0.99
    zero30    30 iterations at 0.99 from zero phase
    spsi30    audio.spsi_phasor + 30 iterations at 0.99
and the spectral convergence each arm ends at on the device (fp32 STFT of the result against the magnitudes).

--parent-root DIR: a checkout of the parent commit with its library built.  Its plain60 is measured by this same script
in child processes (--plain-only), alternating with child processes of this checkout, `--rounds` times each, before the
main measurement: the two builds' default path side by side, with the spread between processes of one build.

    python scripts/spsi_cost.py [--out profiles/spsi_cost.json] [--parent-root DIR] [--frames 804] [--batch 64]
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


def speech_magnitudes(audio, dev, n, hop, B, T):
    import math
    import torch
    L = audio.lws_num_samples(T, hop, n)
    sr = 22050.0 * n / 1024
    g = torch.Generator().manual_seed(3)
    t = (torch.arange(L, dtype=torch.float64, device=dev) / sr)[None, :]
    b = torch.arange(B, dtype=torch.float64, device=dev)[:, None]
    f0 = 110.0 + 2.0 * b + 40.0 * torch.sin(2 * math.pi * 1.5 * t + b)
    phi = 2 * math.pi * torch.cumsum(f0, dim=1) / sr
    voiced = sum(torch.sin(k * phi) / k for k in range(1, 20)) * (0.5 + 0.5 * torch.sin(2 * math.pi * 3 * t))
    y = (0.1 * (voiced + 0.05 * torch.randn(B, L, generator=g, dtype=torch.float64).to(dev))).float().contiguous()
    _, sp = audio.stft(y, T, hop, want_phasor=False, want_spec=True, convention="lws", fft_size=n)
    return sp.norm(dim=-1).contiguous()


def convergence(audio, y, mag, hop, n):
    _, sp = audio.stft(y.contiguous(), mag.shape[1], hop, want_phasor=False, want_spec=True, convention="lws", fft_size=n)
    return float((sp.norm(dim=-1) - mag).norm() / mag.norm())


def measure(args):
    import torch
    from deepvoice3_pytorch_amd import audio, _lib
    from deepvoice3_pytorch_amd.ops import _stream
    assert torch.cuda.is_available(), "spsi_cost needs a GPU"
    dev = torch.device("cuda:0")
    B, T = args.batch, args.frames
    has_spsi = "dv3_spsi_phasor_f32" in _lib.FUNCS and not args.plain_only

    def gl(mag, hop, n, iters, tlen, momentum, spsi):
        init = audio.spsi_phasor(mag, hop, tlen, n) if spsi else None
        kw = dict(momentum=momentum) if momentum else {}
        return audio.griffin_lim(mag, hop, iters, init, "lws", None, tlen, n, **kw)

    arms, launches, sc = {}, {}, {}
    for n, hop in CASES:
        speech = speech_magnitudes(audio, dev, n, hop, B, T)
        tlen = torch.full((B,), T, dtype=torch.int32, device=dev)
        for form, tl in (("batch", None), ("items", tlen)):
            def arm(iters, momentum, spsi, mag=speech, hop=hop, n=n, tl=tl):
                return lambda: gl(mag, hop, n, iters, tl, momentum, spsi)
            arms["%d %s plain60" % (n, form)] = arm(60, 0.0, False)
            if has_spsi:
                arms["%d %s spsi10" % (n, form)] = arm(10, 0.99, True)
                arms["%d %s zero30" % (n, form)] = arm(30, 0.99, False)
                arms["%d %s spsi30" % (n, form)] = arm(30, 0.99, True)
        if has_spsi:
            for name in ("plain60", "spsi10", "zero30", "spsi30"):
                sc["%d %s" % (n, name)] = convergence(audio, arms["%d batch %s" % (n, name)](), speech, hop, n)
            sc["%d spsi0" % n] = convergence(audio, gl(speech, hop, n, 0, None, 0.0, True), speech, hop, n)
            rand = torch.rand(B, T, n // 2 + 1, generator=torch.Generator().manual_seed(0)).to(dev)
            out = torch.empty((B, T, n // 2 + 1, 2), dtype=torch.float32, device=dev)
            for kind, mag in (("speech", speech), ("rand", rand)):
                for form, tl in (("batch", None), ("items", tlen)):
                    def launch(mag=mag, out=out, hop=hop, n=n, tl=tl):
                        for _ in range(args.launches):
                            _lib.call("dv3_spsi_phasor_f32", mag.data_ptr(), out.data_ptr(), B, T, hop,
                                      tl.data_ptr() if tl is not None else None, n, _stream())
                    launches["%d spsi %s %s" % (n, kind, form)] = launch
    for f in list(arms.values()) + list(launches.values()):      # warm: code objects, window tables, allocator blocks
        f()
    torch.cuda.synchronize()
    times = {k: [] for k in list(arms) + list(launches)}
    for _ in range(args.repeats):
        for k, f in list(arms.items()) + list(launches.items()):
            inner = args.inner if k in arms else 1
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(inner):
                f()
            e1.record()
            e1.synchronize()
            times[k].append(e0.elapsed_time(e1) / (inner if k in arms else args.launches))
    res = dict(device=torch.cuda.get_device_name(0), batch=B, frames=T, repeats=args.repeats, inner=args.inner,
               launches=args.launches, arms={k: _stats(v) for k, v in times.items()})
    if has_spsi:
        ratios = {}
        for n, hop in CASES:
            a = lambda k: res["arms"]["%d %s" % (n, k)]["ms_median"]
            per_iter = a("batch plain60") / 60
            ratios["%d spsi launch (speech) in plain iterations" % n] = a("spsi speech batch") / per_iter
            ratios["%d spsi launch (rand) in plain iterations" % n] = a("spsi rand batch") / per_iter
            for form in ("batch", "items"):
                ratios["%d %s spsi10/plain60" % (n, form)] = a("%s spsi10" % form) / a("%s plain60" % form)
                ratios["%d %s spsi30/zero30" % (n, form)] = a("%s spsi30" % form) / a("%s zero30" % form)
        res["ratios"] = ratios
        res["spectral_convergence_on_device"] = sc
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
    ap.add_argument("--launches", type=int, default=10)
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

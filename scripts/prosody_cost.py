# coding: utf-8
"""What speaking rate and pitch at vocoding cost.

  warp    the dv3_prosody_warp_f32 launch alone at 64 x 804 frames, 1024 / 256 (513 bins), speech-like magnitudes (the
          recipe of scripts/spsi_cost.py), into a preallocated buffer: `--launches` back to back between two device
          events, the cases alternating inside every repeat, after a warm-up.  Cases: (rate 1, +4 st), (rate 0.8, 0 st),
          (rate 0.8, +4 st), each with and without envelope preservation.  Bytes: the traffic the algorithm needs, two
          source rows read and one row written per output frame, 3 x 4 x 513 bytes x the output frames; bytes / time is
          the achieved rate and its share of the measured HBM copy rate (6.29 TB/s) the fraction of the roof -- the source
          rows of neighbouring output frames overlap, so the HBM itself sees less than this count.
          Beside it: the 60 plain Griffin-Lim iterations (per-item form, as the warped path runs them) on the same frames.
  synth   synthesis.tts_batch for 64 utterances of 201 decoder steps on deepvoice3_ljspeech with random weights and two
          Griffin-Lim iterations: no option, and rate 0.8 / +4 st on every utterance, alternating, host clock around each
          call, after one warm-up call of each.
  --parent-root DIR: a checkout of the parent commit with its library built.  The default path (audio.inv_spectrogram_batch
          with frame lengths, 60 plain iterations, no option) is measured by this same script in child processes
          (--default-only), alternating with child processes of this checkout, `--rounds` times each.

    python scripts/prosody_cost.py [--out profiles/prosody_cost.json] [--parent-root DIR]
"""
import argparse
import json
import os
import subprocess
import sys
import time

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N_FFT, HOP = 1024, 256
HBM_COPY_RATE = 6.29e12          # bytes/s, the measured float4 copy rate of the MI355X the roof fraction is quoted against


def summary(t):
    import numpy as np
    t = np.array(t)
    return dict(median=float(np.median(t)), min=float(t.min()), max=float(t.max()), n=int(t.size))


def speech_magnitudes(audio, dev, B, T):
    import math
    import torch
    L = audio.lws_num_samples(T, HOP, N_FFT)
    sr = 22050.0
    g = torch.Generator().manual_seed(3)
    t = (torch.arange(L, dtype=torch.float64, device=dev) / sr)[None, :]
    b = torch.arange(B, dtype=torch.float64, device=dev)[:, None]
    f0 = 110.0 + 2.0 * b + 40.0 * torch.sin(2 * math.pi * 1.5 * t + b)
    phi = 2 * math.pi * torch.cumsum(f0, dim=1) / sr
    voiced = sum(torch.sin(k * phi) / k for k in range(1, 20)) * (0.5 + 0.5 * torch.sin(2 * math.pi * 3 * t))
    y = (0.1 * (voiced + 0.05 * torch.randn(B, L, generator=g, dtype=torch.float64).to(dev))).float().contiguous()
    _, sp = audio.stft(y, T, HOP, want_phasor=False, want_spec=True, convention="lws", fft_size=N_FFT)
    return sp.norm(dim=-1).contiguous()


def time_events(cases, inner, repeats):
    """cases {name: fn}: every fn warmed, then `repeats` rounds over all of them, `inner` calls between two events
    -> {name: [ms per call]}"""
    import torch
    for fn in cases.values():
        fn()
    torch.cuda.synchronize()
    times = {k: [] for k in cases}
    for _ in range(repeats):
        for k, fn in cases.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(inner):
                fn()
            e1.record()
            e1.synchronize()
            times[k].append(e0.elapsed_time(e1) / inner)
    return times


def default_path(args, dev):
    """the call every synthesis ends in today: per-item frame counts, 60 plain iterations, no option"""
    import torch
    from deepvoice3_pytorch_amd import audio
    B, T = args.batch, args.frames
    cfg = audio.AudioConfig()
    lin = torch.rand(B, T, N_FFT // 2 + 1, generator=torch.Generator().manual_seed(0)).to(dev)
    times = time_events({"inv_spectrogram_batch items 60": lambda: audio.inv_spectrogram_batch(lin, cfg, frame_lengths=[T] * B)},
                        2, args.repeats)
    return {k: summary(v) for k, v in times.items()}


def time_warp(args, dev):
    import torch
    from deepvoice3_pytorch_amd import _lib, audio
    from deepvoice3_pytorch_amd.ops import _stream
    B, T, F = args.batch, args.frames, N_FFT // 2 + 1
    cfg = audio.AudioConfig()
    mag = speech_magnitudes(audio, dev, B, T)
    W = audio.Prosody().half_width(cfg)
    tin = torch.full((B,), T, dtype=torch.int32, device=dev)
    cases, shapes = {}, {}
    for rate, st in ((1.0, 4.0), (0.8, 0.0), (0.8, 4.0)):
        Tp = audio.warped_frames(T, rate, cfg)
        out = torch.empty((B, Tp, F), dtype=torch.float32, device=dev)
        tout = torch.full((B,), Tp, dtype=torch.int32, device=dev)
        r = torch.full((B,), rate, dtype=torch.float64, device=dev)
        q = torch.full((B,), 2.0 ** (st / 12.0), dtype=torch.float64, device=dev)
        for preserve in (1, 0):
            name = "rate %g, %+g st, %s" % (rate, st, "envelope" if preserve else "plain")

            def launch(out=out, tout=tout, r=r, q=q, Tp=Tp, preserve=preserve):
                _lib.call("dv3_prosody_warp_f32", mag.data_ptr(), out.data_ptr(), B, T, Tp, F, tin.data_ptr(),
                          tout.data_ptr(), r.data_ptr(), q.data_ptr(), W, preserve, _stream())
            cases[name] = launch
            shapes[name] = dict(frames_out=Tp, bytes=3 * 4 * F * B * Tp)
    times = time_events(cases, args.launches, args.repeats)
    res = {}
    for k, v in times.items():
        s = summary(v)
        rate = shapes[k]["bytes"] / (s["median"] * 1e-3)
        res[k] = dict(shapes[k], ms_per_launch=s, bytes_per_s=rate, fraction_of_hbm_copy_rate=rate / HBM_COPY_RATE)
    gl = time_events({"gl": lambda: audio.griffin_lim(mag, HOP, 60, None, "lws", None, tin, N_FFT)}, 1, args.repeats)
    gl60 = summary(gl["gl"])
    return dict(B=B, frames=T, bins=F, env_half_width=W, launches=args.launches, repeats=args.repeats, cases=res,
                griffin_lim_60_plain_items_ms=gl60,
                warp_share_of_griffin_lim={k: v["ms_per_launch"]["median"] / gl60["median"] for k, v in res.items()})


def time_synth(args, dev):
    import numpy as np
    import torch
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
        arms = {"off": {}, "rate 0.8, +4 st": dict(rate=0.8, semitones=4.0)}
        times = {k: [] for k in arms}
        samples = {}
        for i in range(args.repeats + 1):
            for k, kw in arms.items():
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                res = synthesis.tts_batch(model, seqs, audio_cfg=cfg, **kw)
                torch.cuda.synchronize()
                if i:                                   # the first call of each is the warm-up
                    times[k].append((time.perf_counter() - t0) * 1e3)
                samples[k] = int(res[0][3].numel())
        out = {k: summary(v) for k, v in times.items()}
        return dict(preset="deepvoice3_ljspeech", B=B, decoder_steps=int(res[0][2].shape[0]), griffin_lim_iters=2,
                    samples_of_item_0=samples, ms_per_call=out, added_ms=out["rate 0.8, +4 st"]["median"] - out["off"]["median"])
    finally:
        ops.set_gemm_precision(prev)


def child(root, args):
    cmd = [sys.executable, os.path.abspath(__file__), "--root", root, "--default-only", "--frames", str(args.frames),
           "--batch", str(args.batch), "--repeats", str(args.repeats)]
    out = subprocess.run(cmd, check=True, stdout=subprocess.PIPE, timeout=300).stdout.decode()
    return json.loads(out.strip().splitlines()[-1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--root", default=HERE, help="the checkout whose package is measured")
    ap.add_argument("--parent-root", default=None)
    ap.add_argument("--default-only", action="store_true")
    ap.add_argument("--frames", type=int, default=804)
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--launches", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--no-synth", action="store_true")
    args = ap.parse_args()
    sys.path.insert(0, os.path.abspath(args.root))
    processes = []
    if args.parent_root:                                  # before this process opens the device
        for _ in range(args.rounds):
            for name, root in (("parent", args.parent_root), ("this", args.root)):
                processes.append(dict(build=name, ms_per_call=child(root, args)["default_path"]))
    import torch
    assert torch.cuda.is_available(), "prosody_cost needs a GPU"
    dev = torch.device("cuda:0")
    with torch.no_grad():
        res = dict(device=torch.cuda.get_device_name(0), default_path=default_path(args, dev))
        if not args.default_only:
            res["warp"] = time_warp(args, dev)
            if not args.no_synth:
                res["synth"] = time_synth(args, dev)
    if processes:
        res["default_path_by_process"] = processes
    line = json.dumps(res, sort_keys=True)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()

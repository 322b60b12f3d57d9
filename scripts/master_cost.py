# coding: utf-8
"""What deliverable audio costs.

  kernels the three entry points of csrc/master.hip alone at 64 items of audio.num_samples(804, 256, "lws") samples each
          (a padded batch, speech-level noise), into preallocated buffers: `--launches` back to back between two device
          events, the cases alternating inside every repeat, after a warm-up (so a figure holds the launch gaps of a
          back-to-back queue, not the kernel alone).  levels = dv3_wave_levels_f32 (its two launches); gains =
          dv3_wave_gains_f32; master = dv3_wave_master_f32 as audio.master_items lays it out (every item in place) in
          int16, int16 with dither and float32, and as a DOCUMENT (the 64 items crossfaded over 110 samples, int16).
          Floor: the bytes the algorithm needs -- 4 per sample read, 2 or 4 written; the level rows, tables and fades
          are noise -- over the part's peak HBM bandwidth (8.0 TB/s, MI355X_MICROARCH); also quoted against the measured
          copy rate (6.29 TB/s).  Beside them: 60 plain Griffin-Lim iterations (per-item form) on the same batch.
  synth   synthesis.tts_batch for 64 utterances of 201 decoder steps on deepvoice3_ljspeech with random weights and two
          Griffin-Lim iterations: no option, and mastering=Mastering("rms"), alternating, host clock around each call,
          after one warm-up call of each.
  --parent-root DIR: a checkout of the parent commit with its library built.  The default path
          (audio.inv_spectrogram_batch with frame lengths, 60 plain iterations, no option) is measured by this same script
          in child processes (--default-only), alternating with child processes of this checkout, `--rounds` times each.

    python scripts/master_cost.py [--out profiles/master_cost.json] [--parent-root DIR]
"""
import argparse
import json
import os
import subprocess
import sys
import time

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N_FFT, HOP = 1024, 256
HBM_PEAK = 8.0e12                # bytes/s, the part's specified peak: the floor is bytes over this
HBM_COPY_RATE = 6.29e12          # bytes/s, the measured float4 copy rate of the MI355X


def summary(t):
    import numpy as np
    t = np.array(t)
    return dict(median=float(np.median(t)), min=float(t.min()), max=float(t.max()), n=int(t.size))


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


def time_kernels(args, dev):
    import numpy as np
    import torch
    from deepvoice3_pytorch_amd import _lib, audio
    from deepvoice3_pytorch_amd.ops import _stream
    from deepvoice3_pytorch_amd.synthesis import plan_document
    C = _lib.CONSTS
    B, T = args.batch, args.frames
    L = audio.num_samples(T, HOP, "lws", N_FFT)
    Lp = -(-L // 8) * 8
    x = (0.1 * torch.randn(B * L, generator=torch.Generator().manual_seed(1))).to(dev)
    i64 = lambda v: torch.from_numpy(np.asarray(v, dtype=np.int64)).to(dev)
    starts, lens = i64(np.arange(B) * L), i64(np.full(B, L))
    nchunk = -(-L // C["DV3_LEVELS_CHUNK"])
    scratch = torch.empty(B * nchunk * 5, dtype=torch.float64, device=dev)
    levels = torch.empty((B, 5), dtype=torch.float64, device=dev)
    goff = torch.arange(B + 1, dtype=torch.int32, device=dev)
    gain = torch.empty(B, dtype=torch.float32, device=dev)
    flags0 = torch.zeros(B, dtype=torch.int32, device=dev)
    F = 110
    table, N_doc = plan_document(np.full(B, L), 22050, 0.0, F, starts=np.arange(B) * L)
    doc = dict(src=i64(table["src"]), len=i64(table["len"]), dst=i64(table["dst"]),
               flags=torch.from_numpy(table["flags"]).to(dev), fade=audio.fade_table(dev, F))
    out16 = torch.empty(B * Lp, dtype=torch.int16, device=dev)
    out32 = torch.empty(B * Lp, dtype=torch.float32, device=dev)
    dst_items = i64(np.arange(B) * Lp)

    def k_levels():
        _lib.call("dv3_wave_levels_f32", x.data_ptr(), starts.data_ptr(), lens.data_ptr(), B, L, scratch.data_ptr(),
                  levels.data_ptr(), _stream())

    def k_gains():
        _lib.call("dv3_wave_gains_f32", levels.data_ptr(), lens.data_ptr(), goff.data_ptr(), B, B, C["DV3_GAIN_RMS"], 0.1,
                  0.89, 31.6, gain.data_ptr(), _stream())

    def k_master(mode, dither, out, N, doc_layout=False):
        def fn():
            if doc_layout:
                _lib.call("dv3_wave_master_f32", x.data_ptr(), doc["src"].data_ptr(), doc["len"].data_ptr(),
                          doc["dst"].data_ptr(), gain.data_ptr(), doc["flags"].data_ptr(), B, doc["fade"].data_ptr(), F,
                          mode, dither, 7, out.data_ptr(), N, _stream())
            else:
                _lib.call("dv3_wave_master_f32", x.data_ptr(), starts.data_ptr(), lens.data_ptr(), dst_items.data_ptr(),
                          gain.data_ptr(), flags0.data_ptr(), B, None, 0, mode, dither, 7, out.data_ptr(), N, _stream())
        return fn

    n = B * L
    cases = {"levels": k_levels, "gains": k_gains,
             "master items int16": k_master(C["DV3_MASTER_I16"], 0, out16, B * Lp),
             "master items int16 dither": k_master(C["DV3_MASTER_I16"], 1, out16, B * Lp),
             "master items float32": k_master(C["DV3_MASTER_F32"], 0, out32, B * Lp),
             "master items int16 reference": k_master(C["DV3_MASTER_I16_REFERENCE"], 0, out16, B * Lp),
             "master document int16": k_master(C["DV3_MASTER_I16"], 0, out16, N_doc, True)}
    need = {"levels": 4 * n, "gains": B * (5 * 8 + 8 + 4), "master items int16": 4 * n + 2 * B * Lp,
            "master items int16 dither": 4 * n + 2 * B * Lp, "master items float32": 4 * n + 4 * B * Lp,
            "master items int16 reference": 4 * n + 2 * B * Lp, "master document int16": 4 * n + 2 * N_doc}
    k_levels()
    k_gains()
    times = time_events(cases, args.launches, args.repeats)
    res = {}
    for k, v in times.items():
        s = summary(v)
        floor_ms = need[k] / HBM_PEAK * 1e3
        rate = need[k] / (s["median"] * 1e-3)
        res[k] = dict(bytes=need[k], ms_per_launch=s, floor_ms=floor_ms, times_floor=s["median"] / floor_ms,
                      bytes_per_s=rate, fraction_of_hbm_copy_rate=rate / HBM_COPY_RATE)
    mag = torch.rand(B, T, N_FFT // 2 + 1, generator=torch.Generator().manual_seed(2)).to(dev)
    tin = torch.full((B,), T, dtype=torch.int32, device=dev)
    gl = time_events({"gl": lambda: audio.griffin_lim(mag, HOP, 60, None, "lws", None, tin, N_FFT)}, 1, args.repeats)
    gl60 = summary(gl["gl"])
    three = sum(res[k]["ms_per_launch"]["median"] for k in ("levels", "gains", "master items int16"))
    return dict(B=B, frames=T, samples_per_item=L, launches=args.launches, repeats=args.repeats, hbm_peak=HBM_PEAK,
                hbm_copy_rate=HBM_COPY_RATE, cases=res, griffin_lim_60_plain_items_ms=gl60,
                levels_gains_master_ms=three, share_of_griffin_lim=three / gl60["median"])


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
        arms = {"off": {}, "mastering rms int16": dict(mastering=audio.Mastering("rms"))}
        times = {k: [] for k in arms}
        for i in range(args.repeats + 1):
            for k, kw in arms.items():
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                res = synthesis.tts_batch(model, seqs, audio_cfg=cfg, **kw)
                torch.cuda.synchronize()
                if i:                                   # the first call of each is the warm-up
                    times[k].append((time.perf_counter() - t0) * 1e3)
        out = {k: summary(v) for k, v in times.items()}
        return dict(preset="deepvoice3_ljspeech", B=B, decoder_steps=int(res[0][2].shape[0]), griffin_lim_iters=2,
                    samples_of_item_0=int(res[0][3].numel()), ms_per_call=out,
                    added_ms=out["mastering rms int16"]["median"] - out["off"]["median"])
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
    assert torch.cuda.is_available(), "master_cost needs a GPU"
    dev = torch.device("cuda:0")
    with torch.no_grad():
        res = dict(device=torch.cuda.get_device_name(0), default_path=default_path(args, dev))
        if not args.default_only:
            res["kernels"] = time_kernels(args, dev)
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

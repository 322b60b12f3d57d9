# coding: utf-8
"""What the look-ahead limiter costs.

  kernels dv3_wave_limit_f32 alone at 64 items of 205056 samples each at 22.05 kHz (a padded batch, speech-level noise
          times a pre-gain under which one sample in a hundred passes the ceiling, three under the true-peak detector --
          the report's over_fraction is the last call's --), look-ahead 33 samples, release
          50 ms, into preallocated tables: `--launches` calls back to back between two device events, the cases
          alternating inside every repeat, after a warm-up (so a figure holds the launch gaps of a back-to-back queue,
          not the kernels alone).  limit = the four launches under the sample-peak detector; limit true peak = the same
          under the true-peak one; beside them what a further pass adds (dv3_wave_loudness_f64 without a peak table, the
          re-aim's measure) and what the true-peak trim adds (the same call with the table).
          Floor: the bytes a pass must move over the part's peak HBM bandwidth (8.0 TB/s) -- for the limiter one read of
          the samples and one write of the output, 8 per sample (the kernels move 28: pass A reads 4 and stores dq_local,
          8; pass C reads both again and writes 4).
  synth   synthesis.tts_batch for 64 utterances of 201 decoder steps on deepvoice3_ljspeech with random weights and two
          Griffin-Lim iterations: Mastering("lufs") against Mastering("lufs", limiter=Limiter()), and the same pair under
          true_peak=True, alternating in one process, host clock around each call, after one warm-up call of each.
  --parent-root DIR: a checkout of the parent commit with its library built.  The default path
          (audio.inv_spectrogram_batch with frame lengths, 60 plain iterations, no option) is measured by this same script
          in child processes (--default-only), alternating with child processes of this checkout, `--rounds` times each.

    python scripts/limiter_cost.py [--out profiles/limiter_cost.json] [--parent-root DIR]
"""
import argparse
import ctypes
import json
import os
import subprocess
import sys
import time

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N_FFT, HOP = 1024, 256
HBM_PEAK = 8.0e12                # bytes/s, the part's specified peak: the floor is bytes over this
SAMPLE_RATE = 22050


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
    C = _lib.CONSTS
    B, L = args.batch, args.samples
    x = (0.1 * torch.randn(B * L, generator=torch.Generator().manual_seed(1))).to(dev)
    i64 = lambda v: torch.from_numpy(np.asarray(v, dtype=np.int64)).to(dev)
    starts, lens = i64(np.arange(B) * L), i64(np.full(B, L))
    lim = audio.Limiter()
    A, rho = lim.lookahead(SAMPLE_RATE), lim.rho(SAMPLE_RATE)
    T = C["DV3_LIMIT_TILE"]
    f64 = dict(dtype=torch.float64, device=dev)
    ceiling = 10.0 ** (-1.0 / 20.0)
    gain = torch.full((B,), float(ceiling / (0.1 * 2.576)), dtype=torch.float32, device=dev)    # 1 % of a normal's samples
    scratch = torch.empty(B * -(-L // T) * (T + 3), **f64)
    out, report = torch.empty_like(x), torch.empty((B, 2), **f64)
    powers = (ctypes.c_double * C["DV3_LIMIT_RHO_POWERS"])(*audio.rho_powers(rho).tolist())
    table = (ctypes.c_float * 36)(*audio.true_peak_table().reshape(-1).tolist())
    kw = audio.k_weighting(SAMPLE_RATE)
    h = kw["h"]
    K = -(-L // h)
    coef = (ctypes.c_double * 10)(*kw["coef"].tolist())
    Ah = (ctypes.c_double * 16)(*kw["Ah"].reshape(-1).tolist())
    states, energy = torch.empty((B, K, 4), **f64), torch.empty((B, K), **f64)
    tp, tp_scratch = torch.empty(B, **f64), torch.empty(B * -(-L // C["DV3_TRUE_PEAK_CHUNK"]), **f64)

    def k_limit(with_peak):
        def fn():
            _lib.call("dv3_wave_limit_f32", x.data_ptr(), starts.data_ptr(), lens.data_ptr(), B, L, gain.data_ptr(),
                      ceiling, A, ctypes.addressof(powers), ctypes.addressof(table) if with_peak else None,
                      scratch.data_ptr(), out.data_ptr(), report.data_ptr(), _stream())
        return fn

    def k_loudness(with_peak):
        def fn():
            _lib.call("dv3_wave_loudness_f64", out.data_ptr(), starts.data_ptr(), lens.data_ptr(), B, L, h,
                      ctypes.addressof(coef), ctypes.addressof(Ah), ctypes.addressof(table) if with_peak else None,
                      states.data_ptr(), energy.data_ptr(), tp_scratch.data_ptr() if with_peak else None,
                      tp.data_ptr() if with_peak else None, _stream())
        return fn

    n = B * L
    cases = {"limit": k_limit(False), "limit true peak": k_limit(True), "loudness of a further pass": k_loudness(False),
             "loudness with true peak of the trim": k_loudness(True)}
    need = {"limit": 8 * n, "limit true peak": 8 * n, "loudness of a further pass": 2 * 4 * n,
            "loudness with true peak of the trim": 3 * 4 * n}
    times = time_events(cases, args.launches, args.repeats)
    res = {}
    for k, v in times.items():
        s = summary(v)
        floor_ms = need[k] / HBM_PEAK * 1e3
        res[k] = dict(bytes=need[k], ms_per_call=s, floor_ms=floor_ms, times_floor=s["median"] / floor_ms)
    torch.cuda.synchronize()
    rep = report.cpu().numpy()
    return dict(B=B, samples_per_item=L, sample_rate=SAMPLE_RATE, lookahead=A, rho=rho, launches=args.launches,
                repeats=args.repeats, hbm_peak=HBM_PEAK, bytes_moved_per_sample=28, cases=res,
                over_fraction=float(rep[:, 1].sum() / n), gain_min=float(rep[:, 0].min()))


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
        lim = audio.Limiter()
        arms = {"lufs": audio.Mastering("lufs", target_db=-16.0), "lufs limiter": audio.Mastering("lufs", target_db=-16.0, limiter=lim),
                "lufs true peak": audio.Mastering("lufs", target_db=-16.0, true_peak=True),
                "lufs true peak limiter": audio.Mastering("lufs", target_db=-16.0, true_peak=True, limiter=lim)}
        times = {k: [] for k in arms}
        for i in range(args.repeats + 1):
            for k, m in arms.items():
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                res = synthesis.tts_batch(model, seqs, audio_cfg=cfg, mastering=m)
                torch.cuda.synchronize()
                if i:                                   # the first call of each is the warm-up
                    times[k].append((time.perf_counter() - t0) * 1e3)
        out = {k: summary(v) for k, v in times.items()}
        return dict(preset="deepvoice3_ljspeech", B=B, decoder_steps=int(res[0][2].shape[0]), griffin_lim_iters=2,
                    samples_of_item_0=int(res[0][3].numel()), sample_rate=cfg.sample_rate, ms_per_call=out,
                    limiter_minus_lufs_ms=out["lufs limiter"]["median"] - out["lufs"]["median"],
                    true_peak_limiter_minus_lufs_true_peak_ms=out["lufs true peak limiter"]["median"]
                    - out["lufs true peak"]["median"])
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
    ap.add_argument("--samples", type=int, default=205056)
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--launches", type=int, default=10)
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
    assert torch.cuda.is_available(), "limiter_cost needs a GPU"
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

# coding: utf-8
"""What prosody marks cost.

  warp    dv3_curve_warp_f32 against dv3_prosody_warp_f32 on IDENTICAL work: pos = j * rate, a constant ratio, gain 1, at
          64 x 804 frames, 1024 / 256 (513 bins), the three cases of scripts/prosody_cost.py in both envelope modes --
          same process, the two entry points alternating inside every repeat, `--launches` back to back between two
          device events, after a warm-up.  The tables add 20 bytes to the 6 KB a frame moves.
  plan    the dv3_curve_plan_f64 and dv3_curve_fill_f64 launches alone, 64 items of 9 segments with a break and a ramp.
  synth   synthesis.tts_batch for 64 utterances of 201 decoder steps on deepvoice3_ljspeech with random weights and two
          Griffin-Lim iterations: no option, and marks on every utterance (two spans, one break, a transition),
          alternating, host clock around each call, after one warm-up call of each.  The marks of an utterance without
          an admissible monotonic path are not applied (its plan is neutral, the launches are the same); the count of such
          utterances is reported.
  --parent-root DIR: a checkout of the parent commit with its library built.  The default path (audio.inv_spectrogram_batch
          with frame lengths, 60 plain iterations, no option) is measured by scripts/prosody_cost.py --default-only in child
          processes of the two checkouts, alternating, `--rounds` times each.

    python scripts/prosody_curve_cost.py [--out profiles/prosody_curve_cost.json] [--parent-root DIR]
"""
import argparse
import json
import os
import subprocess
import sys
import time
import warnings

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from prosody_cost import HBM_COPY_RATE, N_FFT, speech_magnitudes, summary, time_events  # noqa: E402


def time_warps(args, dev):
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
        pos = (torch.arange(Tp, dtype=torch.float64, device=dev)[None, :] * r[:, None]).contiguous()
        qt = q[:, None].expand(B, Tp).contiguous()
        gain = torch.ones((B, Tp), dtype=torch.float32, device=dev)
        for preserve in (1, 0):
            name = "rate %g, %+g st, %s" % (rate, st, "envelope" if preserve else "plain")

            def scalar(out=out, tout=tout, r=r, q=q, Tp=Tp, preserve=preserve):
                _lib.call("dv3_prosody_warp_f32", mag.data_ptr(), out.data_ptr(), B, T, Tp, F, tin.data_ptr(),
                          tout.data_ptr(), r.data_ptr(), q.data_ptr(), W, preserve, _stream())

            def curve(out=out, tout=tout, pos=pos, qt=qt, gain=gain, Tp=Tp, preserve=preserve):
                _lib.call("dv3_curve_warp_f32", mag.data_ptr(), out.data_ptr(), B, T, Tp, F, tin.data_ptr(),
                          tout.data_ptr(), pos.data_ptr(), qt.data_ptr(), gain.data_ptr(), W, preserve, _stream())
            cases[name + " | scalar"], cases[name + " | curve"] = scalar, curve
            shapes[name] = dict(frames_out=Tp, bytes=3 * 4 * F * B * Tp)
    times = time_events(cases, args.launches, args.repeats)
    res = {}
    for name, shape in shapes.items():
        s, c = summary(times[name + " | scalar"]), summary(times[name + " | curve"])
        rate = shape["bytes"] / (c["median"] * 1e-3)
        res[name] = dict(shape, scalar_ms=s, curve_ms=c, curve_over_scalar=c["median"] / s["median"], curve_bytes_per_s=rate,
                         curve_fraction_of_hbm_copy_rate=rate / HBM_COPY_RATE)
    return dict(B=B, frames=T, bins=F, env_half_width=W, launches=args.launches, repeats=args.repeats, cases=res)


def time_plan(args, dev):
    import numpy as np
    import torch
    from deepvoice3_pytorch_amd import _lib, audio
    from deepvoice3_pytorch_amd.ops import _stream
    B, T = args.batch, args.frames
    cfg = audio.AudioConfig()
    marks = [audio.ProsodyMarks(spans=[(100 * k + b % 50, 100 * k + 60, dict(rate=0.8 + 0.1 * (k % 3), semitones=float(k - 2)))
                                       for k in range(4)], breaks=[(259, 0.3)], units="frames", transition_ms=35.0)
             for b in range(B)]
    plan = audio.plan_prosody(None, [T] * B, marks, cfg)
    t = audio.marks_tables(marks, cfg)
    S, T_out = t["rate"].shape[1], int(plan["pos"].shape[1])
    put = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a)).to(dt).to(dev)
    bounds = put(np.minimum(t["start"], T), torch.int32)
    semi, db = put(t["semitones"], torch.float64), put(t["gain_db"], torch.float64)
    o, tout = torch.empty_like(plan["o"]), torch.empty_like(plan["tlen_out"])
    pos, ratio, gain = torch.empty_like(plan["pos"]), torch.empty_like(plan["ratio"]), torch.empty_like(plan["gain"])
    R = marks[0].ramp_frames(cfg)

    def run_plan():
        _lib.call("dv3_curve_plan_f64", plan["tlen_in"].data_ptr(), B, T, S, plan["nseg"].data_ptr(), bounds.data_ptr(),
                  plan["rate"].data_ptr(), plan["break_frames"].data_ptr(), 4, o.data_ptr(), tout.data_ptr(), _stream())

    def run_fill():
        _lib.call("dv3_curve_fill_f64", plan["tlen_in"].data_ptr(), B, T, S, plan["nseg"].data_ptr(), bounds.data_ptr(),
                  plan["rate"].data_ptr(), semi.data_ptr(), db.data_ptr(), plan["break_frames"].data_ptr(),
                  plan["o"].data_ptr(), plan["tlen_out"].data_ptr(), T_out, R, pos.data_ptr(), ratio.data_ptr(), gain.data_ptr(),
                  _stream())
    times = time_events({"plan": run_plan, "fill": run_fill}, args.launches, args.repeats)
    assert torch.equal(pos, plan["pos"]) and torch.equal(o, plan["o"])
    return dict(B=B, segments=S, frames_out=T_out, ramp_frames=R, plan_ms=summary(times["plan"]), fill_ms=summary(times["fill"]))


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
        marks = [audio.ProsodyMarks(spans=[(5, 20, dict(rate=0.8, semitones=2.0)), (30, 40, dict(gain_db=3.0, semitones=-2.0))],
                                    breaks=[(19, 0.3)], transition_ms=35.0) for _ in seqs]
        arms = {"off": {}, "marks": dict(marks=marks)}
        times = {k: [] for k in arms}
        samples, lost = {}, 0
        for i in range(args.repeats + 1):
            for k, kw in arms.items():
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                with warnings.catch_warnings(record=True) as caught:
                    warnings.simplefilter("always")
                    res = synthesis.tts_batch(model, seqs, audio_cfg=cfg, **kw)
                torch.cuda.synchronize()
                if i:                                   # the first call of each is the warm-up
                    times[k].append((time.perf_counter() - t0) * 1e3)
                samples[k] = int(res[0][3].numel())
                if k == "marks":
                    lost = sum(str(w.message).count(",") + 1 for w in caught if issubclass(w.category, audio.MarksNotApplied))
        out = {k: summary(v) for k, v in times.items()}
        return dict(preset="deepvoice3_ljspeech", B=B, decoder_steps=int(res[0][2].shape[0]), griffin_lim_iters=2,
                    utterances_without_a_path=lost, samples_of_item_0=samples, ms_per_call=out,
                    added_ms=out["marks"]["median"] - out["off"]["median"])
    finally:
        ops.set_gemm_precision(prev)


def child(root, args):
    """scripts/prosody_cost.py --default-only of THIS checkout, measuring the package under `root`"""
    cmd = [sys.executable, os.path.join(HERE, "scripts", "prosody_cost.py"), "--root", root, "--default-only",
           "--frames", str(args.frames), "--batch", str(args.batch), "--repeats", str(args.repeats)]
    out = subprocess.run(cmd, check=True, stdout=subprocess.PIPE, timeout=300).stdout.decode()
    return json.loads(out.strip().splitlines()[-1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--parent-root", default=None)
    ap.add_argument("--frames", type=int, default=804)
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--launches", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--no-synth", action="store_true")
    args = ap.parse_args()
    sys.path.insert(0, HERE)
    processes = []
    if args.parent_root:                                  # before this process opens the device
        for _ in range(args.rounds):
            for name, root in (("parent", os.path.abspath(args.parent_root)), ("this", HERE)):
                processes.append(dict(build=name, ms_per_call=child(root, args)["default_path"]))
    import torch
    assert torch.cuda.is_available(), "prosody_curve_cost needs a GPU"
    dev = torch.device("cuda:0")
    with torch.no_grad():
        res = dict(device=torch.cuda.get_device_name(0), warp=time_warps(args, dev), plan=time_plan(args, dev))
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

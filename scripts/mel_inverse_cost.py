# coding: utf-8
"""What vocoding from a mel costs.  One process:

  kernel  audio.mel_to_linear at B = 64, T = 201 mel frames, upsample 4 (64 x 804 output frames), 80 bands, fft_size 1024,
          125 .. 7600 Hz, speech-like random mel, at 16, 32 and 64 iterations: a queue of `--calls` calls between two
          device events, the cases alternating inside every repeat, after a warm-up; median, minimum and maximum per
          call, and the fused multiply-adds per second that is (2 iters nnz(W) per frame, the two products of an update).
  invert  audio.inv_spectrogram_batch (60 Griffin-Lim iterations, the default AudioConfig) on the 64 x 804 frames the
          32-iteration call made, timed the same way in the same process: what the inversion is added to.
  synth   synthesis.tts_batch for 64 utterances of 201 decoder steps (min = max decoder steps = 200) on
          deepvoice3_ljspeech with random weights and two Griffin-Lim iterations, with from_mel=False and from_mel=True
          alternating, host clock around each call (a call ends in device reads), after one warm-up call of each.

    python scripts/mel_inverse_cost.py [--out FILE] [--calls 10] [--repeats 7] [--kernel-only]
(--kernel-only: a few calls of each kernel case and nothing else, for a kernel trace.)
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

ITERS = (16, 32, 64)


def summary(t):
    t = np.array(t)
    return dict(median=float(np.median(t)), min=float(t.min()), max=float(t.max()), n=int(t.size))


def kernel_cases(dev):
    from deepvoice3_pytorch_amd import audio
    B, T, M, u = 64, 201, 80, 4
    cfg = audio.AudioConfig()
    rng = np.random.RandomState(0)
    # a smooth envelope over the bands plus frame-to-frame movement, in [0, 1]
    env = 0.55 + 0.25 * np.sin(np.linspace(0, 3 * np.pi, M))[None, None, :]
    mel = np.clip(env + 0.1 * rng.randn(B, T, 1) + 0.05 * rng.randn(B, T, M), 0, 1).astype(np.float32)
    x = torch.from_numpy(mel).to(dev)
    cases = {"iters%d" % n: (lambda n=n: audio.mel_to_linear(x, cfg, None, u, audio.MelInverse(iters=n))) for n in ITERS}
    nnz = int(np.count_nonzero(audio.mel_basis(cfg.sample_rate, cfg.fft_size, M)))
    shape = dict(B=B, T=T, n_mels=M, upsample=u, fft_size=cfg.fft_size, frames=B * T * u, basis_nonzeros=nnz)
    return cases, shape, cfg


def timed(cases, calls, repeats):
    for fn in cases.values():
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    times = {k: [] for k in cases}
    for _ in range(repeats):
        for k, fn in cases.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(calls):
                fn()
            e1.record()
            e1.synchronize()
            times[k].append(e0.elapsed_time(e1) / calls)
    return {k: summary(v) for k, v in times.items()}


def time_kernel(dev, calls, repeats):
    from deepvoice3_pytorch_amd import audio
    cases, shape, cfg = kernel_cases(dev)
    lin = cases["iters32"]()
    cases["inv_spectrogram_batch"] = lambda: audio.inv_spectrogram_batch(lin, cfg)
    ms = timed(cases, calls, repeats)
    gfma = {k: 2.0 * n * shape["basis_nonzeros"] * shape["frames"] / (ms["iters%d" % n]["median"] * 1e-3) / 1e9
            for k, n in (("iters%d" % n, n) for n in ITERS)}
    return dict(shape, calls=calls, repeats=repeats, griffin_lim_iters=cfg.griffin_lim_iters, ms_per_call=ms,
                gfma_per_s=gfma)


def time_synth(dev, repeats):
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
        times = {False: [], True: []}
        for i in range(repeats + 1):
            for on in (False, True):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                res = synthesis.tts_batch(model, seqs, audio_cfg=cfg, from_mel=on)
                torch.cuda.synchronize()
                if i:                                   # the first call of each is the warm-up
                    times[on].append((time.perf_counter() - t0) * 1e3)
        off, on = summary(times[False]), summary(times[True])
        return dict(preset="deepvoice3_ljspeech", B=B, decoder_steps=int(res[0][2].shape[0]),
                    mel_frames=int(res[0][0].shape[0]), linear_frames=int(res[0][1].shape[0]),
                    upsample=synthesis.postnet_upsampling(model), griffin_lim_iters=2,
                    ms_per_call=dict(from_mel_off=off, from_mel_on=on), added_ms=on["median"] - off["median"])
    finally:
        ops.set_gemm_precision(prev)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--kernel-only", action="store_true")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "mel_inverse_cost needs a GPU"
    dev = torch.device("cuda:0")
    with torch.no_grad():
        if args.kernel_only:
            cases, _, _ = kernel_cases(dev)
            for fn in cases.values():
                for _ in range(3):
                    fn()
            torch.cuda.synchronize()
            return
        res = dict(device=torch.cuda.get_device_name(0), kernel=time_kernel(dev, args.calls, args.repeats),
                   synth=time_synth(dev, args.repeats))
    line = json.dumps(res, sort_keys=True)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()

# coding: utf-8
"""Rolling admission against rigid waves: deepvoice3_ljspeech at preset width, random weights, f16x3,
256 utterances whose decoder steps are drawn from the LJSpeech-shaped distribution of SURVEY 8d cfg2 (seed 1234); the
done flag is out of the stop rule (min_decoder_steps = the decoder's maximum), every utterance stops at its own cap.

  waves     synthesis.tts_batch in waves of 64.  tts_batch has no per-request cap: a wave's decoder maximum is set to
            the wave's largest cap and EVERY item of the wave runs (and is converted and inverted) to it -- the decode
            loop's length is what a wave costs either way, the post-net and Griffin-Lim work of a wave is overstated;
  rolling   synthesis.tts_stream with 64 slots, chunks of 8 steps, per-request caps.
Arms interleaved, median of 5 after one warm-up of each.  `decode_only` repeats both without post-net and Griffin-Lim
(waves: encoder + Decoder.incremental_forward(text_lengths=) per wave; rolling: admission + decode steps, retirement
only frees the slots).  `step_slope_ms`: the decoder loop's cost per step by slope between 50 and 150 fixed steps, 64
items -- slot mode with all 64 slots admitted at step 0 against the per-utterance launched loop.
Usage: python scripts/rolling_synth_ab.py [out.json]"""
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    import bench
    from deepvoice3_pytorch_amd import audio, builder, ops, synthesis
    from deepvoice3_pytorch_amd.decode_program import cfg2_step_counts, simulate_rolling, simulate_waves
    dev = torch.device("cuda:0")
    ops.set_gemm_precision("f16x3")
    hp = dict(bench.DV3_LJ)
    torch.manual_seed(0)
    model = builder.deepvoice3(**hp).to(dev).eval()
    model.make_generation_fast_()
    dec = model.seq2seq.decoder
    N, SLOTS, CHUNK, CAP = 256, 64, 8, 220
    steps = cfg2_step_counts(N, 1234)                    # decoder steps per utterance; cap = steps - 1
    caps = [s - 1 for s in steps]
    rng = np.random.RandomState(1234)
    lens = rng.randint(20, 101, N).tolist()
    seqs = [rng.randint(2, hp["n_vocab"], s).tolist() for s in lens]
    cfg = audio.AudioConfig(griffin_lim_iters=60)
    sec_per_step = hp["r"] * hp["downsample_step"] * 256 / 22050.0
    audio_s = sum(steps) * sec_per_step

    def waves():
        n = 0
        for i in range(0, N, SLOTS):
            dec.min_decoder_steps = dec.max_decoder_steps = max(caps[i:i + SLOTS])
            n += len(synthesis.tts_batch(model, seqs[i:i + SLOTS], audio_cfg=cfg))
        return n

    def rolling():
        dec.min_decoder_steps = dec.max_decoder_steps = CAP
        return sum(1 for _ in synthesis.tts_stream(model, seqs, slots=SLOTS, max_text_len=100, audio_cfg=cfg, chunk=CHUNK,
                                                   max_decoder_steps=caps))

    def waves_decode():
        for i in range(0, N, SLOTS):
            dec.min_decoder_steps = dec.max_decoder_steps = max(caps[i:i + SLOTS])
            ls = lens[i:i + SLOTS]
            Tt = max(ls)
            text = torch.zeros(len(ls), Tt, dtype=torch.long)
            for b, s in enumerate(seqs[i:i + SLOTS]):
                text[b, :len(s)] = torch.as_tensor(s)
            text = text.to(dev)
            pos = torch.arange(1, Tt + 1, device=dev)[None].expand(len(ls), Tt)
            tpos = torch.where(pos <= torch.tensor(ls, device=dev)[:, None], pos, torch.zeros_like(pos))
            prev, ops.valid = ops.valid, ops.ItemLengths(ls, Tt, dev)
            try:
                with torch.no_grad():
                    mem = model.seq2seq.encoder(text)
                    dec.start_fresh_sequence()
                    dec.incremental_forward(mem, tpos, text_lengths=ls)
            finally:
                ops.valid = prev

    class DecodeOnly(synthesis.RollingSynthesizer):
        def _retire(self, retired):
            self.prog.release([s for _, s, _ in retired])
            for t, _, _ in retired:
                del self._req[t]
            return [(t,) for t, _, _ in retired]

    def rolling_decode():
        dec.min_decoder_steps = dec.max_decoder_steps = CAP
        rs = DecodeOnly(model, slots=SLOTS, max_text_len=100, chunk=CHUNK)
        for s, c in zip(seqs, caps):
            rs.submit(s, max_decoder_steps=c)
        n = sum(1 for _ in rs.drain())
        return n, rs.schedule.steps

    def wall(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        return time.perf_counter() - t0, out

    def ab(fa, fb, reps=5):
        fa(), fb()                                       # warm-up: weight packs, FFT plans, allocator
        ta, tb = [], []
        for _ in range(reps):                            # interleaved
            ta.append(wall(fa)[0])
            tb.append(wall(fb)[0])
        return ta, tb

    res = {"measured_on": "MI355X (gfx950), one GPU, one process", "preset": "deepvoice3_ljspeech", "gemm": "f16x3",
           "utterances": N, "slots": SLOTS, "chunk": CHUNK, "seed": 1234, "text_lengths": "20..100 uniform",
           "griffin_lim_iters": cfg.griffin_lim_iters, "audio_s": audio_s,
           "item_steps": dict(min=min(steps), max=max(steps), mean=sum(steps) / N)}
    sim_roll, _ = simulate_rolling(steps, SLOTS, CHUNK)
    res["simulation"] = dict(rolling_steps=sim_roll, wave_steps=simulate_waves(steps, SLOTS),
                             step_ratio=sim_roll / simulate_waves(steps, SLOTS))
    assert waves() == N and rolling() == N
    ta, tb = ab(waves, rolling)
    for name, ts in (("waves", ta), ("rolling", tb)):
        w = float(np.median(ts))
        res[name] = dict(wall_s=w, wall_s_all=ts, utterances_per_s=N / w, rtf=w / audio_s)
    res["waves"]["note"] = "every item of a wave runs to the wave's largest cap (tts_batch has no per-request cap)"
    res["waves"]["audio_s_run_to_wave_maxima"] = sum((max(caps[i:i + SLOTS]) + 1) * len(caps[i:i + SLOTS])
                                                  for i in range(0, N, SLOTS)) * sec_per_step
    n, executed = rolling_decode()
    assert n == N and executed == sim_roll, (n, executed, sim_roll)
    ta, tb = ab(waves_decode, rolling_decode)
    res["decode_only"] = dict(waves_s=float(np.median(ta)), rolling_s=float(np.median(tb)), waves_s_all=ta, rolling_s_all=tb,
                              rolling_steps_executed=executed)
    # per-step cost by slope, 64 items
    ls = lens[:SLOTS]
    Tt = max(ls)
    text = torch.zeros(SLOTS, Tt, dtype=torch.long)
    for b, s in enumerate(seqs[:SLOTS]):
        text[b, :len(s)] = torch.as_tensor(s)
    text = text.to(dev)
    pos = torch.arange(1, Tt + 1, device=dev)[None].expand(SLOTS, Tt)
    tpos = torch.where(pos <= torch.tensor(ls, device=dev)[:, None], pos, torch.zeros_like(pos))
    with torch.no_grad():
        mem = model.seq2seq.encoder(text)
    dec.min_decoder_steps = dec.max_decoder_steps = CAP
    P = dec.slot_program(SLOTS, 100)
    slope = {}
    for name in ("slots", "per_utterance_launched"):
        ts = {}
        for n in (50, 150):
            if name == "slots":
                def run():
                    P.admit(list(range(SLOTS)), mem, tpos, ls)
                    P.run_steps(n)
            else:
                dec.min_decoder_steps = dec.max_decoder_steps = n - 1

                def run():
                    dec.start_fresh_sequence()
                    with torch.no_grad():
                        dec.incremental_forward(mem, tpos, text_lengths=ls)
            run()
            ts[n] = float(np.median([wall(run)[0] for _ in range(5)]))
        slope[name] = 1e3 * (ts[150] - ts[50]) / 100.0
    res["step_slope_ms"] = slope
    res["step_slope_ms"]["ratio"] = slope["slots"] / slope["per_utterance_launched"]
    res["rolling_pays"] = bool(res["rolling"]["wall_s"] < res["waves"]["wall_s"])
    line = json.dumps(res, indent=1)
    print(line)
    if len(sys.argv) > 1:
        with open(sys.argv[1], "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()

# coding: utf-8
"""Per-utterance synthesis timing (MultiSpeakerTTSModel.synthesize_batch): a ragged batch of 64 utterances (text
lengths spread over 20..100, deepvoice3_ljspeech preset, random weights, f16x3) timed three ways --
  per_utterance   synthesize_batch on the padded batch (each item stops by its own done flag),
  default         model(text, text_positions=...) on the same padded batch (the reference's batch semantics),
  sequential_b1   B = 1 calls for 8 of the utterances, scaled up to 64.
The three RTFs time the model part (encoder, decoder, converter); `griffin_lim` adds the batched per-item Griffin-Lim
(60 iterations) of the per-utterance batch.  RTF = wall seconds / seconds of audio produced, the audio being each item's
own frames (decoder steps x r x downsample_step x hop / sample rate).  `decode_step_slope` is the decoder loop alone, per
step, by slope between two fixed step counts (min = max decoder steps: every item runs every step in both modes).
Usage: python scripts/synth_per_utterance_rtf.py [out.json]"""
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
    from deepvoice3_pytorch_amd import builder, ops
    dev = torch.device("cuda:0")
    ops.set_gemm_precision("f16x3")
    hp = dict(bench.DV3_LJ)
    torch.manual_seed(0)
    model = builder.deepvoice3(**hp).to(dev).eval()
    model.make_generation_fast_()
    dec = model.seq2seq.decoder
    dec.min_decoder_steps, dec.max_decoder_steps = 10, 200
    B = 64
    rng = np.random.RandomState(0)
    lens = np.linspace(20, 100, B).astype(int)
    rng.shuffle(lens)
    Tt = int(lens.max())
    text = torch.zeros(B, Tt, dtype=torch.long)
    tpos = torch.zeros(B, Tt, dtype=torch.long)
    for b, s in enumerate(lens):
        text[b, :s] = torch.from_numpy(rng.randint(2, hp["n_vocab"], s))
        tpos[b, :s] = torch.arange(1, s + 1)
    text, tpos = text.to(dev), tpos.to(dev)
    sec_per_step = hp["r"] * hp["downsample_step"] * 256 / 22050.0

    def timed(fn, reps=3):
        fn()
        torch.cuda.synchronize()
        ts = []
        for _ in range(reps):
            t0 = time.perf_counter()
            out = fn()
            torch.cuda.synchronize()
            ts.append(time.perf_counter() - t0)
        return float(np.median(ts)), out

    res = {"measured_on": "MI355X (gfx950), one GPU", "batch": B, "text_lengths": "20..100 (linspace, shuffled)",
           "preset": "deepvoice3_ljspeech", "gemm": "f16x3", "min_max_decoder_steps": [10, 200],
           "part": "per_utterance / default / sequential_b1: model only (encoder + decoder + converter)"}
    with torch.no_grad():
        w, out = timed(lambda: model.synthesize_batch(text, lens))
        out_pu = out
        frames = out[4].numpy()
        steps = int(out[0].size(1))
        audio = float(frames.sum()) * hp["downsample_step"] * 256 / 22050.0
        res["per_utterance"] = dict(wall_s=w, batch_steps=steps, item_steps_min_max=[int(frames.min()), int(frames.max())],
                                    audio_s=audio, rtf=w / audio, ms_per_step=1e3 * w / steps)
        w, out = timed(lambda: model(text, text_positions=tpos))
        steps = int(out[0].size(1))
        audio = B * steps * sec_per_step
        res["default"] = dict(wall_s=w, batch_steps=steps, audio_s=audio, rtf=w / audio, ms_per_step=1e3 * w / steps)
        tot_w, tot_audio = 0.0, 0.0
        for b in range(8):
            s = int(lens[b])
            w, out = timed(lambda: model(text[b:b + 1, :s], text_positions=tpos[b:b + 1, :s]), reps=1)
            tot_w += w
            tot_audio += int(out[0].size(1)) * sec_per_step
        res["sequential_b1"] = dict(wall_s_8=tot_w, wall_s_scaled_64=tot_w * B / 8, audio_s_8=tot_audio,
                                    rtf=tot_w / tot_audio)
        from deepvoice3_pytorch_amd import audio
        lin = out_pu[1]
        up = lin.size(1) // out_pu[0].size(1)
        cfg = audio.AudioConfig(griffin_lim_iters=60)
        w, _ = timed(lambda: audio.inv_spectrogram_batch(lin, cfg, frame_lengths=out_pu[4] * up))
        res["griffin_lim"] = dict(wall_s=w, frames_padded=int(lin.size(1)), note="per-utterance batch, one call")
        # decoder loop only, by slope
        enc = model.seq2seq.encoder(text)
        slope = {}
        for name, kw in (("default", {}), ("per_utterance", dict(text_lengths=lens))):
            ts = {}
            for n in (50, 150):
                dec.min_decoder_steps = dec.max_decoder_steps = n

                def run():
                    dec.start_fresh_sequence()
                    return dec.incremental_forward(enc, tpos, **kw)
                ts[n], _ = timed(run, reps=5)
            slope[name] = 1e3 * (ts[150] - ts[50]) / 100.0
        res["decode_step_slope_ms"] = slope
    line = json.dumps(res, indent=1)
    print(line)
    if len(sys.argv) > 1:
        with open(sys.argv[1], "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()

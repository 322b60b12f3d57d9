# coding: utf-8
"""The fused decode's step program, entry by entry, for every preset: the per-batch program Decoder.incremental_forward
builds (B = 2, 16 keys) and the slot program (2 slots, 16-key capacity).  One line per entry: its scalar fields, then every
pointer of the descriptor as set / null.  Two commits build the same program iff their listings are equal.
--time adds the host cost of the per-utterance build at B = 1: _fast_decode_eligible alone, and a whole one-step
incremental_forward (program build + one launched step).  Developer tool."""
import ctypes
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402
from deepvoice3_pytorch_amd import builder, decode_program  # noqa: E402

FIELDS = {"dv3_conv_step_f32": ("B", "Cin", "M", "Cg", "J", "dil", "mode", "residual", "L", "t_cap"),
          "dv3_attn_step_f32": ("B", "E", "Tk", "win_back", "win_ahead", "kv_tke", "t_cap")}


def describe(name, d):
    vals = " ".join("%s=%d" % (f, getattr(d, f)) for f in FIELDS[name])
    ptrs = " ".join("%s=%s" % (f, "set" if getattr(d, f) else "null") for f, t in d._fields_ if t is ctypes.c_void_p)
    return "%s %s | %s" % (name[4:-4], vals, ptrs)


def batch_program(dec, enc, tpos, kw):
    """the program of one incremental_forward call, caught where the decoder hands it to StepProgram.decode"""
    caught, decode = [], decode_program.StepProgram.decode

    def spy(self, *a, **k):
        caught.append(self)
        return decode(self, *a, **k)

    decode_program.StepProgram.decode = spy
    try:
        dec.incremental_forward(enc, tpos, **kw)
    finally:
        decode_program.StepProgram.decode = decode
    return caught[0]


def main():
    dev = torch.device("cuda:0")
    B, Tk = 2, 16
    for preset in sorted(bench.PRESETS):
        bname, hp, _ = bench.PRESETS[preset]
        torch.manual_seed(0)
        model = getattr(builder, bname)(**hp).to(dev).eval()
        dec = model.seq2seq.decoder
        dec.min_decoder_steps = dec.max_decoder_steps = 0                   # one step: the listing is of the program
        multi = hp.get("n_speakers", 1) > 1
        text = torch.randint(2, hp["n_vocab"], (B, Tk), generator=torch.Generator().manual_seed(1)).to(dev)
        tpos = torch.arange(1, Tk + 1, device=dev).repeat(B, 1)
        with torch.no_grad():
            se = model.embed_speakers(torch.zeros(B, dtype=torch.long, device=dev)) if multi else None
            enc = model.seq2seq.encoder(text, lengths=None, speaker_embed=se)
            kw = dict(speaker_embed=se) if bname != "nyanko" else {}
            progs = (("batch", batch_program(dec, enc, tpos, kw)), ("slot", dec.slot_program(B, Tk)))
            for mode, P in progs:
                print("%s %s: %d entries per step, eligible(150)=%s eligible(20000)=%s" % (
                    preset, mode, len(P.prog), dec._fast_decode_eligible(150), dec._fast_decode_eligible(20000)))
                for i, (name, d) in enumerate(P.prog):
                    print("  %2d %s" % (i, describe(name, d)))
            if "--time" in sys.argv:
                enc1, kw1 = tuple(x[:1] for x in enc), {k: v if v is None else v[:1] for k, v in kw.items()}
                t0 = time.perf_counter()
                for _ in range(200):
                    dec._fast_decode_eligible(Tk)
                elig = (time.perf_counter() - t0) / 200
                walls = []
                for _ in range(25):
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    dec.incremental_forward(enc1, tpos[:1], **kw1)
                    torch.cuda.synchronize()
                    walls.append(time.perf_counter() - t0)
                print("time %s B=1 %d keys: _fast_decode_eligible %.1f us; one-step incremental_forward median %.3f ms" % (
                    preset, Tk, elig * 1e6, sorted(walls[5:])[10] * 1e3))


if __name__ == "__main__":
    main()

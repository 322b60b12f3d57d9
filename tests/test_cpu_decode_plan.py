# coding: utf-8
"""No GPU: the plan of the fused decode -- which decoders the step program takes (_fast_decode_eligible) and the entries it
would hold, read from the builder's own walk run against a dry StepProgram (meta-device buffers, nothing launched).

PLAN below is the step program of each preset in slot mode (2 slots, 16-key capacity) as the commit before the
builders were unified printed it on an MI355X (scripts/decode_program_listing.py; profiles/
r08_decode_plan_refactor_ab.txt): 16 entries per step for deepvoice3_ljspeech, 12 for deepvoice3_vctk, 27 + 1 for
nyanko_ljspeech.  tests/test_gpu_rolling_decode.py holds the programs built on the device to the same table.
"""
import os
import sys

import pytest
import torch
from torch import nn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402
from deepvoice3_pytorch_amd import builder, ops, deepvoice3, nyanko, conv as _conv  # noqa: E402
from deepvoice3_pytorch_amd.decode_program import StepProgram  # noqa: E402
from deepvoice3_pytorch_amd.modules import Conv1d, Conv1dGLU, HighwayConv1d, conv_relu_layers  # noqa: E402

LIN, RELU, SIG, GLU, HWY = ops.EPI_LINEAR, ops.EPI_RELU, ops.EPI_SIGMOID, ops.EPI_GLU, ops.EPI_HIGHWAY
ATTN = ("attn", 256)                      # an attention read: (kind, E); every other row is a conv step:


def c11(cin, m, mode=LIN):                # (kind, Cin, M, Cg, J, dil, mode, residual)
    return ("conv", cin, m, 0, 1, 1, mode, 0)


def gated(dil, mode=GLU, residual=0):
    return ("conv", 256, 512, 256, 3, dil, mode, residual)


_DV3_TAIL = [c11(256, 80), c11(80, 1, SIG)]
_HW8 = [gated(d, HWY) for d in (1, 3, 9, 27, 1, 3, 9, 27)]
PLAN = {
    "deepvoice3_ljspeech": [c11(80, 256, RELU), gated(1, residual=1), gated(3, residual=1),
                            gated(1), c11(256, 256), ATTN, c11(256, 256), gated(3), gated(9), gated(27),
                            gated(1), c11(256, 256), ATTN, c11(256, 256)] + _DV3_TAIL,
    "deepvoice3_vctk": [c11(80, 256, RELU), gated(1, residual=1),
                        gated(1), c11(256, 256), ATTN, c11(256, 256), gated(3), gated(9), gated(27), gated(1)] + _DV3_TAIL,
    "nyanko_ljspeech": [c11(80, 256, RELU), c11(256, 256, RELU), c11(256, 256)] + _HW8 + [gated(3, HWY), gated(3, HWY)]
                       + [c11(256, 256), ATTN, c11(256, 256)]
                       + [c11(512, 256)] + [gated(d, HWY) for d in (1, 3, 9, 27, 1, 1)] + [c11(256, 256, RELU)] * 3 + _DV3_TAIL,
}


def plan_rows(P):
    """the entries of a step program as PLAN rows"""
    rows = []
    for name, d in P.prog:
        if name == "dv3_conv_step_f32":
            rows.append(("conv", d.Cin, d.M, d.Cg, d.J, d.dil, d.mode, d.residual))
        else:
            rows.append(("attn", d.E))
    return rows


_decoders = {}


def preset_decoder(name):
    if name not in _decoders:
        bname, hp, _ = bench.PRESETS[name]
        torch.manual_seed(0)
        _decoders[name] = getattr(builder, bname)(**hp).eval().seq2seq.decoder
    return _decoders[name]


@pytest.mark.parametrize("preset", sorted(bench.PRESETS))
def test_presets_are_eligible_up_to_the_lds(preset):
    dec = preset_decoder(preset)
    assert dec._fast_decode_eligible(150) is True
    assert dec._fast_decode_eligible(20000) is False          # the attention scores of 20000 keys do not fit the LDS


@pytest.mark.parametrize("preset", sorted(PLAN))
def test_slot_plan_entry_for_entry(preset):
    dec = preset_decoder(preset)
    P = StepProgram(2, "meta", t_cap=dec.max_decoder_steps + 1)
    dec._slot_entries(P, 16)
    assert P.refused is None
    rows = plan_rows(P)
    assert len(rows) == len(PLAN[preset]) == {"deepvoice3_ljspeech": 16, "deepvoice3_vctk": 12, "nyanko_ljspeech": 28}[preset]
    for i, (got, want) in enumerate(zip(rows, PLAN[preset])):
        assert got == want, (preset, i, got, want)
    for name, d in P.prog:
        assert d.B == 2 and d.t_cap == dec.max_decoder_steps + 1
        assert name == "dv3_conv_step_f32" or (d.Tk == 16 and d.win_back == 1 and d.win_ahead == 3)
    n_att = sum(r[0] == "attn" for r in rows)
    assert P.align_scale == 2.0 ** (n_att - 1) / n_att


# ----------------------------------------------------------------------------------------------------------------------
# what the step program does not take (toy decoders)
# ----------------------------------------------------------------------------------------------------------------------
def toy_dv3(**kw):
    torch.manual_seed(1)
    args = dict(embed_dim=16, n_speakers=1, speaker_embed_dim=4, in_dim=8, r=1, max_positions=64,
                preattention=((16, 3, 1),), convolutions=((16, 3, 1), (16, 3, 3)))
    return deepvoice3.Decoder(**dict(args, **kw)).eval()


def toy_nyanko():
    torch.manual_seed(1)
    return nyanko.Decoder(embed_dim=16, in_dim=8, r=1, channels=16, max_positions=64).eval()


def test_toys_are_eligible_as_built():
    assert toy_dv3()._fast_decode_eligible(150) and toy_nyanko()._fast_decode_eligible(150)


def test_preattention_conv_with_taps_is_not_eligible():
    dec = toy_dv3()
    assert isinstance(dec.preattention[0], _conv.Conv1d) and dec.preattention[0].kernel_size == (1,)
    dec.preattention[0] = Conv1d(8, 16, kernel_size=3, padding=2)
    assert dec._fast_decode_eligible(150) is False


def _first_k_that_does_not_fit(cin):
    k = next(k for k in range(2, 1 << 16) if not ops.conv_step_fits(k, cin))
    assert ops.conv_step_fits(k - 1, cin)                     # one notch past DV3_CONV_STEP_LDS_MAX, by the library's answer
    return k


@pytest.mark.parametrize("where", ["preattention", "convolutions"])
def test_glu_window_beyond_the_lds_is_not_eligible(where):
    k = _first_k_that_does_not_fit(16)
    assert toy_dv3(**{where: ((16, k - 1, 1),)})._fast_decode_eligible(150) is True
    assert toy_dv3(**{where: ((16, k, 1),)})._fast_decode_eligible(150) is False


def test_every_conv_entry_is_asked_of_the_library():
    """the projections, last_conv and fc are conv-step entries like the rest: one that does not fit is refused"""
    step = 64
    cin = next(c for c in range(step, 1 << 22, step) if not ops.conv_step_fits(1, c))
    for c, fits in ((cin - step, True), (cin, False)):
        P = StepProgram(1, "meta", t_cap=1)
        P.conv_step(_conv.Linear(c, 1), P.buffer(1, c), ops.EPI_SIGMOID, 1)
        assert (P.refused is None) == fits, (c, P.refused)
        # a decoder whose attention contexts are that wide: every GLU window fits and so do the attention scores, the
        # 1x1 out_projection over the context does not
        assert (c + 16) * 4 <= 64 * 1024
        dec = toy_dv3(embed_dim=c, key_projection=False, value_projection=False)
        assert dec._fast_decode_eligible(16) is fits, c


def test_nyanko_glu_highway_is_not_eligible():
    dec = toy_nyanko()
    i = next(i for i, f in enumerate(dec.audio_decoder_modules) if isinstance(f, HighwayConv1d))
    dec.audio_decoder_modules[i] = HighwayConv1d(16, 16, kernel_size=3, padding=None, dilation=1, causal=True, glu=True)
    assert dec._fast_decode_eligible(150) is False


def test_nyanko_relu_after_a_highway_layer_is_not_eligible():
    dec = toy_nyanko()
    mods = list(dec.audio_encoder_modules)
    i = next(i for i, f in enumerate(mods) if isinstance(f, HighwayConv1d))
    dec.audio_encoder_modules = nn.ModuleList(mods[:i + 1] + [nn.ReLU()] + mods[i + 1:])
    assert dec._fast_decode_eligible(150) is False


# ----------------------------------------------------------------------------------------------------------------------
# the shared iterator
# ----------------------------------------------------------------------------------------------------------------------
def test_conv_relu_layers():
    a, b, c = (Conv1d(4, 4, kernel_size=1) for _ in range(3))
    r1, r2 = nn.ReLU(), nn.ReLU()
    hw, glu = HighwayConv1d(4, 4, kernel_size=3, causal=True), Conv1dGLU(1, 4, 4, 4, 3, 0.0, causal=True)
    assert list(conv_relu_layers([])) == []
    assert list(conv_relu_layers(nn.ModuleList([a, r1, b]))) == [(a, True), (b, False)]               # trailing Conv1d
    assert list(conv_relu_layers([a, b, r1])) == [(a, False), (b, True)]                              # Conv1d + ReLU at the end
    assert list(conv_relu_layers([a, r1, r2, b])) == [(a, True), (r2, False), (b, False)]             # two ReLUs in a row
    assert list(conv_relu_layers([r1, a])) == [(r1, False), (a, False)]                               # a ReLU nothing precedes
    assert list(conv_relu_layers([hw, r1, glu, r2, c, r1])) == [(hw, False), (r1, False), (glu, False), (r2, False), (c, True)]

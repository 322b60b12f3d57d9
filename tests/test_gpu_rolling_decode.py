# coding: utf-8
"""-m gpu: rolling admission -- the decode-step kernels' slot mode, the slot-mode step program of both
decoder families, and synthesis.tts_stream.

  1. kernel level: dv3_conv_step_f32 and dv3_attn_step_f32 with t_off (items at different steps inside one workgroup's
     batch group, one idle slot, one slot that overruns t_cap): every item bit-equal to the same item alone at B = 1 on
     the shared counter, and within the bounds of tests/decode_step_ref.py of the float64 references;
  2. decoder level: 12 utterances through 4 slots with staggered admission, every item bit-equal to
     Decoder.incremental_forward at B = 1 on its own encoder output (slots are reused after longer utterances); the
     per-batch and the slot program of one decoder descriptor for descriptor, and against the presets' table of
     tests/test_cpu_decode_plan.py; a stack the program has no entry for decodes module by module;
  3. end to end: synthesis.tts_stream against synthesis.tts_batch;
  4. the refusals.
"""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tests import decode_step_ref as R  # noqa: E402
from tests.util import assert_close_elementwise, rel_err  # noqa: E402

pytestmark = pytest.mark.gpu

NAN = float("nan")
IDLE = 2 ** 31 - 1


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


def _env():
    from deepvoice3_pytorch_amd import ops, _lib
    return ops, _lib.lib(), _lib.STRUCTS, _lib.CONSTS


def _nan(dev, *shape):
    return torch.full(shape, NAN, device=dev)


def _launch(kind, d, t0, n):
    """steps t0 .. t0 + n - 1 of one descriptor, the step index in t_value (dv3_decode_program_launch)"""
    ops, L, S, C = _env()
    arr = (S["dv3_decode_entry"] * 1)()
    arr[0].kind = kind
    if kind == 0:
        arr[0].conv = d
    else:
        arr[0].attn = d
    p = S["dv3_decode_program"]()
    p.entries_host = ctypes.addressof(arr)
    p.n_entries, p.B, p.t0, p.n_steps = 1, d.B, t0, n
    ops._lib.call("dv3_decode_program_launch", ctypes.byref(p), ops._stream())


# ----------------------------------------------------------------------------------------------------------------------
# 1a. the conv step in slot mode
# ----------------------------------------------------------------------------------------------------------------------
def _conv_desc(dev, S, C, tiles, bias, x, spk, pa, ring, out_seq, y, mode, J, dil, Lr, residual, t_off=None, t_cap=0):
    """x [T][B][Cin] (teacher rows: x_ts), spk [B][Cout] or None, pa [T][B][Cout], ring [L][B][Cin] or None"""
    T, B, Cin = x.shape
    Cout = y.size(1)
    gated = mode in R.GATED
    d = S["dv3_conv_step_desc"]()
    d.x, d.x_bs, d.x_ts = x.data_ptr(), Cin, B * Cin
    if ring is not None:
        d.ring, d.L = ring.data_ptr(), Lr
    d.a = tiles.data_ptr()
    d.bias = bias.data_ptr()
    if spk is not None:
        d.spk, d.spk_bs = spk.data_ptr(), Cout
    d.post_add, d.post_add_ts, d.post_add_bs = pa.data_ptr(), B * Cout, Cout
    d.y, d.y_bs = y.data_ptr(), Cout
    d.out_seq, d.out_seq_ts, d.out_seq_bs = out_seq.data_ptr(), B * Cout, Cout
    d.B, d.Cin, d.M, d.Cg, d.J, d.dil = B, Cin, (2 * Cout if gated else Cout), (Cout if gated else 0), J, dil
    d.mode, d.residual = C["DV3_EPI_" + mode.upper()], int(residual)
    if t_off is not None:
        d.t_off, d.t_cap = t_off.data_ptr(), t_cap
    return d


CONV_CASES = [(mode, J, dil) for mode in ("glu", "highway") for (J, dil) in ((1, 1), (3, 1), (3, 3), (3, 27))]


@pytest.mark.parametrize("mode,J,dil", CONV_CASES)
def test_conv_step_slots_equal_b1(dev, mode, J, dil):
    ops, L, S, C = _env()
    rs = np.random.RandomState(1000 + 10 * J + dil + (7 if mode == "glu" else 0))
    f32 = np.float32
    B, Cin = 6, 40
    Cout, M = Cin, 2 * Cin
    Lr = (J - 1) * dil + 1
    t_cap = Lr + 5
    # one workgroup holds items 0..3: steps 0 / 3 / idle / 7 apart; items 4, 5 share the second (clamped) group
    t_off = [0, 3, IDLE, 7, 2, t_cap - 2]
    Tg = t_cap + 4               # item 0 overruns t_cap by 4 steps, item 1 by 1; 3, 4 stop short; 5 runs 6 steps
    W = (rs.standard_normal((M, J, Cin)) * (1.5 / np.sqrt(J * Cin))).astype(f32)
    bias_h = (rs.standard_normal(M) * 0.5).astype(f32)
    x_h = rs.standard_normal((t_cap, B, Cin)).astype(f32)
    spk_h = rs.standard_normal((B, Cout)).astype(f32) if mode == "glu" else None
    pa_h = rs.standard_normal((t_cap, B, Cout)).astype(f32)
    residual = mode == "glu"
    a_half, lda = Cout, 2 * Cout
    fp = R.fwd_pack_of(W, Cout, lda, a_half)
    n = L.dv3_conv_step_pack_floats(J * Cin, M, Cout)
    tiles = torch.zeros(n, device=dev)
    src = torch.from_numpy(fp).to(dev)
    ops._lib.call("dv3_conv_step_pack_f32", src.data_ptr(), lda, a_half, J * Cin, M, Cout, tiles.data_ptr(), ops._stream())
    bias = torch.from_numpy(bias_h).to(dev)
    x, pa = torch.from_numpy(x_h).to(dev), torch.from_numpy(pa_h).to(dev)
    spk = torch.from_numpy(spk_h).to(dev) if spk_h is not None else None

    # slot mode, all B items in one launch per global step
    ring = torch.zeros(Lr, B, Cin, device=dev) if J > 1 else None
    out_seq, y = _nan(dev, t_cap, B, Cout), _nan(dev, B, Cout)
    toff = torch.tensor(t_off, dtype=torch.int32, device=dev)
    d = _conv_desc(dev, S, C, tiles, bias, x, spk, pa, ring, out_seq, y, mode, J, dil, Lr, residual, toff, t_cap)
    _launch(0, d, 0, Tg)
    torch.cuda.synchronize()

    worst = 0.0
    for b in range(B):
        ran = 0 if t_off[b] == IDLE else min(max(Tg - t_off[b], 0), t_cap)
        # the same item alone, B = 1, shared counter
        x1, pa1 = x[:, b:b + 1].contiguous(), pa[:, b:b + 1].contiguous()
        spk1 = spk[b:b + 1].contiguous() if spk is not None else None
        ring1 = torch.zeros(Lr, 1, Cin, device=dev) if J > 1 else None
        out1, y1 = _nan(dev, t_cap, 1, Cout), _nan(dev, 1, Cout)
        d1 = _conv_desc(dev, S, C, tiles, bias, x1, spk1, pa1, ring1, out1, y1, mode, J, dil, Lr, residual)
        if ran:
            _launch(0, d1, 0, ran)
        torch.cuda.synchronize()
        assert torch.equal(out_seq[:ran, b], out1[:ran, 0]), (b, "stacked rows differ from the B = 1 run")
        assert bool(torch.isnan(out_seq[ran:, b]).all()), (b, "a stacked row outside the item's steps was written")
        if J > 1:
            assert torch.equal(ring[:, b], ring1[:, 0]), (b, "ring columns differ from the B = 1 run")
        # float64, the existing bounds
        for t in range(ran):
            sp = spk_h[b:b + 1] if spk_h is not None else None
            ref = R.conv_step_ref(x_h[:t + 1, b:b + 1], W, bias_h, mode, dil, residual=residual, spk=sp,
                                  post_add=pa_h[t, b:b + 1])
            bnd = R.conv_step_bound(ref, mode, J, Cin, residual=residual, spk=sp, post_add=pa_h[t, b:b + 1])
            worst = max(worst, assert_close_elementwise(out_seq[t, b:b + 1], ref["out_seq"], 0, bnd["y"],
                                                        "conv slots %s J%d d%d item %d step %d" % (mode, J, dil, b, t)))
    print("worst-ratio conv_step slots %s J=%d dil=%d: %.4g" % (mode, J, dil, worst))


# ----------------------------------------------------------------------------------------------------------------------
# 1b. the attention step in slot mode
# ----------------------------------------------------------------------------------------------------------------------
def _attn_desc(S, q, k, v, la, t_dev, ctx, attn_seq, key_len=None, t_off=None, t_cap=0):
    B, E = q.shape
    Tk = k.size(1)
    d = S["dv3_attn_step_desc"]()
    d.q, d.q_bs, d.k, d.v, d.kv_tke = q.data_ptr(), E, k.data_ptr(), v.data_ptr(), 1
    d.last_attended = la.data_ptr() if la is not None else None
    d.win_back, d.win_ahead, d.t = 1, 3, t_dev.data_ptr()
    d.ctx, d.ctx_bs = ctx.data_ptr(), E
    d.attn_seq, d.attn_seq_ts = attn_seq.data_ptr(), B * Tk
    d.B, d.E, d.Tk = B, E, Tk
    if key_len is not None:
        d.key_len = key_len.data_ptr()
    if t_off is not None:
        d.t_off, d.t_cap = t_off.data_ptr(), t_cap
    return d


@pytest.mark.parametrize("monotonic", [True, False])
def test_attn_step_slots_equal_b1(dev, monotonic):
    ops, L, S, C = _env()
    g = torch.Generator().manual_seed(17 + int(monotonic))
    B, E, Tk, t_cap = 6, 96, 40, 7
    kl = [Tk, 3, 9, 17, 1, 25]
    t_off = [0, 2, IDLE, 5, 1, 4]
    Tg = t_cap + 3                                   # items 0, 1, 4 overrun t_cap
    qseq = torch.randn(t_cap, B, E, generator=g).to(dev)
    k = torch.randn(B, Tk, E, generator=g).to(dev)
    v = torch.randn(B, Tk, E, generator=g).to(dev)
    key_len = torch.tensor(kl, dtype=torch.int32, device=dev)
    toff = torch.tensor(t_off, dtype=torch.int32, device=dev)
    la = torch.zeros(2, B, dtype=torch.int32, device=dev) if monotonic else None
    q, ctx = torch.zeros(B, E, device=dev), _nan(dev, B, E)
    attn_seq = _nan(dev, t_cap, B, Tk)
    ctx_seq = _nan(dev, t_cap, B, E)
    t_dev = torch.zeros(1, dtype=torch.int32, device=dev)
    d = _attn_desc(S, q, k, v, la, t_dev, ctx, attn_seq, key_len, toff, t_cap)
    for t in range(Tg):
        tb = [t - o for o in t_off]
        for b in range(B):
            if 0 <= tb[b] < t_cap:
                q[b].copy_(qseq[tb[b], b])
        ctx.fill_(NAN)
        ops._lib.call("dv3_attn_step_f32", ctypes.byref(d), ops._stream())
        for b in range(B):
            if 0 <= tb[b] < t_cap:
                ctx_seq[tb[b], b].copy_(ctx[b])
            else:
                assert bool(torch.isnan(ctx[b]).all()), (t, b, "an idle slot stored a context")
        t_dev.add_(1)
    torch.cuda.synchronize()
    worst = 0.0
    for b in range(B):
        ran = 0 if t_off[b] == IDLE else min(max(Tg - t_off[b], 0), t_cap)
        s = kl[b]
        assert bool(torch.isnan(attn_seq[ran:, b]).all()), (b, "a stacked row outside the item's steps was written")
        if ran == 0:
            if monotonic:
                assert la[:, b].tolist() == [0, 0]
            continue
        # alone: B = 1 over its own s keys, the shared counter, a [2] window pair
        k1, v1 = k[b:b + 1, :s].contiguous(), v[b:b + 1, :s].contiguous()
        la1 = torch.zeros(2, dtype=torch.int32, device=dev) if monotonic else None
        q1, ctx1, attn1 = torch.zeros(1, E, device=dev), _nan(dev, 1, E), _nan(dev, t_cap, 1, s)
        t1 = torch.zeros(1, dtype=torch.int32, device=dev)
        d1 = _attn_desc(S, q1, k1, v1, la1, t1, ctx1, attn1)
        la_ref = 0 if monotonic else None
        for t in range(ran):
            q1[0].copy_(qseq[t, b])
            ops._lib.call("dv3_attn_step_f32", ctypes.byref(d1), ops._stream())
            t1.add_(1)
            torch.cuda.synchronize()
            assert torch.equal(attn_seq[t, b, :s], attn1[t, 0]), (b, t)
            assert not attn_seq[t, b, s:].any(), (b, t)
            assert torch.equal(ctx_seq[t, b], ctx1[0]), (b, t)
            ref = R.attn_step_ref(qseq[t, b].cpu().numpy(), k[b].cpu().numpy(), v[b].cpu().numpy(), la=la_ref, key_len=s)
            ep, ectx = R.attn_step_bound(ref, E, Tk)
            what = "attn slots item %d step %d" % (b, t)
            worst = max(worst, assert_close_elementwise(attn_seq[t, b], ref["p"], 0, ep, what + " p"))
            worst = max(worst, assert_close_elementwise(ctx_seq[t, b], ref["ctx"], 0, ectx, what + " ctx"))
            if monotonic:
                assert ref["gap"] > 1e-4, (what, "near-tie argmax in the test data")
                la_ref = ref["argmax"]
                assert int(la1[(t + 1) & 1]) == la_ref, what
        if monotonic:
            assert la[:, b].tolist() == la1.tolist(), (b, "window pair differs from the B = 1 run")
    print("worst-ratio attn_step slots monotonic=%s: %.4g" % (monotonic, worst))


def test_slots_reset_touches_only_its_slots(dev):
    """dv3_decode_slots_reset: the listed items' ring columns, window rows and decoder-input rows, nothing else"""
    ops, L, S, C = _env()
    B, Cin, Lr, E, Tk = 5, 24, 7, 16, 9
    x, y = torch.ones(B, Cin, device=dev), torch.ones(B, Cin, device=dev)
    ring = torch.ones(Lr, B, Cin, device=dev)
    tiles = torch.zeros(L.dv3_conv_step_pack_floats(3 * Cin, Cin, 0), device=dev)
    la = torch.full((2, B), 5, dtype=torch.int32, device=dev)
    key_len = torch.full((B,), Tk, dtype=torch.int32, device=dev)
    toff = torch.zeros(B, dtype=torch.int32, device=dev)
    arr = (S["dv3_decode_entry"] * 2)()
    c = arr[0].conv
    c.x, c.x_bs, c.ring, c.L, c.a, c.y, c.y_bs = x.data_ptr(), Cin, ring.data_ptr(), Lr, tiles.data_ptr(), y.data_ptr(), Cin
    c.B, c.Cin, c.M, c.J, c.dil, c.mode = B, Cin, Cin, 3, 3, C["DV3_EPI_LINEAR"]
    c.t_off, c.t_cap = toff.data_ptr(), 4
    arr[1].kind = 1
    a = arr[1].attn
    kv, ctx = torch.zeros(B, Tk, E, device=dev), torch.zeros(B, E, device=dev)
    a.q, a.q_bs, a.k, a.v, a.kv_tke, a.ctx, a.ctx_bs = ctx.data_ptr(), E, kv.data_ptr(), kv.data_ptr(), 1, ctx.data_ptr(), E
    a.last_attended, a.key_len, a.B, a.E, a.Tk = la.data_ptr(), key_len.data_ptr(), B, E, Tk
    a.t_off, a.t_cap = toff.data_ptr(), 4
    p = S["dv3_decode_program"]()
    p.entries_host, p.n_entries, p.B = ctypes.addressof(arr), 2, B
    slots = torch.tensor([3, 1], dtype=torch.int32, device=dev)
    ops._lib.call("dv3_decode_slots_reset", ctypes.byref(p), slots.data_ptr(), 2, ops._stream())
    torch.cuda.synchronize()
    for b in range(B):
        want = 0.0 if b in (1, 3) else 1.0
        assert bool((ring[:, b] == want).all()) and bool((x[b] == want).all()), b
        assert la[:, b].tolist() == ([0, 0] if b in (1, 3) else [5, 5]), b
    assert bool((y == 1).all())
    a.key_len = None                                  # one window for the batch: not a slot program
    assert L.dv3_decode_slots_reset(ctypes.byref(p), slots.data_ptr(), 2, ops._stream()) != 0
    assert "key_len" in (L.dv3_last_error() or b"").decode()


# ----------------------------------------------------------------------------------------------------------------------
# 2. the slot-mode step program of the decoders
# ----------------------------------------------------------------------------------------------------------------------
NY_HP = dict(n_vocab=40, embed_dim=32, mel_dim=20, linear_dim=33, r=1, downsample_step=4, padding_idx=0, dropout=0.05,
             kernel_size=3, encoder_channels=64, decoder_channels=64, converter_channels=32, max_positions=128,
             use_memory_mask=True, force_monotonic_attention=True, use_decoder_state_for_postnet_input=True)
DV3_HP = dict(n_vocab=40, embed_dim=32, mel_dim=20, linear_dim=33, r=2, downsample_step=4, padding_idx=0, dropout=0.05,
              kernel_size=3, encoder_channels=64, decoder_channels=32, converter_channels=32,
              use_memory_mask=True, force_monotonic_attention=True, use_decoder_state_for_postnet_input=True,
              key_projection=True, value_projection=True, max_positions=128)
MS_HP = dict(DV3_HP, n_speakers=5, speaker_embed_dim=8, r=1)


def _toy(name, dev):
    from deepvoice3_pytorch_amd import builder
    import bench
    torch.manual_seed(3)
    toys = dict(nyanko=(builder.nyanko, NY_HP), deepvoice3=(builder.deepvoice3, DV3_HP),
                multispeaker=(builder.deepvoice3_multispeaker, MS_HP))
    if name in toys:
        model = toys[name][0](**toys[name][1]).to(dev).eval()
        model.seq2seq.decoder.max_decoder_steps = 40          # the toys' position tables hold 128 rows, the default is 200 steps
        return model, toys[name][1]
    bname, hp, _ = bench.PRESETS[name]                # preset channel counts
    return getattr(builder, bname)(**dict(hp)).to(dev).eval(), dict(hp)


@pytest.mark.parametrize("family", ["nyanko", "deepvoice3", "multispeaker", "deepvoice3_ljspeech"])
def test_slot_program_items_equal_b1(dev, family):
    from deepvoice3_pytorch_amd.decode_program import RollingSchedule
    model, hp = _toy(family, dev)
    dec = model.seq2seq.decoder
    multi = hp.get("n_speakers", 1) > 1
    g = torch.Generator().manual_seed(11)
    lens = [31, 9, 23, 4, 17, 12, 28, 6, 20, 3, 15, 26]              # 12 utterances, all different
    steps = [24, 5, 17, 9, 21, 3, 12, 24, 7, 14, 2, 10]              # decoder steps of each
    U, n_slots, chunk, N = len(lens), 4, 3, 23
    texts = [torch.randint(2, hp["n_vocab"], (1, s), generator=g).to(dev) for s in lens]
    tpos = [torch.arange(1, s + 1, device=dev)[None] for s in lens]
    spk = torch.randint(0, hp.get("n_speakers", 1), (U,), generator=g).to(dev) if multi else None
    with torch.no_grad():
        se = model.embed_speakers(spk) if multi else None
        encs = [model.seq2seq.encoder(tx, **(dict(speaker_embed=se[b:b + 1]) if multi else {})) for b, tx in enumerate(texts)]
        want = []
        for b in range(U):                           # each utterance alone, stopped by max_decoder_steps after steps[b]
            dec.min_decoder_steps = dec.max_decoder_steps = steps[b] - 1
            dec.start_fresh_sequence()
            kw = dict(speaker_embed=se[b:b + 1]) if multi else {}
            want.append(dec.incremental_forward(encs[b], tpos[b], **kw))
            assert want[-1][0].size(1) == steps[b]
    dec.min_decoder_steps = dec.max_decoder_steps = N
    P = dec.slot_program(n_slots, max(lens) + 5)
    assert P.t_cap == N + 1 and P.B == n_slots
    sch = RollingSchedule(n_slots, chunk)
    arrivals = {0: [0, 1], 1: [2, 3, 4], 2: list(range(5, U))}       # staggered: two, then three, then the rest
    got, history, rnd = {}, {s: [] for s in range(n_slots)}, 0
    while sch.pending() or rnd < 3:
        for tk in arrivals.get(rnd, []):
            sch.submit(tk)
        new = sch.admit()
        if new:
            tks = [tk for tk, _ in new]
            Tmax = max(lens[tk] for tk in tks)
            D = encs[0][0].size(2)
            K = torch.randn(len(tks), Tmax, D, generator=g).to(dev)      # junk padding: a slot must not read it
            V = torch.randn(len(tks), Tmax, D, generator=g).to(dev)
            TP = torch.zeros(len(tks), Tmax, dtype=torch.long, device=dev)
            for i, tk in enumerate(tks):
                K[i, :lens[tk]], V[i, :lens[tk]] = encs[tk][0][0], encs[tk][1][0]
                TP[i, :lens[tk]] = tpos[tk][0]
            P.admit([s for _, s in new], (K, V), TP, [lens[tk] for tk in tks], se[torch.tensor(tks).to(dev)] if multi else None)
            assert P.t == sch.t
            for tk, s in new:
                history[s].append(tk)
        if sch.busy():
            P.run_steps(sch.advance())
            for s in sch.busy():
                tk = sch.slot_ticket[s]
                if sch.steps_run(s) >= steps[tk]:
                    got[tk] = P.read_slot(s, steps[tk])
                    sch.retire(s)
                    P.release([s])
        rnd += 1
    torch.cuda.synchronize()
    assert sorted(got) == list(range(U))
    # a slot was handed to a shorter utterance (fewer steps and fewer keys) after a longer one
    assert any(steps[a] > steps[b] and lens[a] > lens[b] for h in history.values() for a, b in zip(h[:-1], h[1:])), history
    assert len(set(off for _, _, off, _ in sch.log)) >= 4
    for b, (wo, wa, wd, ws) in enumerate(want):
        out, ali, done, st = got[b]
        s = lens[b]
        assert torch.equal(out, wo[0]), (family, b, "outputs")
        assert torch.equal(st, ws[0]), (family, b, "states")
        assert torch.equal(ali[:, :s], wa[0]), (family, b, "alignments")
        assert not ali[:, s:].any(), (family, b)
        assert torch.equal(done, torch.cat([d.reshape(1) for d in wd])), (family, b, "done flags")


def _batch_program(dec, *args, **kw):
    """the program one incremental_forward call builds, caught where the decoder hands it to StepProgram.decode"""
    from deepvoice3_pytorch_amd.decode_program import StepProgram
    caught, decode = [], StepProgram.decode

    def spy(self, *a, **k):
        caught.append(self)
        return decode(self, *a, **k)

    StepProgram.decode = spy
    try:
        dec.incremental_forward(*args, **kw)
    finally:
        StepProgram.decode = decode
    assert len(caught) == 1
    return caught[0]


SLOT_FIELDS = ("t_off", "t_cap", "key_len")           # what a slot program sets and a per-batch program does not


def _descriptor(d):
    """every field of a step descriptor the two builders must agree in: the shape and mode fields by value, the pointers
    as set / null; strides and the slot fields aside"""
    shape = ("B", "Cin", "M", "Cg", "J", "dil", "mode", "residual", "L", "E", "Tk", "win_back", "win_ahead", "kv_tke")
    out = {}
    for f, t in d._fields_:
        if f in SLOT_FIELDS:
            continue
        if t is ctypes.c_void_p:
            out[f] = bool(getattr(d, f))
        elif f in shape:
            out[f] = getattr(d, f)
    return out


@pytest.mark.parametrize("family", ["nyanko", "deepvoice3", "multispeaker", "deepvoice3_ljspeech", "deepvoice3_vctk",
                                    "nyanko_ljspeech"])
def test_batch_and_slot_programs_agree(dev, family):
    """Decoder._incremental_fast and Decoder.slot_program append the same entries (one walk, _step_entries): kind, B,
    Cin, M, Cg, J, dil, mode, residual, L and which optional pointers are set, entry for entry; built from a preset they
    are the table of tests/test_cpu_decode_plan.py"""
    from tests.test_cpu_decode_plan import PLAN, plan_rows
    model, hp = _toy(family, dev)
    dec = model.seq2seq.decoder
    dec.min_decoder_steps = dec.max_decoder_steps = 3
    multi = hp.get("n_speakers", 1) > 1
    B, Tk = 2, 16
    g = torch.Generator().manual_seed(5)
    text = torch.randint(2, hp["n_vocab"], (B, Tk), generator=g).to(dev)
    tpos = torch.arange(1, Tk + 1, device=dev).repeat(B, 1)
    with torch.no_grad():
        se = model.embed_speakers(torch.tensor([1, 0], device=dev)) if multi else None
        enc = model.seq2seq.encoder(text, **(dict(speaker_embed=se) if multi else {}))
        kw = dict(speaker_embed=se) if multi else {}
        batch = _batch_program(dec, enc, tpos, **kw)
        per_item = _batch_program(dec, enc, tpos, text_lengths=[Tk, 9], **kw)
        slot = dec.slot_program(B, Tk)
    assert len(batch.prog) == len(per_item.prog) == len(slot.prog)
    for i, ((nb, db), (ni, di), (ns, ds)) in enumerate(zip(batch.prog, per_item.prog, slot.prog)):
        assert nb == ni == ns, (family, i)
        assert _descriptor(db) == _descriptor(di) == _descriptor(ds), (family, i, nb, _descriptor(db), _descriptor(ds))
        assert ds.t_cap == slot.t_cap and ds.t_off and not db.t_off and not db.t_cap, (family, i)
        if nb == "dv3_attn_step_f32":
            assert ds.key_len and di.key_len and not db.key_len, (family, i)
    assert batch.align_scale == slot.align_scale
    if family in PLAN:
        assert plan_rows(batch) == plan_rows(slot) == PLAN[family], family


def test_stray_relu_falls_back_to_the_module_path(dev):
    """a nyanko stack with a ReLU directly after a HighwayConv1d: the step program has no entry for it, so the decoder
    is not eligible and incremental_forward runs module by module -- the tensors of fast_decode = False, bit for bit"""
    from torch import nn
    from deepvoice3_pytorch_amd.modules import HighwayConv1d
    model, hp = _toy("nyanko", dev)
    dec = model.seq2seq.decoder
    mods = list(dec.audio_decoder_modules)
    i = next(i for i, f in enumerate(mods) if isinstance(f, HighwayConv1d))
    dec.audio_decoder_modules = nn.ModuleList(mods[:i + 1] + [nn.ReLU()] + mods[i + 1:])
    dec.min_decoder_steps, dec.max_decoder_steps = 4, 9
    assert dec._fast_decode_eligible(16) is False
    with pytest.raises(RuntimeError, match="not eligible"):
        dec.slot_program(2, 16)
    g = torch.Generator().manual_seed(9)
    text = torch.randint(2, hp["n_vocab"], (2, 13), generator=g).to(dev)
    tpos = torch.arange(1, 14, device=dev).repeat(2, 1)
    taken = []                                        # which path answered: (name, it returned a result)
    for name in ("_incremental_fast", "_incremental_modules"):
        def spy(*a, _f=getattr(dec, name), _n=name, **k):
            out = _f(*a, **k)
            taken.append((_n, out is not None))
            return out
        setattr(dec, name, spy)
    with torch.no_grad():
        enc = model.seq2seq.encoder(text)
        for tl in (None, [13, 6]):
            res = {}
            for fast in (True, False):
                dec.fast_decode = fast
                dec.start_fresh_sequence()
                del taken[:]
                res[fast] = dec.incremental_forward(enc, tpos, text_lengths=tl)
                # fast: the program's build was refused and the module path took the call; else the module path alone
                assert taken == ([("_incremental_fast", False)] if fast else []) + [("_incremental_modules", True)], taken
            a, b = res[True], res[False]
            assert 5 <= a[0].size(1) <= 10 and bool(torch.isfinite(a[0]).all())
            assert len(a) == len(b) == (4 if tl is None else 5) and len(a[2]) == len(b[2])
            for x, y in zip((a[0], a[1], a[3]) + tuple(a[2]) + tuple(a[4:]), (b[0], b[1], b[3]) + tuple(b[2]) + tuple(b[4:])):
                assert torch.equal(x, y), tl


# ----------------------------------------------------------------------------------------------------------------------
# 3. tts_stream against tts_batch
# ----------------------------------------------------------------------------------------------------------------------
def test_tts_stream_matches_tts_batch(dev):
    """40 ragged utterances through 8 slots against tts_batch on the same list.  The utterances stop at different steps by
    per-request caps (tts_stream(max_decoder_steps=[...]): 8, 16 or 24 steps) with the done flag out of the rule
    (min_decoder_steps = the decoder's maximum), so the stops do not hang on a random-weight flag's distance to 0.5;
    tts_batch has no per-request cap and is run on the list's three cap groups with the decoder's own maximum set to the
    group's.  Tolerances: test_tts_batch_64_utterances' for batch against alone."""
    import bench
    from deepvoice3_pytorch_amd import builder, ops, synthesis, audio
    from deepvoice3_pytorch_amd.decode_program import simulate_rolling
    prev = ops.set_gemm_precision("f16x3")
    try:
        bname, hp, _ = bench.PRESETS["deepvoice3_ljspeech"]
        hp = dict(hp)
        torch.manual_seed(0)
        model = builder.deepvoice3(**hp).to(dev).eval()
        dec = model.seq2seq.decoder
        rng = np.random.RandomState(21)
        n_utt, n_slots, chunk = 40, 8, 8
        lens = rng.randint(20, 101, n_utt).tolist()
        seqs = [rng.randint(2, hp["n_vocab"], s).tolist() for s in lens]
        caps = [int(c) for c in rng.choice([7, 15, 23], n_utt)]
        cfg = audio.AudioConfig(griffin_lim_iters=2)
        want = [None] * n_utt
        for cap in sorted(set(caps)):
            idx = [i for i in range(n_utt) if caps[i] == cap]
            dec.min_decoder_steps = dec.max_decoder_steps = cap
            for i, res in zip(idx, synthesis.tts_batch(model, [seqs[i] for i in idx], audio_cfg=cfg)):
                want[i] = res
        dec.min_decoder_steps = dec.max_decoder_steps = 23
        order, got = [], {}
        for tk, mel, lin, ali, wav in synthesis.tts_stream(model, iter(seqs), slots=n_slots, max_text_len=100, audio_cfg=cfg,
                                                           chunk=chunk, max_decoder_steps=iter(caps)):
            assert tk not in got
            order.append(tk)
            got[tk] = (mel, lin, ali, wav)
        assert sorted(got) == list(range(n_utt))
        # completion order: the schedule's (the tickets are the list's indices)
        _, sim = simulate_rolling([c + 1 for c in caps], n_slots, chunk)
        assert order == [tk for tk, _, _, _ in sim.log]
        assert order != sorted(order)
        for i in range(n_utt):
            (mel, lin, ali, wav), (wm, wl, wa, ww) = got[i], want[i]
            assert mel.shape == wm.shape == ((caps[i] + 1) * hp["r"], hp["mel_dim"]), i      # equal frame counts
            assert lin.shape == wl.shape and ali.shape == wa.shape and wav.shape == ww.shape, i
            errs = (rel_err(mel.cpu(), wm.cpu()), rel_err(lin.cpu(), wl.cpu()), rel_err(ali.cpu(), wa.cpu()))
            werr = float((wav - ww).abs().max() / ww.abs().max())
            print("utterance %2d cap %2d: mel %.2e linear %.2e alignment %.2e wav %.2e" % ((i, caps[i]) + errs + (werr,)))
            assert max(errs) < 1e-4, (i, errs)
            assert werr < 1e-3, (i, werr)
    finally:
        ops.set_gemm_precision(prev)


# ----------------------------------------------------------------------------------------------------------------------
# 4. refusals
# ----------------------------------------------------------------------------------------------------------------------
def test_persistent_program_refuses_slot_mode(dev):
    ops, L, S, C = _env()
    B, Cin = 2, 16
    x, y = torch.zeros(B, Cin, device=dev), _nan(dev, B, Cin)
    tiles = torch.zeros(L.dv3_conv_step_pack_floats(Cin, Cin, 0), device=dev)
    toff = torch.zeros(B, dtype=torch.int32, device=dev)
    arr = (S["dv3_decode_entry"] * 1)()
    c = arr[0].conv
    c.x, c.x_bs, c.a, c.y, c.y_bs = x.data_ptr(), Cin, tiles.data_ptr(), y.data_ptr(), Cin
    c.B, c.Cin, c.M, c.J, c.dil, c.mode = B, Cin, Cin, 1, 1, C["DV3_EPI_LINEAR"]
    c.t_off, c.t_cap = toff.data_ptr(), 4
    entries = torch.frombuffer(bytearray(bytes(arr)), dtype=torch.uint8).to(dev)
    sync = torch.zeros(L.dv3_decode_program_sync_ints(B), dtype=torch.int32, device=dev)
    steps_out = torch.zeros(1, dtype=torch.int32, device=dev)
    p = S["dv3_decode_program"]()
    p.entries, p.entries_host, p.n_entries, p.B = entries.data_ptr(), ctypes.addressof(arr), 1, B
    p.t0, p.n_steps, p.sync, p.steps_out = 0, 2, sync.data_ptr(), steps_out.data_ptr()
    rc = L.dv3_decode_program_run(ctypes.byref(p), ops._stream())
    msg = (L.dv3_last_error() or b"").decode()
    assert rc != 0 and "slot mode" in msg and "t_off" in msg, (rc, msg)
    torch.cuda.synchronize()
    assert bool(torch.isnan(y).all())                 # nothing was launched
    # ... and the Python layer says the same before it gets there
    model, _ = _toy("nyanko", dev)
    P = model.seq2seq.decoder.slot_program(2, 16)
    with pytest.raises(RuntimeError, match="persistent"):
        P.decode(None, None, None, 1, 1, False, persistent=True)


def test_slot_mode_refuses_ineligible_configurations(dev):
    from deepvoice3_pytorch_amd import synthesis
    for family in ("nyanko", "deepvoice3"):
        model, _ = _toy(family, dev)
        dec = model.seq2seq.decoder
        with pytest.raises(RuntimeError, match="not eligible"):
            dec.slot_program(4, 20000)                # the attention scores of 20000 keys do not fit the LDS
        dec.fast_decode = False                       # the module-by-module path is no fallback here
        with pytest.raises(RuntimeError, match="no module-by-module fallback"):
            synthesis.RollingSynthesizer(model, slots=4, max_text_len=16)


def test_submit_rejects_bad_requests(dev):
    from deepvoice3_pytorch_amd import audio, builder, synthesis
    torch.manual_seed(3)
    model = builder.nyanko(**dict(NY_HP, linear_dim=513)).to(dev).eval()     # 513 bins: retirement ends in Griffin-Lim
    model.seq2seq.decoder.max_decoder_steps = 40
    rs = synthesis.RollingSynthesizer(model, slots=2, max_text_len=12, audio_cfg=audio.AudioConfig(griffin_lim_iters=2))
    with pytest.raises(ValueError, match="empty"):
        rs.submit([])
    with pytest.raises(ValueError, match="max_text_len"):
        rs.submit(list(range(2, 15)))
    with pytest.raises(ValueError, match="max_decoder_steps"):
        rs.submit([3, 4], max_decoder_steps=model.seq2seq.decoder.max_decoder_steps + 1)
    with pytest.raises(ValueError, match="speaker_id"):
        rs.submit([3, 4], speaker_id=1)
    assert not rs.pending() and rs.poll() == []
    assert rs.submit([3, 4, 5]) == 0 and rs.submit([6] * 12, max_decoder_steps=3) == 1
    res = list(rs.drain())
    assert sorted(r[0] for r in res) == [0, 1] and not rs.pending()
    by = {r[0]: r for r in res}
    assert by[1][1].size(0) == 4 * NY_HP["r"]          # capped: 3 + 1 steps
    for tk, mel, lin, ali, wav in res:
        assert lin.shape == (mel.size(0) * NY_HP["downsample_step"], 513) and ali.size(1) == (3 if tk == 0 else 12)
        assert wav.numel() == audio.num_samples(lin.size(0), 256, "lws") and bool(torch.isfinite(wav).all())

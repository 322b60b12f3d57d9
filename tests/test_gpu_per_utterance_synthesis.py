# coding: utf-8
"""Per-utterance batched synthesis: each item of a ragged batch decodes as if it were alone.

  * the attention step kernel in its per-item mode (dv3_attn_step_f32 with key_len) against itself at B = 1 and
    Tk = key_len[b] (bit for bit) and an fp64 restatement;
  * the per-item zero tail on both activation layouts;
  * the decoder's per-item stop on every loop (library-launched, Python-launched, step graph, module by module)
    against B = 1 decodes, bit for bit;
  * MultiSpeakerTTSModel.synthesize_batch on the three presets against the oracle run on each utterance alone, and
    the default batched call as a control that the two semantics differ;
  * synthesis.tts_batch at 64 utterances against B = 1 library calls and, for 8 of them, the oracle;
  * Griffin-Lim with per-item frame counts (both framings) against each item's B = 1 call, bit for bit.
"""
import ctypes

import numpy as np
import pytest
import torch

from oracle import dv3_oracle as O
from tests.util import rel_err

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


def _preset(name):
    import bench
    bname, hp, _ = bench.PRESETS[name]
    return bname, dict(hp)


# -- 1. the attention step kernel ---------------------------------------------------------------------------------------
def _attn_step(q, k, v, tke, key_len, la, t, wb=1, wa=3):
    from deepvoice3_pytorch_amd import ops
    from deepvoice3_pytorch_amd._lib import STRUCTS
    B, E = q.shape
    Tk = k.size(1) if tke else k.size(2)
    ctx = torch.full((B, E), float("nan"), device=q.device)
    attn = torch.full((B, Tk), float("nan"), device=q.device)
    d = STRUCTS["dv3_attn_step_desc"]()
    d.q, d.q_bs, d.k, d.v, d.kv_tke = q.data_ptr(), E, k.data_ptr(), v.data_ptr(), int(tke)
    d.last_attended = la.data_ptr() if la is not None else None
    t_dev = torch.tensor([t], dtype=torch.int32, device=q.device)
    d.win_back, d.win_ahead, d.t = wb, wa, t_dev.data_ptr()
    d.ctx, d.ctx_bs, d.attn = ctx.data_ptr(), E, attn.data_ptr()
    d.B, d.E, d.Tk = B, E, Tk
    d.key_len = key_len.data_ptr() if key_len is not None else None
    ops._lib.call("dv3_attn_step_f32", ctypes.byref(d), ops._stream())
    torch.cuda.synchronize()
    return ctx, attn


@pytest.mark.parametrize("tke", [0, 1])
@pytest.mark.parametrize("monotonic", [True, False])
def test_attn_step_per_item_equals_b1(dev, tke, monotonic):
    g = torch.Generator().manual_seed(7)
    B, E, Tk = 7, 96, 40
    kl = [1, 3, 17, Tk, 25, 2, Tk]            # 1, below the window, mid, Tmax
    la0 = [0, 2, 9, 35, 0, 1, Tk - 1]         # starting windows, each inside its own keys
    q = torch.randn(B, E, generator=g).to(dev)
    k = torch.randn(B, Tk, E, generator=g).to(dev)
    v = torch.randn(B, Tk, E, generator=g).to(dev)
    kk, vv = (k, v) if tke else (k.transpose(1, 2).contiguous(), v.transpose(1, 2).contiguous())
    key_len = torch.tensor(kl, dtype=torch.int32, device=dev)
    t = 3                                     # reads slot 1, writes slot 0
    la = None
    if monotonic:
        la = torch.full((2, B), -7, dtype=torch.int32, device=dev)
        la[1] = torch.tensor(la0, dtype=torch.int32)
    ctx, attn = _attn_step(q, kk, vv, tke, key_len, la, t)
    torch.cuda.synchronize()
    for b in range(B):
        s = kl[b]
        k1 = k[b:b + 1, :s].contiguous() if tke else k[b:b + 1, :s].transpose(1, 2).contiguous()
        v1 = v[b:b + 1, :s].contiguous() if tke else v[b:b + 1, :s].transpose(1, 2).contiguous()
        la1 = torch.tensor([-7, la0[b]], dtype=torch.int32, device=dev) if monotonic else None
        c1, a1 = _attn_step(q[b:b + 1].contiguous(), k1, v1, tke, None, la1, t)
        torch.cuda.synchronize()
        assert torch.equal(attn[b, :s], a1[0]), b
        assert torch.equal(attn[b, s:], torch.zeros_like(attn[b, s:])), b
        assert torch.equal(ctx[b], c1[0]), b
        if monotonic:
            assert int(la[0, b]) == int(la1[0]), b
        # fp64 restatement (deepvoice3.py:143-171 at Tq = 1 with Tk = s)
        qd, kd, vd = q[b].double().cpu(), k[b, :s].double().cpu(), v[b, :s].double().cpu()
        sc = kd @ qd
        lo, hi = 0, s
        if monotonic:
            lo, hi = max(la0[b] - 1, 0), min(la0[b] + 3, s)
        m = torch.full((s,), float("-inf"), dtype=torch.float64)
        m[lo:hi] = sc[lo:hi]
        p = torch.softmax(m, 0)
        cw = (p @ vd) * (s * np.sqrt(1.0 / s))
        assert rel_err(attn[b, :s].cpu().double(), p) < 1e-5
        assert rel_err(ctx[b].cpu().double(), cw) < 1e-5
        if monotonic:
            assert int(la[0, b]) == int(torch.argmax(p))


# -- 2. the per-item zero tail --------------------------------------------------------------------------------------------
def test_zero_tail_per_item(dev):
    from deepvoice3_pytorch_amd import ops
    B, C, T, mult = 5, 40, 24, 2
    lens = torch.tensor([12, 1, 7, 0, 10], dtype=torch.int32)
    ld = lens.to(dev)
    x = torch.randn(B, C, T, device=dev)
    keep = (torch.arange(T)[None, :] < (lens[:, None] * mult)).to(dev)       # (B, T)
    want = x * keep[:, None, :]
    tail = T - int(lens.min()) * mult
    y = x.clone()
    ops.zero_tail(y, ld, tail, mult)
    assert torch.equal(y, want)
    # the channel-blocked bf16 layout [B][C8][T][8] (C = 40 pads to 64 channels)
    x8 = ops.to_c8(x)
    want8 = ops.from_c8(x8, C) * keep[:, None, :]
    ops.zero_tail(x8, ld, tail, mult)
    assert torch.equal(ops.from_c8(x8, C), want8)


# -- 3. per-item stop on every decode loop ---------------------------------------------------------------------------------
NY_HP = dict(n_vocab=40, embed_dim=32, mel_dim=20, linear_dim=33, r=1, downsample_step=4, padding_idx=0, dropout=0.05,
             kernel_size=3, encoder_channels=64, decoder_channels=64, converter_channels=32, max_positions=128,
             use_memory_mask=True, force_monotonic_attention=True, use_decoder_state_for_postnet_input=True)


def _pad_enc(encs, Tmax, g):
    """B = 1 encoder outputs padded into one batch; the padding is junk (the per-item decode must not read it)"""
    D = encs[0][0].size(2)
    K = torch.randn(len(encs), Tmax, D, generator=g).to(encs[0][0].device)
    V = torch.randn(len(encs), Tmax, D, generator=g).to(encs[0][0].device)
    for b, (k, v) in enumerate(encs):
        K[b, :k.size(1)] = k[0]
        V[b, :v.size(1)] = v[0]
    return K, V


def _set_mode(dec, mode):
    dec.fast_decode = mode != "module"
    dec.launched_decode = {"launched": True, "python": False, "graph": False}.get(mode)
    dec.use_step_graph = mode == "graph"


@pytest.mark.parametrize("mode", ["launched", "python", "graph", "module"])
def test_decoder_per_item_stop_equals_b1(dev, mode):
    from deepvoice3_pytorch_amd import builder
    torch.manual_seed(3)
    model = builder.nyanko(**NY_HP).to(dev).eval()
    dec = model.seq2seq.decoder
    _set_mode(dec, mode)
    g = torch.Generator().manual_seed(11)
    lens = [23, 9, 31, 4, 17, 12]
    B, Tmax = len(lens), max(lens)
    texts = [torch.randint(2, NY_HP["n_vocab"], (1, s), generator=g).to(dev) for s in lens]
    tpos = [torch.arange(1, s + 1, device=dev)[None] for s in lens]
    with torch.no_grad():
        encs = [model.seq2seq.encoder(tx) for tx in texts]
    K, V = _pad_enc(encs, Tmax, g)
    TP = torch.zeros(B, Tmax, dtype=torch.long, device=dev)
    for b, s in enumerate(lens):
        TP[b, :s] = tpos[b][0]

    def b1(b, per_item_module=True):
        dec.start_fresh_sequence()
        if mode == "module" and per_item_module:
            # The module loop's per-item attention read is the step kernel (dv3_attn_step_f32), its default one is the
            # attention forward kernel: bit for bit it can only be held to itself at B = 1, which shows the batch is
            # independent of B.  Against the ordinary B = 1 module decode it is held to a tolerance below.
            return dec.incremental_forward(encs[b], tpos[b], text_lengths=[lens[b]])[:4]
        return dec.incremental_forward(encs[b], tpos[b])

    # the done head shifted so that the items stop at different steps: a bias between the items' first crossings
    N = 24
    dec.min_decoder_steps = dec.max_decoder_steps = N
    with torch.no_grad():
        logits = []
        for b in range(B):
            dn = torch.cat([d.reshape(1) for d in b1(b)[2]]).double().cpu().clamp(1e-12, 1 - 1e-12)
            logits.append(torch.log(dn / (1 - dn)))
    L = torch.stack(logits)                               # (B, N + 1)
    best, delta = (0, 0.0), 0.0
    cs = torch.sort(L[:, 2:].reshape(-1)).values.tolist()
    for lo, hi in zip(cs[:-1], cs[1:]):
        cand = -0.5 * (lo + hi)                           # a threshold between two logits, away from both
        firsts = set(int(torch.nonzero(L[b, 2:] + cand > 0)[0]) if bool((L[b, 2:] + cand > 0).any()) else -1
                     for b in range(B))
        score = (len(firsts), hi - lo)
        if score > best:
            best, delta = score, cand
    with torch.no_grad():
        dec.fc.bias.add_(delta)
    dec.min_decoder_steps, dec.max_decoder_steps = 2, N
    with torch.no_grad():
        want = [b1(b) for b in range(B)]
        dec.start_fresh_sequence()
        out, ali, done, st, steps = dec.incremental_forward((K, V), TP, text_lengths=lens)
    torch.cuda.synchronize()
    stops = [w[0].size(1) for w in want]
    assert steps.tolist() == stops
    assert len(set(stops)) >= 3, (stops, best, L.min().item(), L.max().item())
    assert out.size(1) == max(stops)
    for b, (wo, wa, wd, ws) in enumerate(want):
        n, s = stops[b], lens[b]
        assert torch.equal(out[b, :n], wo[0]), b
        assert torch.equal(st[b, :n], ws[0]), b
        assert torch.equal(ali[b, :n, :s], wa[0]), b
        assert not ali[b, :n, s:].any() and not out[b, n:].any() and not st[b, n:].any() and not ali[b, n:].any()
        assert torch.equal(torch.cat([d[b].reshape(1) for d in done[:n]]), torch.cat([d.reshape(1) for d in wd]))
        assert not any(bool(d[b].any()) for d in done[n:])
    if mode == "module":                # against the ordinary B = 1 module-by-module decode (the reference's path)
        with torch.no_grad():
            plain = [b1(b, per_item_module=False) for b in range(B)]
        for b, (po, pa, pd, ps) in enumerate(plain):
            n = min(stops[b], po.size(1))
            assert rel_err(out[b, :n].cpu(), po[0, :n].cpu()) < 1e-5, b
            assert rel_err(st[b, :n].cpu(), ps[0, :n].cpu()) < 1e-5, b
            assert rel_err(ali[b, :n, :lens[b]].cpu(), pa[0, :n].cpu()) < 1e-5, b


def test_persistent_program_refuses_per_item(dev):
    from deepvoice3_pytorch_amd import builder
    torch.manual_seed(3)
    model = builder.nyanko(**NY_HP).to(dev).eval()
    dec = model.seq2seq.decoder
    dec.persistent_decode = True
    dec.min_decoder_steps = dec.max_decoder_steps = 5
    text = torch.randint(2, 40, (2, 9), device=dev)
    with torch.no_grad():
        enc = model.seq2seq.encoder(text)
        with pytest.raises(RuntimeError, match="persistent"):
            dec.incremental_forward(enc, torch.arange(1, 10, device=dev).repeat(2, 1), text_lengths=[9, 5])


# -- 4. / 5. synthesize_batch against the oracle per utterance, and the control ------------------------------------------
def _ragged(hp, lens, seed):
    rng = np.random.RandomState(seed)
    B, Tt = len(lens), max(lens)
    text = torch.zeros(B, Tt, dtype=torch.long)
    tpos = torch.zeros(B, Tt, dtype=torch.long)
    for b, s in enumerate(lens):
        text[b, :s] = torch.from_numpy(rng.randint(2, hp["n_vocab"], s))
        tpos[b, :s] = torch.arange(1, s + 1)
    spk = torch.from_numpy(rng.randint(0, hp["n_speakers"], B)) if hp["n_speakers"] > 1 else None
    return text, tpos, spk


@pytest.mark.parametrize("preset", ["deepvoice3_ljspeech", "nyanko_ljspeech", "deepvoice3_vctk"])
def test_synthesize_batch_matches_oracle_per_utterance(dev, preset):
    from deepvoice3_pytorch_amd import builder, ops
    prev = ops.set_gemm_precision("f16x3")
    try:
        bname, hp = _preset(preset)
        torch.manual_seed(13)
        model = getattr(builder, bname)(**hp).to(dev).eval()
        if bname == "nyanko":
            # nyanko has no key / value projections and its text embedding is initialised at std 0.01: the keys are
            # then its position code and nothing else, every item's attention follows the same path and the values
            # (the context) are ~0 -- the batch semantics could not show.  Text embeddings at std 0.3 make them show.
            with torch.no_grad():
                model.seq2seq.encoder.embed_tokens.weight.mul_(30.0)
        sd = {k: v.detach().cpu().clone() for k, v in model.state_dict().items()}
        spec = O.build_spec(bname, **hp)
        lens, steps = [57, 23, 40], 10
        B = len(lens)
        text, tpos, spk = _ragged(hp, lens, 5)
        dec = model.seq2seq.decoder
        dec.min_decoder_steps = dec.max_decoder_steps = steps
        spk_d = spk.to(dev) if spk is not None else None
        with torch.no_grad():
            mel, lin, ali, done, frames = model.synthesize_batch(text.to(dev), lens, spk_d)
            ctrl = model(text.to(dev), speaker_ids=spk_d, text_positions=tpos.to(dev))
            # teacher forced, per item (the encoder with the per-item zero tails, as synthesize_batch runs it)
            rng = np.random.RandomState(9)
            tf_in = torch.from_numpy(rng.rand(B, 12, hp["mel_dim"] * hp["r"]).astype(np.float32))
            prev_valid, ops.valid = ops.valid, ops.ItemLengths(lens, text.size(1), dev)
            try:
                se = model.embed_speakers(spk_d) if spk is not None else None
                enc = model.seq2seq.encoder(text.to(dev), speaker_embed=se)
            finally:
                ops.valid = prev_valid
            dec.start_fresh_sequence()
            kw = dict(speaker_embed=se) if se is not None else {}
            tf = dec.incremental_forward(enc, tpos.to(dev), test_inputs=tf_in.to(dev), text_lengths=lens, **kw)
            dec.start_fresh_sequence()
            tf_default = dec.incremental_forward(enc, tpos.to(dev), test_inputs=tf_in.to(dev), **kw)
        assert frames.tolist() == [steps + 1] * B
        ctrl_errs = {}

        def note(name, e):
            ctrl_errs[name] = max(ctrl_errs.get(name, 0.0), e)
        for b, s in enumerate(lens):
            tb, pb = text[b:b + 1, :s], tpos[b:b + 1, :s]
            sb = spk[b:b + 1] if spk is not None else None
            wm, wl, wa, _ = O.model_generate(sd, spec, tb, pb, sb, max_decoder_steps=steps, min_decoder_steps=steps)
            errs = dict(mel=rel_err(mel[b].cpu(), wm[0]), linear=rel_err(lin[b].cpu(), wl[0]),
                        alignments=rel_err(ali[b, :, :s].cpu(), wa[0]))
            for n, e in errs.items():
                assert e < 5e-4, (preset, b, n, e)
            assert not ali[b, :, s:].any()
            if b > 0:
                note("free mel", rel_err(ctrl[0][b].cpu(), wm[0]))
                note("free linear", rel_err(ctrl[1][b].cpu(), wl[0]))
                note("free alignments", rel_err(ctrl[2][b][..., :s].reshape(wa[0].shape).cpu(), wa[0]))
            se_c = torch.nn.functional.embedding(sb, sd["embed_speakers.weight"]) if sb is not None else None
            if bname == "nyanko":
                want = O.ny_incremental_decode(sd, spec, O.ny_encoder(sd, spec, tb), pb, test_inputs=tf_in[b:b + 1])
            else:
                want = O.dv3_incremental_decode(sd, spec, O.dv3_encoder(sd, spec, tb, se_c), pb, se_c,
                                                test_inputs=tf_in[b:b + 1])
            assert rel_err(tf[0][b].cpu(), want[0][0]) < 1e-4, (preset, b, "tf mel")
            assert rel_err(tf[3][b].cpu(), want[3][0]) < 1e-4, (preset, b, "tf states")
            assert rel_err(tf[1][b, :, :s].cpu(), want[1][0]) < 1e-4, (preset, b, "tf alignments")
            if b > 0:
                note("tf mel", rel_err(tf_default[0][b].cpu(), want[0][0]))
                note("tf states", rel_err(tf_default[3][b].cpu(), want[3][0]))
                note("tf alignments", rel_err(tf_default[1][b][..., :s].reshape(want[1][0].shape).cpu(), want[1][0]))
        # control: the default calls (free running and teacher forced) keep the reference's batch semantics -- item 0's
        # window, the padded keys' sqrt(Tk) -- which must differ from the per-utterance oracle for items 1..B-1
        assert max(ctrl_errs.values()) > 1e-2, ctrl_errs
    finally:
        ops.set_gemm_precision(prev)


# -- 6. config 5 at its stated size through tts_batch -------------------------------------------------------------------
def test_tts_batch_64_utterances(dev):
    from deepvoice3_pytorch_amd import builder, ops, synthesis, audio
    from oracle import audio_oracle as AO
    prev = ops.set_gemm_precision("f16x3")
    try:
        bname, hp = _preset("deepvoice3_ljspeech")
        torch.manual_seed(0)
        model = builder.deepvoice3(**hp).to(dev).eval()
        sd = {k: v.detach().cpu().clone() for k, v in model.state_dict().items()}
        spec = O.build_spec(bname, **hp)
        dec = model.seq2seq.decoder
        dec.min_decoder_steps = dec.max_decoder_steps = 23            # 24 steps
        rng = np.random.RandomState(21)
        lens = rng.randint(20, 101, 64).tolist()
        seqs = [rng.randint(2, hp["n_vocab"], s).tolist() for s in lens]
        cfg = audio.AudioConfig(griffin_lim_iters=2)
        res = synthesis.tts_batch(model, seqs, audio_cfg=cfg)
        assert len(res) == 64
        for b, (mel, lin, ali, wav) in enumerate(res):
            tb = torch.tensor([seqs[b]], device=dev)
            with torch.no_grad():
                wm, wl, wa, _ = model(tb, text_positions=torch.arange(1, lens[b] + 1, device=dev)[None])
            assert mel.shape == wm[0].shape and lin.shape == wl[0].shape and ali.shape == wa[0].shape
            assert rel_err(mel.cpu(), wm[0].cpu()) < 1e-4, b
            assert rel_err(lin.cpu(), wl[0].cpu()) < 1e-4, b
            assert rel_err(ali.cpu(), wa[0].cpu()) < 1e-4, b
            if b % 8 == 0:
                om, ol, oa, _ = O.model_generate(sd, spec, tb.cpu(), torch.arange(1, lens[b] + 1)[None],
                                                 max_decoder_steps=23, min_decoder_steps=23)
                assert rel_err(mel.cpu(), om[0]) < 5e-4 and rel_err(lin.cpu(), ol[0]) < 5e-4, b
                wwant = AO.inv_preemphasis(AO.lws_griffin_lim(AO.magnitudes(ol.numpy()), 2), 0.97)[0]
                assert wav.shape == (wwant.shape[0],)
                assert float(np.abs(wav.cpu().numpy() - wwant).max() / np.abs(wwant).max()) < 1e-3, b
    finally:
        ops.set_gemm_precision(prev)


# -- 7. Griffin-Lim per item --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("convention", ["lws", "torch"])
def test_griffin_lim_per_item_equals_b1(dev, convention):
    from deepvoice3_pytorch_amd import audio
    g = torch.Generator().manual_seed(5)
    frames = [37, 4, 60, 23, 5]                       # 4: the fewest the lws framing takes at hop 256, 5 the torch one
    if convention == "torch":
        frames[1] = 5
    B, T = len(frames), max(frames)
    lin = torch.rand(B, T, 513, generator=g).to(dev)
    cfg = audio.AudioConfig(griffin_lim_iters=3, convention=convention)
    wav, samples = audio.inv_spectrogram_batch(lin, cfg, frame_lengths=frames)
    torch.cuda.synchronize()
    assert wav.shape == (B, audio.num_samples(T, 256, convention))
    for b, n in enumerate(frames):
        want = audio.inv_spectrogram_batch(lin[b:b + 1, :n].contiguous(), cfg)[0]
        torch.cuda.synchronize()
        assert int(samples[b]) == want.numel() == audio.num_samples(n, 256, convention), b
        assert torch.equal(wav[b, :want.numel()], want), (b, float((wav[b, :want.numel()] - want).abs().max()))
        assert not wav[b, want.numel():].any(), b

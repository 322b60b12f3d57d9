# coding: utf-8
"""-m gpu: duration control -- decoding under a prescribed token alignment.

  1. dv3_guide_from_durations_i32 bit for bit against tests/guided_ref.guide_table: key counts 1, 63, 64, 65, 130 at
     B = 5, T equal to, below and above the sum, zero-duration runs at the start, in the middle and at the end, a strided
     table whose guard band keeps its pattern, every flag bit provoked by data, key counts outside [1, Tk] clamped;
  2. dv3_attn_step_guided_f32 element by element against decode_step_ref.attn_step_ref at the guide's key, within
     decode_step_ref.attn_step_bound, exact zeros outside the window, last_attended untouched;
  3. guided at the free run's own centres is the free run, bit for bit (one attention layer, both families);
  4. a guided batch of 5 ragged items equals the five B = 1 guided calls, bit for bit;
  5. the launched driver (one dv3_decode_program_launch_guided call) and the Python-driven one agree bit for bit on the
     decoder with two attention layers;
  6. tts_batch(durations=D, guide_window=(0, 1), timings=True, diagnostics=True): one-hot rows at the guide, the searched
     durations are D, every length follows from sum(D); fit_durations' result decodes to exactly its total;
  7. the refusals, each by its message.
"""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tests import decode_step_ref as R, guided_ref  # noqa: E402
from tests.test_gpu_rolling_decode import NY_HP, DV3_HP  # noqa: E402  (the toy hyper-parameters)

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


def _i32(v, dev):
    return torch.as_tensor(np.asarray(v), dtype=torch.int32).to(dev)


# ----------------------------------------------------------------------------------------------------------------------
# 1. the guide table
# ----------------------------------------------------------------------------------------------------------------------
KEY_LENS = [1, 63, 64, 65, 130]
SUM = 150


def _durations():
    """(5, 130) durations, every item summing to SUM over its own keys, with runs of zeros at the start (item 1), in the
    middle (item 2), at the end (item 3) and all three (item 4); past an item's keys: junk that must not be read"""
    rng = np.random.RandomState(7)
    Tk = max(KEY_LENS)
    dur = rng.randint(50, 90, (len(KEY_LENS), Tk))
    zero = {1: [(0, 5)], 2: [(30, 41)], 3: [(60, 65)], 4: [(0, 3), (64, 70), (120, 130)]}
    for b, n in enumerate(KEY_LENS):
        d = rng.randint(0, 4, n)
        for lo, hi in zero.get(b, []):
            d[lo:hi] = 0
        live = np.nonzero(d)[0] if d.any() else np.array([0])
        d[live[0]] += SUM - d.sum() if d.sum() <= SUM else 0
        while d.sum() > SUM:                      # take the excess off the largest entries
            d[np.argmax(d)] -= 1
        dur[b, :n] = d
        assert d.sum() == SUM and d.min() >= 0
    return dur


@pytest.mark.parametrize("T", [SUM, 97, 200])
def test_guide_table_bit_for_bit(dev, T):
    from deepvoice3_pytorch_amd import ops
    dur = _durations()
    want_g, want_s, want_f = guided_ref.guide_table(dur, KEY_LENS, T)
    for b, n in enumerate(KEY_LENS):              # the restatement is np.repeat, here too
        rep = np.repeat(np.arange(n), dur[b, :n])[:T]
        assert np.array_equal(want_g[b, :len(rep)], rep) and want_s[b] == len(rep)
    buf = torch.full((len(KEY_LENS), T + 9), -7777, dtype=torch.int32, device=dev)
    g, steps, flags = ops.guide_from_durations(_i32(dur, dev), _i32(KEY_LENS, dev), T, guide=buf[:, :T])
    torch.cuda.synchronize()
    assert g.data_ptr() == buf.data_ptr() and g.stride(0) == T + 9
    assert np.array_equal(g.cpu().numpy(), want_g)
    assert steps.tolist() == want_s.tolist() == [min(SUM, T)] * len(KEY_LENS)
    assert flags.tolist() == want_f.tolist() == [guided_ref.OVER if SUM > T else 0] * len(KEY_LENS)
    assert bool((buf[:, T:] == -7777).all()), "the guard band past the table's rows was written"
    fresh = ops.guide_from_durations(_i32(dur, dev), _i32(KEY_LENS, dev), T)
    assert fresh[0].shape == (len(KEY_LENS), T) and torch.equal(fresh[0], g) and torch.equal(fresh[1], steps)


def test_guide_table_flags_and_clamps(dev):
    from deepvoice3_pytorch_amd import ops, _lib
    big = 2 ** 31 - 1
    dur = np.array([[3, -2, 4, 0, 1, 9, 9, 9],            # negative
                    [0, 0, 0, 0, 0, 0, 0, 0],             # empty
                    [5, 5, 5, 5, 5, 5, 5, 5],             # over
                    [big, big, big, -big, 1, 1, 1, 1],    # over + negative, sums that leave int32
                    [2, 1, 0, 0, 0, 0, 0, 0],             # key_len above Tk: clamped to 8
                    [4, 7, 7, 7, 7, 7, 7, 7]])            # key_len 0: clamped to 1
    key_len = [5, 8, 8, 8, 500, 0]
    T = 12
    want_g, want_s, want_f = guided_ref.guide_table(dur, key_len, T)
    assert want_f.tolist() == [guided_ref.NEGATIVE, guided_ref.EMPTY, guided_ref.OVER,
                               guided_ref.OVER | guided_ref.NEGATIVE, 0, 0]
    assert want_s.tolist() == [8, 0, 12, 12, 3, 4]
    g, steps, flags = ops.guide_from_durations(_i32(dur, dev), _i32(key_len, dev), T)
    torch.cuda.synchronize()
    assert flags.tolist() == want_f.tolist() and steps.tolist() == want_s.tolist()
    assert np.array_equal(g.cpu().numpy(), want_g)
    assert int(g.min()) >= 0 and int(g.max()) < 8
    assert [ops.guide_flag_names(f) for f in flags.tolist()[:4]] == [("negative",), ("empty",), ("over",),
                                                                      ("negative", "over")]
    # the entry point by name: what the host refuses
    L = _lib.lib()
    d, kl = _i32(dur, dev), _i32(key_len, dev)
    assert L.dv3_guide_from_durations_i32(d.data_ptr(), 8, kl.data_ptr(), 6, 8, T, g.data_ptr(), T - 1, steps.data_ptr(),
                                          flags.data_ptr(), ops._stream()) != 0
    assert "guide_bs" in (L.dv3_last_error() or b"").decode()
    assert L.dv3_guide_from_durations_i32(d.data_ptr(), 8, kl.data_ptr(), 6, 4096, T, g.data_ptr(), T, steps.data_ptr(),
                                          flags.data_ptr(), ops._stream()) != 0
    assert "Tk" in (L.dv3_last_error() or b"").decode()


# ----------------------------------------------------------------------------------------------------------------------
# 2. the guided attention step
# ----------------------------------------------------------------------------------------------------------------------
ATTN_SHAPES = {"b5_e96_tk40": (5, 96, 40, [40, 7, 23, 1, 33], [6, 1, 9, 3, 12]),
               "b3_e300_tk257": (3, 300, 257, [257, 130, 65], [10, 4, 7])}


@pytest.fixture(scope="module")
def attn_data():
    """per shape: q, k (B, Tk, E), v, the guide table and its fp64 inputs, made once"""
    out = {}
    for name, (B, E, Tk, key_len, steps) in ATTN_SHAPES.items():
        rng = np.random.RandomState(len(name))
        q = rng.standard_normal((B, E)).astype(np.float32) * 0.5
        k = rng.standard_normal((B, Tk, E)).astype(np.float32) * 0.5
        v = rng.standard_normal((B, Tk, E)).astype(np.float32)
        T = max(steps) + 3
        guide = np.stack([rng.randint(0, key_len[b], T) for b in range(B)]).astype(np.int32)
        guide[0, 0], guide[0, 1] = 0, key_len[0] - 1          # both ends of the key axis
        out[name] = (q, k, v, guide)
    return out


@pytest.mark.parametrize("window", [(1, 3), (0, 1), (2, 5)])
@pytest.mark.parametrize("tke", [0, 1])
@pytest.mark.parametrize("shape", sorted(ATTN_SHAPES))
def test_attn_step_guided_elementwise(dev, attn_data, shape, tke, window):
    from deepvoice3_pytorch_amd import ops
    B, E, Tk, key_len, steps = ATTN_SHAPES[shape]
    q, k, v, guide = attn_data[shape]
    wb, wa = window
    qd = torch.from_numpy(q).to(dev).reshape(B, E, 1)
    kd, vd = (torch.from_numpy(a if tke else np.ascontiguousarray(a.transpose(0, 2, 1))).to(dev) for a in (k, v))
    gd, sd, kl = _i32(guide, dev), _i32(steps, dev), _i32(key_len, dev)
    pattern = torch.arange(2 * B, dtype=torch.int32, device=dev).reshape(2, B) * 37 - 11
    la = pattern.clone()
    t_dev = torch.zeros(1, dtype=torch.int32, device=dev)
    ts = sorted({0, min(steps) - 1, min(steps), max(steps) - 1, max(steps), max(steps) + 2})
    for i, t in enumerate(ts):                    # 0, below, at and past the items' steps
        if i % 2:                                 # the step from the device counter, and as a host value
            t_dev.fill_(t)
        ctx, attn = ops.attn_step_guided(qd, kd, vd, kl, gd, sd, t_dev if i % 2 else t, wb, wa, last_attended=la,
                                         kv_tke=bool(tke))
        torch.cuda.synchronize()
        ctx, attn = ctx.cpu().numpy()[:, :, 0].astype(np.float64), attn.cpu().numpy()[:, 0].astype(np.float64)
        for b in range(B):
            centre = int(guide[b][min(t, steps[b] - 1)])
            ref = R.attn_step_ref(q[b], k[b], v[b], la=centre, win_back=wb, win_ahead=wa, key_len=key_len[b])
            ep, ectx = R.attn_step_bound(ref, E, Tk)
            out = np.ones(Tk, dtype=bool)
            out[ref["lo"]:ref["hi"]] = False
            assert ref["lo"] <= centre < ref["hi"] <= key_len[b]
            assert not attn[b][out].any(), (shape, t, b, "probabilities outside the window are exact zeros")
            err_p, err_c = np.abs(attn[b] - ref["p"]), np.abs(ctx[b] - ref["ctx"])
            assert (err_p <= ep).all(), (shape, tke, window, t, b, float((err_p - ep).max()))
            assert (err_c <= ectx).all(), (shape, tke, window, t, b, float((err_c - ectx).max()))
    assert torch.equal(la, pattern), "the guided step wrote last_attended"


def test_attn_step_guided_refuses(dev):
    """dv3_attn_step_guided_f32 and dv3_decode_program_launch_guided by name: what the host refuses, nothing launched"""
    from deepvoice3_pytorch_amd import ops, _lib
    L = _lib.lib()
    B, E, Tk = 2, 8, 6
    f = lambda *s: torch.zeros(*s, device=dev)
    q, k, v, ctx = f(B, E), f(B, Tk, E), f(B, Tk, E), f(B, E)
    kl, guide, steps, toff = _i32([6, 3], dev), _i32(np.zeros((B, 4)), dev), _i32([4, 2], dev), _i32([0, 0], dev)

    def desc(**kw):
        d = _lib.STRUCTS["dv3_attn_step_desc"]()
        d.q, d.q_bs, d.k, d.v, d.kv_tke = q.data_ptr(), E, k.data_ptr(), v.data_ptr(), 1
        d.ctx, d.ctx_bs, d.B, d.E, d.Tk = ctx.data_ptr(), E, B, E, Tk
        d.win_back, d.win_ahead, d.key_len, d.t_value = 1, 3, kl.data_ptr(), 0
        for name, val in kw.items():
            setattr(d, name, val)
        return d

    def refused(d, word, guide_bs=4):
        assert L.dv3_attn_step_guided_f32(ctypes.byref(d), guide.data_ptr(), guide_bs, steps.data_ptr(), ops._stream()) != 0
        assert word in (L.dv3_last_error() or b"").decode(), L.dv3_last_error()

    t_dev = torch.zeros(1, dtype=torch.int32, device=dev)
    refused(desc(t_off=toff.data_ptr(), t_cap=4, t=t_dev.data_ptr()), "slot mode")
    refused(desc(key_len=None), "key_len")
    refused(desc(win_ahead=0), "win_ahead")
    refused(desc(win_back=-1), "win_back")
    refused(desc(t_value=4), "guide_bs")
    Entry, Prog = _lib.STRUCTS["dv3_decode_entry"], _lib.STRUCTS["dv3_decode_program"]
    arr = (Entry * 1)()
    arr[0].kind, arr[0].attn = 1, desc()
    p = Prog()
    p.entries_host, p.n_entries, p.B, p.t0, p.n_steps = ctypes.addressof(arr), 1, B, 2, 3
    assert L.dv3_decode_program_launch_guided(ctypes.byref(p), guide.data_ptr(), 4, steps.data_ptr(), ops._stream()) != 0
    assert "guide_bs" in (L.dv3_last_error() or b"").decode()
    arr[0].attn = desc(t_off=toff.data_ptr(), t_cap=4)
    assert L.dv3_decode_program_launch_guided(ctypes.byref(p), guide.data_ptr(), 8, steps.data_ptr(), ops._stream()) != 0
    assert "slot mode" in (L.dv3_last_error() or b"").decode()
    torch.cuda.synchronize()


# ----------------------------------------------------------------------------------------------------------------------
# 3. - 5. the decoders
# ----------------------------------------------------------------------------------------------------------------------
LENS = [20, 3, 11, 7, 16]
N_STEPS = 12


def _memory(dev, lens, enc, seed):
    """encoder outputs (keys, values) (B, Tt, .) of random ragged texts (padding id 0 past each item's length) -- from the
    toy model's encoder, or random ones of 32 channels for the bare decoder -- and the text positions"""
    g = torch.Generator().manual_seed(seed)
    B, Tt = len(lens), max(lens)
    text = torch.zeros(B, Tt, dtype=torch.long)
    TP = torch.zeros(B, Tt, dtype=torch.long)
    for b, s in enumerate(lens):
        text[b, :s] = torch.randint(2, 40, (s,), generator=g)
        TP[b, :s] = torch.arange(1, s + 1)
    if enc is None:
        mem = tuple((torch.randn(B, Tt, 32, generator=g) * 0.3).to(dev) for _ in range(2))
    else:
        with torch.no_grad():
            mem = tuple(m.contiguous() for m in enc(text.to(dev)))
    return mem, TP.to(dev)


def _decoder(family, dev):
    from deepvoice3_pytorch_amd import builder, deepvoice3
    torch.manual_seed(3)
    enc = None
    if family == "nyanko":                        # one attention layer: the family's only kind
        model = builder.nyanko(**NY_HP).to(dev).eval()
        enc, dec = model.seq2seq.encoder, model.seq2seq.decoder
    elif family == "deepvoice3_one":              # a deepvoice3 decoder with a single attention flag
        dec = deepvoice3.Decoder(32, 1, 16, in_dim=20, r=2, max_positions=128, padding_idx=0, preattention=[(32, 3, 1)],
                                 convolutions=[(32, 3, 1), (32, 3, 3)], attention=[True, False], dropout=0.05,
                                 force_monotonic_attention=True, key_projection=True, value_projection=True).to(dev).eval()
    else:                                         # the toy deepvoice3: attention on its first and last layer
        model = builder.deepvoice3(**DV3_HP).to(dev).eval()
        enc, dec = model.seq2seq.encoder, model.seq2seq.decoder
        assert sum(a is not None for a in dec.attention) == 2
    dec.min_decoder_steps, dec.max_decoder_steps = 2, N_STEPS
    return dec, enc


def _run(dec, mem, TP, lens, **kw):
    dec.start_fresh_sequence()
    with torch.no_grad():
        out = dec.incremental_forward(mem, TP, text_lengths=lens, **kw)
    torch.cuda.synchronize()
    return out


def _same_results(a, b, steps, lens, what):
    (ao, aa, ad, ast, an), (bo, ba, bd, bst, bn) = a, b
    for i, n in enumerate(steps):
        assert torch.equal(ao[i, :n], bo[i, :n]), (what, i, "mel")
        assert torch.equal(aa[i, :n, :lens[i]], ba[i, :n, :lens[i]]), (what, i, "alignment")
        assert torch.equal(ast[i, :n], bst[i, :n]), (what, i, "states")
        assert torch.equal(torch.cat([d[i].reshape(1) for d in ad[:n]]), torch.cat([d[i].reshape(1) for d in bd[:n]])), \
            (what, i, "done")


@pytest.mark.parametrize("family", ["nyanko", "deepvoice3_one"])
def test_guided_at_free_centres_is_free_run(dev, family):
    """(the decoder call synthesize_batch makes, on random memories: Decoder.incremental_forward(text_lengths=...))"""
    dec, enc = _decoder(family, dev)
    mem, TP = _memory(dev, LENS, enc, 5)
    free = _run(dec, mem, TP, LENS)
    steps = [int(n) for n in free[4]]
    assert max(steps) <= N_STEPS + 1 and min(steps) >= 3
    ali = free[1].cpu().numpy()
    T = N_STEPS + 1
    guide = np.zeros((len(LENS), T), dtype=np.int32)
    for b, n in enumerate(steps):
        for t in range(1, n):
            guide[b, t] = int(np.argmax(ali[b, t - 1]))              # the first maximum
        guide[b, n:] = guide[b, n - 1]
    assert guide.max() > 0, "the free run never left key 0: the test would show nothing"
    got = _run(dec, mem, TP, LENS, guide=(_i32(guide, dev), _i32(steps, dev)))
    assert got[4].tolist() == steps and got[0].size(1) == max(steps)
    _same_results(got, free, steps, LENS, family)
    for b, n in enumerate(steps):                 # zero tails, as the free run has them
        assert not got[0][b, n:].any() and not got[1][b, n:].any()


def _guide_for(dev, lens, seed, T):
    rng = np.random.RandomState(seed)
    dur = np.zeros((len(lens), max(lens)), dtype=np.int32)
    for b, s in enumerate(lens):
        want = int(rng.randint(max(3, T // 2), T + 1))
        cuts = np.sort(rng.randint(0, want + 1, s - 1))
        dur[b, :s] = np.diff(np.concatenate([[0], cuts, [want]]))
    from deepvoice3_pytorch_amd import ops
    g, steps, flags = ops.guide_from_durations(_i32(dur, dev), _i32(lens, dev), T)
    assert not flags.any()
    return g, steps, dur


@pytest.mark.parametrize("family", ["nyanko", "deepvoice3_two"])
def test_guided_batch_items_as_if_alone(dev, family):
    dec, enc = _decoder(family, dev)
    mem, TP = _memory(dev, LENS, enc, 6)
    g, steps, _ = _guide_for(dev, LENS, 8, N_STEPS + 1)
    counts = steps.tolist()
    assert len(set(counts)) >= 3
    batch = _run(dec, mem, TP, LENS, guide=(g, steps))
    assert batch[4].tolist() == counts
    for b, s in enumerate(LENS):
        one = _run(dec, (mem[0][b:b + 1, :s].contiguous(), mem[1][b:b + 1, :s].contiguous()), TP[b:b + 1, :s].contiguous(),
                   [s], guide=(g[b:b + 1].contiguous(), steps[b:b + 1].contiguous()))
        n = counts[b]
        assert one[0].size(1) == n
        assert torch.equal(batch[0][b, :n], one[0][0]), (b, "mel")
        assert torch.equal(batch[1][b, :n, :s], one[1][0]), (b, "alignment")
        assert torch.equal(batch[3][b, :n], one[3][0]), (b, "states")
        assert torch.equal(torch.cat([d[b].reshape(1) for d in batch[2][:n]]), torch.cat([d.reshape(1) for d in one[2]]))
        assert not batch[0][b, n:].any() and not batch[1][b, n:].any() and not batch[1][b, :, s:].any()


@pytest.mark.parametrize("window", [None, (0, 2)])
def test_guided_drivers_agree(dev, window):
    dec, enc = _decoder("deepvoice3_two", dev)
    mem, TP = _memory(dev, LENS, enc, 9)
    g, steps, _ = _guide_for(dev, LENS, 10, N_STEPS + 1)
    dec.launched_decode = True
    launched = _run(dec, mem, TP, LENS, guide=(g, steps), guide_window=window)
    dec.launched_decode = False
    stepped = _run(dec, mem, TP, LENS, guide=(g, steps), guide_window=window)
    assert launched[4].tolist() == stepped[4].tolist() == steps.tolist()
    _same_results(launched, stepped, steps.tolist(), LENS, "drivers")
    if window is not None:                        # the window is the override: at most 2 keys of a row are not zero
        assert int((launched[1] != 0).sum(dim=2).max()) <= 2


# ----------------------------------------------------------------------------------------------------------------------
# 6. the public API
# ----------------------------------------------------------------------------------------------------------------------
def _toy(family, dev):
    from deepvoice3_pytorch_amd import builder, audio
    torch.manual_seed(3)
    make, hp = dict(nyanko=(builder.nyanko, NY_HP), deepvoice3=(builder.deepvoice3, DV3_HP))[family]
    hp = dict(hp, linear_dim=257)                 # the bins of a 512-point FFT: results end in Griffin-Lim
    model = make(**hp).to(dev).eval()
    model.seq2seq.decoder.max_decoder_steps = 40
    cfg = audio.AudioConfig(fft_size=512, hop_size=128, sample_rate=16000, griffin_lim_iters=2)
    return model, hp, cfg


@pytest.mark.parametrize("family", ["nyanko", "deepvoice3"])
def test_tts_batch_hard_window_round_trip(dev, family):
    from deepvoice3_pytorch_amd import audio, ops, synthesis
    model, hp, cfg = _toy(family, dev)
    rng = np.random.RandomState(5)
    lens = [9, 3, 14, 6]
    seqs = [rng.randint(2, hp["n_vocab"], s).tolist() for s in lens]
    D = [rng.randint(1, 4, s).tolist() for s in lens]               # every token spoken: the J = 1 search can find it
    r, up = hp["r"], max(hp["downsample_step"] // hp["r"], 1)
    sps = r * up * 128 / 16000.0

    def check(D, res):
        for b, (mel, linear, ali, wav, stats, span) in enumerate(res):
            n = sum(D[b])
            centre = np.repeat(np.arange(lens[b]), D[b])
            onehot = torch.zeros(n, lens[b], device=dev)
            onehot[torch.arange(n), torch.from_numpy(centre).to(dev)] = 1.0
            assert ali.shape == (n, lens[b]) and torch.equal(ali, onehot), (b, "one-hot rows at the guide")
            assert mel.shape == (n * r, hp["mel_dim"]) and linear.shape == (n * r * up, 257)
            assert wav.numel() == audio.num_samples(n * r * up, cfg.hop_size, cfg.convention, cfg.fft_size)
            assert stats["steps"] == n and stats["keys"] == lens[b]
            assert span["durations"].tolist() == D[b] and span["path"].tolist() == centre.tolist()
            ends = np.cumsum(D[b]).astype(np.float64) * sps
            assert span["end"].tolist() == ends.tolist()
            assert span["start"].tolist() == ((np.cumsum(D[b]) - np.asarray(D[b])).astype(np.float64) * sps).tolist()
            _, _, searched = ops.monotonic_path(ali[None].contiguous(), _i32([n], dev), _i32([lens[b]], dev))
            assert searched[0].tolist() == D[b]

    res = synthesis.tts_batch(model, seqs, audio_cfg=cfg, durations=D, guide_window=(0, 1), timings=True, diagnostics=True)
    check(D, res)
    _, _, _, _, frames = model.synthesize_batch(*_padded(seqs, dev), durations=D, guide_window=(0, 1))
    assert frames.tolist() == [sum(d) * r for d in D]
    # the same durations fitted to another total decode to exactly that total
    totals = [sum(d) + 5 for d in D[:2]] + [sum(d) - 4 for d in D[2:]]
    fitted = [synthesis.fit_durations(d, n, min_steps=1) for d, n in zip(D, totals)]
    assert [sum(d) for d in fitted] == totals
    check(fitted, synthesis.tts_batch(model, seqs, audio_cfg=cfg, durations=fitted, guide_window=(0, 1), timings=True,
                                      diagnostics=True))
    # the durations as the device tensor ops.monotonic_path returns: the same bits as the lists
    dt = torch.zeros(len(lens), max(lens), dtype=torch.int32)
    for b, d in enumerate(D):
        dt[b, :len(d)] = torch.tensor(d, dtype=torch.int32)
    again = synthesis.tts_batch(model, seqs, audio_cfg=cfg, durations=dt.to(dev), guide_window=(0, 1))
    for a, b in zip(again, res):
        assert all(torch.equal(x, y) for x, y in zip(a[:4], b[:4]))


def _padded(seqs, dev):
    lens = [len(s) for s in seqs]
    text = torch.zeros(len(seqs), max(lens), dtype=torch.long)
    for b, s in enumerate(seqs):
        text[b, :len(s)] = torch.tensor(s)
    return text.to(dev), lens


# ----------------------------------------------------------------------------------------------------------------------
# 7. refusals
# ----------------------------------------------------------------------------------------------------------------------
def test_guided_refusals(dev):
    from deepvoice3_pytorch_amd import synthesis
    model, hp, cfg = _toy("nyanko", dev)
    dec = model.seq2seq.decoder
    seqs = [[5, 6, 7, 8], [9, 10]]
    D = [[1, 2, 1, 1], [2, 2]]
    kw = dict(audio_cfg=cfg)
    with pytest.raises(ValueError, match="stall_limit"):
        synthesis.tts_batch(model, seqs, durations=D, stall_limit=4, **kw)
    with pytest.raises(ValueError, match="item 1 has 3 durations for its 2 tokens"):
        synthesis.tts_batch(model, seqs, durations=[D[0], [1, 1, 1]], **kw)
    with pytest.raises(ValueError, match="item 0 are flagged negative"):
        synthesis.tts_batch(model, seqs, durations=[[1, -2, 1, 1], D[1]], **kw)
    with pytest.raises(ValueError, match="item 1 are flagged empty"):
        synthesis.tts_batch(model, seqs, durations=[D[0], [0, 0]], **kw)
    cap = dec.max_decoder_steps + 1
    synthesis.tts_batch(model, seqs, durations=[D[0], [cap - 1, 1]], **kw)            # the cap itself is taken
    with pytest.raises(ValueError, match="item 1 are flagged over"):
        synthesis.tts_batch(model, seqs, durations=[D[0], [cap, 1]], **kw)
    with pytest.raises(ValueError, match="slot mode"):
        list(synthesis.tts_stream(model, seqs, durations=D, **kw))
    # the decoder and the step program
    mem, TP = _memory(dev, [4, 2], model.seq2seq.encoder, 1)
    guide = (_i32([[0, 1, 2, 3], [0, 0, 1, 1]], dev), _i32([4, 3], dev))
    dec.persistent_decode = True
    with pytest.raises(RuntimeError, match="persistent=True does not take a guide"):
        _run(dec, mem, TP, [4, 2], guide=guide)
    dec.persistent_decode = None
    with pytest.raises(ValueError, match="a guide needs text_lengths"):
        dec.incremental_forward(mem, TP, guide=guide)
    dec.fast_decode = False
    with pytest.raises(RuntimeError, match="fused decode-step kernels only"):
        _run(dec, mem, TP, [4, 2], guide=guide)
    dec.fast_decode = True
    P = dec.slot_program(2, 8)
    with pytest.raises(RuntimeError, match="a slot-mode program does not take a guide"):
        P.decode(None, None, P.dones_seq, 1, 5, False, stops=[0, 0], guide=guide)
    torch.cuda.synchronize()

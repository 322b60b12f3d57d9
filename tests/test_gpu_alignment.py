# coding: utf-8
"""-m gpu: alignment diagnostics and the end-of-text stop.

  1. dv3_alignment_stats_f32 against tests/alignment_ref.py at the wave boundary (Tk 63 / 64 / 65), one key, several
     passes per lane (130), one, two and 67 steps, in both layouts (the stacked one as a genuinely strided view), with
     planted ties, a maximum on the last valid key and a NaN row; everything outside an item's own rows and keys is NaN;
  2. the refusals;
  3. tts_batch(diagnostics=True) on toy models of both decoder families;
  4. the stop rule through tts_stream at chunk 1, 3 and 8 and through tts_batch.
"""
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tests import alignment_ref as AR  # noqa: E402
from tests.test_gpu_rolling_decode import NY_HP, DV3_HP  # noqa: E402  (the toy hyper-parameters)

pytestmark = pytest.mark.gpu

NAN = float("nan")
B = 5


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


# ----------------------------------------------------------------------------------------------------------------------
# 1. the kernel
# ----------------------------------------------------------------------------------------------------------------------
def _case(T, Tk):
    """-> attn (B, T, Tk) fp32 with NaN outside every item's own rows and keys, steps, key_len (as the caller passes
    them: steps[2] = 2 exceeds T = 1 and is clamped by the kernel)"""
    rng = np.random.RandomState(1000 * T + Tk)
    steps = [0, 1, 2, T, T - 1]
    keys = [Tk, 1, Tk, max((2 * Tk) // 3, min(Tk, 2)), max(Tk - 1, 1)]
    a = np.full((B, T, Tk), NAN, dtype=np.float32)
    for b in range(B):
        n, m = min(max(steps[b], 0), T), keys[b]
        s = rng.randn(n, m).astype(np.float32) * 3.0
        e = np.exp(s - s.max(axis=1, keepdims=True))
        a[b, :n, :m] = (e / e.sum(axis=1, keepdims=True)).astype(np.float32)

    def plant(b, t, kind):
        n, m = min(max(steps[b], 0), T), keys[b]
        if t >= n:
            return
        r = a[b, t, :m]
        top = np.float32(r.max() * 1.5)
        if kind == "tie" and m >= 2:
            j = sorted(rng.choice(m, 2, replace=False))
            r[j[0]] = r[j[1]] = top                   # the first of the two wins
        elif kind == "last":
            r[m - 1] = top
        elif kind == "nan":
            r[rng.randint(m)] = NAN

    plant(1, 0, "tie")          # (one key: nothing to tie)
    plant(2, 0, "last")
    plant(2, 1, "tie")
    plant(3, 0, "nan")
    if T >= 3:
        plant(3, T // 2, "tie")
        plant(3, T - 1, "last")
        plant(4, 1, "last")
        plant(4, T - 2, "tie")
    return a, steps, keys


def _bits(t):
    return t.contiguous().view(torch.int32)


@pytest.mark.parametrize("layout", ["btk", "tbk"])
@pytest.mark.parametrize("T", [1, 2, 67])
@pytest.mark.parametrize("Tk", [1, 63, 64, 65, 130])
def test_alignment_stats_against_reference(dev, Tk, T, layout):
    from deepvoice3_pytorch_amd import ops
    a, steps, keys = _case(T, Tk)
    want = AR.batch_stats(a, steps, keys)
    if T >= 3 and Tk >= 3:       # the planted rows are in play
        assert want[3]["bad_rows"] == 1 and want[3]["end_step"] >= 0
    if layout == "btk":
        buf = torch.from_numpy(a).to(dev)
        view = buf
    else:                        # the stacked (T, B, Tk) image inside a larger NaN buffer: no stride is the dense one
        buf = torch.full((T + 1, B + 2, Tk + 3), NAN, device=dev)
        view = buf[:T, 1:B + 1, :Tk]
        view.copy_(torch.from_numpy(a).transpose(0, 1))
        assert not view.is_contiguous()
    before = _bits(buf).clone()
    st = torch.tensor(steps, dtype=torch.int32, device=dev)
    kl = torch.tensor(keys, dtype=torch.int32, device=dev)
    got = ops.alignment_stats(view, st, kl, layout)
    again = ops.alignment_stats(view, st, kl, layout)
    torch.cuda.synchronize()
    assert got.shape == (B, 13) and got.dtype == torch.float32
    assert torch.equal(_bits(got), _bits(again))                  # two calls, bit for bit
    assert torch.equal(_bits(buf), before)                        # attn is only read
    rows = got.cpu().numpy()
    assert np.isfinite(rows).all()
    for b in range(B):
        for c, name in enumerate(AR.COLUMNS):
            g, w = float(rows[b, c]), want[b][name]
            if name.startswith("focus"):
                # the fp32 row sum (<= 4096 terms, lane-strided then a 64-lane tree) errs below 4e-6 relative
                err = abs(g - w) / w if w else abs(g)
                print("Tk %3d T %2d %s item %d %s: %.9g want %.9g rel %.2e" % (Tk, T, layout, b, name, g, w, err))
                assert err <= 1e-5, (b, name, g, w)
            else:
                assert g == w, (b, name, g, w)


def test_alignment_stats_refusals(dev):
    from deepvoice3_pytorch_amd import _lib
    lib = _lib.lib()
    attn = torch.zeros(2, 3, 8, device=dev)
    st = torch.tensor([3, 3], dtype=torch.int32, device=dev)
    kl = torch.tensor([8, 8], dtype=torch.int32, device=dev)
    out = torch.full((2, 13), 7.0, device=dev)
    scratch = torch.zeros(4096, dtype=torch.uint8, device=dev)

    def call(B_=2, T=3, Tk=8, steps=st.data_ptr(), attn_p=attn.data_ptr(), out_p=out.data_ptr()):
        return lib.dv3_alignment_stats_f32(attn_p, T * Tk, Tk, B_, T, Tk, steps, kl.data_ptr(), out_p, scratch.data_ptr(), None)

    assert call() == 0
    torch.cuda.synchronize()
    assert out[:, 0].tolist() == [3.0, 3.0]
    out.fill_(7.0)
    for kw, word in ((dict(Tk=4097), "Tk = 4097"), (dict(B_=0), "B = 0"), (dict(steps=None), "steps"), (dict(T=0), "T = 0"),
                     (dict(attn_p=None), "attn"), (dict(out_p=out.data_ptr() + 2), "out")):
        assert call(**kw) != 0, kw
        assert word in lib.dv3_last_error().decode(), (kw, lib.dv3_last_error())
    torch.cuda.synchronize()
    assert bool((out == 7.0).all())                               # nothing was launched
    assert lib.dv3_alignment_stats_scratch_bytes(0, 5) == 0 and lib.dv3_alignment_stats_scratch_bytes(2, 3) == 48


# ----------------------------------------------------------------------------------------------------------------------
# 3. / 4. synthesis
# ----------------------------------------------------------------------------------------------------------------------
def _toy(family, dev, max_steps):
    from deepvoice3_pytorch_amd import builder, audio
    torch.manual_seed(3)
    make, hp = dict(nyanko=(builder.nyanko, NY_HP), deepvoice3=(builder.deepvoice3, DV3_HP))[family]
    hp = dict(hp, linear_dim=257)                                 # the bins of a 512-point FFT: results end in Griffin-Lim
    model = make(**hp).to(dev).eval()
    dec = model.seq2seq.decoder
    dec.min_decoder_steps, dec.max_decoder_steps = 0, max_steps
    cfg = audio.AudioConfig(fft_size=512, hop_size=128, sample_rate=16000, griffin_lim_iters=2)
    return model, hp, cfg


def _check_row(row, ali, n_keys):
    want = AR.item_stats(ali.cpu().numpy(), ali.size(0), n_keys)
    assert sorted(row) == sorted(AR.COLUMNS + ("flags",))
    for name in AR.COLUMNS:
        if name.startswith("focus"):
            assert isinstance(row[name], float) and abs(row[name] - want[name]) <= 1e-5 * want[name], (name, row[name], want[name])
        else:
            assert isinstance(row[name], int) and row[name] == want[name], (name, row[name], want[name])
    return want


@pytest.mark.parametrize("family", ["nyanko", "deepvoice3"])
def test_tts_batch_diagnostics(dev, family):
    from deepvoice3_pytorch_amd import synthesis
    model, hp, cfg = _toy(family, dev, 40)
    rng = np.random.RandomState(5)
    lens = [31, 9, 23, 4, 17, 12]
    seqs = [rng.randint(2, hp["n_vocab"], s).tolist() for s in lens]
    plain = synthesis.tts_batch(model, seqs, audio_cfg=cfg)
    diag = synthesis.tts_batch(model, seqs, audio_cfg=cfg, diagnostics=True)
    assert len(plain) == len(diag) == len(seqs)
    for b, (p, d) in enumerate(zip(plain, diag)):
        assert len(p) == 4 and len(d) == 5
        for x, y in zip(p, d[:4]):
            assert torch.equal(x, y), (family, b)
        ali, row = d[2], d[4]
        assert ali.shape[1] == lens[b] and row["steps"] == ali.shape[0] and row["keys"] == lens[b]
        _check_row(row, ali, lens[b])
        assert row["flags"] == synthesis.alignment_flags(row, model.seq2seq.decoder.max_decoder_steps)
        print(family, b, row)
    # the rolling path returns the same rows for the same utterances
    got = {r[0]: r for r in synthesis.tts_stream(model, seqs, slots=8, audio_cfg=cfg, chunk=8, diagnostics=True)}
    for b in range(len(seqs)):
        assert len(got[b]) == 6
        _check_row(got[b][5], got[b][3], lens[b])


@pytest.mark.parametrize("family", ["nyanko", "deepvoice3"])
def test_end_of_text_stop(dev, family):
    """min_decoder_steps 0, max_decoder_steps 11, stall_limit 3.  The one-id texts reach their end at step 0 (their only
    key is their last), so they stop after 4 steps unless the done flag is earlier; the 40-id text cannot reach key 39 in
    12 steps under the default window (window_ahead = 3: at most 2 keys a step) and runs to its done flag or the cap."""
    from deepvoice3_pytorch_amd import synthesis
    from deepvoice3_pytorch_amd.decode_program import stall_stop
    K, CAP = 3, 11
    model, hp, cfg = _toy(family, dev, CAP)
    r = hp["r"]
    rng = np.random.RandomState(9)
    lens = [1, 40, 1, 2, 3, 9]
    seqs = [rng.randint(2, hp["n_vocab"], s).tolist() for s in lens]
    n = len(seqs)

    def stream(chunk, **kw):
        got = {res[0]: res[1:] for res in synthesis.tts_stream(model, seqs, slots=8, audio_cfg=cfg, chunk=chunk, **kw)}
        return [got[i] for i in range(n)]

    # n_done from the item's own done flags (the first step n > min_decoder_steps = 0 with done > 0.5), or the cap
    text = torch.zeros(n, max(lens), dtype=torch.long)
    for b, s in enumerate(seqs):
        text[b, :len(s)] = torch.tensor(s)
    done = model.synthesize_batch(text.to(dev), lens)[3]
    flags = (torch.cat([d.reshape(n, 1) for d in done], dim=1) > 0.5).cpu().numpy()
    n_done = [int(np.argmax(flags[b])) + 1 if flags[b].any() else CAP + 1 for b in range(n)]

    runs = {"batch": (synthesis.tts_batch(model, seqs, audio_cfg=cfg),
                      synthesis.tts_batch(model, seqs, audio_cfg=cfg, stall_limit=K))}
    for chunk in (1, 3, 8):
        runs["stream chunk %d" % chunk] = (stream(chunk), stream(chunk, stall_limit=K))
    counts = {}
    for name, (free, stopped) in runs.items():
        counts[name] = [res[2].size(0) for res in stopped]
        for b in range(n):
            mel0, ali0 = free[b][0], free[b][2]
            mel, lin, ali, wav = stopped[b][:4]
            steps = ali.size(0)
            assert ali0.size(0) == n_done[b], (name, b, ali0.size(0), n_done[b])      # without stall_limit: the done flag's count
            end = AR.item_stats(ali.cpu().numpy(), steps, lens[b])["end_step"]
            s = stall_stop(end, K, 0)
            want = min(n_done[b], s) if s else n_done[b]
            print("%s %-14s item %d (%2d ids): n_done %2d end_step %2d stall_stop %2d -> %2d steps" % (
                family, name, b, lens[b], n_done[b], end, s, steps))
            assert steps == want, (name, b, steps, want)
            assert mel.size(0) == steps * r and ali.size(1) == lens[b]
            assert lin.size(0) * mel0.size(0) == free[b][1].size(0) * mel.size(0)         # the converter's upsampling
            assert torch.equal(mel, mel0[:steps * r]), (name, b)
            assert torch.equal(ali, ali0[:steps]), (name, b)
            assert torch.isfinite(wav).all() and wav.numel() > 0
    assert all(c == counts["batch"] for c in counts.values()), counts            # the chunk size changes no step count
    by_rule = [b for b in range(n) if counts["batch"][b] < n_done[b]]
    assert by_rule, (counts, n_done)                                             # at least one item stopped by the new rule
    assert len(by_rule) < n, (counts, n_done)                                    # and at least one did not
    for b in (0, 2):             # the one-id texts: 4 steps, or the done flag if it came first
        assert counts["batch"][b] == min(4, n_done[b])
    assert counts["batch"][1] == n_done[1]                                       # the 40-id text never reached its end

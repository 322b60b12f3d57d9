# coding: utf-8
"""The float64 references of tests/decode_step_ref.py, pinned on the CPU: against the oracle's whole-sequence and
incremental layers, its attention layer, its decode loop's stop rule and decode_program.item_stops; the step-tile image
round trip; and the preconditions the GPU file (tests/test_gpu_decode_step.py) relies on -- every windowed attention case
has a top-2 probability gap above its element-wise bound (so an argmax comparison never hinges on rounding, and no case
is passed over for a tie), and every shape list crosses the kernel thresholds it claims to cross."""
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tests import decode_step_ref as R  # noqa: E402
from tests.util import load_golden, split_model_fixture  # noqa: E402
from oracle import dv3_oracle as O  # noqa: E402

ALL_CONV = R.CONV_SWEEP + R.CONV_TAIL
JD = sorted(set((c["J"], c["dil"]) for c in ALL_CONV))


def _layer(J, Cin, M, seed):
    rs = np.random.RandomState(seed)
    w = rs.standard_normal((M, Cin, J)) / np.sqrt(J * Cin)            # the oracle's (out, in, k)
    b = rs.standard_normal(M) * 0.3
    sd = {"l.conv.weight": torch.from_numpy(w), "l.conv.bias": torch.from_numpy(b)}
    return sd, np.ascontiguousarray(w.transpose(0, 2, 1)), b           # dense [M][J][Cin]


@pytest.mark.parametrize("J,dil", JD)
def test_conv_step_ref_equals_oracle_layers(J, dil):
    """step by step == the oracle's causal conv1d / conv1d_glu / highway_conv1d on the whole sequence, and == its
    incremental modules (_IncConv, _IncGated) fed the same frames: 1e-12 in float64"""
    B, C, T = 3, 6, 3 * ((J - 1) * dil + 1) + 2
    rs = np.random.RandomState(J * 100 + dil)
    x = rs.standard_normal((T, B, C))
    x_bct = torch.from_numpy(np.ascontiguousarray(x.transpose(1, 2, 0)))
    pad = (J - 1) * dil
    # plain
    sd, W, b = _layer(J, C, 5, 1)
    whole = O.conv1d(sd, "l.conv", x_bct, dil, pad)[:, :, :T].numpy()
    inc = O._IncConv(sd, "l.conv", dil)
    for t in range(T):
        got = R.conv_step_ref(x[:t + 1], W, b, "linear", dil)["y"]
        assert np.abs(got - whole[:, :, t]).max() < 1e-12, t
        assert np.abs(got - inc.step(torch.from_numpy(x[t]).unsqueeze(1))[:, 0].numpy()).max() < 1e-12, t
    # gated: GLU with and without the residual, highway
    sd, W, b = _layer(J, C, 2 * C, 2)
    for mode, residual in (("glu", False), ("glu", True), ("highway", False)):
        if mode == "glu":
            whole = O.conv1d_glu(sd, "l", x_bct, J, dil, True, residual).numpy()
        else:
            whole = O.highway_conv1d(sd, "l", x_bct, J, dil, True).numpy()
        inc = O._IncGated(sd, "l", dil, mode, residual)
        for t in range(T):
            got = R.conv_step_ref(x[:t + 1], W, b, mode, dil, residual=residual)["y"]
            assert np.abs(got - whole[:, :, t]).max() < 1e-12, (mode, residual, t)
            assert np.abs(got - inc.step(torch.from_numpy(x[t]).unsqueeze(1))[:, 0].numpy()).max() < 1e-12, (mode, t)


def test_conv_step_ref_tails():
    """the tails the oracle has no single call for, against their expressions (include/dv3hip.h: mode list)"""
    rs = np.random.RandomState(3)
    B, C, M = 2, 4, 5
    x = rs.standard_normal((3, B, C))
    sd, W, b = _layer(2, C, M, 4)
    r, r2, pa = (rs.standard_normal((B, M)) for _ in range(3))
    pre = R.conv_step_ref(x, W, b, "linear", 1)["y"]
    h = np.sqrt(0.5)
    for mode, f in (("linear", lambda v: v), ("relu", lambda v: np.maximum(v, 0)), ("sigmoid", lambda v: 1 / (1 + np.exp(-v))),
                    ("softsign", lambda v: v / (1 + np.abs(v)))):
        o = R.conv_step_ref(x, W, b, mode, 1, r=r, r2=r2, post_add=pa, want_act=True)
        want = ((f(pre) + r) * h + r2) * h
        assert np.abs(o["y_pre"] - want).max() < 1e-12 and np.abs(o["y"] - (want + pa)).max() < 1e-12
        assert np.abs(o["y_act"] - 1 / (1 + np.exp(-(want + pa)))).max() < 1e-12 and o["out_seq"] is o["y_act"]
        assert R.conv_step_ref(x, W, b, mode, 1, r2=r2)["out_seq"] is not None
    # gated: speaker bias on the `a` half only, then r2; S counts |w||x| + |bias| + |spk|
    sd, W, b = _layer(2, C, 2 * C, 5)
    spk = rs.standard_normal((B, C))
    o0 = R.conv_step_ref(x, W, b, "glu", 1)
    o = R.conv_step_ref(x, W, b, "glu", 1, spk=spk, r2=r2[:, :C], residual=True)
    sg = 1 / (1 + np.exp(-o0["gate"]))
    assert np.abs(o["y"] - (((o0["pre"] + spk) * sg + x[-1]) * h + r2[:, :C]) * h).max() < 1e-12
    assert np.abs(o["S"] - (o0["S"] + np.abs(spk))).max() < 1e-12 and (o["S"] >= np.abs(o["pre"]) - 1e-12).all()
    nb = R.conv_step_ref(x, W, None, "glu", 1)
    assert np.abs(nb["S"] + np.abs(b[:C]) - o0["S"]).max() < 1e-12


@pytest.mark.parametrize("Tk,las", [(1, (None, 0)), (3, (None, 0, 2)), (12, (None, 0, 1, 5, 9, 11))])
def test_attn_step_ref_equals_oracle_attention(Tk, las):
    """== O.attention_layer at Tq = 1 with last_attended (identity projections), the per-utterance mode == the same call
    on the item's own keys"""
    E = 6
    rs = np.random.RandomState(Tk)
    sd = {"a.query_projection.weight": torch.eye(E, dtype=torch.float64), "a.query_projection.bias": torch.zeros(E, dtype=torch.float64),
          "a.out_projection.weight": torch.eye(E, dtype=torch.float64), "a.out_projection.bias": torch.zeros(E, dtype=torch.float64)}
    q, k, v = rs.standard_normal(E), rs.standard_normal((Tk, E)), rs.standard_normal((Tk, E))
    for s in sorted(set((Tk, max(Tk // 2, 1), 1))):
        for la in las:
            if la is not None and la >= s:
                continue
            for wb, wa in ((1, 3), (0, 2), (2, 5)):
                got = R.attn_step_ref(q, k, v, la, wb, wa, None if s == Tk else s)
                out, attn = O.attention_layer(sd, "a", torch.from_numpy(q).view(1, 1, E),
                                              torch.from_numpy(k[:s].T.copy()).unsqueeze(0), torch.from_numpy(v[:s]).unsqueeze(0),
                                              last_attended=la, window_ahead=wa, window_backward=wb)
                ctx = out[0, 0].numpy() / np.sqrt(0.5) - q           # undo the layer's (x + residual) * sqrt(.5)
                assert np.abs(got["p"][:s] - attn[0, 0].numpy()).max() < 1e-12 and not got["p"][s:].any()
                assert np.abs(got["ctx"] - ctx).max() < 1e-12
                assert got["argmax"] == int(attn.max(-1)[1].view(-1)[0])
                lo, hi = R.attn_window(la, wb, wa, s)
                assert not got["p"][:lo].any() and not got["p"][hi:].any()          # exact zeros outside the window
    ref = R.attn_step_ref(q, k, v)
    top = np.sort(ref["p"])[::-1]
    assert ref["gap"] == (top[0] - top[1] if Tk > 1 else 1.0)
    assert R.attn_step_ref(q, np.zeros((Tk, E)), v)["argmax"] == 0                  # a tie: the first maximum


def test_stop_steps_equals_item_stops():
    from deepvoice3_pytorch_amd.decode_program import item_stops
    rs = np.random.RandomState(0)
    for trial in range(400):
        n_rows = 24
        rows = [[bool(rs.rand() < (0.15 if trial % 3 else 0.6))] for _ in range(n_rows)]
        t0, n_steps = int(rs.randint(0, 6)), int(rs.randint(1, 14))
        mn, mx = int(rs.randint(0, 8)), int(rs.randint(0, 16))
        got = R.stop_steps(rows, t0, n_steps, mn, mx, True)
        stops = [0]
        item_stops(rows[t0:t0 + n_steps], t0, mn, mx, stops)
        assert got == (stops[0] - t0 if stops[0] else n_steps), (trial, t0, n_steps, mn, mx)
        assert R.stop_steps(rows, t0, n_steps, mn, mx, False) == n_steps
    # B > 1: all items at once, not each on its own
    rows = [[True, False], [False, True], [True, True], [True, True]]
    assert R.stop_steps(rows, 0, 4, 0, 10, True) == 3 and R.stop_steps(rows, 0, 4, 3, 10, True) == 4
    assert R.stop_steps(rows, 0, 4, 0, 1, True) == 2 and R.stop_steps(rows, 2, 2, 0, 1, True) == 1


@pytest.mark.parametrize("bias,mn,mx", [(30.0, 3, 9), (30.0, 0, 9), (-30.0, 3, 6), (None, 2, 7), (30.0, 8, 5)])
def test_stop_steps_equals_oracle_decode_loop(bias, mn, mx):
    """the number of steps O.dv3_incremental_decode takes == stop_steps on the done flags it produced"""
    fx = load_golden("model_dv3_tiny")
    builder, hp, sd, x = split_model_fixture(fx)
    spec = O.build_spec(builder, **hp)
    sd = dict(sd)
    if bias is not None:
        sd["seq2seq.decoder.fc.bias"] = torch.full_like(sd["seq2seq.decoder.fc.bias"], bias)
    with torch.no_grad():
        enc = O.dv3_encoder(sd, spec, x["text"][:2])
        _, _, dones, _ = O.dv3_incremental_decode(sd, spec, enc, x["text_positions"][:2], max_decoder_steps=mx,
                                                  min_decoder_steps=mn)
        # the flags of a run that never stops early: the loop is causal, so its first len(dones) rows are the same run
        _, _, full, _ = O.dv3_incremental_decode(sd, spec, enc, x["text_positions"][:2], max_decoder_steps=mx,
                                                 min_decoder_steps=mx + 1)
    rows = [(d.reshape(-1) > 0.5).tolist() for d in full]
    assert len(full) == mx + 1
    assert len(dones) == R.stop_steps(rows, 0, mx + 5, mn, mx, True)
    assert len(dones) == R.stop_steps(rows, 0, mx + 1, mn, mx, True)


@pytest.mark.parametrize("case", R.PACK_CASES)
def test_step_tile_image_round_trip(case):
    Ktot, M, Cg, lda, a_half = case
    rs = np.random.RandomState(Ktot + M)
    fp = rs.standard_normal((Ktot, lda)).astype(np.float32)
    img = R.step_tile_image(fp, lda, a_half, Ktot, M, Cg)
    assert img.size == R.pack_floats(Ktot, M, Cg) and img.dtype == np.float32
    back = R.untile_image(img, lda, a_half, Ktot, M, Cg)
    rows = Cg if Cg else M
    owned = np.zeros((Ktot, lda), dtype=bool)
    owned[:, :rows] = True
    if Cg:
        owned[:, a_half:a_half + Cg] = True
    assert np.array_equal(back[owned], fp[owned]) and np.isnan(back[~owned]).all()
    # everything else in the image is an exact zero: as many non-zeros as owned elements
    assert np.count_nonzero(img) == int(owned.sum())
    # and the image is the dense weight where the header says: [row block][j*Cin + c][row in block]
    W = rs.standard_normal((M, 1, Ktot)).astype(np.float32)
    img = R.step_tile_image(R.fwd_pack_of(W, Cg, lda, a_half), lda, a_half, Ktot, M, Cg)
    kpad = R.cdiv(Ktot, 64) * 64
    for m in (0, rows - 1, M - 1):
        half, row = (1, m - Cg) if (Cg and m >= Cg) else (0, m)
        rec = 32 if Cg else 16
        for kk in (0, Ktot - 1):
            assert img[((row // 16) * kpad + kk) * rec + half * 16 + row % 16] == W[m, 0, kk]


def test_pack_cases_cover_what_they_claim():
    P = R.PACK_CASES
    assert any(Cg == 0 for _, _, Cg, _, _ in P) and any(Cg > 0 for _, _, Cg, _, _ in P)
    assert any((Cg or M) % 16 for _, M, Cg, _, _ in P) and any(Cg == 0 and M == 1 for _, M, Cg, _, _ in P)
    assert any(Cg == 1 for _, M, Cg, _, _ in P)
    assert any(K % 64 for K, _, _, _, _ in P) and any(Cg == 0 and lda > M for _, M, Cg, lda, _ in P)
    assert any(Cg > 0 and ah > Cg for _, _, Cg, _, ah in P) and any(Cg > 0 and lda > ah + Cg for _, _, Cg, lda, ah in P)


def test_conv_cases_cross_their_thresholds():
    """kpad = ceil(J*Cin/64)*64; nu = kpad / (gated ? 32 : 64); the loop after the prefetch iff nu > 24, its last block
    partial iff (nu - 24) % 8 != 0; dv3_conv_step_lds_bytes <= 65536 (restated from csrc/decode_step.hip)"""
    for c in ALL_CONV:
        assert R.lds_bytes(c["J"], c["Cin"]) <= R.LDS_MAX, R.case_name(c)
        assert c["L"] >= (c["J"] - 1) * c["dil"] + 1 and c["steps"] >= 3 * c["L"] + 2
        if c["gated"] and (c["mode"] == "highway" or c["residual"]):
            assert c["Cin"] == c["Cout"]
    assert R.lds_bytes(3, 512) == R.LDS_MAX and R.lds_bytes(1, 1537) > R.LDS_MAX
    nus = {}
    for c in R.CONV_TAIL:
        if c["gated"]:
            nu = R.nu_of(c["J"], c["Cin"], True)
            nus[nu] = nus.get(nu, 0) + 1
            assert R.kpad_of(c["J"], c["Cin"]) == 32 * nu
    assert nus == R.TAIL_NU
    assert not R.tail_path(3, 256, True) and R.tail_path(2, 416, True) and R.partial_tail(2, 416, True)
    assert R.tail_path(2, 512, True) and not R.partial_tail(2, 512, True)
    assert R.tail_path(3, 512, True) and not R.partial_tail(3, 512, True) and R.kpad_of(3, 512) == 1536
    assert any(R.partial_tail(c["J"], c["Cin"], True) and (c["J"] * c["Cin"]) % 64 for c in R.CONV_TAIL)   # both at once
    assert any(not c["gated"] and R.nu_of(c["J"], c["Cin"], False) == 24 for c in R.CONV_TAIL)
    assert not any(R.tail_path(c["J"], c["Cin"], False) for c in ALL_CONV if not c["gated"])      # LDS ends plain layers at nu 24
    S = R.CONV_SWEEP
    assert set(c["mode"] for c in S) == set(R.MODES)
    assert any(c["mode"] == "glu" and c["residual"] for c in S) and any(c["mode"] == "glu" and not c["residual"] for c in S)
    for gated in (False, True):
        G = [c for c in S if c["gated"] == gated]
        assert any(c["r2"] and not c["r"] for c in G)
        if not gated:
            assert any(c["r"] and not c["r2"] for c in G) and any(c["r"] and c["r2"] for c in G)
    assert any(c["spk"] for c in S) and any(not c["bias"] for c in S)
    assert set(c["post_add"] for c in S) == {None, "t", "b"}
    assert all(any(c[k] for c in S) for k in ("y_pre", "y_act", "out_seq", "x_ts", "x_pad"))
    assert set(c["J"] for c in S) == {1, 2, 3, 5} and set(c["dil"] for c in S if c["J"] > 1) >= {1, 3, 9, 27}
    assert any(c["L"] == (c["J"] - 1) * c["dil"] + 1 for c in S if c["J"] > 1)
    assert any(c["L"] == (c["J"] - 1) * c["dil"] + 4 for c in S if c["J"] > 1)
    assert set(c["B"] for c in S) >= {1, 3, 4, 5, 9} and max(c["B"] for c in S) > 16
    cins = set(c["Cin"] for c in S)
    assert cins >= {1, 5, 80, 128, 256} and any(v > 256 and v % 4 for v in cins)
    for rows in (set(c["Cout"] for c in S if not c["gated"]), set(c["Cout"] for c in S if c["gated"])):
        assert rows >= {1, 7, 16, 80, 256} and any(v % 16 and v > 16 for v in rows)
    assert any(c["Cin"] * c["J"] % 64 for c in S)


def test_preset_decoder_layers_are_listed():
    """the walker the GPU file uses finds the decoders' layers (built on the CPU from bench.PRESETS)"""
    import bench
    from deepvoice3_pytorch_amd import builder
    for name in ("deepvoice3_ljspeech", "deepvoice3_vctk", "nyanko_ljspeech"):
        bname, hp, _ = bench.PRESETS[name]
        torch.manual_seed(0)
        dec = getattr(builder, bname)(**dict(hp)).seq2seq.decoder
        cases = R.preset_conv_cases(dec, 5)
        assert len(cases) >= 6, (name, len(cases))
        assert any(c["gated"] and c["J"] > 1 and c["dil"] == 27 for c in cases), name
        assert any(not c["gated"] for c in cases)
        if name == "deepvoice3_vctk":
            assert any(c["spk"] for c in cases)
        if name == "nyanko_ljspeech":
            assert any(c["mode"] == "highway" for c in cases)
        for c in cases:
            assert R.lds_bytes(c["J"], c["Cin"]) <= R.LDS_MAX


def test_attention_cases_cover_what_they_claim():
    A = R.ATTN_CASES
    assert set(c["Tk"] for c in A) == {1, 3, 4, 40, 257, 700} and set(c["E"] for c in A) == {1, 64, 96, 256, 300}
    for Tk in (1, 3, 4, 40, 257, 700):
        T = [c for c in A if c["Tk"] == Tk]
        assert set(c["tke"] for c in T) == {0, 1}
        plain = [c for c in T if c["la"] is not None and c["key_len"] is None]
        assert set(c["la"][0] for c in plain) == set(min(max(v, 0), Tk - 1) for v in (0, 1, Tk - 3, Tk - 1))
        assert any(c["la"] is None and c["key_len"] is None for c in T)
        assert any(c["la"] is not None and c["key_len"] is not None for c in T)
        assert any(c["la"] is None and c["key_len"] is not None for c in T)
    assert set(c["outs"] for c in A) == {"attn", "seq", "both"}
    assert any((c["wb"], c["wa"]) != (1, 3) for c in A if c["la"] is not None)
    assert any(c["q_pad"] for c in A) and any(c["ctx_pad"] for c in A)
    assert any(c["Tk"] > 256 for c in A) and any(c["E"] > 256 and c["E"] % 64 for c in A)
    # windows clipped at the front, at the back, at both ends and at neither
    clips = set()
    for c in A:
        if c["la"] is not None and c["key_len"] is None:
            la = c["la"][0]
            clips.add((la - c["wb"] <= 0, la + c["wa"] >= c["Tk"]))
    assert clips == {(True, False), (False, True), (True, True), (False, False)}
    assert any(r[4] for r in R.ATTN_RUNS) and any(not r[4] for r in R.ATTN_RUNS) and all(r[5] >= 6 for r in R.ATTN_RUNS)
    assert set(r[3] for r in R.ATTN_RUNS) == {0, 1} and any(r[6] % 2 for r in R.ATTN_RUNS) and any(r[6] % 2 == 0 for r in R.ATTN_RUNS)


def test_attention_cases_have_no_near_ties():
    """precondition of the GPU file's argmax comparisons: in every case with the window on, every item whose argmax is
    stored has a reference top-2 gap above twice its largest probability bound -- no exclusions"""
    n = 0
    for c in R.ATTN_CASES:
        if c["la"] is None:
            continue
        for b, (ref, (ep, _)) in enumerate(R.attn_case_refs(c)):
            if b == 0 or c["key_len"] is not None:
                assert ref["gap"] > 2 * ep.max(), (c, b, ref["gap"], ep.max())
                n += 1
    assert n > 100
    for run in R.ATTN_RUNS:
        refs, la = R.attn_run_refs(run)
        per_item = run[4]
        for s, row in enumerate(refs):
            for b, (ref, (ep, _)) in enumerate(row):
                if b == 0 or per_item:
                    assert ref["gap"] > 2 * ep.max(), (run, s, b, ref["gap"], ep.max())
        # the run moves: the window does not sit on one key for all steps
        assert len(set(tuple(r) for r in la)) >= 3, (run, la)

# coding: utf-8
"""-m gpu: the decode-step entry points of csrc/decode_step.hip, each against the float64 references of
tests/decode_step_ref.py computed from the same fp32 inputs, element by element (tests.util.assert_close_elementwise).

  (a) dv3_conv_step_pack_f32: bit-equal to the step-tile image the header describes;
  (b) dv3_conv_step_f32: single launches driven for 3L + 2 steps from hand-built descriptors (ring length, strides and
      the step counter are free), every mode and tail, the layers around the end of the weight prefetch, the presets' own
      decoder layers; the ring afterwards; the documented refusals;
  (c) dv3_attn_step_f32: probabilities, context and argmax, both key layouts, window off / clipped at either end / both,
      per-utterance key counts, and the last_attended hand-over over consecutive steps;
  (d) dv3_decode_program_launch / dv3_decode_program_run on a synthetic six-entry program: bit-identical to launch by
      launch, for every workgroup-to-tile mapping, with the stop rule of decode_step_ref.stop_steps.

Every output buffer starts as NaN; strided buffers carry NaN guard columns that must still be NaN afterwards.  The bounds
are derived in decode_step_ref.py (conv_step_bound, attn_step_bound) from the kernels' summation depths -- none is
measured; tests/test_cpu_decode_step_ref.py asserts the preconditions (no near-tie argmax, thresholds crossed)."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tests import decode_step_ref as R  # noqa: E402
from tests.util import assert_close_elementwise  # noqa: E402

pytestmark = pytest.mark.gpu

NAN = float("nan")
GUARD = 8 * 32 * 32          # floats after a weight image: one block of the loop after the prefetch, were it not clamped


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


def _env():
    from deepvoice3_pytorch_amd import ops, _lib
    return ops, _lib.lib(), _lib.STRUCTS, _lib.CONSTS


def _report(what, ratio):
    print("worst-ratio %-72s %.4g" % (what, ratio))


def _bits(a, b):
    return torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def _nan(dev, *shape):
    return torch.full(shape, NAN, device=dev)


def _padded(dev, arr, pad):
    """host [..., C] -> device [..., C + pad] with NaN guard columns; -> (buffer, view of the data)"""
    a = torch.from_numpy(np.ascontiguousarray(arr, dtype=np.float32))
    buf = _nan(dev, *(tuple(a.shape[:-1]) + (a.shape[-1] + pad,)))
    buf[..., :a.shape[-1]] = a.to(dev)
    return buf, buf[..., :a.shape[-1]]


def _guards_intact(buf, C):
    return bool(torch.isnan(buf[..., C:]).all())


def _launch_entry(kind, d, t):
    """one descriptor at step t with NO device counter: the step index travels in t_value, which is the host-driven
    loop's way (dv3_decode_program_launch; the single-launch entry points insist on `t`)"""
    ops, L, S, C = _env()
    arr = (S["dv3_decode_entry"] * 1)()
    arr[0].kind = kind
    if kind == 0:
        arr[0].conv = d
    else:
        arr[0].attn = d
    p = S["dv3_decode_program"]()
    p.entries_host = ctypes.addressof(arr)
    p.n_entries, p.B, p.t0, p.n_steps = 1, d.B, t, 1
    ops._lib.call("dv3_decode_program_launch", ctypes.byref(p), ops._stream())


def _mode_const(C, mode):
    return C["DV3_EPI_" + mode.upper()]


# ------------------------------------------------------------------------------------------------------------------
# (a) the weight re-layout
# ------------------------------------------------------------------------------------------------------------------
def _pack(dev, fp, lda, a_half, Ktot, M, Cg):
    ops, L, S, C = _env()
    n = L.dv3_conv_step_pack_floats(Ktot, M, Cg)
    assert n == R.pack_floats(Ktot, M, Cg)
    out = _nan(dev, n + GUARD)
    src = torch.from_numpy(fp).to(dev)
    ops._lib.call("dv3_conv_step_pack_f32", src.data_ptr(), lda, a_half, Ktot, M, Cg, out.data_ptr(), ops._stream())
    torch.cuda.synchronize()
    return out, n


@pytest.mark.parametrize("case", R.PACK_CASES)
def test_pack_is_the_step_tile_image(dev, case):
    Ktot, M, Cg, lda, a_half = case
    rs = np.random.RandomState(Ktot * 7 + M)
    # the columns no row owns are NaN in the source: a pack that reads one puts a NaN where a zero belongs
    fp = R.fwd_pack_of(rs.standard_normal((M, 1, Ktot)).astype(np.float32), Cg, lda, a_half)
    out, n = _pack(dev, fp, lda, a_half, Ktot, M, Cg)
    want = torch.from_numpy(R.step_tile_image(fp, lda, a_half, Ktot, M, Cg)).to(dev)
    assert _bits(out[:n], want), case
    assert bool(torch.isnan(out[n:]).all()), case


# ------------------------------------------------------------------------------------------------------------------
# (b) the conv step
# ------------------------------------------------------------------------------------------------------------------
def _conv_data(c, seed):
    rs = np.random.RandomState(seed)
    B, Cin, Cout, M, J, T = c["B"], c["Cin"], c["Cout"], c["M"], c["J"], c["steps"]
    f32 = np.float32
    d = dict(W=(rs.standard_normal((M, J, Cin)) * (1.5 / np.sqrt(J * Cin))).astype(f32),
             x=rs.standard_normal((T, B, Cin)).astype(f32),
             bias=(rs.standard_normal(M) * 0.5).astype(f32) if c["bias"] else None,
             spk=rs.standard_normal((B, Cout)).astype(f32) if c["spk"] else None,
             r=rs.standard_normal((B, Cout)).astype(f32) if c["r"] else None,
             r2=rs.standard_normal((B, Cout)).astype(f32) if c["r2"] else None, post_add=None)
    if c["post_add"] == "t":
        d["post_add"] = rs.standard_normal((T, B, Cout)).astype(f32)
    elif c["post_add"] == "b":
        d["post_add"] = np.broadcast_to(rs.standard_normal((1, B, Cout)).astype(f32), (T, B, Cout)).copy()
    return d


def _run_conv(dev, c, data, tiles, use_counter):
    """all steps of one case -> dict of stacked device results and the buffers whose guards are checked"""
    ops, L, S, C = _env()
    B, Cin, Cout, M, J, T, Lr = c["B"], c["Cin"], c["Cout"], c["M"], c["J"], c["steps"], c["L"]
    keep = []
    d = S["dv3_conv_step_desc"]()
    xpad = c["x_pad"]
    xbuf, xall = _padded(dev, data["x"], xpad)                     # [T][B][Cin + pad]
    if c["x_ts"]:
        d.x, d.x_bs, d.x_ts = xbuf.data_ptr(), Cin + xpad, B * (Cin + xpad)
        xcur = None
    else:
        xcur = _nan(dev, B, Cin + xpad)
        d.x, d.x_bs = xcur.data_ptr(), Cin + xpad
    nring = Lr * B * Cin                                           # NaN guards of a whole ring before, 64 floats after
    ring = _nan(dev, 2 * nring + 64)
    ring[nring:2 * nring] = 0
    d.ring, d.L = ring.data_ptr() + 4 * nring, Lr
    t_dev = torch.zeros(1, dtype=torch.int32, device=dev)
    d.t = t_dev.data_ptr() if use_counter else None
    d.a, d.lda, d.a_half = tiles.data_ptr(), 0, 0                  # lda / a_half are ignored (the header says so)
    if data["bias"] is not None:
        bias = torch.from_numpy(data["bias"]).to(dev)
        d.bias = bias.data_ptr()
        keep.append(bias)
    for name, pad in (("spk", 3), ("r", 2), ("r2", 1)):
        if data[name] is not None:
            buf, _ = _padded(dev, data[name], pad)
            setattr(d, name, buf.data_ptr())
            setattr(d, name + "_bs", Cout + pad)
            keep.append(buf)
    if c["post_add"] == "t":
        pa, _ = _padded(dev, data["post_add"], 1)
        d.post_add, d.post_add_ts, d.post_add_bs = pa.data_ptr(), B * (Cout + 1), Cout + 1
        keep.append(pa)
    elif c["post_add"] == "b":
        pa, _ = _padded(dev, data["post_add"][0], 2)
        d.post_add, d.post_add_ts, d.post_add_bs = pa.data_ptr(), 0, Cout + 2
        keep.append(pa)
    y = _nan(dev, B, Cout + 3)
    d.y, d.y_bs = y.data_ptr(), Cout + 3
    outs = {"y": _nan(dev, T, B, Cout + 3)}
    cur = {"y": y}
    if c["y_pre"]:
        cur["y_pre"] = _nan(dev, B, Cout + 1)
        d.y_pre, d.y_pre_bs = cur["y_pre"].data_ptr(), Cout + 1
        outs["y_pre"] = _nan(dev, T, B, Cout + 1)
    if c["y_act"]:
        cur["y_act"] = _nan(dev, B, Cout + 2)
        d.y_act, d.y_act_bs = cur["y_act"].data_ptr(), Cout + 2
        outs["y_act"] = _nan(dev, T, B, Cout + 2)
    if c["out_seq"]:
        outs["out_seq"] = _nan(dev, T, B, Cout + 1)
        d.out_seq, d.out_seq_ts, d.out_seq_bs = outs["out_seq"].data_ptr(), B * (Cout + 1), Cout + 1
    d.B, d.Cin, d.M, d.Cg, d.J, d.dil = B, Cin, M, (Cout if c["gated"] else 0), J, c["dil"]
    d.mode, d.residual = _mode_const(C, c["mode"]), int(c["residual"])
    stream = ops._stream()
    for t in range(T):
        if xcur is not None:
            xcur[:, :Cin].copy_(xall[t])
        if use_counter:
            ops._lib.call("dv3_conv_step_f32", ctypes.byref(d), stream)
        else:
            _launch_entry(0, d, t)
        for k, buf in cur.items():
            outs[k][t].copy_(buf)
        if use_counter:
            t_dev.add_(1)
    torch.cuda.synchronize()
    outs["ring"] = ring
    return outs


def _check_conv(dev, c, seed, label):
    ops, L, S, C = _env()
    B, Cin, Cout, M, J, T, Lr = c["B"], c["Cin"], c["Cout"], c["M"], c["J"], c["steps"], c["L"]
    Cg = Cout if c["gated"] else 0
    name = R.case_name(c)
    assert L.dv3_conv_step_lds_bytes(J, Cin) == R.lds_bytes(J, Cin) <= R.LDS_MAX, name
    data = _conv_data(c, seed)
    a_half = (Cg + 3) // 4 * 4 + (4 if Cg % 8 == 0 else 0) if Cg else 0
    lda = (2 * a_half if Cg else (M + 3) // 4 * 4) + 4
    fp = R.fwd_pack_of(data["W"], Cg, lda, a_half)
    tiles, n = _pack(dev, fp, lda, a_half, J * Cin, M, Cg)
    assert _bits(tiles[:n], torch.from_numpy(R.step_tile_image(fp, lda, a_half, J * Cin, M, Cg)).to(dev)), name
    by_counter = _run_conv(dev, c, data, tiles, True)
    by_value = _run_conv(dev, c, data, tiles, False)
    for k in by_counter:
        assert _bits(by_counter[k], by_value[k]), "%s: %s differs between the device counter and t = NULL with t_value" % (name, k)
    assert bool(torch.isnan(tiles[n:]).all()), name
    got = {k: v.cpu().double().numpy() for k, v in by_counter.items()}
    # the ring holds the last L frames bit-exactly, slot t mod L; its guard is untouched
    ring, nring = by_counter["ring"].cpu(), Lr * B * Cin
    assert bool(torch.isnan(ring[:nring]).all()) and bool(torch.isnan(ring[2 * nring:]).all()), name
    ring = ring[nring:2 * nring].view(Lr, B, Cin)
    for t in range(T - Lr, T):
        assert torch.equal(ring[t % Lr].view(torch.int32), torch.from_numpy(data["x"][t]).view(torch.int32)), (name, t)
    want = {k: np.empty((T, B, Cout)) for k in ("y", "y_pre", "y_act", "out_seq")}
    bnd = {k: np.empty((T, B, Cout)) for k in ("y", "y_pre", "y_act")}
    for t in range(T):
        pa = None if data["post_add"] is None else data["post_add"][t]
        ref = R.conv_step_ref(data["x"][:t + 1], data["W"], data["bias"], c["mode"], c["dil"], residual=c["residual"],
                              spk=data["spk"], r=data["r"], r2=data["r2"], post_add=pa, want_act=c["y_act"])
        b = R.conv_step_bound(ref, c["mode"], J, Cin, residual=c["residual"], spk=data["spk"], r=data["r"], r2=data["r2"],
                              post_add=pa, has_bias=c["bias"])
        for k in want:
            if ref[k] is not None:
                want[k][t] = ref[k]
        for k in bnd:
            bnd[k][t] = b[k]
    worst = 0.0
    for k in ("y", "y_pre", "y_act", "out_seq"):
        if k not in got:
            continue
        g = got[k]
        assert np.isnan(g[..., Cout:]).all(), "%s: %s guard columns written" % (name, k)
        bk = bnd["y_act" if (k == "out_seq" and c["y_act"]) else ("y" if k == "out_seq" else k)]
        worst = max(worst, assert_close_elementwise(g[..., :Cout], want[k], 0, bk, "%s %s" % (name, k)))
    _report("%s %s" % (label, name), worst)
    return worst


@pytest.mark.parametrize("i", range(len(R.CONV_SWEEP)))
def test_conv_step_sweep(dev, i):
    _check_conv(dev, R.CONV_SWEEP[i], 100 + i, "conv_step")


@pytest.mark.parametrize("i", range(len(R.CONV_TAIL)))
def test_conv_step_around_the_prefetch_end(dev, i):
    _check_conv(dev, R.CONV_TAIL[i], 200 + i, "conv_step tail")


@pytest.mark.parametrize("preset", ["deepvoice3_ljspeech", "deepvoice3_vctk", "nyanko_ljspeech"])
def test_conv_step_preset_decoder_layers(dev, preset):
    import bench
    from deepvoice3_pytorch_amd import builder
    bname, hp, _ = bench.PRESETS[preset]
    torch.manual_seed(0)
    dec = getattr(builder, bname)(**dict(hp)).seq2seq.decoder
    cases = R.preset_conv_cases(dec, 5)
    assert len(cases) >= 6
    worst = 0.0
    for i, c in enumerate(cases):
        worst = max(worst, _check_conv(dev, c, 300 + i, "conv_step " + preset))
    _report("conv_step %s (%d layers)" % (preset, len(cases)), worst)


def test_conv_step_refusals(dev):
    """the documented refusals: a return code and dv3_last_error, nothing launched (y stays NaN)"""
    ops, L, S, C = _env()
    B, Cin, Cout = 2, 8, 8
    x = torch.zeros(B, Cin, device=dev)
    ring = torch.zeros(64 * B * Cin, device=dev)
    a = torch.zeros(R.pack_floats(3 * 1600, 2 * Cout, Cout) + 4, device=dev)
    y = _nan(dev, B, Cout)
    t_dev = torch.zeros(1, dtype=torch.int32, device=dev)

    def desc(**kw):
        d = S["dv3_conv_step_desc"]()
        d.x, d.x_bs, d.ring, d.L, d.t, d.a = x.data_ptr(), Cin, ring.data_ptr(), 7, t_dev.data_ptr(), a.data_ptr()
        d.y, d.y_bs, d.B, d.Cin, d.M, d.Cg, d.J, d.dil = y.data_ptr(), Cout, B, Cin, Cout, 0, 3, 3
        d.mode = C["DV3_EPI_LINEAR"]
        for k, v in kw.items():
            setattr(d, k, v)
        return d

    ok = desc()
    assert L.dv3_conv_step_f32(ctypes.byref(ok), ops._stream()) == 0          # the base descriptor itself is taken
    torch.cuda.synchronize()
    y.fill_(NAN)
    for what, d, text in (("L too small", desc(L=6), "L >="),
                          ("LDS too large", desc(Cin=1600, J=1, x_bs=1600), "LDS"),
                          ("gated residual with Cin != Cg", desc(mode=C["DV3_EPI_GLU"], residual=1, M=8, Cg=4), "Cin == Cout"),
                          ("highway with Cin != Cg", desc(mode=C["DV3_EPI_HIGHWAY"], M=8, Cg=4), "Cin == Cout"),
                          ("misaligned a", desc(a=a.data_ptr() + 4), "16-byte aligned")):
        rc = L.dv3_conv_step_f32(ctypes.byref(d), ops._stream())
        msg = (L.dv3_last_error() or b"").decode()
        assert rc != 0 and text in msg, (what, rc, msg)
    torch.cuda.synchronize()
    assert bool(torch.isnan(y).all())


# ------------------------------------------------------------------------------------------------------------------
# (c) the attention step
# ------------------------------------------------------------------------------------------------------------------
def _attn_desc(dev, B, E, Tk, tke, q, k, v, la, wb, wa, key_len, outs, q_pad, ctx_pad, steps):
    ops, L, S, C = _env()
    qbuf = _nan(dev, B, E + q_pad)
    kd = torch.from_numpy(k if tke else np.ascontiguousarray(k.transpose(0, 2, 1))).to(dev)
    vd = torch.from_numpy(v if tke else np.ascontiguousarray(v.transpose(0, 2, 1))).to(dev)
    ctx = _nan(dev, B, E + ctx_pad)
    d = S["dv3_attn_step_desc"]()
    d.q, d.q_bs, d.k, d.v, d.kv_tke = qbuf.data_ptr(), E + q_pad, kd.data_ptr(), vd.data_ptr(), int(tke)
    d.win_back, d.win_ahead = wb, wa
    d.ctx, d.ctx_bs = ctx.data_ptr(), E + ctx_pad
    bufs = dict(q=qbuf, k=kd, v=vd, ctx=ctx, la=la)
    if la is not None:
        d.last_attended = la.data_ptr()
    if outs in ("attn", "both"):
        bufs["attn"] = _nan(dev, B, Tk)
        d.attn = bufs["attn"].data_ptr()
    if outs in ("seq", "both"):
        bufs["seq"] = _nan(dev, steps, B, Tk)
        d.attn_seq, d.attn_seq_ts = bufs["seq"].data_ptr(), B * Tk
    if key_len is not None:
        bufs["kl"] = torch.tensor(key_len, dtype=torch.int32, device=dev)
        d.key_len = bufs["kl"].data_ptr()
    d.B, d.E, d.Tk = B, E, Tk
    return d, bufs


def _check_attn_item(got_p, got_ctx, ref, bound, what):
    ep, ectx = bound
    lo, hi = ref["lo"], ref["hi"]
    assert not got_p[:lo].any() and not got_p[hi:].any(), what + ": probabilities outside the window are not 0.0"
    r1 = assert_close_elementwise(got_p, ref["p"], 0, ep, what + " p")
    r2 = assert_close_elementwise(got_ctx, ref["ctx"], 0, ectx, what + " ctx")
    return max(r1, r2)


@pytest.mark.parametrize("Tk", [1, 3, 4, 40, 257, 700])
def test_attn_step_elementwise(dev, Tk):
    ops, L, S, C = _env()
    worst, n = 0.0, 0
    for c in R.ATTN_CASES:
        if c["Tk"] != Tk:
            continue
        B, E = c["B"], c["E"]
        q, k, v = R.attn_inputs(c)
        per_item = c["key_len"] is not None
        t = 3 + (c["seed"] & 1)                      # reads slot t & 1, writes slot (t + 1) & 1
        la = None
        if c["la"] is not None:
            la = torch.full((2, B) if per_item else (2,), -7, dtype=torch.int32, device=dev)
            la[t & 1] = torch.tensor(c["la"] if per_item else c["la"][0], dtype=torch.int32)
        d, bufs = _attn_desc(dev, B, E, Tk, c["tke"], q, k, v, la, c["wb"], c["wa"], c["key_len"], c["outs"], c["q_pad"],
                             c["ctx_pad"], t + 1)
        bufs["q"][:, :E] = torch.from_numpy(q).to(dev)
        if c["seed"] & 2:
            _launch_entry(1, d, t)                   # t = NULL: the step index travels in the descriptor
        else:
            t_dev = torch.tensor([t], dtype=torch.int32, device=dev)
            d.t = t_dev.data_ptr()
            ops._lib.call("dv3_attn_step_f32", ctypes.byref(d), ops._stream())
        torch.cuda.synchronize()
        what = "attn_step B%d E%d Tk%d tke%d la%s w(%d,%d) kl%s %s" % (B, E, Tk, c["tke"], c["la"], c["wb"], c["wa"],
                                                                     c["key_len"], c["outs"])
        ctx = bufs["ctx"].cpu().double().numpy()
        assert np.isnan(ctx[:, E:]).all() and _guards_intact(bufs["q"], E), what
        ps = []
        if "attn" in bufs:
            ps.append(bufs["attn"].cpu().double().numpy())
        if "seq" in bufs:
            seq = bufs["seq"].cpu().double().numpy()
            assert np.isnan(seq[:t]).all(), what + ": attn_seq rows of other steps written"
            ps.append(seq[t])
        if len(ps) == 2:
            assert np.array_equal(ps[0], ps[1]), what
        refs = R.attn_case_refs(c, q, k, v)
        for b, (ref, bound) in enumerate(refs):
            worst = max(worst, _check_attn_item(ps[0][b], ctx[b, :E], ref, bound, "%s item %d" % (what, b)))
        if la is not None:
            lah = la.cpu().numpy()
            if per_item:
                assert lah[(t + 1) & 1].tolist() == [r[0]["argmax"] for r in refs], what
                assert lah[t & 1].tolist() == c["la"], what
            else:
                assert int(lah[(t + 1) & 1]) == refs[0][0]["argmax"] and int(lah[t & 1]) == c["la"][0], what
        n += 1
    _report("attn_step Tk %d (%d cases)" % (Tk, n), worst)


@pytest.mark.parametrize("pair", [(3, 4), (7, 8), (1, 66), (2, 258), (130, 131)])
def test_attn_step_first_maximum_on_exact_ties(dev, pair):
    """two bit-identical keys share the largest probability exactly (no rounding involved: the same arithmetic on the
    same bits): the FIRST one is the argmax (torch.max / deepvoice3.py:445), whichever lanes and waves hold the two"""
    ops, L, S, C = _env()
    B, E, Tk = 2, 64, 300
    c = R.attn_case(B, E, Tk, 1, seed=900 + pair[0])
    q, k, v = R.attn_inputs(c)
    for b in range(B):
        k[b, pair[0]] = k[b, pair[1]] = q[b] * np.float32(8.0)
    for per_item in (False, True):
        la = torch.full((2, B) if per_item else (2,), 5, dtype=torch.int32, device=dev)
        d, bufs = _attn_desc(dev, B, E, Tk, 1, q, k, v, la, Tk, Tk, [Tk, Tk - 1] if per_item else None, "attn", 0, 0, 1)
        bufs["q"][:, :E] = torch.from_numpy(q).to(dev)
        t_dev = torch.zeros(1, dtype=torch.int32, device=dev)
        d.t = t_dev.data_ptr()
        ops._lib.call("dv3_attn_step_f32", ctypes.byref(d), ops._stream())
        torch.cuda.synchronize()
        p = bufs["attn"].cpu().numpy()
        for b in range(B if per_item else 1):
            ref = R.attn_step_ref(q[b], k[b], v[b], 5, Tk, Tk, (Tk - b) if per_item else None)
            assert ref["argmax"] == pair[0] and ref["gap"] == 0.0
            assert p[b, pair[0]] == p[b, pair[1]] == p[b].max(), (pair, b)
            got = la.cpu().numpy()[1]
            assert int(got[b] if per_item else got) == pair[0], (pair, per_item, b, got)


@pytest.mark.parametrize("run", R.ATTN_RUNS)
def test_attn_step_hands_last_attended_over(dev, run):
    """consecutive steps with a new query each: slot t & 1 is read, slot (t + 1) & 1 written; plain mode: every item
    follows item 0's window, per-item mode: each its own -- against the reference's running last_attended"""
    ops, L, S, C = _env()
    B, E, Tk, tke, per_item, steps, t0 = run
    q, k, v, kl = R.attn_run_inputs(run)
    refs, la_ref = R.attn_run_refs(run, q, k, v, kl)
    la = torch.full((2, B) if per_item else (2,), -7, dtype=torch.int32, device=dev)
    la[t0 & 1] = 0
    d, bufs = _attn_desc(dev, B, E, Tk, tke, q[0], k, v, la, 1, 3, kl, "both", 1, 2, t0 + steps)
    t_dev = torch.tensor([t0], dtype=torch.int32, device=dev)
    d.t = t_dev.data_ptr()
    qd = torch.from_numpy(q).to(dev)
    ctxs, las = [], []
    for s in range(steps):
        bufs["q"][:, :E].copy_(qd[s])
        ops._lib.call("dv3_attn_step_f32", ctypes.byref(d), ops._stream())
        ctxs.append(bufs["ctx"].clone())
        las.append(la.clone())
        t_dev.add_(1)
    torch.cuda.synchronize()
    seq = bufs["seq"].cpu().double().numpy()
    assert np.isnan(seq[:t0]).all()
    worst = 0.0
    for s in range(steps):
        t = t0 + s
        lah = las[s].cpu().numpy()
        want = la_ref[s + 1] if per_item else la_ref[s + 1][0]
        assert np.array_equal(lah[(t + 1) & 1], want), (run, s, lah.tolist(), la_ref[s + 1])
        ctx = ctxs[s].cpu().double().numpy()
        assert np.isnan(ctx[:, E:]).all()
        for b, (ref, bound) in enumerate(refs[s]):
            worst = max(worst, _check_attn_item(seq[t, b], ctx[b, :E], ref, bound, "attn run %s step %d item %d" % (run, s, b)))
    assert np.array_equal(bufs["attn"].cpu().double().numpy(), seq[t0 + steps - 1])
    _report("attn_step run %s" % (run,), worst)


# ------------------------------------------------------------------------------------------------------------------
# (d) synthetic step programs
# ------------------------------------------------------------------------------------------------------------------
D_IN, C_GLU, E_ATT, TK = 24, 40, 32, 9          # 40 gated rows: 3 tiles, more than a 1- or 2-member group has workgroups
N_MAX, MIN_STEPS, MAX_STEPS = 16, 4, 10
_layers = {}


def _prog_layers(dev):
    if "l" not in _layers:
        from deepvoice3_pytorch_amd.conv import Conv1d, Linear
        torch.manual_seed(11)
        ls = dict(glu=Conv1d(D_IN, 2 * C_GLU, 3, dilation=2), query=Linear(C_GLU, E_ATT), out=Linear(E_ATT, C_GLU),
                  last=Linear(C_GLU, D_IN), fc=Linear(D_IN, 1))
        for m in ls.values():
            m.to(dev).eval()
            with torch.no_grad():
                m.weight.mul_(2.0)
                m.bias.normal_(0, 0.3)
        with torch.no_grad():
            ls["fc"].bias.fill_(-30.0)                 # sigmoid ~ 0: the schedule added through post_add decides `done`
        g = torch.Generator().manual_seed(5)
        _layers["l"] = ls
        _layers["kv"] = (torch.randn(9, E_ATT, TK, generator=g).to(dev), torch.randn(9, E_ATT, TK, generator=g).to(dev))
        _layers["x0"] = torch.rand(9, D_IN, generator=g).to(dev)
    return _layers["l"], _layers["kv"], _layers["x0"]


def _schedule(kind, B):
    """done flags added to the (zero) sigmoid output of the done layer: [N_MAX][B][1] of 0 / 1"""
    s = torch.zeros(N_MAX, B, 1)
    if kind == "before":            # fires from step 1 on, long before min_steps: the loop still runs min_steps + 1 steps
        s[1:] = 1
    elif kind == "exact":           # fires at step index min_steps only (steps = min_steps + 1), never again
        s[MIN_STEPS] = 1
    elif kind == "some":            # item 0 early, the last item at step index 7: the batch stops when all have
        s[2:, 0] = 1
        s[7:, 1:] = 1
        s[6, B - 1] = 0
    else:
        assert kind == "never"
    return s


def _build_program(dev, B, sched):
    from deepvoice3_pytorch_amd import ops
    from deepvoice3_pytorch_amd.decode_program import StepProgram
    ls, (k, v), x0 = _prog_layers(dev)
    with torch.no_grad():
        P = StepProgram(B, dev)
        cur = P.buffer(B, D_IN)
        cur.copy_(x0[:B])
        outs, dones, aligns = _nan(dev, N_MAX, B, D_IN), _nan(dev, N_MAX, B, 1), _nan(dev, N_MAX, B, TK)
        states = _nan(dev, N_MAX, B, C_GLU)
        pa = sched.to(dev)
        xg = P.conv_step(ls["glu"], cur, ops.EPI_GLU, C_GLU, k=3, dil=2, gated=True)
        q = P.conv_step(ls["query"], xg, ops.EPI_LINEAR, E_ATT)
        ctx = P.attn_step(q, k[:B].contiguous(), v[:B].contiguous(), 1, 3, True, attn_seq=aligns)
        st = P.conv_step(ls["out"], ctx, ops.EPI_LINEAR, C_GLU, r=xg, out_seq=states)
        pre = P.conv_step(ls["last"], st, ops.EPI_LINEAR, D_IN, y_act=cur, out_seq=outs)
        P.conv_step(ls["fc"], pre, ops.EPI_SIGMOID, 1, post_add=pa, out_seq=dones)
        P.keep.extend([outs, dones, aligns, states, pa])
    return P, dict(cur=cur, outs=outs, dones=dones, aligns=aligns, states=states, xg=xg, q=q, ctx=ctx, st=st, pre=pre)


def _call_program(P, bufs, entry, t0, n_steps, have_done, wg):
    """one dv3_decode_program_run / _launch call -> steps_out (run) or n_steps (launch)"""
    ops, L, S, C = _env()
    arr, _ = P._entries(bufs["cur"], None)
    p = S["dv3_decode_program"]()
    p.entries_host = ctypes.addressof(arr)
    p.n_entries, p.B, p.t0, p.n_steps = len(P.prog), P.B, t0, n_steps
    if entry == "dv3_decode_program_launch":
        ops._lib.call(entry, ctypes.byref(p), ops._stream())
        torch.cuda.synchronize()
        return n_steps
    entries = torch.frombuffer(bytearray(bytes(arr)), dtype=torch.uint8).to(P.dev)
    sync = torch.empty(L.dv3_decode_program_sync_ints(P.B), dtype=torch.int32, device=P.dev)
    steps_out = torch.full((1,), -5, dtype=torch.int32, device=P.dev)
    p.entries = entries.data_ptr()
    if have_done:
        p.done_seq, p.done_ts = bufs["dones"].data_ptr(), bufs["dones"].stride(0)
    p.min_steps, p.max_steps = MIN_STEPS, MAX_STEPS
    p.sync, p.steps_out, p.wg_per_group = sync.data_ptr(), steps_out.data_ptr(), wg
    ops._lib.call(entry, ctypes.byref(p), ops._stream())
    torch.cuda.synchronize()
    n = int(steps_out.item())
    if n == -1:
        pytest.exit("dv3_decode_program_run: a device barrier timed out (B %d, wg_per_group %d)" % (P.B, wg), returncode=3)
    return n


SEQS = ("outs", "dones", "aligns", "states")


@pytest.mark.parametrize("B", [1, 4, 5, 9])
@pytest.mark.parametrize("wg", [0, 1, 3, 8])
def test_program_drivers_equal_launch_by_launch(dev, B, wg):
    """wg_per_group 0 / 1 / 3 / 8: P = 16 (the & 7 mapping), one workgroup for a group's three tiles and four attention
    reads, the plain mapping, the & 7 mapping at 8 -- all bit-identical to one launch per entry per step"""
    for kind in ("before", "exact", "some", "never"):
        sched = _schedule(kind, B)
        # launch by launch, N_MAX steps: the yardstick
        P0, b0 = _build_program(dev, B, sched)
        for _ in range(N_MAX):
            P0.run_step()
        torch.cuda.synchronize()
        assert all(bool(torch.isfinite(b0[k]).all()) for k in SEQS)
        rows = (b0["dones"].reshape(N_MAX, B) > 0.5).tolist()
        assert rows == (sched.reshape(N_MAX, B) > 0.5).tolist()
        for n_steps, have_done in ((6, True), (14, True), (13, False)):
            want = R.stop_steps(rows, 0, n_steps, MIN_STEPS, MAX_STEPS, have_done)
            P1, b1 = _build_program(dev, B, sched)
            assert _call_program(P1, b1, "dv3_decode_program_launch", 0, n_steps, have_done, wg) == n_steps
            P2, b2 = _build_program(dev, B, sched)
            got = _call_program(P2, b2, "dv3_decode_program_run", 0, n_steps, have_done, wg)
            what = "B %d wg %d %s n_steps %d done_seq %s" % (B, wg, kind, n_steps, have_done)
            assert got == want, "%s: steps_out %d, the stop rule gives %d" % (what, got, want)
            own = (b2["dones"][:got].reshape(got, B) > 0.5).tolist()
            assert got == R.stop_steps(own + [[False] * B] * N_MAX, 0, n_steps, MIN_STEPS, MAX_STEPS, have_done), what
            for k in SEQS:
                assert _bits(b1[k][:n_steps], b0[k][:n_steps]), "%s: launch %s" % (what, k)
                assert _bits(b2[k][:got], b0[k][:got]), "%s: run %s" % (what, k)
                assert bool(torch.isnan(b2[k][got:]).all()), "%s: run wrote %s past its last step" % (what, k)
                assert bool(torch.isnan(b1[k][n_steps:]).all()), what
        # t0 > 0: three steps by a first call (no stop: below min_steps), the rest by a second one
        for entry in ("dv3_decode_program_launch", "dv3_decode_program_run"):
            P3, b3 = _build_program(dev, B, sched)
            assert _call_program(P3, b3, entry, 0, 3, True, wg) == 3
            got = _call_program(P3, b3, entry, 3, 11, True, wg)
            want = R.stop_steps(rows, 3, 11, MIN_STEPS, MAX_STEPS, True) if entry.endswith("run") else 11
            assert got == want, (entry, B, wg, kind, got, want)
            for k in SEQS:
                assert _bits(b3[k][:3 + got], b0[k][:3 + got]), (entry, B, wg, kind, k)


@pytest.mark.parametrize("B", [1, 4, 5, 9])
def test_program_first_step_elementwise(dev, B):
    """one step of the persistent program at every workgroup mapping: each entry against float64 of ITS OWN fp32 inputs
    as the device left them (nothing compounds), and launch by launch the same bits"""
    ls, (k, v), x0 = _prog_layers(dev)
    sched = _schedule("never", B)
    worst = 0.0

    def host(t):
        return t.detach().cpu().numpy()

    def dense(m):
        w = host(m.weight)
        return np.ascontiguousarray(w.transpose(0, 2, 1)) if w.ndim == 3 else w[:, None, :]

    for wg in (0, 1, 3, 8):
        P, b = _build_program(dev, B, sched)
        assert _call_program(P, b, "dv3_decode_program_run", 0, 1, True, wg) == 1
        x = host(x0[:B])
        chain = [("glu", ls["glu"], x, "glu", dict(), b["xg"], 3 * D_IN),
                 ("query", ls["query"], host(b["xg"]), "linear", dict(), b["q"], C_GLU),
                 ("out", ls["out"], host(b["ctx"]), "linear", dict(r=host(b["xg"])), b["states"][0], E_ATT),
                 ("last", ls["last"], host(b["st"]), "linear", dict(want_act=True), b["outs"][0], C_GLU),
                 ("fc", ls["fc"], host(b["pre"]), "sigmoid", dict(post_add=host(sched[0])), b["dones"][0], D_IN)]
        for name, m, xin, mode, kw, got, K in chain:
            J = 3 if name == "glu" else 1
            ref = R.conv_step_ref(xin[None], dense(m), host(m.bias), mode, 2, **kw)
            bkw = {kk: vv for kk, vv in kw.items() if kk != "want_act"}
            bnd = R.conv_step_bound(ref, mode, J, xin.shape[1], **bkw)
            key = "y_act" if kw.get("want_act") else "y"
            worst = max(worst, assert_close_elementwise(got, ref["out_seq"], 0, bnd[key], "program B %d wg %d %s" % (B, wg, name)))
        assert _bits(b["cur"], b["outs"][0])                       # y_act feeds the next step's input
        kh, vh, qh = host(k[:B]).transpose(0, 2, 1), host(v[:B]).transpose(0, 2, 1), host(b["q"])
        for i in range(B):
            ref = R.attn_step_ref(qh[i], kh[i], vh[i], 0, 1, 3)
            worst = max(worst, _check_attn_item(host(b["aligns"][0, i]).astype(np.float64), host(b["ctx"][i]).astype(np.float64),
                                                ref, R.attn_step_bound(ref, E_ATT, TK), "program B %d wg %d attn item %d" % (B, wg, i)))
    _report("program first step B %d" % B, worst)

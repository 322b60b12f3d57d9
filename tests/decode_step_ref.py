# coding: utf-8
"""float64 restatements of the decode-step entry points (include/dv3hip.h, "Autoregressive decode step"), the shape
lists the GPU tests run, and the error bounds they hold the kernels to.

Written from the header contract and the reference expressions it cites (conv.py:17-46, modules.py:157-164 / 224-226,
deepvoice3.py:143-171 / 463-470), not from csrc/decode_step.hip.  What IS restated from the kernel is said so: the tile
constants of the step-tile image (the header gives its order, the kernel its padding quantum) and the summation depths the
bounds count.  tests/test_cpu_decode_step_ref.py pins every function here against the oracle.

u = 2^-24 is the fp32 unit roundoff; an operation documented to 1 ulp errs by <= 2u relative.
"""
import math

import numpy as np

U = 2.0 ** -24
SQRT_HALF = math.sqrt(0.5)
MODES = ("linear", "relu", "sigmoid", "softsign", "glu", "highway")
GATED = ("glu", "highway")
# restated from csrc/decode_step.hip: rows per tile, batch items per workgroup, prefetched weights per thread, padding
# quantum of the window, unroll of the loop after the prefetch
MT, NB, KPF, KPAD_Q, TAIL_U = 16, 4, 24, 64, 8
LDS_MAX = 65536


def cdiv(a, b):
    return -(-a // b)


def kpad_of(J, Cin):
    return cdiv(J * Cin, KPAD_Q) * KPAD_Q


def nu_of(J, Cin, gated):
    """window elements one thread accumulates (its FMA chain length)"""
    return kpad_of(J, Cin) // (32 if gated else 64)


def tail_path(J, Cin, gated):
    return nu_of(J, Cin, gated) > KPF


def partial_tail(J, Cin, gated):
    return tail_path(J, Cin, gated) and (nu_of(J, Cin, gated) - KPF) % TAIL_U != 0


def lds_bytes(J, Cin):
    return (kpad_of(J, Cin) * NB + 64 * MT * 2 * NB + 16 * MT * 2 * NB) * 4


def pack_floats(Ktot, M, Cg):
    rows = Cg if Cg > 0 else M
    return cdiv(rows, MT) * cdiv(Ktot, KPAD_Q) * KPAD_Q * (2 * MT if Cg > 0 else MT)


# ------------------------------------------------------------------------------------------------------------------
# weights
# ------------------------------------------------------------------------------------------------------------------
def fwd_pack_of(W, Cg, lda, a_half, fill=np.nan):
    """dense W [M][J][Cin] -> dv3_weight_norm_pack_f32's fwd_pack [J*Cin][lda] (gated: `a` rows at column 0, gate rows at
    column a_half); the columns no row owns hold `fill` (the pack must not read them)"""
    M, J, Cin = W.shape
    out = np.full((J * Cin, lda), fill, dtype=np.float32)
    wt = W.reshape(M, J * Cin).T
    if Cg > 0:
        out[:, :Cg] = wt[:, :Cg]
        out[:, a_half:a_half + Cg] = wt[:, Cg:]
    else:
        out[:, :M] = wt
    return out


def step_tile_image(fwd_pack, lda, a_half, Ktot, M, Cg):
    """the image dv3_conv_step_pack_f32 must write: [row block of 16][window element, zero-padded to a multiple of 64]
    [16 rows] (gated: [16 `a` rows | 16 gate rows]); rows past the layer and padding window elements are 0.0"""
    fp = np.asarray(fwd_pack, dtype=np.float32).reshape(-1, lda)
    rows = Cg if Cg > 0 else M
    nblk, kpad = cdiv(rows, MT), cdiv(Ktot, KPAD_Q) * KPAD_Q
    halves = 2 if Cg > 0 else 1
    img = np.zeros((nblk, kpad, halves, MT), dtype=np.float32)
    for blk in range(nblk):
        n = min(MT, rows - blk * MT)
        for h in range(halves):
            c0 = (a_half if h else 0) + blk * MT
            img[blk, :Ktot, h, :n] = fp[:Ktot, c0:c0 + n]
    out = img.reshape(-1)
    assert out.size == pack_floats(Ktot, M, Cg)
    return out


def untile_image(img, lda, a_half, Ktot, M, Cg, fill=np.nan):
    """the inverse of step_tile_image on the elements a row owns"""
    rows = Cg if Cg > 0 else M
    nblk, kpad = cdiv(rows, MT), cdiv(Ktot, KPAD_Q) * KPAD_Q
    halves = 2 if Cg > 0 else 1
    img = np.asarray(img).reshape(nblk, kpad, halves, MT)
    fp = np.full((Ktot, lda), fill, dtype=np.float32)
    for blk in range(nblk):
        n = min(MT, rows - blk * MT)
        for h in range(halves):
            c0 = (a_half if h else 0) + blk * MT
            fp[:, c0:c0 + n] = img[blk, :Ktot, h, :n]
    return fp


# ------------------------------------------------------------------------------------------------------------------
# conv step
# ------------------------------------------------------------------------------------------------------------------
def _sigmoid(v):
    return 1.0 / (1.0 + np.exp(-v))


def conv_step_ref(x_hist, W, bias, mode, dil=1, residual=False, spk=None, r=None, r2=None, post_add=None,
                  want_act=False):
    """one incremental conv layer at step t = len(x_hist) - 1, in float64.

    x_hist [t+1][B][Cin]: the fp32 frames of steps 0..t (frames before step 0 are zeros: the cleared ring);
    W [M][J][Cin] dense (gated: rows [0, Cg) are the `a` half, [Cg, 2Cg) the gate); bias [M] or None; spk / r / r2 [B][Cout];
    post_add [B][Cout]: the step's own row.  -> dict: y, y_pre (before post_add), y_act (sigmoid(y) when want_act),
    out_seq (y_act if want_act else y), and for the bounds: pre (the `a` half / the plain pre-activation), S = sum|w||x| +
    |bias| + |spk| of it, gate and Sg of the gate half, xr (the new frame as residual / carry)."""
    x_hist = np.asarray(x_hist, dtype=np.float64)
    W = np.asarray(W, dtype=np.float64)
    M, J, Cin = W.shape
    t, B = x_hist.shape[0] - 1, x_hist.shape[1]
    win = np.zeros((B, J, Cin))
    for j in range(J):                      # tap J-1 = the new frame, tap j = the frame (J-1-j)*dil steps back
        s = t - (J - 1 - j) * dil
        if s >= 0:
            win[:, j] = x_hist[s]
    acc = win.reshape(B, -1) @ W.reshape(M, -1).T
    mag = np.abs(win).reshape(B, -1) @ np.abs(W).reshape(M, -1).T
    if bias is not None:
        b64 = np.asarray(bias, dtype=np.float64)
        acc, mag = acc + b64, mag + np.abs(b64)
    out = {}
    gated = mode in GATED
    if gated:
        Cg = M // 2
        a, g = acc[:, :Cg], acc[:, Cg:]
        Sa, Sg = mag[:, :Cg], mag[:, Cg:]
        if spk is not None:
            s64 = np.asarray(spk, dtype=np.float64)
            a, Sa = a + s64, Sa + np.abs(s64)
        sg = _sigmoid(g)
        xr = x_hist[t] if (mode == "highway" or residual) else None
        if mode == "glu":                   # modules.py:157-164
            y = a * sg
            if residual:
                y = (y + xr) * SQRT_HALF
        else:                               # modules.py:224-226
            y = sg * a + (1.0 - sg) * xr
        out.update(pre=a, S=Sa, gate=g, Sg=Sg, xr=xr)
    else:
        v = acc
        out.update(pre=acc, S=mag, gate=None, Sg=None, xr=None)
        if mode == "relu":
            v = np.maximum(v, 0.0)
        elif mode == "sigmoid":
            v = _sigmoid(v)
        elif mode == "softsign":
            v = v / (1.0 + np.abs(v))
        else:
            assert mode == "linear", mode
        if r is not None:
            v = (v + np.asarray(r, dtype=np.float64)) * SQRT_HALF
        y = v
    if r2 is not None:
        y = (y + np.asarray(r2, dtype=np.float64)) * SQRT_HALF
    out["y_pre"] = y
    if post_add is not None:
        y = y + np.asarray(post_add, dtype=np.float64)
    out["y"] = y
    out["y_act"] = _sigmoid(y) if want_act else None
    out["out_seq"] = out["y_act"] if want_act else y
    return out


def _sig_err(v, ev):
    """|fl(1 / (1 + expf(-v))) - sigmoid(v)| for an argument off by <= ev: sigmoid' <= s(1-s) + |s''| ev with |s''| <= 0.1,
    then expf (1 ulp = 2u, weighted by 1-s), the add (u) and the division (1 ulp = 2u), all relative to s"""
    s = _sigmoid(v)
    return (s * (1.0 - s) + 0.1 * ev) * ev + s * ((1.0 - s) * 2 * U + 3 * U)


def _res_err(y_out, e):
    """(y + r) * sqrt(.5): the incoming error scaled, plus the add, the rounded constant and the multiply (3u of the result)"""
    return SQRT_HALF * e + 3 * U * np.abs(y_out)


def conv_step_bound(ref, mode, J, Cin, residual=False, spk=None, r=None, r2=None, post_add=None, has_bias=True):
    """per-element |kernel - float64| bounds for y, y_pre and y_act of one conv step, from the kernel's arithmetic:
    a thread's chain of nu FMAs (one rounding each; the zero padding adds none), NKS/16 - 1 adds in the first reduction
    stage, 15 adds in the second, then one add per bias / speaker bias: k = nu + NKS/16 - 1 + 15 + addends roundings, each
    at most u times the running magnitude <= S, and 1.001 for the second-order terms (k u < 1e-5).  The tails propagate
    that bound through each operation's derivative and add the operation's own roundings."""
    gated = mode in GATED
    nu = nu_of(J, Cin, gated)
    nks = 32 if gated else 64
    k0 = nu + nks // 16 - 1 + 15
    ea = 1.001 * (k0 + int(has_bias) + int(gated and spk is not None)) * U * ref["S"]
    if gated:
        a, g, xr = ref["pre"], ref["gate"], ref["xr"]
        eg = 1.001 * (k0 + int(has_bias)) * U * ref["Sg"]
        sg = _sigmoid(g)
        es = _sig_err(g, eg)
        if mode == "glu":
            y = a * sg
            e = sg * ea + np.abs(a) * es + ea * es + U * np.abs(y)          # the product: both factors off, one rounding
            if residual:
                y = (y + xr) * SQRT_HALF
                e = _res_err(y, e)
        else:
            t1, t2 = sg * a, (1.0 - sg) * xr
            y = t1 + t2
            # sgm*a (u), 1-sgm (u), *xr (u), the sum (u; a contracted fma rounds less): <= 3u (|t1| + |t2|)
            e = sg * ea + (np.abs(a) + np.abs(xr)) * es + ea * es + 3 * U * (np.abs(t1) + np.abs(t2))
    else:
        v = ref["pre"]
        if mode == "relu":                  # 1-Lipschitz, exact
            y, e = np.maximum(v, 0.0), ea
        elif mode == "sigmoid":
            y, e = _sigmoid(v), _sig_err(v, ea)
        elif mode == "softsign":            # d/dv = 1 / (1 + |v|)^2 at the nearest point of [v - e, v + e]; add (u), division (2u)
            y = v / (1.0 + np.abs(v))
            e = ea / (1.0 + np.maximum(np.abs(v) - ea, 0.0)) ** 2 + 3 * U * np.abs(y)
        else:
            y, e = v, ea
        if r is not None:
            y = (y + np.asarray(r, dtype=np.float64)) * SQRT_HALF
            e = _res_err(y, e)
    if r2 is not None:
        y = (y + np.asarray(r2, dtype=np.float64)) * SQRT_HALF
        e = _res_err(y, e)
    out = {"y_pre": e * 1.001}
    if post_add is not None:                # one add
        y = y + np.asarray(post_add, dtype=np.float64)
        e = e + U * np.abs(y)
    out["y"] = e * 1.001
    out["y_act"] = _sig_err(y, out["y"]) * 1.001
    return out


# ------------------------------------------------------------------------------------------------------------------
# attention step
# ------------------------------------------------------------------------------------------------------------------
def attn_window(la, win_back, win_ahead, s):
    """deepvoice3.py:150-156 on s keys -> [lo, hi)"""
    lo, hi = 0, s
    if la is not None:
        if la - win_back > 0:
            lo = la - win_back
        if la + win_ahead < s:
            hi = la + win_ahead
    return lo, hi


def attn_step_ref(q, k, v, la=None, win_back=1, win_ahead=3, key_len=None):
    """one attention read of ONE item at Tq = 1 (deepvoice3.py:143-171): q [E], k / v [Tk][E] fp32; la: last attended key or
    None (window off); key_len: the item's own key count s (per-utterance mode: keys n >= s take no part, the context
    scale is s sqrt(1/s)) or None (s = Tk).
    -> dict: p [Tk] (exact 0.0 outside the window), ctx [E], argmax (first maximum), gap (largest minus second largest
    probability; the runner-up of a single key is 0), and for the bounds: Ssc [Tk] = sum|q||k|, sc, lo, hi, s."""
    q, k, v = (np.asarray(a, dtype=np.float64) for a in (q, k, v))
    Tk = k.shape[0]
    s = Tk if key_len is None else min(max(int(key_len), 1), Tk)
    lo, hi = attn_window(la, win_back, win_ahead, s)
    assert lo < hi, "empty window"
    sc = k @ q
    p = np.zeros(Tk)
    e = np.exp(sc[lo:hi] - sc[lo:hi].max())
    p[lo:hi] = e / e.sum()
    ctx = (p[lo:hi] @ v[lo:hi]) * (s * math.sqrt(1.0 / s))
    top = np.sort(p)[::-1]
    return dict(p=p, ctx=ctx, argmax=int(np.argmax(p)), gap=float(top[0] - (top[1] if Tk > 1 else 0.0)),
                Ssc=np.abs(k) @ np.abs(q), sc=sc, lo=lo, hi=hi, s=s, absv=np.abs(v))


def attn_step_bound(ref, E, Tk):
    """per-element bounds for the probabilities and the context of one item.
    scores: ceil(E/64) FMAs per lane, then a 6-level wave sum: ks = ceil(E/64) + 6 roundings of <= u Ssc[n] each;
    the subtraction of the maximum rounds once more (u |sc - max|).  A probability is shift-invariant, so score errors
    <= D move log p by <= 2D: p (exp(2D) - 1).  Then expf in the numerator and in every term of the denominator (2u
    each), the denominator's ceil(Tk/256) + 8 adds, the reciprocal (2u) and the product (u).  A flushed subnormal expf
    costs <= 2^-126 absolute.  context: the probabilities' errors times |v|, a chain of (hi - lo) FMAs over sum p|v|,
    then the scale s * sqrtf(1/s) (reciprocal 2u, sqrtf 2u, product u) and the final product (u): 6u of the result."""
    lo, hi, s = ref["lo"], ref["hi"], ref["s"]
    sc = ref["sc"][lo:hi]
    ks = cdiv(E, 64) + 6
    D = float((1.001 * ks * U * ref["Ssc"][lo:hi]).max() + 2 * U * np.abs(sc - sc.max()).max())
    rel = math.expm1(2 * D) + (4 + cdiv(Tk, 256) + 8 + 3) * U
    ep = np.zeros(Tk)
    ep[lo:hi] = 1.001 * rel * ref["p"][lo:hi] + 2.0 ** -126
    scale = s * math.sqrt(1.0 / s)
    absv = ref["absv"][lo:hi]
    ectx = scale * 1.001 * (ep[lo:hi] @ absv + (hi - lo) * U * (ref["p"][lo:hi] @ absv)) + 6 * U * np.abs(ref["ctx"])
    return ep, ectx


# ------------------------------------------------------------------------------------------------------------------
# the device stop rule
# ------------------------------------------------------------------------------------------------------------------
def stop_steps(done_rows, t0, n_steps, min_steps, max_steps, have_done):
    """dv3_decode_program_run's steps_out, as the header states the rule: after step t (steps = t + 1) stop if there is a
    done_seq and (steps > min_steps and done_seq[t][b] > 0.5 for all b, or steps > max_steps); without one, n_steps run.
    done_rows[t]: the B booleans done > 0.5 of ABSOLUTE step t.  -> the number of steps executed in the call"""
    for s in range(n_steps):
        steps = t0 + s + 1
        if have_done and ((steps > min_steps and all(done_rows[t0 + s])) or steps > max_steps):
            return s + 1
    return n_steps


# ------------------------------------------------------------------------------------------------------------------
# the cases of tests/test_gpu_decode_step.py (tests/test_cpu_decode_step_ref.py asserts what each list claims)
# ------------------------------------------------------------------------------------------------------------------
# (Ktot, M, Cg, lda, a_half): plain and gated, rows off the 16-row tile, one row, Ktot off the 64 quantum, lda > M, a_half > Cg
PACK_CASES = [(64, 16, 0, 16, 0), (5, 1, 0, 4, 0), (130, 23, 0, 28, 0), (3 * 80, 80, 0, 80, 0), (256, 7, 0, 8, 0),
              (64, 32, 16, 32, 16), (7, 2, 1, 8, 4), (3 * 21, 2 * 23, 23, 52, 24), (5 * 128, 2 * 80, 80, 168, 84),
              (832, 2 * 7, 7, 16, 8)]


def conv_case(mode, B, Cin, Cout, J=1, dil=1, Lx=0, **kw):
    """Lx: ring slots beyond the minimum (J-1)*dil + 1.  kw: residual, spk, r, r2, bias (default True), post_add
    ("t": dense [t][B][Cout], "b": batch-strided), y_pre, y_act, out_seq, x_ts (teacher forcing), x_pad (x_bs - Cin)"""
    c = dict(mode=mode, B=B, Cin=Cin, Cout=Cout, J=J, dil=dil, L=(J - 1) * dil + 1 + Lx, residual=False, spk=False,
             r=False, r2=False, bias=True, post_add=None, y_pre=False, y_act=False, out_seq=False, x_ts=False, x_pad=0)
    c.update(kw)
    c["gated"] = mode in GATED
    c["M"] = 2 * Cout if c["gated"] else Cout
    c["steps"] = 3 * c["L"] + 2
    return c


def case_name(c):
    flags = [k for k in ("residual", "spk", "r", "r2", "y_pre", "y_act", "out_seq", "x_ts") if c[k]]
    return "%s B%d Cin%d Cout%d J%d d%d L%d %s%s%s%s" % (
        c["mode"], c["B"], c["Cin"], c["Cout"], c["J"], c["dil"], c["L"], "+".join(flags), "" if c["bias"] else " nobias",
        (" post_add:" + c["post_add"]) if c["post_add"] else "", " x_pad%d" % c["x_pad"] if c["x_pad"] else "")


# every mode, with and without the tails; J x dil x L beyond the minimum; batch and channel edges
CONV_SWEEP = [
    conv_case("linear", 1, 1, 1),
    conv_case("linear", 3, 5, 7, J=2, dil=1, Lx=3, r=True, out_seq=True),
    conv_case("linear", 4, 80, 16, J=3, dil=3, r2=True, y_pre=True, post_add="t"),
    conv_case("linear", 5, 128, 80, J=1, r=True, r2=True, y_act=True, out_seq=True, x_pad=3),
    conv_case("linear", 9, 256, 256, J=2, dil=9, Lx=3, bias=False, post_add="b", x_ts=True),
    conv_case("linear", 3, 301, 23, J=2, dil=1, Lx=1, x_pad=5),                 # Cin > 256, not a multiple of 4
    conv_case("relu", 4, 80, 128, J=1, x_ts=True),
    conv_case("relu", 5, 5, 1, J=5, dil=27, Lx=3, r=True),
    conv_case("relu", 37, 16, 23, J=3, dil=1, Lx=2, r2=True),                   # the larger batch: 10 batch groups
    conv_case("sigmoid", 9, 128, 1, J=1, out_seq=True),
    conv_case("sigmoid", 3, 7, 16, J=5, dil=3, Lx=3, r=True, r2=True, y_pre=True, post_add="t"),
    conv_case("softsign", 4, 16, 7, J=3, dil=9, y_act=True),
    conv_case("softsign", 1, 80, 80, J=2, dil=27, Lx=3, r=True, bias=False),
    conv_case("glu", 1, 1, 1, J=1),
    conv_case("glu", 3, 7, 7, J=3, dil=1, residual=True, spk=True),
    conv_case("glu", 4, 16, 16, J=3, dil=3, Lx=3, residual=True, r2=True, out_seq=True),
    conv_case("glu", 5, 80, 23, J=2, dil=9, Lx=1, spk=True, post_add="t", y_pre=True),
    conv_case("glu", 9, 128, 128, J=5, dil=1, residual=True, bias=False, x_ts=True, x_pad=4),
    conv_case("glu", 4, 256, 256, J=3, dil=27, Lx=3, residual=True, spk=True, y_act=True, out_seq=True),
    conv_case("glu", 3, 5, 80, J=1, r2=True, post_add="b"),
    conv_case("highway", 1, 16, 16, J=3, dil=1),
    conv_case("highway", 5, 7, 7, J=2, dil=3, Lx=3, r2=True),
    conv_case("highway", 9, 80, 80, J=3, dil=9, y_pre=True, post_add="t"),
    conv_case("highway", 4, 23, 23, J=5, dil=27, Lx=3, x_ts=True),
]
# gated layers around the end of the prefetch: nu = kpad / 32 = 24 (all prefetched), 26 (a partial block of the loop after
# it), 32 (one whole block), 48 (J*Cin = 1536: the LDS limit); the plain layer at nu = 24 for the other template
CONV_TAIL = [
    conv_case("glu", 5, 256, 23, J=3, dil=1, residual=False, spk=True),                  # nu 24
    conv_case("glu", 4, 416, 7, J=2, dil=3, Lx=3, r2=True),                              # nu 26
    conv_case("highway", 3, 270, 270, J=3, dil=1, Lx=1),                                 # kpad 832: nu 26, Ktot off the quantum
    conv_case("glu", 9, 512, 16, J=2, dil=1, y_act=True, out_seq=True),                  # nu 32
    conv_case("glu", 3, 512, 80, J=3, dil=9, Lx=3, spk=True, post_add="t"),              # nu 48
    conv_case("highway", 5, 307, 307, J=5, dil=1),                                       # kpad 1536, Ktot 1535: nu 48
    conv_case("linear", 4, 512, 23, J=3, dil=1, r=True),                                 # plain, nu 24
]
TAIL_NU = {24: 1, 26: 2, 32: 1, 48: 2}      # gated nu -> how many CONV_TAIL cases sit there


def preset_conv_cases(decoder, B):
    """the conv / projection layers of a built decoder (builder.<preset>(**bench.PRESETS[..]).seq2seq.decoder) that
    fit the step kernel's LDS window, as conv_cases: every distinct (kind, Cin, Cout, k, dil); gated layers with the
    decoder's own residual / speaker-bias settings, plain ones with the tails the decoders hang on them in turn"""
    out, seen = [], set()
    plain_kw = [dict(), dict(r=True, r2=True, out_seq=True), dict(y_act=True, out_seq=True), dict(y_pre=True, post_add="t")]
    plain_mode = ["linear", "relu", "sigmoid"]
    inner = set()
    for name, m in decoder.named_modules():
        kind = type(m).__name__
        if kind in ("Conv1dGLU", "HighwayConv1d"):
            inner.add(id(m.conv))
            inner.add(id(getattr(m, "speaker_proj", None)))
            cv = m.conv
            Cin, Cout, k, d = cv.in_channels, cv.out_channels // 2, cv.kernel_size[0], cv.dilation[0]
            if kind == "Conv1dGLU":
                c = conv_case("glu", B, Cin, Cout, J=k, dil=d, residual=bool(m.residual), spk=m.speaker_proj is not None)
            else:
                c = conv_case("highway", B, Cin, Cout, J=k, dil=d)
        elif kind in ("Conv1d", "Linear") and id(m) not in inner:
            if kind == "Conv1d":
                Cin, Cout, k, d = m.in_channels, m.out_channels, m.kernel_size[0], m.dilation[0]
            else:
                Cin, Cout, k, d = m.in_features, m.out_features, 1, 1
            c = conv_case(plain_mode[len(out) % 3], B, Cin, Cout, J=k, dil=d, **plain_kw[len(out) % 4])
        else:
            continue
        key = (c["gated"], c["mode"] if c["gated"] else "", Cin, Cout, k, d)
        if key in seen or lds_bytes(k, Cin) > LDS_MAX:
            continue
        seen.add(key)
        out.append(c)
    return out


def attn_case(B, E, Tk, tke, la=None, wb=1, wa=3, key_len=None, outs="attn", q_pad=0, ctx_pad=0, seed=0):
    """la: list of B last-attended keys (window on) or None; key_len: list of B or None; outs: attn / seq / both"""
    return dict(B=B, E=E, Tk=Tk, tke=tke, la=la, wb=wb, wa=wa, key_len=key_len, outs=outs, q_pad=q_pad, ctx_pad=ctx_pad,
                seed=seed)


def _la_set(Tk):
    """last attended keys 0, 1, Tk-3, Tk-1, each inside the keys"""
    return sorted(set(min(max(v, 0), Tk - 1) for v in (0, 1, Tk - 3, Tk - 1)))


def _attn_cases():
    cases = []
    i = 0
    for Tk in (1, 3, 4, 40, 257, 700):
        for E in (1, 64, 96, 256, 300):
            i += 1
            tke = i & 1
            outs = ("attn", "seq", "both")[i % 3]
            cases.append(attn_case(3, E, Tk, tke, outs=outs, q_pad=i % 4, ctx_pad=(i + 1) % 3, seed=i))       # window off
            las = _la_set(Tk)
            wb, wa = ((1, 3), (0, 2), (2, 5))[i % 3]
            # plain mode: every item reads item 0's window
            for la in las:
                cases.append(attn_case(3, E, Tk, 1 - tke, la=[la] * 3, wb=wb, wa=wa, outs=outs, q_pad=(i + 1) % 4,
                                       ctx_pad=i % 3, seed=100 + i))
            # per-item mode: own key counts (clamped to [1, Tk]) and own windows, each inside its own keys
            kl = [Tk, max(Tk // 2, 1), 1, max(Tk - 1, 1), min(3, Tk)]
            la5 = [min(las[j % len(las)], kl[j] - 1) for j in range(5)]
            cases.append(attn_case(5, E, Tk, tke, la=la5, wb=wb, wa=wa, key_len=kl, outs=outs, seed=200 + i))
            cases.append(attn_case(5, E, Tk, 1 - tke, key_len=kl, outs="both", seed=300 + i))
    return cases


ATTN_CASES = _attn_cases()
# multi-step runs: (B, E, Tk, tke, per_item, steps, t0)
ATTN_RUNS = [(5, 96, 40, 1, False, 8, 0), (5, 96, 40, 0, True, 8, 3), (3, 300, 257, 1, True, 6, 1),
             (4, 64, 12, 0, False, 7, 2)]


def attn_inputs(c):
    """fp32 q [B][E], k / v [B][Tk][E]: scores of a few units (the softmax is neither flat nor one-hot)"""
    rs = np.random.RandomState(1000 + c["seed"])
    B, E, Tk = c["B"], c["E"], c["Tk"]
    q = (rs.standard_normal((B, E)) * (2.0 / math.sqrt(E))).astype(np.float32)
    k = rs.standard_normal((B, Tk, E)).astype(np.float32)
    v = rs.standard_normal((B, Tk, E)).astype(np.float32)
    return q, k, v


def attn_case_refs(c, q=None, k=None, v=None):
    """-> per item (ref, (ep, ectx)).  Plain mode with the window on: every item reads item 0's last_attended"""
    if q is None:
        q, k, v = attn_inputs(c)
    out = []
    for b in range(c["B"]):
        la = None if c["la"] is None else (c["la"][b] if c["key_len"] is not None else c["la"][0])
        ref = attn_step_ref(q[b], k[b], v[b], la, c["wb"], c["wa"], None if c["key_len"] is None else c["key_len"][b])
        out.append((ref, attn_step_bound(ref, c["E"], c["Tk"])))
    return out


def attn_run_inputs(run):
    B, E, Tk, tke, per_item, steps, t0 = run
    rs = np.random.RandomState(77 + E + Tk)
    q = (rs.standard_normal((steps, B, E)) * (3.0 / math.sqrt(E))).astype(np.float32)
    k = rs.standard_normal((B, Tk, E)).astype(np.float32)
    v = rs.standard_normal((B, Tk, E)).astype(np.float32)
    kl = [max(Tk - 3 * b, 1) for b in range(B)] if per_item else None
    return q, k, v, kl


def attn_run_refs(run, q=None, k=None, v=None, kl=None):
    """the reference's running last_attended (deepvoice3.py:445), from 0: -> refs[step][b], la[step + 1][b]"""
    B, E, Tk, tke, per_item, steps, t0 = run
    if q is None:
        q, k, v, kl = attn_run_inputs(run)
    la = [[0] * B]
    refs = []
    for s in range(steps):
        row = []
        for b in range(B):
            ref = attn_step_ref(q[s, b], k[b], v[b], la[-1][b if per_item else 0], 1, 3, kl[b] if per_item else None)
            row.append((ref, attn_step_bound(ref, E, Tk)))
        refs.append(row)
        la.append([row[b if per_item else 0][0]["argmax"] for b in range(B)])
    return refs, la

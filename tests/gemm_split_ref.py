# coding: utf-8
"""Host-side restatement of the split-operand GEMMs (include/dv3hip.h, "Split-bf16" / "f16x3") in float64.

What csrc/common.h builds per operand (dv3_split8_f16, dv3_pair_word), what the three tap-GEMMs compute from (B, C, T)
tensors, the value a three-term kernel would return in exact arithmetic, and a DERIVED per-element error bound against
the float64 reference.  tests/test_cpu_gemm_split_ref.py proves this file without a GPU; tests/test_gpu_gemm_operands.py
holds the kernels to it.  The GEMM functions are plain torch and run on whatever device their arguments live on (the
B = 64 references are float64 matrix products on the GPU); the SPLITS always run on the host, in numpy, because what the
device does with fp16 subnormals is the thing under test.

Operand forms (`form`): ("f16", s) -- a = v * 2^s as an fp16 hi / lo pair; ("bf16",) -- a bf16 hi / lo pair of v;
("bf16_1",) -- the single bf16 value bf16_rn(v), no lo plane (mode "bf16": split_terms == 1 / split_bf16 == 2; csrc/common.h
converts with (__bf16)v, round to nearest even); None -- the fp32 value itself (mode "f32").

The single-term mode is held to the SAME-ROUNDING reference: the float64 GEMM of the rounded operands (`reference` with the
forms given, = `three_term`).  Its operand term is zero by construction and only the accumulation term remains; where the
result is stored as bf16 (the c8 tensors, DV3_IO_AB_BF16) `bf16_out_bound` adds the one rounding of the store.  tests/
test_cpu_gemm_bf16_ref.py proves these parts without a GPU; tests/test_gpu_gemm_bf16.py holds the kernels to them.

The bound of one output element, both parts tensors of the output's shape:
  operand term       sum |w| d(a) + d(w) |a| + |lo_a| |lo_w|      d() = the header's per-operand statement:
                     f16 pair: max(2^-23 |a|, 2^-25) in a-units; bf16 pair: 2^-17 |v|.  hi + lo = a - e with |e| <= d(a),
                     the kernel sums (hi + lo)(hi' + lo') - lo lo', so the first-order error of a product is
                     e w + a e' + lo lo'.  (The second-order e e' is < 2^-17 of the first and is not carried.)
                     Zero in the f32 mode.
  accumulation term  (n + c) 2^-24 (sum |w| |x| + |addend|)       n products summed into one output in fp32, each addition
                     rounded to nearest: the order-independent worst case (Higham, Accuracy and Stability, sec. 4.2,
                     first order), so tile, k-split, stream-K and slab forms share it; c = 2 for the epilogue's bias
                     add and store.  Products of two fp16 (11 x 11 bits) or bf16 (8 x 8 bits) values are exact in fp32.
"""
import numpy as np
import torch
import torch.nn.functional as F

F16_ACT_SHIFT, F16_WEIGHT_SHIFT = 4, 8          # DV3_F16_ACT_SHIFT / DV3_F16_WEIGHT_SHIFT (include/dv3hip.h)
F16_MAX = 65504.0
U32 = 2.0 ** -24                                # unit roundoff of fp32
EPILOGUE_OPS = 2


# ---------------------------------------------------------------------------------------------------------------
# operand forms
# ---------------------------------------------------------------------------------------------------------------
def forms(gemm, mode):
    """(form of the activation-side operand, form of the weight-side operand) of `gemm` in GEMM mode `mode`.
    gemm: "fwd" (x, w), "dgrad" (g, w), "wgrad" (g, x).  The forward of the default mode runs on scaled fp16 pairs, every
    gradient GEMM of both split modes on bf16 pairs (deepvoice3_pytorch_amd/ops.py, "GEMM arithmetic")."""
    if mode == "f32":
        return None, None
    if mode == "bf16":          # one bf16 MFMA per product in all three GEMMs
        return ("bf16_1",), ("bf16_1",)
    if mode == "f16x3" and gemm == "fwd":
        return ("f16", F16_ACT_SHIFT), ("f16", F16_WEIGHT_SHIFT)
    assert mode in ("f16x3", "bf16x3"), mode
    return ("bf16",), ("bf16",)


def _np64(v):
    if torch.is_tensor(v):
        v = v.detach().cpu().numpy()
    v = np.asarray(v)
    assert v.dtype in (np.float32, np.float64), v.dtype
    v64 = v.astype(np.float64)
    assert np.array_equal(v64.astype(np.float32).astype(np.float64), v64), "operands must be fp32 values"
    return v64


def _rn_f16(a, flush):
    with np.errstate(over="ignore"):
        h = a.astype(np.float16).astype(np.float64)       # round to nearest even, subnormals kept (IEEE)
    if flush:
        h = np.where(np.abs(h) < 2.0 ** -14, 0.0, h)
    return h


def split_f16(v, shift, flush=False):
    """dv3_split8_f16: a = v * 2^shift, hi = fp16_rn(clamp(a, +-65504)), lo = fp16_rn(a - hi) with the residual taken from
    the UNCLAMPED a.  -> (hi, lo) as float64 arrays in a-units.  flush=True models a device on which fp16 subnormals become
    zero (in the conversion or at the MFMA inputs -- the same to the sum): only for the sensitivity tests."""
    a = _np64(v) * 2.0 ** shift
    assert np.all(np.abs(a[np.isfinite(a)]) < 2.0 ** 127), "v * 2^shift must stay an fp32 value"
    hi = _rn_f16(np.clip(a, -F16_MAX, F16_MAX), flush)
    with np.errstate(invalid="ignore"):
        lo = _rn_f16(a - hi, flush)                       # a - hi is exact in fp32 (and here)
    return hi, lo


def _rn_bf16(v64):
    t = torch.from_numpy(np.ascontiguousarray(v64.astype(np.float32)))
    return t.to(torch.bfloat16).to(torch.float64).numpy()  # round to nearest even on the host


def bf16_rn(v):
    """(__bf16)v of csrc/common.h: round to nearest, ties to even -- on the host, as float64"""
    return _rn_bf16(_np64(v))


def split_bf16_pair(v):
    """dv3_pair_word / split8 of the gradient GEMMs: hi = bf16_rn(v), lo = bf16_rn(v - hi).  -> (hi, lo), float64."""
    v = _np64(v)
    hi = _rn_bf16(v)
    lo = _rn_bf16(v - hi)                                 # v - hi is exact in fp32
    return hi, lo


def pair_words(v):
    """the PAIR WORD tensor of v (include/dv3hip.h), built on the host: int32 bits to be viewed as float32"""
    hi, lo = split_bf16_pair(v)
    hb = torch.from_numpy(hi.astype(np.float32)).view(torch.int32) & -65536
    lb = (torch.from_numpy(lo.astype(np.float32)).view(torch.int32) >> 16) & 0xffff
    return (hb | lb).view(torch.float32)


def split(v, form, flush=False):
    """-> (hi, lo, shift): the pair in the units the kernel accumulates in (v * 2^shift); form None: (v, 0, 0)."""
    if form is None:
        v = _np64(v)
        return v, np.zeros_like(v), 0
    if form[0] == "f16":
        hi, lo = split_f16(v, form[1], flush)
        return hi, lo, form[1]
    if form[0] == "bf16_1":
        hi = bf16_rn(v)
        return hi, np.zeros_like(hi), 0
    hi, lo = split_bf16_pair(v)
    return hi, lo, 0


def single(form):
    return form is not None and form[0] == "bf16_1"


def rounded(v, form):
    """the operand the reference of a mode multiplies: bf16_rn(v) in the single-term mode, v itself otherwise"""
    return bf16_rn(v) if single(form) else _np64(v)


def delta(v, form):
    """the header's per-operand statement |a - hi - lo| <= delta, in v-units (float64 array)"""
    v = np.abs(_np64(v))
    if form is None or single(form):        # single-term: the reference multiplies the rounded operand itself
        return np.zeros_like(v)
    if form[0] == "f16":
        return np.maximum(2.0 ** -23 * v, 2.0 ** (-25 - form[1]))
    return 2.0 ** -17 * v


# ---------------------------------------------------------------------------------------------------------------
# the three GEMMs in float64 (torch; any device)
# ---------------------------------------------------------------------------------------------------------------
def _t64(a, device=None):
    t = torch.from_numpy(np.ascontiguousarray(a)) if isinstance(a, np.ndarray) else a
    return t.to(dtype=torch.float64, device=device if device is not None else t.device)


def shifted(x, J, dil, padL):
    """x (B, C, T) -> (B, J, C, T): tap j holds x[t + j*dil - padL], zero outside the sequence"""
    T = x.shape[-1]
    padR = max((J - 1) * dil - padL, 0)
    xp = F.pad(x, (padL, padR))
    return torch.stack([xp[..., j * dil: j * dil + T] for j in range(J)], dim=1)


def conv_fwd(x, w, dil, padL):
    """y[b, m, t] = sum_j sum_c w[m, c, j] x[b, c, t + j*dil - padL]      (Tout = Tin, zero padding; no bias)"""
    xs = shifted(x, w.shape[2], dil, padL)                                  # (B, J, C, T)
    B, J, C, T = xs.shape
    y = torch.matmul(w.permute(0, 2, 1).reshape(w.shape[0], J * C), xs.reshape(B, J * C, T))
    return y


def conv_dgrad(g, w, dil, padL):
    """dx[b, c, t] = sum_j sum_m w[m, c, j] g[b, m, t - j*dil + padL]: the input gradient of conv_fwd"""
    J = w.shape[2]
    return conv_fwd(g, w.transpose(0, 1).flip(2), dil, (J - 1) * dil - padL)


def conv_wgrad(g, x, J, dil, padL):
    """dw[j, m, c] = sum_b sum_t g[b, m, t] x[b, c, t + j*dil - padL]: the weight gradient of conv_fwd, per tap (the
    layout of the kernel's slabs).  A dropout keep mask and its 1 / (1 - p) are applied to x by the caller."""
    xs = shifted(x, J, dil, padL)                                           # (B, J, C, T)
    return torch.einsum("bmt,bjct->jmc", g, xs)


def make_mm(gemm, dil, padL, J):
    """the bilinear map (activation-side operand, weight-side operand) -> output of one GEMM"""
    if gemm == "fwd":
        return lambda a, w: conv_fwd(a, w, dil, padL)
    if gemm == "dgrad":
        return lambda a, w: conv_dgrad(a, w, dil, padL)
    assert gemm == "wgrad", gemm
    return lambda a, w: conv_wgrad(a, w, J, dil, padL)


def n_products(gemm, mode, *, J, K, B, T, n_slabs=1, k_split=False):
    """products summed into one output element in fp32: 3 J Kp (Kp = K rounded up to the 32-channel chunk) for the split
    tap-GEMMs, J K in the f32 mode.  Weight gradient: the frames of the LARGEST SLAB (the slabs are added in float64 on
    the host), three terms each in the split modes -- a k-split launch cuts the B ceil(T / 32) frame chunks into n_slabs
    contiguous ranges of ceil(. / n_slabs) chunks, the others give slab s the batch items s, s + n_slabs, ...
    (csrc/wgrad_gemm.hip, wgrad_gemm_bf16x3.hip, wgrad_taps2.hip)."""
    terms = 1 if mode in ("f32", "bf16") else 3
    if mode == "bf16" and gemm != "wgrad":
        return J * ((K + 31) // 32 * 32)        # one term, over the 32-channel chunks the MFMAs consume
    if gemm == "wgrad":
        if k_split:
            chunks = B * ((T + 31) // 32)
            frames = min(B * T, -(-chunks // n_slabs) * 32)
        else:
            frames = -(-B // n_slabs) * T
        return terms * frames
    return terms * J * ((K + 31) // 32 * 32 if terms == 3 else K)


# ---------------------------------------------------------------------------------------------------------------
# expectation and bound
# ---------------------------------------------------------------------------------------------------------------
def reference(mm, act, wgt, addend=None, device=None, form_a=None, form_w=None):
    """the float64 GEMM -- of the operands as given, or (single-term forms) of the operands rounded as the kernel rounds"""
    y = mm(_t64(rounded(act, form_a), device), _t64(rounded(wgt, form_w), device))
    return y if addend is None else y + _t64(_np64(addend), device)


def three_term(mm, act, wgt, form_a, form_w, addend=None, flush=False, drop_lo=None, device=None):
    """What a split kernel returns in exact arithmetic: sum(hi hi' + hi lo' + lo hi') in the accumulator's units, times the
    epilogue's 2^-(s_a + s_w) (2^-12 for f16x3, 1 for bf16 pairs), plus the addend (bias).  form None: the plain product.
    drop_lo (defect model): ("act" | "wgt", boolean array of that operand's shape), True where its lo plane is lost."""
    ah, al, sa = split(act, form_a, flush)
    wh, wl, sw = split(wgt, form_w, flush)
    if drop_lo is not None:
        al = np.where(drop_lo[1], 0.0, al) if drop_lo[0] == "act" else al
        wl = np.where(drop_lo[1], 0.0, wl) if drop_lo[0] == "wgt" else wl
    ah, al, wh, wl = (_t64(t, device) for t in (ah, al, wh, wl))
    y = mm(ah, wh)
    if form_a is not None and not single(form_a):
        y = y + mm(ah, wl) + mm(al, wh)
    y = y * 2.0 ** -(sa + sw)
    return y if addend is None else y + _t64(_np64(addend), device)


def bound(mm, act, wgt, form_a, form_w, n, addend=None, device=None):
    """per-element bound of |kernel - float64 reference| (module docstring) -> (bound, operand term, accumulation term)"""
    A, W = np.abs(rounded(act, form_a)), np.abs(rounded(wgt, form_w))
    At, Wt = _t64(A, device), _t64(W, device)
    mag = mm(At, Wt)
    if addend is not None:
        mag = mag + _t64(np.abs(_np64(addend)), device)
    acc = (n + EPILOGUE_OPS) * U32 * mag
    if form_a is None or single(form_a):
        return acc, torch.zeros_like(acc), acc
    _, al, sa = split(act, form_a)
    _, wl, sw = split(wgt, form_w)
    op = mm(_t64(delta(act, form_a), device), Wt) + mm(At, _t64(delta(wgt, form_w), device)) + \
        mm(_t64(np.abs(al), device), _t64(np.abs(wl), device)) * 2.0 ** -(sa + sw)
    return op + acc, op, acc


def emulate(gemm, act, wgt, form_a, form_w, *, J, dil, padL, addend=None, flush=False, drop_lo=None, seed=0):
    """A split kernel on the host: the three exact products of every (tap, channel) -- or (batch item, frame) -- pair,
    added in fp32 (every addition rounded) in a random order, descaled, plus the addend in fp32.  Small shapes only."""
    ah, al, sa = split(act, form_a, flush)
    wh, wl, sw = split(wgt, form_w, flush)
    if drop_lo is not None:
        al = np.where(drop_lo[1], 0.0, al) if drop_lo[0] == "act" else al
        wl = np.where(drop_lo[1], 0.0, wl) if drop_lo[0] == "wgt" else wl
    planes = [(ah, wh)] if (form_a is None or single(form_a)) else [(ah, wh), (ah, wl), (al, wh)]
    terms = []                                            # each (n_k, outputs...) of exact float64 products
    for a, w in planes:
        a, w = _t64(a), _t64(w)
        if gemm == "wgrad":
            xs = shifted(w, J, dil, padL)                 # (B, J, C, T)
            p = torch.einsum("bmt,bjct->btjmc", a, xs)
            terms.append(p.reshape(-1, *p.shape[2:]))
        else:
            if gemm == "dgrad":
                w, pl = w.transpose(0, 1).flip(2), (J - 1) * dil - padL
            else:
                pl = padL
            xs = shifted(a, J, dil, pl)                   # (B, J, C, T)
            p = torch.einsum("mcj,bjct->jcbmt", w, xs)
            terms.append(p.reshape(-1, *p.shape[2:]))
    p = torch.cat(terms, 0).numpy()
    if form_a is not None:
        assert np.array_equal(p.astype(np.float32).astype(np.float64), p), "a product is not exact in fp32"
    order = np.random.RandomState(seed).permutation(p.shape[0])
    acc = np.zeros(p.shape[1:], np.float32)
    for k in order:         # (f32 mode: the fp32 MFMA's fused multiply-add -- the product enters the sum unrounded)
        acc = (acc.astype(np.float64) + p[k]).astype(np.float32)
    acc = acc * np.float32(2.0 ** -(sa + sw))
    if addend is not None:
        acc = acc + _np64(addend).astype(np.float32)
    return torch.from_numpy(acc.astype(np.float64))


# ---------------------------------------------------------------------------------------------------------------
# shapes and input families (shared by the CPU proof and the GPU test)
# ---------------------------------------------------------------------------------------------------------------
# (B, C, T, k, d, causal): the edge set of test_conv_gemm_bf16x3_forward -- column tiles spanning batch items, d = 27
# causal, 5 taps, Cin not a multiple of 32, one frame, sequences shorter than the receptive field, a 1 x 1 conv
EDGE_SHAPES = [(3, 64, 200, 3, 1, False), (3, 96, 150, 3, 27, True), (5, 24, 37, 5, 3, False), (2, 128, 513, 3, 9, True),
               (7, 40, 50, 2, 4, True), (1, 8, 1, 3, 1, True), (1, 16, 3, 3, 2, False), (2, 8, 33, 1, 1, False)]
BENCH_SHAPES = [(64, 512, 150, 3, 1, False), (64, 512, 150, 3, 27, False)]
# shapes the stream-K form of the 256 x 256 tap-GEMM takes when forced (csrc/conv_gemm_pp2.hip: three taps, at least 8
# tiles and 2 units per CU, power-of-two chunk and row-tile counts) -- those of test_stream_k_form_of_the_256x256_tap_gemm
STREAMK_SHAPES = [(24, 256, 410, 3, 1, False), (48, 256, 201, 3, 3, False)]
EXACT = ("E1", "E2", "E3", "E4")
EXACT_BF16 = EXACT + ("E5",)                    # E5 (bf16 midpoints in fp32 storage) belongs to the single-term mode
BOUNDED = ("B1", "B2", "B3", "B4", "B5")
SMALL_MAGNITUDE = ("B2", "B3")                  # where a lost subnormal or a lost lo plane must show (with E2 / E4)


def pad_left(k, d, causal):
    return (k - 1) * d if causal else (k - 1) // 2 * d


def _ints(rng, shape, m):
    return rng.randint(-m, m + 1, size=shape).astype(np.float64)


def _e4(rng, shape, kind):
    """values H + L with hi = H and lo = L exactly: H = h 2^e with h in 5..7 (inside one binade of the format, away from
    its lower edge), |L| below half an ulp of H.  f16 pairs (a-units): H in 1280..1792 (ulp 1), L = l/16, |l| <= 7;
    bf16 pairs: H in 160..224 (ulp 1), L = l/16; f32 mode (no planes): the bf16 H and L = l/4, |l| <= 1, so that eight
    full products still add exactly."""
    hexp, lexp, lmax = {"f16": (8, -4, 7), "bf16": (5, -4, 7), "f32": (5, -2, 1)}[kind]
    h = rng.randint(5, 8, size=shape) * rng.choice([-1.0, 1.0], size=shape)
    l = rng.randint(-lmax, lmax + 1, size=shape)
    return h * 2.0 ** hexp + l * 2.0 ** lexp


def _sparse_channels(C, per_dot):
    """at most per_dot channels, straddling a 32-channel chunk boundary where there is one"""
    want = [31, 32, 0, C - 1, 63, 64, 1, C - 2]
    out = []
    for c in want:
        if 0 <= c < C and c not in out:
            out.append(c)
    return out[:max(1, per_dot)]


def _sparse_frames(B, T):
    """at most 8 (batch item, frame) positions: sequence edges, batch-item boundaries, a 32-frame chunk boundary"""
    want = [(0, 0), (0, T - 1), (B - 1, 0), (B - 1, T - 1), (0, 31), (0, 32), (B // 2, T // 2), (B - 1, 1)]
    out = []
    for b, t in want:
        if 0 <= t < T and (b, t) not in out:
            out.append((b, t))
    return out[:8]


def family(fam, gemm, mode, shape, seed=0):
    """-> dict(act, wgt, addend, quantum): fp32 operands of one input family for one GEMM / mode / shape.
    fwd: act = x (B, C, T), wgt = w (M, C, k) with M = 2 C, addend = bias (M);  dgrad: act = g (B, M, T), wgt = w;
    wgrad: act = g (B, M, T), wgt = x (B, C, T).  quantum (exact families): every product, partial sum and the addend is
    a whole multiple of it."""
    B, C, T, k, d, causal = shape[:6]
    M = shape[6] if len(shape) > 6 else 2 * C         # (the plain c8 shapes name their output channels)
    rng = np.random.RandomState(seed + 1000 * (ord(fam[0]) + int(fam[1])) + C + T + k + d)
    fa, fw = forms(gemm, mode)
    kind = "f32" if fa is None else "bf16" if single(fa) else fa[0]     # E1 .. E4: the single-term form takes bf16's values
    sa = fa[1] if kind == "f16" else 0
    sw = fw[1] if kind == "f16" else 0
    a_shape = (B, C, T) if gemm == "fwd" else (B, M, T)
    w_shape = (B, C, T) if gemm == "wgrad" else (M, C, k)
    Ka = a_shape[1]
    quantum, addend = None, None
    if fam in ("E1", "E2", "E3"):
        mx = 15 if fam != "E2" else 3
        if kind == "f16":       # E2: a = m 2^-16, w' = n 2^-10 (fp16 subnormals / lowest binades); E3: |a|, |w'| <= 15 * 2^11
            qa, qw = {"E1": (0, 0), "E2": (-20, -18), "E3": (7, 3)}[fam]
        else:                   # bf16 pairs and fp32 have fp32's exponent range
            qa, qw = {"E1": (0, 0), "E2": (-60, -60), "E3": (60, 40)}[fam]
        act = _ints(rng, a_shape, mx) * 2.0 ** qa
        wgt = _ints(rng, w_shape, mx) * 2.0 ** qw
        quantum = 2.0 ** (qa + qw)
        if gemm == "fwd":
            addend = _ints(rng, (M,), mx) * quantum
    elif fam == "E4":
        act = _e4(rng, a_shape, kind) * 2.0 ** -sa
        wgt = _e4(rng, w_shape, kind) * 2.0 ** -sw
        keep = np.zeros(a_shape, bool)
        if gemm == "wgrad":
            for b, t in _sparse_frames(B, T):
                keep[b, :, t] = True
        else:
            keep[:, _sparse_channels(Ka, 8 // k), :] = True
        act = np.where(keep, act, 0.0)
        lexp = {"f16": -4, "bf16": -4, "f32": -2}[kind]
        # hi lo' and lo hi' are multiples of 2^(hexp + lexp); the f32 mode also sums lo lo': 2^(2 lexp)
        quantum = 2.0 ** ((2 * lexp if kind == "f32" else ({"f16": 8, "bf16": 5}[kind] + lexp)) - sa - sw)
    elif fam == "E5":
        # bf16 midpoints and their fp32 neighbours: with the bf16 value h 2^(e-7), h in 128 .. 255, the midpoint to the next
        # one is (2h + 1) 2^(e-8); one fp32 ulp is 2^(e-23).  Round to nearest even gives h (h even) or h + 1 (h odd) at the
        # midpoint, truncation always h, round-half-away always h + 1; below / above the midpoint all but truncation agree.
        # The rounded operands are 9-bit integers times 2^(e-7): with e in -1 .. 1 (act) and 0 .. 1 (wgt) and at most
        # 8 products per sum every partial sum stays below 2^(18 + 2 + 1 + 3) / 2 = 2^23 quanta
        def mid(shape_, exps):
            h = rng.randint(128, 256, size=shape_).astype(np.float64)
            e = rng.choice(exps, size=shape_).astype(np.float64)
            off = rng.choice([-1.0, 0.0, 0.0, 1.0], size=shape_)
            return ((2 * h + 1) * 2.0 ** (e - 8) + off * 2.0 ** (e - 23)) * rng.choice([-1.0, 1.0], size=shape_)
        act, wgt = mid(a_shape, [-1, 0, 1]), mid(w_shape, [0, 1])
        keep = np.zeros(a_shape, bool)
        if gemm == "wgrad":
            for b, t in _sparse_frames(B, T):
                keep[b, :, t] = True
        else:
            keep[:, _sparse_channels(Ka, 8 // k), :] = True
        act = np.where(keep, act, 0.0)
        quantum = 2.0 ** (-1 - 7 + 0 - 7)
    else:
        # the weight gradient sums over (b, t): its second operand is an activation, scaled like the first
        if gemm == "wgrad":
            ws = {"B1": 1.0, "B2": 0.05, "B3": 2.0 ** -14, "B4": 1.0, "B5": 1.0}[fam]
        else:
            ws = {"B1": 0.2, "B2": 0.05, "B3": 2.0 ** -14, "B4": 0.05, "B5": 0.2}[fam]
        xs = {"B1": 1.0, "B2": 2.0 ** -12, "B3": 2.0 ** -12, "B4": 1.0, "B5": 1.0}[fam]
        act = rng.standard_normal(a_shape) * xs
        wgt = rng.standard_normal(w_shape) * ws
        if fam == "B4":         # per-channel scales 2^-20 .. 2^6 on the activation, per-row 2^-12 .. 2^2 on the other operand
            act = act * 2.0 ** rng.uniform(-20, 6, size=(1, Ka, 1))
            wgt = wgt * 2.0 ** rng.uniform(-12, 2, size=(1, w_shape[1], 1) if gemm == "wgrad" else (w_shape[0], 1, 1))
        if fam == "B5":         # neighbours along the summed axis: equal on one side, opposite up to 2^-10 on the other
            u = 1.0 + 2.0 ** -10 * rng.uniform(-1, 1, size=w_shape)
            if gemm == "wgrad":                 # summed axis: frames
                act[:, :, 1::2] = act[:, :, 0:-1:2][:, :, :act[:, :, 1::2].shape[2]]
                wgt[:, :, 1::2] = (-wgt * u)[:, :, 0:-1:2][:, :, :wgt[:, :, 1::2].shape[2]]
            else:                               # summed axis: the weight's input channels = the activation's channels
                ax = 1 if gemm == "fwd" else 0
                act[:, 1::2, :] = act[:, 0:-1:2, :][:, :act[:, 1::2, :].shape[1], :]
                wv = np.moveaxis(wgt, ax, 0)
                uv = np.moveaxis(u, ax, 0)
                wv[1::2] = (-wv * uv)[0:-1:2][:wv[1::2].shape[0]]
        if gemm == "fwd":
            addend = rng.uniform(-0.2, 0.2, size=(M,)) * xs * ws / 0.2
    out = dict(act=act.astype(np.float32), wgt=wgt.astype(np.float32), quantum=quantum,
               addend=None if addend is None else addend.astype(np.float32))
    for key in ("act", "wgt", "addend"):      # the families are stated in fp32: nothing may have been rounded away
        if out[key] is not None and fam in EXACT_BF16:
            assert np.array_equal(out[key].astype(np.float64), {"act": act, "wgt": wgt, "addend": addend}[key]), (fam, key)
    return out


def bias_bcast(addend):
    """bias (M,) -> broadcastable against (B, M, T)"""
    return None if addend is None else np.asarray(addend).reshape(1, -1, 1)


# ---------------------------------------------------------------------------------------------------------------
# channel-blocked bf16 storage ("c8", include/dv3hip.h), numpy only
# ---------------------------------------------------------------------------------------------------------------
def c8_groups(C):
    return (C + 31) // 32 * 4


def bf16_bits(v):
    """bf16 values (asserted) -> their 16 bits, uint16"""
    v32 = np.ascontiguousarray(np.asarray(v, dtype=np.float32))
    bits = v32.view(np.uint32)
    assert not np.any(bits & 0xffff), "not bf16 values"
    return (bits >> 16).astype(np.uint16)


def bf16_from_bits(bits):
    return (np.asarray(bits).astype(np.uint32) << 16).view(np.float32).astype(np.float64)


def c8_pack(v):
    """(B, C, T) bf16 values -> uint16 [B][round_up(C, 32) / 8][T][8]: channel c of frame t is element c % 8 of unit
    (b, c / 8, t); channels >= C are zero"""
    v = np.asarray(v)
    B, C, T = v.shape
    full = np.zeros((B, c8_groups(C) * 8, T), np.uint16)
    full[:, :C] = bf16_bits(v)
    return np.ascontiguousarray(full.reshape(B, c8_groups(C), 8, T).transpose(0, 1, 3, 2))


def c8_unpack(bits, C):
    """uint16 [B][G][T][8] -> ((B, C, T) float64, largest |padding channel| -- zero in a well-formed tensor)"""
    bits = np.asarray(bits)
    B, G, T, e = bits.shape
    assert e == 8 and G == c8_groups(C), (bits.shape, C)
    full = bf16_from_bits(bits.transpose(0, 1, 3, 2).reshape(B, G * 8, T))
    pad = float(np.abs(full[:, C:]).max()) if G * 8 > C else 0.0
    return full[:, :C], pad


def keep_bytes(keep):
    """keep (B, C, T) bool -> uint8 [B][round_up(C, 32) / 8][T]: bit e of byte (b, g, t) keeps channel 8 g + e"""
    keep = np.asarray(keep, bool)
    B, C, T = keep.shape
    full = np.zeros((B, c8_groups(C) * 8, T), np.uint8)
    full[:, :C] = keep
    full = full.reshape(B, c8_groups(C), 8, T)
    out = np.zeros((B, c8_groups(C), T), np.uint8)
    for e in range(8):
        out |= (full[:, :, e, :] << e).astype(np.uint8)
    return out


def keep_bits_words(keep):
    """keep (B, C, T) bool -> the keep-BITS form int32 [B * C][ceil(T / 32)]: bit t % 32 of word t / 32 (dv3_conv_desc.xmask)"""
    keep = np.asarray(keep, bool)
    B, C, T = keep.shape
    rs = (T + 31) // 32
    full = np.zeros((B * C, rs * 32), np.uint64)
    full[:, :T] = keep.reshape(B * C, T)
    w = (full.reshape(B * C, rs, 32) << np.arange(32, dtype=np.uint64)).sum(-1)
    return w.astype(np.uint32).view(np.int32), rs


def ulp_bf16(a):
    """spacing of the bf16 numbers in the binade of |a| (8 significand bits; the subnormal spacing 2^-133 below 2^-126)"""
    a = np.abs(np.asarray(a, np.float64))
    e = np.frexp(np.maximum(a, 2.0 ** -126))[1] - 1           # a in [2^e, 2^(e+1))
    return np.ldexp(1.0, e - 7)


def bf16_out_bound(ref, bnd):
    """A value stored as bf16 (round to nearest) from an fp32 tail within `bnd` of `ref`: the tail t has |t| <= |ref| + bnd,
    the store moves it by at most half a bf16 ulp of its own binade: |got - ref| <= bnd + ulp_bf16(|ref| + bnd) / 2."""
    if torch.is_tensor(ref):
        r, b = ref.detach().cpu().numpy(), bnd.detach().cpu().numpy()
        return torch.from_numpy(b + 0.5 * ulp_bf16(np.abs(r) + b)).to(ref.device)
    return bnd + 0.5 * ulp_bf16(np.abs(ref) + bnd)


def expect_bf16(mm, act, wgt, n, *, act_keep=None, wgt_keep=None, out_keep=None, scale=1.0, addend=None,
                ops=EPILOGUE_OPS, device=None):
    """The single-term mode's same-rounding expectation with the dropout forms of the kernels:
        tail = out_keep * scale * mm(bf16_rn(act) * act_keep, bf16_rn(wgt) * wgt_keep) + addend
    in float64 -- the exact value of the kernel's fp32 tail (keeps are 0 / 1 arrays of the operand's / output's shape, scale
    the 1 / (1 - p) the kernel multiplies its ACCUMULATORS by, addend the bias or the input gradient's r_scale * r) -- and
    the bound of the kernel's fp32 tail against it: (n + ops) 2^-24 (out_keep * scale * sum |a| |w| + |addend|), n products
    added in fp32 plus `ops` further roundings in the epilogue (the caller states which).  -> (tail, bound)"""
    a, w = bf16_rn(act), bf16_rn(wgt)
    if act_keep is not None:
        a = a * np.asarray(act_keep, np.float64)
    if wgt_keep is not None:
        w = w * np.asarray(wgt_keep, np.float64)
    y = mm(_t64(a, device), _t64(w, device)) * scale
    mag = mm(_t64(np.abs(a), device), _t64(np.abs(w), device)) * abs(scale)
    if out_keep is not None:
        k = _t64(np.asarray(out_keep, np.float64), device)
        y, mag = y * k, mag * k
    if addend is not None:
        r = _t64(np.asarray(addend, np.float64), device)
        y, mag = y + r, mag + r.abs()
    return y, (n + ops) * U32 * mag


def check_bf16(exact, got, tail, bnd, what, out_bf16=False):
    """One output of a single-term kernel against expect_bf16's (tail, bound).  exact (the E families): every element equals
    the tail -- stored as bf16: equals bf16_rn(tail), nothing else.  Otherwise every element lies inside `bnd` -- stored as
    bf16: inside bf16_out_bound(tail, bnd).  -> the worst ratio to the bound (0 for an exact match)"""
    return check_prepared(exact, got, *prepare_bf16(exact, tail, bnd, what, out_bf16), what=what)


def prepare_bf16(exact, tail, bnd, what="", out_bf16=False):
    """-> (want, bound) of check_bf16, for the callers that check several outputs against one expectation"""
    if exact:
        want = tail
        if out_bf16:
            t32 = tail.float()
            assert torch.equal(t32.double(), tail), what + ": the exact value is not an fp32 value"
            want = t32.cpu().to(torch.bfloat16).double().to(tail.device)        # round to nearest even, on the host
        return want, None
    if out_bf16:
        a = (tail.abs() + bnd).clamp_min(2.0 ** -126)
        bnd = bnd + 0.5 * torch.ldexp(torch.ones_like(a), torch.frexp(a)[1] - 8)     # = bf16_out_bound, on the tensor's device
    return tail, bnd


def check_prepared(exact, got, want, bnd, what):
    got = got.detach().double()
    assert got.shape == want.shape, "%s: shape %s != %s" % (what, tuple(got.shape), tuple(want.shape))
    assert bool(torch.isfinite(got).all()), what + ": not finite"
    if exact:
        if not torch.equal(got, want):
            bad = got != want
            i = tuple(int(v) for v in bad.nonzero()[0])
            raise AssertionError("%s: %d of %d elements differ; first at %s: got %r want %r" %
                                 (what, int(bad.sum()), bad.numel(), i, float(got[i]), float(want[i])))
        return 0.0
    err = (got - want).abs()          # decide where the tensors live, fetch them only to report a failure
    if bool((err <= bnd).all()):
        return float(torch.where(err == 0, torch.zeros_like(err), err / bnd).max())
    from tests.util import assert_close_elementwise
    return assert_close_elementwise(got, want, 0, bnd, what)


def c8_slabs(B, T, S):
    """the K-split of wgrad_c8 (csrc/wgrad_c8.hip): the B ceil(T / 32) (batch item, 32-frame chunk) steps in order, cut into
    S slabs of q = ceil(B ceil(T / 32) / S) steps; trailing slabs may be empty.  -> bool (S, B, T): frames of each slab"""
    n_tc = (T + 31) // 32
    total = B * n_tc
    q = -(-total // S)
    own = np.zeros((S, B, T), bool)
    for s in range(S):
        for gs in range(s * q, min((s + 1) * q, total)):
            b, tc = divmod(gs, n_tc)
            own[s, b, tc * 32: min(T, tc * 32 + 32)] = True
    return own


def c8_slab_frames(B, T, S):
    """frames of the largest slab: the accumulation depth of one element of a wgrad_c8 slab"""
    return int(c8_slabs(B, T, S).reshape(S, -1).sum(1).max())


# (B, C, T, k, d, causal[, M]): what the c8 kernels accept -- J in {1, 3}, (J - 1) d <= 64, same length, Cg % 8 == 0 for the
# gated forms (M = 2 C).  The eligible edge shapes; the halo limit (J - 1) d = 64, causal; a plain 1 x 1 pair whose channel
# counts are multiples of nothing (these two carry M and run the plain forms only)
C8_SHAPES = [(3, 64, 200, 3, 1, False), (3, 96, 150, 3, 27, True), (2, 128, 513, 3, 9, True), (1, 8, 1, 3, 1, True),
             (1, 16, 3, 3, 2, False), (2, 8, 33, 1, 1, False), (2, 40, 50, 3, 4, True), (5, 24, 37, 3, 3, False),
             (2, 32, 70, 3, 32, True), (2, 513, 40, 1, 1, False, 64), (2, 64, 40, 1, 1, False, 513)]
C8_HALO_MAX = 64


def c8_shape_M(shape):
    return shape[6] if len(shape) > 6 else 2 * shape[1]


def c8_reach(shape):
    """which of the places a c8 kernel can go wrong this shape reaches (tests/test_cpu_gemm_bf16_ref.py asserts the set
    C8_SHAPES reaches every one; the tile sizes are those of csrc/conv_planes.hip, conv_c8pp.hip, wgrad_c8.hip)"""
    B, C, T, k, d, causal = shape[:6]
    M = c8_shape_M(shape)
    return dict(spans_items=B > 1 and T % 64 != 0,          # a 64 / 128 / 256-column tile of the flat (b, t) axis holds two items
                one_frame=T == 1, short=T < 4, ragged_chunk=T % 32 != 0, ragged_channels=C % 32 != 0 or M % 32 != 0,
                wgrad_row_tiles=M > 128, wgrad_col_tiles=C > 128,
                wgrad_wide=16 * (32 + (k - 1) * d) > 1024, wgrad_narrow=16 * (32 + (k - 1) * d) <= 1024,
                halo_limit=(k - 1) * d == C8_HALO_MAX, gated_ok=len(shape) == 6 and C % 8 == 0)

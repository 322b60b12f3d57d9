# coding: utf-8
"""Host-side restatement of the tap-GEMMs' nonlinear tails in float64, with DERIVED per-element bounds.

The tails (csrc/conv_common.h: conv_epilogue, conv_epilogue_glu_interior_t, conv_epilogue_glu_wide, conv_epilogue_c8;
csrc/common.h: dv3_gate_deriv; csrc/elementwise.hip: gate_bwd_kernel, gate_bwd_c8_kernel) are the GLU and highway gate
(modules.py:157-164, :224-226), ReLU / sigmoid / softsign with the fused residuals, and the gate backward.
tests/test_cpu_gate_ref.py proves this file without a GPU (a faithful fp32 emulation stays inside the bounds, a list of
defect models does not); tests/test_gpu_gate_tails.py holds the kernels to it.

Input family "G" (family_g): x = integers in [-3, 3] times 2^-2, w = integers in [-3, 3] times 2^-3 (dense), bias per
output channel from LADDER.  Every operand is exact as a scaled fp16 pair (shifts 4 / 8), as a bf16 hi with a zero lo
and in single-term bf16; every product and partial sum is a multiple of 2^-5 below 2^9: the fp32 pre-gate pair is THE
SAME EXACT NUMBER in every GEMM mode, kernel form and summation order, so whatever a tail returns is the tail's own
arithmetic.  The ladder moves whole channels into the sigmoid's saturation: |g| = 17 (1 - s below fp32's resolution at
1), 87 .. 89 (exp(|g|) crosses FLT_MAX = exp(88.72), 1 / (1 + exp(|g|)) crosses 2^-126 = exp(-87.34)), 104 (exp(-|g|)
below the smallest subnormal), 200.

Accuracy of the two hardware operations: v_exp_f32 and v_rcp_f32 are taken as 1 ulp = 2u (HW_ULP), the suite's existing
convention (test_gpu_step_kernels_at_scale.py: "v_rcp_f32 is 1 ulp (2u)").  NOBODY HAS MEASURED THIS CONSTANT ON gfx950
and no header or document at hand states another figure; the bounds below carry it as a named assumption.  Both
operations flush a subnormal result to zero: FLUSH = 2^-126 times the multiplier wherever one may return a subnormal.
fp32 multiplies, adds and fmas keep subnormals (TINY = 2^-149: one rounding in the subnormal range).

The sigmoid of the tails, s^ = rcp(1 + exp2(rn(-g * L))) with L = fp32(log2 e) (__expf), against s = 1 / (1 + e^-g):
    p^ = rn(-g L)         |p^ - (-g log2 e)| <= |g| log2 e (dL + u)     L's own error dL, one rounding of the product
    e^ = v_exp_f32(p^)    relative (ln 2)(that) + HW_ULP = |g| (dL + u) + HW_ULP =: eps_e      (grows with |g|)
    d^ = rn(1 + e^)       relative eps_e e / (1 + e) + u
    s^ = v_rcp_f32(d^)    relative (1 - s) eps_e + u + HW_ULP;   absolute: times s, plus FLUSH
    q^ = rn(1 - s^)       |q^ - (1 - s)| <= ds + u (1 - s + ds): the ABSOLUTE error of s^ lands on 1 - s unreduced
"""
import numpy as np
import torch

from tests import gemm_split_ref as R

U = 2.0 ** -24                        # unit roundoff of fp32
HW_ULP = 2.0 * U                      # ASSUMED accuracy of v_exp_f32 and of v_rcp_f32 (1 ulp); unmeasured on gfx950
FLUSH = 2.0 ** -126                   # a hardware op that would return a subnormal returns zero
TINY = 2.0 ** -149                    # one fp32 rounding in the subnormal range (the sweeps hold +-2^-130)
UB = 2.0 ** -8                        # unit roundoff of bf16 (8 significand bits)
TINY_B = 2.0 ** -134                  # one bf16 rounding in the subnormal range
SECOND = 1.0 + 2.0 ** -12             # second-order terms: every relative term above is below 2^-15 (|g| <= 200)
LOG2E = 1.4426950408889634
L32 = float(np.float32(LOG2E))
DL = abs(L32 - LOG2E) / LOG2E         # 2^-26.2
RS2 = float(np.sqrt(0.5))
RS2_32 = float(np.float32(0.70710678118654752440))
DK = abs(RS2_32 - RS2) / RS2          # the fp32 image of sqrt(.5)
LADDER = (0.0, 0.5, -0.5, 4.0, -4.0, 12.0, -12.0, 17.0, -17.0, 40.0, -40.0, 87.0, -87.0, 88.5, -88.5, 89.0, -89.0,
          104.0, -104.0, 200.0, -200.0)
KINDS = ("glu", "glu_res", "highway")
ACTS = ("linear", "relu", "sigmoid", "softsign")


def rn_bf16(v):
    """float array -> bf16_rn of its fp32 image, as float64 (host rounding: nearest even, subnormals kept)"""
    t = torch.from_numpy(np.ascontiguousarray(np.asarray(v, dtype=np.float32)))
    return t.to(torch.bfloat16).to(torch.float64).numpy()


# ---------------------------------------------------------------------------------------------------------------
# the G family
# ---------------------------------------------------------------------------------------------------------------
def pair_channels(Cg):
    """two (interior, edge) channel pairs: interior below 32 * (Cg // 32), edge in the last, partial 32-row sub-tile;
    where Cg has no partial sub-tile the edge channel sits in the last 32 rows, below 32 channels both in the only one"""
    full = 32 * (Cg // 32)
    if full and full < Cg:
        lo, hi = (0, full), (full, Cg)
    elif Cg >= 64:
        lo, hi = (0, Cg - 32), (Cg - 32, Cg)
    else:
        lo, hi = (0, Cg // 2), (Cg // 2, Cg)
    out = [(lo[0] + (lo[1] - lo[0]) // 3, hi[1] - 1)]
    if lo[1] - lo[0] >= 2 and hi[1] - hi[0] >= 2:
        out.append((lo[1] - 1, hi[0]))
    return out


def sweep(rng, shape, frame_axes=(0, 2)):
    """per-frame magnitude sweep of an input that is no GEMM operand (residual, speaker bias, dy): class of frame
    (b, t) = (b T + t) mod 16 -> 0, +2^-130, -2^-130, then N(0, 1) times 2^-6 .. 2^6"""
    v = rng.standard_normal(shape)
    idx = np.zeros(shape, dtype=np.int64)
    mult = 1
    for ax in reversed(frame_axes):
        sh = [1] * len(shape)
        sh[ax] = shape[ax]
        idx = idx + mult * np.arange(shape[ax]).reshape(sh)
        mult *= shape[ax]
    cls = idx % 16
    scale = 2.0 ** (cls - 9.0)                   # classes 3 .. 15 -> 2^-6 .. 2^6
    out = v * scale
    out = np.where(cls == 0, 0.0, out)
    out = np.where(cls == 1, 2.0 ** -130, out)
    out = np.where(cls == 2, -2.0 ** -130, out)
    return out.astype(np.float32)


def family_g(shape, seed=0):
    """-> dict(x (B, C, T), w (2C, C, k), bias (2C), pairs, r, spk2 (B, C), spk3 (B, C, T), dy), fp32 arrays.  The two
    channel pairs share weight rows, bias (both halves), residual rows and speaker-bias rows."""
    B, C, T, k, d, causal = shape
    rng = np.random.RandomState(seed + 7919 + C + 31 * T + 1009 * k + d)
    x = rng.randint(-3, 4, size=(B, C, T)) * 2.0 ** -2
    w = rng.randint(-3, 4, size=(2 * C, C, k)) * 2.0 ** -3
    lad = np.asarray(LADDER)
    bias = np.concatenate([lad[(rng.permutation(C) + rng.randint(21)) % 21], lad[(rng.permutation(C) + rng.randint(21)) % 21]])
    r = sweep(rng, (B, C, T))
    spk2 = sweep(rng, (B, C), frame_axes=(0, 1))
    spk3 = sweep(rng, (B, C, T))
    dy = sweep(rng, (B, C, T))
    pairs = pair_channels(C)
    for i, e in pairs:
        w[e], w[C + e] = w[i], w[C + i]
        bias[e], bias[C + e] = bias[i], bias[C + i]
        r[:, e], spk2[:, e], spk3[:, e] = r[:, i], spk2[:, i], spk3[:, i]
    return dict(x=x.astype(np.float32), w=w.astype(np.float32), bias=bias.astype(np.float32), pairs=pairs, r=r,
                spk2=spk2, spk3=spk3, dy=dy)


def pre_gates(f, shape, device=None):
    """the exact pre-activations (B, 2C, T) of family_g in float64 (numpy): conv + bias, checked to be multiples of 2^-5
    below 2^9 -- the statement that makes them the same fp32 number whatever the order of the additions"""
    B, C, T, k, d, causal = shape
    padL = R.pad_left(k, d, causal)
    x = torch.from_numpy(f["x"]).to(dtype=torch.float64, device=device)
    w = torch.from_numpy(f["w"]).to(dtype=torch.float64, device=device)
    pre = R.conv_fwd(x, w, d, padL) + torch.from_numpy(f["bias"]).to(dtype=torch.float64, device=device).view(1, -1, 1)
    mag = R.conv_fwd(x.abs(), w.abs(), d, padL) + torch.from_numpy(np.abs(f["bias"])).to(dtype=torch.float64, device=device).view(1, -1, 1)
    pre, mag = pre.cpu().numpy(), mag.cpu().numpy()
    assert mag.max() < 2.0 ** 9 and np.array_equal(np.round(pre * 32.0), pre * 32.0)
    return pre


def add32(a, b):
    """rn_fp32(a + b) of fp32 values, as float64: ONE rounding (numpy's float32 add)"""
    return (np.asarray(a, dtype=np.float32) + np.asarray(b, dtype=np.float32)).astype(np.float64)


def with_cancellation(kind, r, a, g, pairs=(), bf16=False):
    """r with one frame class (b T + t) mod 16 == 9 replaced by the value that cancels the gate's sum to within a few
    ulp: GLU a s + x ~ 0, highway s a + (1 - s) x ~ 0 (only where 1 - s is not tiny)"""
    B, C, T = r.shape
    s, q = sigmoid64(g)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        tgt = -(a * s) if kind != "highway" else np.where(q > 2.0 ** -20, -(a * s) / q, 0.0)
    tgt = np.where(np.isfinite(tgt) & (np.abs(tgt) < 2.0 ** 20), tgt, 0.0)
    j = (np.arange(C).reshape(1, C, 1) % 5 - 2.0)                  # -2 .. 2 ulp off the cancelling value
    tgt = (tgt * (1.0 + j * 2.0 ** -23)).astype(np.float32)
    cls = (np.arange(B).reshape(B, 1, 1) * T + np.arange(T).reshape(1, 1, T)) % 16
    out = np.where(cls == 9, tgt, r).astype(np.float32)
    for i, e in pairs:
        out[:, e] = out[:, i]
    return rn_bf16(out).astype(np.float32) if bf16 else out


# ---------------------------------------------------------------------------------------------------------------
# float64 restatement
# ---------------------------------------------------------------------------------------------------------------
def sigmoid64(g):
    """-> (s, 1 - s), each computed without cancellation"""
    g = np.asarray(g, dtype=np.float64)
    with np.errstate(over="ignore"):
        return 1.0 / (1.0 + np.exp(-g)), 1.0 / (1.0 + np.exp(g))


def gate_fwd(kind, a, g, x):
    """modules.py:157-164: GLU (a sigmoid(g) [+ x]) [sqrt(.5)];  :224-226 highway: T = sigmoid(g), T a + (1 - T) x"""
    s, q = sigmoid64(g)
    if kind == "glu":
        return a * s
    if kind == "glu_res":
        return (a * s + x) * RS2
    assert kind == "highway", kind
    return s * a + q * x


def gate_fwd_torch(kind, a, g, x):
    """the same in torch float64, for autograd"""
    s = torch.sigmoid(g)
    if kind == "glu":
        return a * s
    if kind == "glu_res":
        return (a * s + x) * RS2
    return s * a + (1.0 - s) * x


def gate_bwd(kind, dy, a, g, x):
    """autograd of gate_fwd -> (da, dg, dres): dres = the gradient of the residual / highway input through the tail"""
    s, q = sigmoid64(g)
    d = dy * RS2 if kind == "glu_res" else dy
    if kind == "highway":
        return d * s, d * (a - x) * (s * q), d * q
    return d * s, d * a * (s * q), d


def act_fwd(act, v, r=None, r2=None):
    """conv -> activation -> (+ r) sqrt(.5) -> (+ r2) sqrt(.5) (the fused residual chain of the plain layers)"""
    y = {"linear": lambda t: t, "relu": lambda t: np.maximum(t, 0.0), "sigmoid": lambda t: sigmoid64(t)[0],
         "softsign": lambda t: t / (1.0 + np.abs(t))}[act](np.asarray(v, dtype=np.float64))
    for t in (r, r2):
        if t is not None:
            y = (y + t) * RS2
    return y


def act_bwd(act, dy, y, alpha):
    """gradient of the pre-activation from the SAVED OUTPUT y of the activation (dv3_gate_bwd_f32, plain modes)"""
    d = dy * alpha
    return {"linear": d, "relu": d * (y > 0), "sigmoid": d * y * (1.0 - y), "softsign": d * (1.0 - np.abs(y)) ** 2}[act]


# ---------------------------------------------------------------------------------------------------------------
# bounds
# ---------------------------------------------------------------------------------------------------------------
def sigmoid_err(g):
    """-> (s, q = 1 - s, ds, dq): the bounds of the module docstring, per element"""
    g = np.asarray(g, dtype=np.float64)
    s, q = sigmoid64(g)
    eps_e = np.abs(g) * (DL + U) + HW_ULP             # rounding of -g * log2e (grows with |g|) and v_exp_f32
    rel = q * eps_e                                   # ... through 1 + e: e / (1 + e) = 1 - s of it
    rel = rel + U                                     # the add 1 + e
    rel = rel + HW_ULP                                # v_rcp_f32
    ds = s * rel * SECOND + FLUSH                     # flush floor: exp or rcp returned zero for a subnormal
    dq = ds + U * (q + ds)                            # absolute rounding of 1 - s, on top of s^'s absolute error
    return s, q, ds, dq


def to_bf16_bound(ref, bnd):
    """a bf16 store of a value inside `bnd` of ref: the fp32 bound plus one bf16 rounding"""
    return bnd + UB * (np.abs(ref) + bnd) + TINY_B


def gate_fwd_bound(kind, a, g, x, contracted=True):
    """|tail - gate_fwd| per element.  contracted=True: dv3_gate_out's explicit fma (fp32 tails); False: the c8 tail,
    whose contraction is the compiler's (either product of the highway sum may be the fused one)."""
    a, x = np.abs(np.asarray(a, dtype=np.float64)), np.abs(np.asarray(x, dtype=np.float64))
    s, q, ds, dq = sigmoid_err(g)
    if kind in ("glu", "glu_res"):
        b = a * ds                                    # the sigmoid's error through a
        b = b + U * (a * s + x)                       # dv3_gate_out's fma: one rounding, against |a s| + |x|
        if kind == "glu_res":
            b = b * RS2                               # ... carried through the output scale
        return b * SECOND + 2 * TINY, s
    b = x * dq                                        # (1 - s)'s error through x
    b = b + U * q * x                                 # t = rn((1 - s) x)
    b = b + a * ds                                    # the sigmoid's error through a
    b = b + U * (s * a + q * x) * (1.0 if contracted else 2.0)   # fma(s, a, t): one rounding, against |s a| + |t|
    return b * SECOND + 2 * TINY, s


def fwd_bound(kind, a, g, x, contracted=True):
    """-> (reference y, bound) of one gated tail in fp32"""
    a, g = np.asarray(a, dtype=np.float64), np.asarray(g, dtype=np.float64)
    x = np.zeros_like(a) if (x is None or kind == "glu") else np.asarray(x, dtype=np.float64)
    y = gate_fwd(kind, a, g, x)
    b, _ = gate_fwd_bound(kind, a, g, x, contracted)
    if kind == "glu_res":
        b = b + np.abs(y) * (U + DK) * SECOND         # the output scale: fp32(sqrt(.5))'s own error and the product's rounding
    return y, b


def act_bound(act, v, r=None, r2=None):
    """-> (reference, bound) of a plain tail (conv_common.h:336-341): exact for LINEAR and RELU without a residual"""
    v = np.asarray(v, dtype=np.float64)
    y = act_fwd(act, v)
    if act == "sigmoid":
        b = sigmoid_err(v)[2]
    elif act == "softsign":
        b = np.abs(y) * (U + HW_ULP + U) * SECOND     # rn(1 + |v|), v_rcp_f32 (never subnormal: 1 + |v| < 2^9), the product
    else:
        b = np.zeros_like(y)
    for t in (r, r2):
        if t is not None:
            t = np.asarray(t, dtype=np.float64)
            b = (b + U * np.abs(y + t)) * RS2         # what came in, and the rounding of v + r
            y = (y + t) * RS2
            b = b + np.abs(y) * (U + DK)              # * fp32(sqrt(.5)): its own error and the product's rounding
            b = b * SECOND + TINY
    return y, b


def bwd_bound(kind, dy, a, g, x):
    """-> ((da, dg, dres), (bound_da, bound_dg, bound_dres)) of dv3_gate_deriv (common.h:89-101; the c8 kernel's
    ((d a) s)(1 - s) has the same first-order bound)"""
    dy, a, g = (np.asarray(t, dtype=np.float64) for t in (dy, a, g))
    x = np.zeros_like(a) if x is None else np.asarray(x, dtype=np.float64)
    ref = gate_bwd(kind, dy, a, g, x)
    s, q, ds, dq = sigmoid_err(g)
    d = np.abs(dy) * (RS2 if kind == "glu_res" else 1.0)
    ed = d * (U + DK) + TINY if kind == "glu_res" else 0.0 * d      # d = rn(dy * fp32(sqrt(.5)))
    b_a = d * ds + s * ed + U * np.abs(ref[0])               # va = rn(d s^)
    et = q * ds + s * dq + U * s * q + TINY                  # t = rn(s^ (1 - s^))
    if kind == "highway":
        w = np.abs(a - x)
        em = w * ed + d * U * w + U * d * w + TINY           # rn(a - x), then m = rn(d (a - x))
        b_r = d * dq + q * ed + U * np.abs(ref[2])           # vr = rn(d (1 - s^))
    else:
        w = np.abs(a)
        em = w * ed + U * d * w + TINY                       # m = rn(d a)
        b_r = ed
    b_g = d * w * et + s * q * em + U * np.abs(ref[1])       # vg = rn(m t)
    return ref, tuple(b * SECOND + TINY for b in (b_a, b_g, b_r))


def act_bwd_bound(act, dy, y, alpha):
    """plain modes of dv3_gate_bwd_f32 (elementwise.hip:133-138); alpha is an fp32 number"""
    dy, y = np.asarray(dy, dtype=np.float64), np.asarray(y, dtype=np.float64)
    ref = act_bwd(act, dy, y, alpha)
    # roundings, each relative u of the result: dy alpha | d y, 1 - y, the product | q = 1 - |y| (enters twice), d q, q
    n = {"linear": 1, "relu": 1, "sigmoid": 4, "softsign": 5}[act]
    b = n * U * np.abs(ref)
    return ref, b * SECOND + TINY


def row_sum_bound(terms_abs_sum, elem_bound_sum, depth):
    """a row sum in fp32 of `depth` sequential additions: depth u sum|terms| (order-independent worst case) on top of
    the terms' own bounds"""
    return elem_bound_sum + depth * U * terms_abs_sum * SECOND + TINY


def depth_gate_bwd(T, vec4):
    """summation depth of gate_bwd_kernel's row sums (elementwise.hip:44-123): a lane adds its head / tail element and
    four values per 16-byte quad it owns (quads lane, lane + 64, ...), or every 64th element; then a 6-step butterfly"""
    if vec4:
        return 1 + 4 * (-(-(T // 4 + 1) // 64)) + 6
    return -(-T // 64) + 6


def depth_gate_bwd_c8(T):
    """gate_bwd_c8_kernel (elementwise.hip:207-268): a thread adds every 256th frame, 16 partials per slice, a 4-step
    butterfly over 16 lanes"""
    return -(-T // 256) + 16 + 4


def pair_value(words):
    """pair words (int32 bits) -> hi + lo in float64"""
    w = np.asarray(words).view(np.int32)
    hi = (w & np.int32(-65536)).view(np.float32).astype(np.float64)
    lo = (w << 16).view(np.float32).astype(np.float64)
    return hi + lo


def pair_mismatch(y, pairs, axis=1):
    """number of elements at which the paired channels of family_g differ in their BITS"""
    bits = np.ascontiguousarray(np.asarray(y)).view({4: np.int32, 8: np.int64, 2: np.int16}[np.asarray(y).dtype.itemsize])
    n = 0
    for i, e in pairs:
        n += int((np.take(bits, i, axis=axis) != np.take(bits, e, axis=axis)).sum())
    return n


def worst_ratio(got, ref, bnd):
    """-> (max |got - ref| / bnd with 0 / 0 = 0, index of the worst element); NaN / Inf in got counts as infinite"""
    got, ref, bnd = (np.asarray(t, dtype=np.float64) for t in (got, ref, bnd))
    err = np.abs(got - ref)
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = np.where(err == 0, 0.0, err / bnd)
    ratio = np.where(np.isfinite(got) & np.isfinite(ratio), ratio, np.inf)
    if ratio.size == 0:
        return 0.0, ()
    i = np.unravel_index(int(np.argmax(ratio)), ratio.shape)
    return float(ratio[i]), tuple(int(v) for v in i)

# coding: utf-8
"""float64 restatements of csrc/weight_norm.hip's entry points (include/dv3hip.h, "Weight normalisation ... + packing"
and "Backward of weight norm from wgrad slabs"), the shape lists the GPU tests run, and the per-element error bounds
they hold the kernels to.  Plain numpy from fp32 inputs; tests/test_cpu_weight_norm_ref.py pins every function here
against torch in float64 and against an fp32 emulation of the kernels' order, tests/test_gpu_weight_norm.py holds the
kernels to it.

    w = g * v / ||v||     v [O][I][J] (Conv1d / Linear: norm per o)    v [I][O][J] (ConvTranspose1d: norm per i)

Written from the header contract.  What IS restated from the kernels is the SUMMATION DEPTH the bounds count: 256
threads per row, a 64-lane wave reduction (6 additions), 4 wave partials (3 additions), the 8- / 4- / 1-unrolled slab
loops and the 4-accumulator loop of the [O][n_part] bias form.  Rows whose squared norm underflows or overflows in fp32
are out of scope (scale becomes Inf / 0 as torch._weight_norm's does in fp32); no family here builds one.

Bounds.  u = 2^-24, gamma(n) = n u / (1 - n u) (Higham, Accuracy and Stability, lemma 3.1): a sum in which every term
passes through at most n rounded operations, IN ANY ORDER of that depth, errs by at most gamma(n) * sum |term|.  Every
bound below is first order in u with its first-order terms written out; the second-order remainder is covered by the
common factor SLACK = 1 + 2^-6 (every gamma used is < 2^-15, so the remainder is < 2^-15 of the bound).  A fused
multiply-add rounds once where the count assumes twice: the count is an upper limit either way.

  scale     s^ = sum of len squares: one rounding per square, then a chain of ceil(len / 256) additions per thread, 6 in
            the wave, 3 over the waves: depth D = ceil(len/256) + 10, all terms >= 0, so |s^ - s| <= gamma(D) s.  sqrt
            halves a relative error; sqrtf and the division are each allowed 1 ulp (2u):
                |scale^ - scale| <= (gamma(D) / 2 + 4u) |scale|                                   (scale_rel)
  packed    w^ = fl(fl(g * scale^) * v): two more roundings:  |w^ - w| <= (scale_rel + 2u) |w|.  g NULL: w^ = v exactly.
  split     the decoded (hi, lo) of the fused split pack equal the host split of the fp32 value w^ the fp32 pack produced
            bit for bit (same fp32 expression, then conversions that round to nearest even): no bound.
  dW        partial k goes to accumulator k % 8 in the 8-loop, k % 4 in the 4-loop, 0 in the tail; accumulator 0 is the
            longest chain: n/8 + [n % 8 >= 4] + n % 4 additions, then 3 levels of the closing tree:
                |dW^ - dW| <= gamma(Dw) A,   A = sum_s |slab_s|                                     (E_dW)
  dot       sum of len rounded products dW^ v at the depth of `scale`:
                E_dot = gamma(D) sum (|dW| + E_dW) |v| + sum E_dW |v|
  dg        fl(dot^ * scale) (scale is an INPUT of the backward: exact):  E_dg = |scale| E_dot + u |dg|
  dv        c1^ = fl(g scale) (1 rounding), c2^ = fl(fl(c1^ scale) dg^) (3 roundings and dg's error), then
            fl(fl(c1^ dW^) - fl(c2^ v)) (3 roundings):
                E_dv = |c1| E_dW + 3u |c1| |dW| + 5u |c2| |v| + |g| scale^2 E_dg |v|
            -- in terms of |c1||dW| + |c2||v| and the propagated error of the dot, NOT of the (possibly cancelled) result.
            g NULL: dv^ = dW^:  E_dv = E_dW.
  dbias     [n_part][O]: depth ceil(n_part / 256) + 9;  [O][n_part]: the longest chain of any thread -- t1 trips of the
            4-accumulator loop, t2 <= 3 of the 1-accumulator loop into accumulator 0 (a thread whose first loop ends early
            takes up to three there: at n_part = 769 thread 0 has (1, 0), thread 1 (0, 3)), 2 levels of tree, + 9:
            gamma(Db) sum |part|.
  accumulate  out = fl(start + grad^): one more rounding:  E + u |start + grad|.
"""
import numpy as np

from tests.gemm_split_ref import F16_WEIGHT_SHIFT, split_bf16_pair, split_f16

U = 2.0 ** -24
SLACK = 1.0 + 2.0 ** -6
THREADS, WAVE_ADDS, BLOCK_ADDS = 256, 6, 3
SENTINEL = 0x7fc1                 # uint16 prefill of the split images: a NaN in bf16 and in fp16 alike
# cap on bound / |reference| the GENERIC family stays inside (tests/test_cpu_weight_norm_ref.py shows it from the
# reference alone): scale and packed values are relative by construction (every element); dW, dg, dv and dbias are
# sums with cancellation and are held at their MEDIAN element (a random sum of n terms loses about sqrt(n) against its
# absolute sum: sqrt(771) * (gamma(14) + sqrt(16) gamma(5)) for dg on the longest row, sqrt(1281) gamma(15) for dbias)
# -- about 920 u = 2^-14.2 and 650 u = 2^-14.7: the caps are twice that)
VACUITY_CAP = {"scale": 2.0 ** -20, "pack": 2.0 ** -20, "dW": 2.0 ** -17, "dg": 2.0 ** -13, "dv": 2.0 ** -14,
               "dbias": 2.0 ** -13}

# (O, I, J, glu_cg): the smallest shapes at which each index path of the pack kernels differs
NT_SHAPES = [(1, 1, 1, 0), (33, 31, 3, 0), (64, 40, 5, 0), (513, 80, 1, 0), (12, 36, 3, 6), (80, 40, 3, 40),
             (66, 33, 2, 33), (96, 257, 3, 0)]
# pad columns beyond round_up(O, 4) in the forward image, per shape: (64, 40, 5) gets four, so that a multiple-of-4 O
# has pads as well
NT_LDA_PAD = dict(zip(NT_SHAPES, [0, 0, 4, 0, 0, 0, 0, 0]))
T_SHAPES = [(40, 24, 2), (5, 3, 2), (33, 7, 3)]                    # (I, O, J)
N_SLABS = [1, 2, 3, 4, 5, 7, 8, 9, 12, 13, 16]
N_PART = [1, 255, 256, 257, 769, 1024, 1027, 1281]
# (I, O, J, transposed): rows of the launch against bias channels (the `o += nrows` loop)
ROWS_VS_O = [(5, 13, 2, True), (40, 24, 2, True), (7, 7, 3, True), (8, 24, 3, False)]
FAMILIES = ("generic", "wide", "cancel")


def cdiv(a, b):
    return -(-a // b)


def rup(a, b):
    return cdiv(a, b) * b


def gamma(n):
    return n * U / (1.0 - n * U)


def layout(O, I, J, glu_cg=0, transposed=False, lda_pad=0):
    """leading dimensions as ops.py lays the images out -> dict(lda, a_half, ldb, K, Kb, Jp): fwd image [Jp][K][lda], bwd
    image [Jp][Kb][ldb]; lda_pad more pad columns in the forward image of a layer without GLU."""
    if transposed:
        return dict(lda=rup(J * O, 4), a_half=0, ldb=rup(I, 4), K=I, Kb=J * O, Jp=1)
    if glu_cg > 0:
        a_half = rup(glu_cg, 4)
        lda = 2 * a_half
    else:
        a_half, lda = 0, rup(O, 4) + lda_pad
    return dict(lda=lda, a_half=a_half, ldb=rup(I, 4), K=I, Kb=O, Jp=J)


# ------------------------------------------------------------------------------------------------------------------
# forward: scale, weight, the two operand images
# ------------------------------------------------------------------------------------------------------------------
def _f64(a):
    a = np.asarray(a)
    assert a.dtype == np.float32, a.dtype
    return a.astype(np.float64)


def scale_ref(v, g):
    """[rows] = 1 / ||v[r]|| over every dim but 0; exactly 1 when g is None"""
    v = _f64(v)
    if g is None:
        return np.ones(v.shape[0])
    return 1.0 / np.sqrt((v * v).reshape(v.shape[0], -1).sum(1))


def weight_ref(v, g):
    """w = g * scale * v by rows of dim 0 (v itself when g is None)"""
    if g is None:
        return _f64(v)
    return (_f64(g).reshape(-1) * scale_ref(v, g))[:, None, None] * _f64(v)


def col_of(o, glu_cg, a_half):
    return o if (glu_cg == 0 or o < glu_cg) else a_half + (o - glu_cg)


def fwd_pack_of(w, lda, a_half=0, glu_cg=0, transposed=False, fill=np.nan):
    """-> (image [J'][K][lda] float64, owned mask).  Conv / Linear (w [O][I][J]): fwd[j][i][col(o)]; transposed
    (w [I][O][J]): fwd[0][i][j*O + o].  Positions no weight owns (pad columns) hold `fill`."""
    w = np.asarray(w, dtype=np.float64)
    if transposed:
        I, O, J = w.shape
        out = np.full((1, I, lda), fill)
        out[0, :, :J * O] = w.transpose(0, 2, 1).reshape(I, J * O)
    else:
        O, I, J = w.shape
        out = np.full((J, I, lda), fill)
        cols = np.array([col_of(o, glu_cg, a_half) for o in range(O)])
        out[:, :, cols] = w.transpose(2, 1, 0)
    own = np.zeros(out.shape, bool)
    if transposed:
        own[0, :, :J * O] = True
    else:
        own[:, :, cols] = True
    return out, own


def bwd_pack_of(w, ldb, transposed=False, fill=np.nan):
    """-> (image [J'][K'][ldb], owned mask).  Conv / Linear: bwd[J-1-j][o][i]; transposed: bwd[0][j*O + o][i]."""
    w = np.asarray(w, dtype=np.float64)
    if transposed:
        I, O, J = w.shape
        out = np.full((1, J * O, ldb), fill)
        out[0, :, :I] = w.transpose(2, 1, 0).reshape(J * O, I)
    else:
        O, I, J = w.shape
        out = np.full((J, O, ldb), fill)
        out[:, :, :I] = w[:, :, ::-1].transpose(2, 0, 1)
    own = np.zeros(out.shape, bool)
    own[:, :, :I] = True
    return out, own


def scale_rel_bound(length, g_given=True):
    if not g_given:
        return 0.0
    return (gamma(cdiv(length, THREADS) + 1 + WAVE_ADDS + BLOCK_ADDS) / 2 + 4 * U) * SLACK


def pack_rel_bound(length, g_given=True):
    """relative to |w|; 0 when g is None (1.0f * v is v)"""
    return (scale_rel_bound(length) + 2 * U * SLACK) if g_given else 0.0


# ------------------------------------------------------------------------------------------------------------------
# split images  [plane][j][k8][m][8], Kp = round_up(K, 32)
# ------------------------------------------------------------------------------------------------------------------
def split_words(n_j, K, lda):
    return 2 * n_j * rup(K, 32) * lda


def _to_bits(hi, lo, dtype):
    if dtype == "bf16":
        f = lambda a: (np.ascontiguousarray(a.astype(np.float32)).view(np.uint32) >> 16).astype(np.uint16)
    else:
        f = lambda a: np.ascontiguousarray(a.astype(np.float16)).view(np.uint16)
    return f(hi), f(lo)


def _from_bits(w, dtype):
    if dtype == "bf16":
        return (w.astype(np.uint32) << 16).view(np.float32).astype(np.float64)
    return np.ascontiguousarray(w).view(np.float16).astype(np.float64)


def host_split(x, dtype):
    """the expected (hi, lo) of fp32 values: bf16 pair of x, or fp16 pair of x * 2^DV3_F16_WEIGHT_SHIFT (a-units)"""
    return split_bf16_pair(x) if dtype == "bf16" else split_f16(x, F16_WEIGHT_SHIFT)


def encode_split(x, dtype):
    """fp32 [J][K][lda] -> uint16 image (flat): the host split of every value, rows K..Kp zero"""
    x = np.asarray(x, dtype=np.float32)
    n_j, K, lda = x.shape
    Kp = rup(K, 32)
    xp = np.zeros((n_j, Kp, lda), np.float32)
    xp[:, :K] = x
    planes = _to_bits(*host_split(xp, dtype), dtype)
    img = np.stack([p.reshape(n_j, Kp // 8, 8, lda).transpose(0, 1, 3, 2) for p in planes])
    return np.ascontiguousarray(img).reshape(-1)


def decode_split_words(img, n_j, K, lda):
    """uint16 image -> words [plane][j][Kp][lda]"""
    Kp = rup(K, 32)
    a = np.asarray(img, dtype=np.uint16).reshape(2, n_j, Kp // 8, lda, 8)
    return np.ascontiguousarray(a.transpose(0, 1, 2, 4, 3)).reshape(2, n_j, Kp, lda)


def decode_split(img, n_j, K, lda, dtype):
    """-> (hi, lo) float64 [j][Kp][lda] (fp16 form: in a-units, v * 2^8)"""
    w = decode_split_words(img, n_j, K, lda)
    return _from_bits(w[0], dtype), _from_bits(w[1], dtype)


# ------------------------------------------------------------------------------------------------------------------
# backward
# ------------------------------------------------------------------------------------------------------------------
def slab_buffer(slabs, rows_of_slabs, ldo, fill=np.nan, tail=64):
    """logical slabs [S][J'][M][I] fp32 -> (flat fp32 buffer, slab_ss, row stride) in one of the two layouts
    ops.weight_norm_bwd produces: slab-major [S][J'][M][ldo] (slab_ss = J' M ldo, row stride ldo) or rows of slabs
    [J'][M][S][ldo] (slab_ss = ldo, row stride S ldo).  Pad columns and `tail` floats after the last slab hold `fill`."""
    S, Jp, M, I = slabs.shape
    if rows_of_slabs:
        buf = np.full((Jp, M, S, ldo), fill, np.float32)
        buf[..., :I] = slabs.transpose(1, 2, 0, 3)
        ss, rs = ldo, S * ldo
    else:
        buf = np.full((S, Jp, M, ldo), fill, np.float32)
        buf[..., :I] = slabs
        ss, rs = Jp * M * ldo, ldo
    return np.concatenate([buf.reshape(-1), np.full(tail, fill, np.float32)]), ss, rs


def _to_param(x, O, I, J, transposed):
    """[J'][M][I] (one slab's indexing) -> the parameter's layout: [O][I][J], or [I][O][J] when transposed"""
    if transposed:
        return x[0].reshape(J, O, I).transpose(2, 1, 0)
    return x.transpose(1, 2, 0)


def dw_depth(n_slabs):
    return n_slabs // 8 + (1 if n_slabs % 8 >= 4 else 0) + n_slabs % 4 + 3


def dW_ref(slabs, O, I, J, transposed):
    """-> (dW, A = sum_s |slab_s|) in the parameter's layout, from logical slabs [S][J'][M][I]"""
    s = _f64(slabs)
    return _to_param(s.sum(0), O, I, J, transposed), _to_param(np.abs(s).sum(0), O, I, J, transposed)


def sum_depth(length):
    return cdiv(length, THREADS) + WAVE_ADDS + BLOCK_ADDS


def bwd_ref(slabs, v, g, scale, O, I, J, transposed):
    """-> dict(dW, dg, dv, E_dW, E_dg, E_dv) float64.  v, g, scale are the kernel's fp32 INPUTS (g None: plain weight:
    dv = dW, no dg)."""
    dW, A = dW_ref(slabs, O, I, J, transposed)
    v = _f64(v)
    E_dW = gamma(dw_depth(slabs.shape[0])) * A * SLACK
    if g is None:
        return dict(dW=dW, dv=dW, dg=None, E_dW=E_dW, E_dv=E_dW, E_dg=None)
    g, sc = _f64(g).reshape(-1, 1, 1), np.asarray(scale, dtype=np.float64).reshape(-1, 1, 1)
    rsum = lambda a: a.reshape(a.shape[0], -1).sum(1).reshape(-1, 1, 1)
    dot = rsum(dW * v)
    D = sum_depth(v[0].size) + 1
    E_dot = (gamma(D) * rsum((np.abs(dW) + E_dW) * np.abs(v)) + rsum(E_dW * np.abs(v))) * SLACK
    dg = dot * sc
    E_dg = (np.abs(sc) * E_dot + U * np.abs(dg)) * SLACK
    c1, c2 = g * sc, g * sc ** 3 * dot
    dv = c1 * dW - c2 * v
    E_dv = (np.abs(c1) * E_dW + 3 * U * np.abs(c1 * dW) + 5 * U * np.abs(c2 * v) +
            np.abs(g) * sc ** 2 * E_dg * np.abs(v)) * SLACK
    return dict(dW=dW, dg=dg.reshape(-1), dv=dv, E_dW=E_dW, E_dg=E_dg.reshape(-1), E_dv=E_dv,
                mag_dv=np.abs(c1 * dW) + np.abs(c2 * v))


def part_trips(n_part, tid=0):
    """thread `tid` of the [O][n_part] loop: (trips of the 4-accumulator loop, trips of the 1-accumulator loop)"""
    k, t1, t2 = tid, 0, 0
    while k + 768 < n_part:
        t1, k = t1 + 1, k + 1024
    while k < n_part:
        t2, k = t2 + 1, k + 256
    return t1, t2


def dbias_depth(n_part, part_t):
    if part_t:
        return max(sum(part_trips(n_part, t)) for t in range(THREADS)) + 2 + WAVE_ADDS + BLOCK_ADDS
    return sum_depth(n_part)


def dbias_ref(part, part_t):
    """part [n_part][O] (part_t: [O][n_part]) fp32 -> (dbias [O], bound)"""
    p = _f64(part)
    ax = 1 if part_t else 0
    return p.sum(ax), gamma(dbias_depth(p.shape[ax], part_t)) * np.abs(p).sum(ax) * SLACK


def accumulated(start, grad, E):
    """accumulate = 1: -> (start + grad, E + one rounding of the sum)"""
    tot = _f64(start) + grad
    return tot, (E + U * np.abs(tot)) * SLACK


# ------------------------------------------------------------------------------------------------------------------
# input families
# ------------------------------------------------------------------------------------------------------------------
def family(fam, rows, inner, seed):
    """-> (v [rows] + inner, g [rows]) fp32.  generic: normal v, g in [0.5, 1.5]; wide (and cancel): row norms spread
    over 2^+-20 with g spread likewise (independently), so a small row is not hidden by a large one."""
    rs = np.random.RandomState(seed)
    v = rs.standard_normal((rows,) + tuple(inner))
    g = rs.uniform(0.5, 1.5, rows)
    if fam != "generic":
        v = v * 2.0 ** rs.uniform(-20, 20, (rows,) + (1,) * len(inner))
        g = g * 2.0 ** rs.uniform(-20, 20, rows)
    return v.astype(np.float32), g.astype(np.float32)


def slabs_for(fam, v, n_slabs, O, I, J, transposed, seed, eps=2.0 ** -16):
    """logical slabs [S][J'][M][I] fp32.  generic / wide: normal (wide: per-row magnitudes spread over 2^+-20, the
    REVERSE of v's order being irrelevant: drawn independently).  cancel: dW[r] = alpha_r v[r] + eps |alpha_r v[r]| noise
    split over the slabs with random positive weights, so dv's two terms agree to about eps."""
    rs = np.random.RandomState(seed + 7)
    Jp, M = (1, J * O) if transposed else (J, O)
    v64 = v.astype(np.float64)
    rows = v.shape[0]

    def to_slab(x):                     # parameter layout -> [J'][M][I]
        if transposed:
            return x.transpose(2, 1, 0).reshape(1, J * O, I)
        return x.transpose(2, 0, 1)
    if fam == "cancel":
        alpha = rs.uniform(0.5, 2.0, (rows, 1, 1)) * rs.choice([-1.0, 1.0], (rows, 1, 1))
        dW = alpha * v64 * (1.0 + eps * rs.standard_normal(v.shape))
        wts = rs.uniform(0.5, 1.5, (n_slabs,) + (1, 1, 1))
        wts = wts / wts.sum(0)
        return (wts * to_slab(dW)[None]).astype(np.float32)
    s = rs.standard_normal((n_slabs, Jp, M, I))
    if fam == "wide":
        mag = 2.0 ** rs.uniform(-20, 20, (rows, 1, 1))
        s = s * to_slab(np.broadcast_to(mag, v.shape))[None]
    return s.astype(np.float32)

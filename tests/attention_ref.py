# coding: utf-8
"""float64 restatements of the four entry points of csrc/attention.hip (include/dv3hip.h, "Attention"), the case lists
tests/test_gpu_attention.py runs, and the per-element bounds it holds the kernels to.

The references restate AttentionLayer.forward's core (deepvoice3.py:143-171: padding mask, monotonic window, softmax,
dropout, context, the s * sqrt(1/s) scale) and the derivative of softmax, from the same fp32 inputs the kernels get.  What
IS restated from the kernels is said so: the summation depths the bounds count (64 lanes and a 6-level butterfly per row in
the unfused kernels; 8 threads and 3 levels per row, and K-sequential fp32 MFMA accumulation, in the fused one).
tests/test_cpu_attention_ref.py proves this file without a GPU: an fp32 emulation of each kernel's order of operations
stays inside every bound, and fifteen defect models each leave one.

U = 2^-24 is the fp32 unit roundoff; an operation documented to 1 ulp errs by <= 2U relative.  Three input families make
each rounding attributable:
  X  exact scores: everything on a 1/16 grid (scores on 2^-8), |s - max| <= 32: no product or partial sum of the score
     contraction rounds, what comes back is the softmax's own arithmetic;
  R  plain fp32 Gaussians: brings in the score bound depth * U * sum|q||k|;
  L  a ladder: keys 17, 87, 88.5, 89, 104 and 200 below the row maximum (expf crosses the subnormal range and underflows)
     and two keys within one fp32 ulp of each other at the maximum.
"""
import math

import numpy as np

from tests.decode_step_ref import attn_window, cdiv

U = 2.0 ** -24
TINY = 2.0 ** -126                  # a flushed subnormal costs this much, absolute
# expf is libm's (ocml), not v_exp_f32; taken as 1 ulp = 2U under the suite's convention.  NOBODY HAS MEASURED IT ON gfx950:
# the bounds below carry this as an assumption (1.0f / x and sqrtf are IEEE: U).
EXPF_REL = 2 * U
LDS_MAX = 65536
ROWS_PER_WG, LANES, ROW_THREADS = 4, 64, 8      # restated from csrc/attention.hip
F32 = np.float32


def f32(x):
    return np.asarray(x, dtype=np.float32)


def f64(x):
    return np.asarray(x, dtype=np.float64)


# ------------------------------------------------------------------------------------------------------------------
# references
# ------------------------------------------------------------------------------------------------------------------
def row_ranges(B, Tk, key_len, la, win_back, win_ahead):
    """[lo, hi) per ITEM: the window of deepvoice3.py:150-156 on all Tk keys (last_attended is one value for the whole
    batch), intersected with the item's own keys [0, key_len[b]).  An empty intersection is asserted out: the reference
    returns NaN there"""
    wlo, whi = attn_window(la, win_back, win_ahead, Tk)
    lo = np.full(B, wlo, dtype=np.int64)
    hi = np.array([min(whi, Tk if key_len is None else int(key_len[b])) for b in range(B)], dtype=np.int64)
    assert (0 <= lo).all() and (lo < hi).all() and (hi <= Tk).all(), "empty window"
    return lo, hi


def softmax_ref(s, key_len, la, win_back, win_ahead, keep, drop_scale, pd_scale):
    """s [B][Tq][Tk]; key_len [B] or None; la: the batch's last attended key or None (window off); keep [B][Tq][Tk] of
    0 / 1 or None; drop_scale, pd_scale: the fp32 factors, multiplied here in float64 (pd_scale: the product of the
    descriptor's and the device scalar's).  -> P, pd [B][Tq][Tk] (exactly 0.0 outside [lo, hi)), lo, hi [B * Tq]"""
    s = f64(s)
    B, Tq, Tk = s.shape
    lo, hi = row_ranges(B, Tk, key_len, la, win_back, win_ahead)
    P = np.zeros_like(s)
    for b in range(B):
        x = s[b, :, lo[b]:hi[b]]
        e = np.exp(x - x.max(axis=1, keepdims=True))
        P[b, :, lo[b]:hi[b]] = e / e.sum(axis=1, keepdims=True)
    pd = P * (float(drop_scale) * float(pd_scale))
    if keep is not None:
        pd = pd * f64(keep)
    return P, pd, np.repeat(lo, Tq), np.repeat(hi, Tq)


def softmax_bwd_ref(P, dpd, dp_direct, keep, scale):
    """dS = P * (d - sum(d * P)), d = dpd * keep * scale + dp_direct; dpd or dp_direct may be None.  -> dS, d, dot
    [rows][1], A = |dpd| keep scale + |dp_direct| (the magnitudes the bound needs)"""
    P = f64(P)
    d, A = np.zeros_like(P), np.zeros_like(P)
    if dpd is not None:
        t = f64(dpd) * float(scale) * (1.0 if keep is None else f64(keep))
        d, A = d + t, A + np.abs(t)
    if dp_direct is not None:
        d, A = d + f64(dp_direct), A + np.abs(f64(dp_direct))
    dot = (d * P).sum(axis=-1, keepdims=True)
    return P * (d - dot), d, dot, A


def attn_fwd_ref(q, k, vT, key_len, keep, drop_scale, pd_scale):
    """q [B][E][Tq], k [B][E][Tk], vT [B][Tk][E] fp32 -> dict: s, P, pd [B][Tq][Tk], ctx [B][E][Tq], lo, hi [B * Tq] and
    the absolute-value chains Ssc = sum_e |q||k| and Sctx = sum_n |v||pd|, absv = |vT|"""
    q, k, vT = f64(q), f64(k), f64(vT)
    s = np.einsum("bet,ben->btn", q, k)
    P, pd, lo, hi = softmax_ref(s, key_len, None, 0, 0, keep, drop_scale, pd_scale)
    return dict(s=s, P=P, pd=pd, lo=lo, hi=hi, ctx=np.einsum("bne,btn->bet", vT, pd),
                Ssc=np.einsum("bet,ben->btn", np.abs(q), np.abs(k)),
                Sctx=np.einsum("bne,btn->bet", np.abs(vT), np.abs(pd)), absv=np.abs(vT))


def argmax_ref(row):
    """the first maximum (torch.max, deepvoice3.py:445)"""
    return int(np.argmax(np.asarray(row)))


# ------------------------------------------------------------------------------------------------------------------
# bounds, from the kernels' own arithmetic
# ------------------------------------------------------------------------------------------------------------------
def sum_depth(lo, hi, fused):
    """roundings of a row sum.  Unfused: a lane adds ceil((hi - lo) / 64) terms serially, then 6 butterfly levels.
    Fused: 8 threads per row add ceil(hi / 8) terms serially, then 3 shuffle levels"""
    return cdiv(hi, ROW_THREADS) + 3 if fused else cdiv(hi - lo, LANES) + 6


def softmax_bound(s, P, lo, hi, fused=False, e_score=None):
    """|kernel - float64| per element of P.  s, P [B][Tq][Tk] float64, lo / hi per row, e_score: per-element bound on the
    error of the scores the softmax reads (the fused kernel's own contraction) or None (exact scores)"""
    s, P = f64(s), f64(P)
    B, Tq, Tk = s.shape
    ep = np.zeros_like(P)
    for r in range(B * Tq):
        b, t = divmod(r, Tq)
        l, h = int(lo[r]), int(hi[r])
        x = s[b, t, l:h] - s[b, t, l:h].max()
        p = P[b, t, l:h]
        es = np.zeros(h - l) if e_score is None else f64(e_score)[b, t, l:h]
        # the argument of expf: the score's own error, and one rounding of s - max (|s~ - max~| <= |x| + 2 max es)
        delta = es + U * (np.abs(x) + 2 * es.max())
        # p is shift invariant: an argument error delta_n moves the numerator by exp(+-delta_n) and the denominator by at
        # most exp(sum_m p_m delta_m) (Jensen), so log p moves by <= delta_n + sum_m p_m delta_m
        rel = np.expm1(delta + float(p @ delta))
        rel = rel + 2 * EXPF_REL                    # expf in the numerator, and in every (positive) term of the sum
        rel = rel + sum_depth(l, h, fused) * U      # the adds of the row sum: positive terms, so relative
        rel = rel + U                               # inv = 1.0f / sum, IEEE
        rel = rel + U                               # the product expf * inv
        # expf, or the product, lands in the subnormal range: 0.0 or within 2^-126 (inv <= 1: the maximum's term is 1)
        ep[b, t, l:h] = 1.001 * rel * p + TINY
    return ep


def pd_bound(ep, pd, factor):
    """pd = (P * drop_scale) * (pd_scale * pd_scale_dev): P's error times the factor (0 where dropped), three roundings
    (the scalar product, * drop_scale, * pd_scale) of the result, and a flushed product"""
    return 1.001 * (ep * factor + 3 * U * np.abs(pd)) + TINY * (np.asarray(factor) != 0)


def softmax_bwd_bound(P, dS, A, Tk):
    """|kernel - float64| per element of dS; absolute, because d - dot cancels.  A = |dpd| keep scale + |dp_direct|"""
    P, A = f64(P), f64(A)
    S = (A * P).sum(axis=-1, keepdims=True)
    e = 3 * U * A                                   # d: drop_scale * scale_dev, dpd * that, + dp_direct: <= 3U A_n
    e = e + (cdiv(Tk, LANES) + 6 + 4) * U * S       # dot: d's 3U and the product's U per term, then the row sum's depth
    e = e + U * (A + S)                             # the subtraction d - dot rounds once
    return 1.001 * P * e + U * np.abs(dS) + TINY    # the product with P rounds once; an underflowing product flushes


def mfma_depth(K):
    """the exact-fp32 MFMA (32x32x2) accumulates K terms in sequence, two per instruction: one rounding per term at most,
    and one more allowed for the product"""
    return 2 * cdiv(K, 2) + 1


def attn_fwd_bound(ref, E, Tk, factor, exact_scores):
    """-> ep, epd [B][Tq][Tk], ectx [B][E][Tq] for dv3_attn_fwd_f32.  factor [B][Tq][Tk] = keep * drop_scale * pd_scale"""
    es = None if exact_scores else 1.001 * mfma_depth(E) * U * ref["Ssc"]       # depth * U * sum|q||k|
    ep = softmax_bound(ref["s"], ref["P"], ref["lo"], ref["hi"], fused=True, e_score=es)
    epd = pd_bound(ep, ref["pd"], factor)
    ectx = np.einsum("bne,btn->bet", ref["absv"], epd)          # pd's error times |v|
    ectx = ectx + mfma_depth(Tk) * U * ref["Sctx"]              # depth * U * sum|v||pd|
    ectx = 1.001 * ectx + TINY * np.einsum("bne,btn->bet", ref["absv"], (ref["pd"] != 0) * 1.0)  # a subnormal pd flushed
    return ep, epd, ectx


# ------------------------------------------------------------------------------------------------------------------
# inputs
# ------------------------------------------------------------------------------------------------------------------
LADDER_TOP = 3.0
# offsets below the row maximum; None: one fp32 ulp below it; the last three are ordinary keys
LADDER = (0.0, None, 17.0, 87.0, 88.5, 89.0, 104.0, 200.0, 3.0, 1.0, 6.5)
LADDER_PLAIN = (8, 9, 10)           # slots a second channel may move (by < 1) without reaching the maximum


def ladder_values(idx):
    """fp32 scores LADDER_TOP - LADDER[idx % 11]"""
    top = F32(LADDER_TOP)
    tab = np.array([np.nextafter(top, F32(0)) if o is None else top - F32(o) for o in LADDER], dtype=np.float32)
    return tab[np.asarray(idx) % len(LADDER)]


def q16(rs, shape, scale):
    """values on a 1/16 grid with |x| < 2 (as _q16 of tests/test_gpu_step_kernels_at_scale.py)"""
    return np.clip(np.round(rs.standard_normal(shape) * scale * 16) / 16, -31 / 16, 31 / 16).astype(np.float32)


def draw_scores(rs, family, B, Tq, Tk):
    if family == "X":               # what a q16 contraction gives: multiples of 2^-8, |s| <= 15 so |s - max| <= 30
        return np.clip(np.round(rs.standard_normal((B, Tq, Tk)) * 4 * 256) / 256, -15, 15).astype(np.float32)
    if family == "R":
        return (rs.standard_normal((B, Tq, Tk)) * 3).astype(np.float32)
    assert family == "L"
    r = np.arange(B * Tq).reshape(B, Tq, 1)
    return ladder_values(np.arange(Tk).reshape(1, 1, Tk) + 3 * r)


def draw_mask(rs, rows, Tk, kind):
    """-> (uint32 words [rows][mask_rs] drawn directly, mask_rs, keep [rows][Tk] of 0 / 1) or (None, 0, None)"""
    if kind == "none":
        return None, 0, None
    rs_ = cdiv(Tk, 32) + (2 if kind == "wide" else 0)
    words = rs.randint(0, 2 ** 32, size=(rows, rs_), dtype=np.uint64).astype(np.uint32)
    n = np.arange(Tk)
    keep = (words[:, n >> 5] >> (n & 31).astype(np.uint32)) & np.uint32(1)
    return words, rs_, keep.astype(np.float64)


DROP_SCALE = F32(1.0 / (1.0 - 0.05))


def pd_scale_of(Tk):
    return F32(Tk * math.sqrt(1.0 / Tk))        # deepvoice3.py:170-171


# ------------------------------------------------------------------------------------------------------------------
# dv3_attn_softmax_f32
# ------------------------------------------------------------------------------------------------------------------
def sm_case(B, Tq, Tk, fam, la=None, win=(1, 3), key_len=None, mask="none", psd=None, pd=True):
    return dict(B=B, Tq=Tq, Tk=Tk, fam=fam, la=la, win=win, key_len=key_len, mask=mask, psd=psd, pd=pd)


# rows B * Tq in {1, 3, 4, 5, 9} (off the 4-row workgroup); Tk in {1, 2, 33, 63, 64, 65, 130}; window off / on with la in
# {0, 1, interior, Tk - 3, Tk - 1} so that each clip is taken and not taken; windows (1,3) (0,1) (2,5); the window inside
# key_len, beyond it, and with key_len == Tk; key_len in {1, 2, Tk}; mask absent / tight / wide stride; pd_scale_dev; no pd
SOFTMAX_CASES = [
    sm_case(1, 1, 1, "X"),
    sm_case(1, 1, 1, "R", la=0, key_len=[1], mask="tight", psd=0.75),
    sm_case(3, 1, 2, "X", key_len=[1, 2, 2], mask="wide"),
    sm_case(1, 3, 2, "R", la=1, win=(0, 1), key_len=[2], pd=False),
    sm_case(2, 2, 63, "X", la=0, win=(1, 3), mask="tight", psd=0.75),                 # low clip not taken, high taken
    sm_case(1, 3, 63, "R", la=1, win=(0, 1), mask="wide"),                            # one key: [1, 2)
    sm_case(1, 5, 63, "L", key_len=[63], mask="wide"),
    sm_case(3, 3, 64, "R", la=1, win=(2, 5), key_len=[64, 10, 4], mask="tight"),      # key_len == Tk, inside, whi > key_len
    sm_case(1, 4, 64, "X", la=30, win=(1, 3), psd=0.75, pd=False),                    # both clips taken
    sm_case(1, 1, 64, "X", la=63, win=(1, 3)),                                        # Tk - 1: high clip not taken
    sm_case(1, 5, 65, "R", la=62, win=(2, 5), mask="wide", psd=0.75),                 # Tk - 3
    sm_case(3, 3, 65, "L", la=64, win=(0, 1), key_len=[65, 65, 65], mask="tight"),    # the last key alone, third word
    sm_case(1, 1, 130, "L"),
    sm_case(2, 2, 130, "R", la=70, win=(1, 3), key_len=[130, 71], mask="wide", psd=0.75),   # whi = 73 > key_len = 71
    sm_case(3, 1, 130, "X", la=1, win=(1, 3), key_len=[1, 2, 130], mask="tight"),
    sm_case(1, 9, 130, "R", la=127, win=(1, 3)),                                      # Tk - 3 with win_ahead = 3: not clipped
    sm_case(1, 9, 130, "L", la=66, win=(2, 5), key_len=[130], mask="tight", psd=0.75),
    sm_case(1, 3, 33, "R", key_len=[33], mask="tight"),
    sm_case(1, 4, 33, "X", la=31, win=(2, 5), mask="wide", psd=0.75),                 # the window crosses a mask word
]


def sm_name(c):
    return "B%d Tq%d Tk%d %s la%s w%s kl%s mask:%s psd%s%s" % (c["B"], c["Tq"], c["Tk"], c["fam"], c["la"], c["win"],
                                                              c["key_len"], c["mask"], c["psd"], "" if c["pd"] else " nopd")


def sm_data(c, seed):
    """-> dict: s [B][Tq][Tk] fp32, words / mask_rs / keep, drop_scale, pd_scale, psd (fp32 or None)"""
    rs = np.random.RandomState(4000 + seed)
    B, Tq, Tk = c["B"], c["Tq"], c["Tk"]
    assert c["pd"] or c["mask"] == "none"
    words, mask_rs, keep = draw_mask(rs, B * Tq, Tk, c["mask"])
    return dict(s=draw_scores(rs, c["fam"], B, Tq, Tk), words=words, mask_rs=mask_rs,
                keep=None if keep is None else keep.reshape(B, Tq, Tk),
                drop_scale=DROP_SCALE if words is not None else F32(1.0), pd_scale=pd_scale_of(Tk),
                psd=None if c["psd"] is None else F32(c["psd"]))


def sm_ref(c, d):
    """-> P, pd, ep, epd, lo, hi"""
    ps = float(d["pd_scale"]) * (1.0 if d["psd"] is None else float(d["psd"]))
    P, pd, lo, hi = softmax_ref(d["s"], c["key_len"], c["la"], c["win"][0], c["win"][1], d["keep"], d["drop_scale"], ps)
    ep = softmax_bound(d["s"], P, lo, hi)
    factor = float(d["drop_scale"]) * ps * (1.0 if d["keep"] is None else d["keep"])
    return P, pd, ep, pd_bound(ep, pd, factor * np.ones_like(P)), lo, hi


# ------------------------------------------------------------------------------------------------------------------
# dv3_attn_softmax_bwd_f32
# ------------------------------------------------------------------------------------------------------------------
def bwd_case(B, Tq, Tk, fam, form, mask="none", sdev=None, la=None, win=(1, 3), key_len=None, onehot=None):
    """form: dpd / direct / both; P = fp32(softmax_ref) of family `fam` scores under (la, win, key_len): exact zeros outside
    the window; onehot: (row, key) of a row replaced by a one-hot P"""
    return dict(B=B, Tq=Tq, Tk=Tk, fam=fam, form=form, mask=mask, sdev=sdev, la=la, win=win, key_len=key_len, onehot=onehot)


SOFTMAX_BWD_CASES = [
    bwd_case(1, 1, 1, "X", "dpd"),                                                    # Tk = 1: P = [1], dS = 0
    bwd_case(3, 1, 2, "R", "direct"),
    bwd_case(1, 3, 33, "R", "dpd", mask="tight", sdev=0.75, key_len=[20]),
    bwd_case(2, 2, 63, "X", "both", mask="tight", sdev=0.75, la=30),
    bwd_case(1, 5, 64, "R", "dpd", mask="wide", key_len=[40]),
    bwd_case(3, 3, 65, "R", "both", mask="wide", sdev=0.75, la=62, win=(2, 5), onehot=(4, 64)),
    bwd_case(1, 4, 130, "X", "dpd", sdev=0.75, onehot=(1, 66)),
    bwd_case(1, 4, 130, "R", "direct", la=66, win=(2, 5)),
    bwd_case(1, 9, 130, "L", "both", mask="tight"),
]


def bwd_name(c):
    return "B%d Tq%d Tk%d %s %s mask:%s sdev%s la%s kl%s onehot%s" % (c["B"], c["Tq"], c["Tk"], c["fam"], c["form"], c["mask"],
                                                                     c["sdev"], c["la"], c["key_len"], c["onehot"])


def bwd_data(c, seed):
    rs = np.random.RandomState(5000 + seed)
    B, Tq, Tk = c["B"], c["Tq"], c["Tk"]
    P, _, lo, hi = softmax_ref(draw_scores(rs, c["fam"], B, Tq, Tk), c["key_len"], c["la"], c["win"][0], c["win"][1],
                               None, 1.0, 1.0)
    P = P.astype(np.float32).reshape(B * Tq, Tk)
    if c["onehot"] is not None:
        P[c["onehot"][0]] = 0
        P[c["onehot"][0], c["onehot"][1]] = 1
    draw = (lambda: q16(rs, (B * Tq, Tk), 1.0)) if c["fam"] == "X" else (lambda: rs.standard_normal((B * Tq, Tk)).astype(np.float32))
    dpd = draw() if c["form"] in ("dpd", "both") else None
    dpx = draw() if c["form"] in ("direct", "both") else None
    words, mask_rs, keep = draw_mask(rs, B * Tq, Tk, c["mask"])
    return dict(P=P, dpd=dpd, dpx=dpx, words=words, mask_rs=mask_rs, keep=keep, lo=lo, hi=hi,
                drop_scale=F32(float(DROP_SCALE) * float(pd_scale_of(Tk))) if words is not None else pd_scale_of(Tk),
                sdev=None if c["sdev"] is None else F32(c["sdev"]))


def bwd_ref(c, d):
    """-> dS, bound [rows][Tk]"""
    scale = float(d["drop_scale"]) * (1.0 if d["sdev"] is None else float(d["sdev"]))
    dS, _, _, A = softmax_bwd_ref(d["P"], d["dpd"], d["dpx"], d["keep"], scale)
    return dS, softmax_bwd_bound(d["P"], dS, A, c["Tk"])


# ------------------------------------------------------------------------------------------------------------------
# dv3_attn_fwd_f32
# ------------------------------------------------------------------------------------------------------------------
def fwd_case(B, E, Tq, Tk, fam, key_len=None, mask="none", psd=None):
    return dict(B=B, E=E, Tq=Tq, Tk=Tk, fam=fam, key_len=key_len, mask=mask, psd=psd)


# E in {1, 2, 31, 32, 33, 63, 64, 65, 97, 129}: every exit of the channel double-buffer, both parities of lhi; Tk in
# {1, 7, 8, 9, 31, 32, 33, 64, 65, 97, 129} and 511 (LDS = 64 KiB exactly); Tq in {1, 31, 32, 33, 65}; key_len in {1, 5, Tk}
FWD_CASES = [
    fwd_case(1, 1, 1, 1, "X"),
    fwd_case(2, 2, 31, 7, "R", key_len=[7, 5], mask="tight"),
    fwd_case(3, 31, 32, 8, "X", key_len=[8, 1, 5], mask="wide", psd=0.75),
    fwd_case(1, 32, 33, 9, "R", key_len=[5]),
    fwd_case(2, 33, 33, 65, "X", key_len=[65, 40], mask="tight", psd=0.75),
    fwd_case(1, 63, 1, 32, "R", key_len=[32], mask="wide"),
    fwd_case(2, 64, 33, 33, "L", key_len=[33, 20], mask="tight"),
    fwd_case(1, 65, 32, 64, "R", psd=0.75),
    fwd_case(2, 97, 31, 31, "X", key_len=[31, 5], mask="wide"),
    fwd_case(1, 129, 65, 97, "R", key_len=[97], mask="tight", psd=0.75),
    fwd_case(3, 33, 1, 129, "L", key_len=[129, 1, 100]),
    fwd_case(1, 32, 33, 511, "X", key_len=[511], mask="tight"),
]
CONSISTENCY_CASE = 4                # B = 2, E = 33, Tq = 33, Tk = 65, family X


def fwd_name(c):
    return "B%d E%d Tq%d Tk%d %s kl%s mask:%s psd%s" % (c["B"], c["E"], c["Tq"], c["Tk"], c["fam"], c["key_len"], c["mask"],
                                                       c["psd"])


def fwd_lds_bytes(Tk):
    return 32 * (Tk + 1) * 4


def fwd_data(c, seed):
    rs = np.random.RandomState(6000 + seed)
    B, E, Tq, Tk, fam = c["B"], c["E"], c["Tq"], c["Tk"], c["fam"]
    if fam == "X":
        sc = min(1.0, 1.5 / E ** 0.25)
        q, k, vT = q16(rs, (B, E, Tq), sc), q16(rs, (B, E, Tk), sc), q16(rs, (B, Tk, E), 1.0)
    elif fam == "R":
        q = (rs.standard_normal((B, E, Tq)) * (2.0 / math.sqrt(E))).astype(np.float32)
        k, vT = rs.standard_normal((B, E, Tk)).astype(np.float32), rs.standard_normal((B, Tk, E)).astype(np.float32)
    else:
        # channel 0 carries the ladder (q = 1: the score IS k), channel 1 moves the ordinary keys by |q k| <= 1/2, the
        # other channels of k are zero: every score is exact
        assert fam == "L" and E >= 2
        q, k, vT = q16(rs, (B, E, Tq), 1.0), np.zeros((B, E, Tk), dtype=np.float32), q16(rs, (B, Tk, E), 1.0)
        slot = (np.arange(Tk).reshape(1, Tk) + 3 * np.arange(B).reshape(B, 1)) % len(LADDER)
        q[:, 0, :] = 1.0
        q[:, 1, :] = rs.randint(-8, 9, size=(B, Tq)) / 16.0
        k[:, 0, :] = ladder_values(slot)
        k[:, 1, :] = np.where(np.isin(slot, LADDER_PLAIN), rs.randint(-16, 17, size=(B, Tk)) / 16.0, 0.0)
    words, mask_rs, keep = draw_mask(rs, B * Tq, Tk, c["mask"])
    return dict(q=q, k=k, vT=vT, words=words, mask_rs=mask_rs, keep=None if keep is None else keep.reshape(B, Tq, Tk),
                drop_scale=DROP_SCALE if words is not None else F32(1.0), pd_scale=pd_scale_of(Tk),
                psd=None if c["psd"] is None else F32(c["psd"]))


def fwd_ref(c, d):
    """-> ref dict of attn_fwd_ref, (ep, epd, ectx)"""
    ps = float(d["pd_scale"]) * (1.0 if d["psd"] is None else float(d["psd"]))
    ref = attn_fwd_ref(d["q"], d["k"], d["vT"], c["key_len"], d["keep"], d["drop_scale"], ps)
    factor = float(d["drop_scale"]) * ps * (np.ones_like(ref["P"]) if d["keep"] is None else d["keep"])
    return ref, attn_fwd_bound(ref, c["E"], c["Tk"], factor, exact_scores=c["fam"] in ("X", "L"))


# ------------------------------------------------------------------------------------------------------------------
# dv3_attn_argmax_i32
# ------------------------------------------------------------------------------------------------------------------
# (kind, Tk, parameter): tie: exact tie of the two named keys at the maximum (a lane tie, the same lane across strides, a
# tie across the butterfly): the first wins; equal / zero: all keys equal / 0.0 -> 0; random: a row of softmax_ref with
# one key lifted so that the gap between the two largest exceeds the bound on P
ARGMAX_CASES = [("tie", 63, (3, 4)), ("tie", 65, (3, 4)), ("tie", 200, (1, 66)), ("tie", 200, (2, 130)), ("tie", 64, (62, 63)),
                ("tie", 65, (62, 63)), ("equal", 1, None), ("equal", 64, None), ("equal", 65, None), ("zero", 1, None),
                ("zero", 200, None)] + [("random", Tk, j) for Tk in (1, 63, 64, 65, 200) for j in range(3)]


def argmax_row(case):
    """-> (fp32 row, expected index, fp64 gap between the two largest minus twice the bound on P; None where exact)"""
    kind, Tk, par = case
    if kind == "zero":
        return np.zeros(Tk, dtype=np.float32), 0, None
    if kind == "equal":
        return np.full(Tk, 1.0 / Tk, dtype=np.float32), 0, None
    rs = np.random.RandomState(7000 + Tk + (par if kind == "random" else 31 * par[0]))
    s = draw_scores(rs, "R", 1, 1, Tk)
    if kind == "random":
        s[0, 0, rs.randint(Tk)] = s.max() + F32(1.0)
        P, _, lo, hi = softmax_ref(s, None, None, 0, 0, None, 1.0, 1.0)
        ep = softmax_bound(s, P, lo, hi)
        top = np.sort(P[0, 0])[::-1]
        gap = float(top[0] - (top[1] if Tk > 1 else 0.0))
        return P[0, 0].astype(np.float32), argmax_ref(P[0, 0]), gap - 2 * float(ep.max())
    s[0, 0, par[0]] = s[0, 0, par[1]] = s.max() + F32(0.5)
    P, _, _, _ = softmax_ref(s, None, None, 0, 0, None, 1.0, 1.0)
    row = P[0, 0].astype(np.float32)
    assert row[par[0]] == row[par[1]] == row.max() and (row == row.max()).sum() == 2
    return row, par[0], None

# coding: utf-8
"""No GPU: proves tests/attention_ref.py, the references, bounds and case lists tests/test_gpu_attention.py holds
csrc/attention.hip to.

  * an fp32 numpy emulation of each kernel's order of operations (lane-strided serial partial sums, the xor butterfly, the
    8-thread rows and the K-sequential accumulation of the fused kernel; one rounding after every operation; expf modelled
    as correctly rounded, and again with every expf moved by +-1 ulp at random) stays inside every bound of every case;
  * fifteen defect models, each applied to that emulation, leave a bound (or write a nonzero outside a window) in at least
    one case of the list they concern -- the case is named in the output;
  * what the case lists claim: every axis value occurs, no window is empty, the family X cap, the argmax gaps, the LDS size.
"""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tests import attention_ref as A  # noqa: E402
from tests.decode_step_ref import attn_window  # noqa: E402

F32 = np.float32
XOR64 = [np.arange(64) ^ off for off in (32, 16, 8, 4, 2, 1)]
XOR8 = [np.arange(8) ^ off for off in (4, 2, 1)]


# ------------------------------------------------------------------------------------------------------------------
# the emulation
# ------------------------------------------------------------------------------------------------------------------
class Expf:
    """expf correctly rounded; with a RandomState, every result moved by one ulp up or down at random (a deterministic
    function of the call order, as the device's expf is one of its argument)"""

    def __init__(self, rs=None):
        self.rs = rs

    def __call__(self, x):
        with np.errstate(under="ignore"):
            e = np.exp(np.asarray(x, dtype=np.float64)).astype(np.float32)
        if self.rs is not None:
            up = self.rs.randint(0, 2, size=e.shape).astype(bool)
            e = np.where(up, np.nextafter(e, F32(np.inf)), np.nextafter(e, F32(-np.inf))).astype(np.float32)
            e = np.maximum(e, F32(0))
        return e


def _strided_sum(v, nthreads, xors):
    """thread j adds v[j], v[j + nthreads], ... serially from 0.0f, then the xor butterfly; -> the value every thread holds"""
    v = np.asarray(v, dtype=np.float32)
    n = -(-max(v.size, 1) // nthreads) * nthreads
    pad = np.zeros(n, dtype=np.float32)
    pad[:v.size] = v
    part = np.zeros(nthreads, dtype=np.float32)
    for chunk in pad.reshape(-1, nthreads):
        part = part + chunk
    for x in xors:
        part = part + part[x]
    assert (part == part[0]).all()
    return part[0]


def _keep_bit(words, mask_rs, row, n, defect, Tk, rows):
    if defect == "mask_tight_stride":           # word indexed with ceil(Tk / 32) instead of mask_rs
        return (int(words.reshape(-1)[row * (-(-Tk // 32)) + (n >> 5)]) >> (n & 31)) & 1
    if defect == "keep_neighbour_row":
        row = (row + 1) % rows
    return (int(words[row, n >> 5]) >> (n & 31)) & 1


def emu_softmax(c, d, expf, defect=None):
    """attn_softmax_kernel -> P, pd (None without pd) fp32 [B][Tq][Tk]"""
    B, Tq, Tk = c["B"], c["Tq"], c["Tk"]
    s = d["s"].reshape(B * Tq, Tk)
    P = np.zeros_like(s)
    pd = np.zeros_like(s) if c["pd"] else None
    pd_scale = d["pd_scale"] if d["psd"] is None or defect == "pd_scale_dev_ignored" else F32(d["pd_scale"] * d["psd"])
    for row in range(B * Tq):
        b = row // Tq
        lo, hi = 0, Tk
        if c["key_len"] is not None:
            hi = min(hi, c["key_len"][b])
        if c["la"] is not None:
            wlo, whi = c["la"] - c["win"][0], c["la"] + c["win"][1]
            if defect == "window_lo_off_by_one":
                wlo += 1
            if defect == "window_hi_off_by_one":
                whi += 1
            if defect == "key_len_ignored_with_window":
                hi = Tk
            if wlo > 0:
                lo = max(lo, wlo)
            if defect == "window_against_key_len":
                # `hi = whi < key_len ? whi : Tk`: the ahead clip is tested against key_len and stands in for it.  (Testing
                # against key_len and KEEPING the key_len clip gives min(key_len, whi) either way: not a defect)
                hi = whi if whi < hi else Tk
            elif whi < Tk:
                hi = min(hi, whi)
        if lo >= hi:                            # a defect emptied the row: no key is in range, every store is 0.0f
            continue
        x = s[row, lo:hi]
        mx = x.max()
        e = expf(x - mx)
        tot = _strided_sum(e[:64] if defect == "sum_drops_64" else e, 64, XOR64)
        inv = F32(1.0) / tot
        v = e * inv
        P[row, lo:hi] = v
        if pd is not None:
            dd = P[row].copy()
            if d["words"] is not None:
                kb = np.array([_keep_bit(d["words"], d["mask_rs"], row, n, defect, Tk, B * Tq) for n in range(Tk)])
                dd = np.where(kb == 1, dd * d["drop_scale"], F32(0))
            pd[row] = dd * pd_scale
        if defect == "pd_scale_on_P":
            P[row] = P[row] * pd_scale
    return P.reshape(B, Tq, Tk), None if pd is None else pd.reshape(B, Tq, Tk)


def emu_softmax_bwd(c, d, defect=None):
    """attn_softmax_bwd_kernel -> dS fp32 [rows][Tk]"""
    rows, Tk = d["P"].shape
    ds = d["drop_scale"] if d["sdev"] is None or defect == "scale_dev_ignored" else F32(d["drop_scale"] * d["sdev"])
    out = np.zeros_like(d["P"])
    for row in range(rows):
        p = d["P"][row]
        dd = np.zeros(Tk, dtype=np.float32)
        if d["dpd"] is not None:
            dd = d["dpd"][row] * ds
            if d["keep"] is not None:
                if defect == "drop_scale_on_dropped_only":      # the scale lands on the elements that are then zeroed
                    dd = d["dpd"][row].copy()
                dd = np.where(d["keep"][row] == 1, dd, F32(0)).astype(np.float32)
        ddot = dd
        if d["dpx"] is not None:
            dd = dd + d["dpx"][row]
            if defect != "direct_left_out_of_dot":
                ddot = dd
        dot = _strided_sum(ddot * p, 64, XOR64)
        out[row] = p * (dd - dot)
    return out


def emu_fwd(c, d, expf, defect=None):
    """attn_fwd_kernel -> P, pd [B][Tq][Tk], ctx [B][E][Tq] fp32"""
    B, E, Tq, Tk = c["B"], c["E"], c["Tq"], c["Tk"]
    q, k, vT = d["q"], d["k"], d["vT"]
    nE = E
    if defect == "odd_E_last_channel_dropped" and E % 2:
        nE = E - 1
    if defect == "second_channel_batch_skipped" and 32 < E <= 64:
        nE = 32
    s = np.zeros((B, Tq, Tk), dtype=np.float32)
    for e in range(nE):                         # the MFMA's K-sequential accumulation, one rounding per product and add
        s = s + q[:, e, :, None] * k[:, e, None, :]
    if defect == "c_tile_transposed":           # sc[i][n0 + j] takes the tile's element [j][i] (rows and keys clamped)
        t, n = np.arange(Tq), np.arange(Tk)
        ti, nj = t % 32, n % 32
        src_t = np.minimum((t - ti)[:, None] + nj[None, :], Tq - 1)
        src_n = np.minimum((n - nj)[None, :] + ti[:, None], Tk - 1)
        s = s[:, src_t, src_n]
    P = np.zeros_like(s)
    pd = np.zeros_like(s)
    pd_scale = d["pd_scale"] if d["psd"] is None or defect == "pd_scale_dev_ignored" else F32(d["pd_scale"] * d["psd"])
    for b in range(B):
        hi = Tk if c["key_len"] is None else min(Tk, c["key_len"][b])
        for t in range(Tq):
            x = s[b, t, :hi]
            ex = expf(x - x.max())
            tot = _strided_sum(ex[:8] if defect == "sum_drops_8" else ex, 8, XOR8)
            P[b, t, :hi] = ex * (F32(1.0) / tot)
        dd = P[b]
        if d["words"] is not None:
            kp = d["keep"][b]
            if defect == "keep_neighbour_row":
                kp = d["keep"].reshape(B * Tq, Tk)[(np.arange(Tq) + b * Tq + 1) % (B * Tq)]
            dd = np.where(kp == 1, dd * d["drop_scale"], F32(0)).astype(np.float32)
        pd[b] = dd * pd_scale
        if defect == "pd_scale_on_P":
            P[b] = P[b] * pd_scale
    nK = Tk
    if defect == "second_key_batch_skipped" and 32 < Tk <= 64:
        nK = 32
    ctx = np.zeros((B, E, Tq), dtype=np.float32)
    for n in range(nK):
        ctx = ctx + vT[:, n, :, None] * pd[:, None, :, n]
    return P, pd, ctx


def emu_argmax(row, defect=None):
    """attn_argmax_kernel"""
    best = np.full(64, -np.inf, dtype=np.float32)
    bi = np.full(64, 0x7fffffff, dtype=np.int64)
    for n, v in enumerate(row):
        lane = n % 64
        if v > best[lane] or (defect == "last_maximum" and v >= best[lane]):
            best[lane], bi[lane] = v, n
    for x in XOR64:
        ov, oi = best[x], bi[x]
        if defect == "last_maximum":
            take = (ov > best) | ((ov == best) & (oi > bi))
        else:
            take = (ov > best) | ((ov == best) & (oi < bi))
        best, bi = np.where(take, ov, best), np.where(take, oi, bi)
    return int(bi[0])


# ------------------------------------------------------------------------------------------------------------------
# checks of one case: -> (worst ratio to the bound, or inf where an exact-zero / one-hot claim breaks)
# ------------------------------------------------------------------------------------------------------------------
def _ratio(got, want, bound):
    err = np.abs(np.asarray(got, dtype=np.float64) - want)
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(err == 0, 0.0, err / bound)
    return float(np.nan_to_num(r, nan=np.inf).max()) if r.size else 0.0


def _outside_zero(got, lo, hi):
    g = np.asarray(got).reshape(len(lo), -1)
    return all(not g[r, :lo[r]].any() and not g[r, hi[r]:].any() for r in range(len(lo)))


_REFS = {}


def _case(kind, i):
    """-> (case, its data, its reference and bounds), computed once"""
    if (kind, i) not in _REFS:
        cases, data, ref = {"sm": (A.SOFTMAX_CASES, A.sm_data, A.sm_ref), "bwd": (A.SOFTMAX_BWD_CASES, A.bwd_data, A.bwd_ref),
                            "fwd": (A.FWD_CASES, A.fwd_data, A.fwd_ref)}[kind]
        d = data(cases[i], i)
        _REFS[kind, i] = (cases[i], d, ref(cases[i], d))
    return _REFS[kind, i]


def check_softmax(i, expf, defect=None):
    c, d, (P, pd, ep, epd, lo, hi) = _case("sm", i)
    gP, gpd = emu_softmax(c, d, expf, defect)
    r = _ratio(gP, P, ep)
    ok = _outside_zero(gP, lo, hi)
    if gpd is not None:
        r = max(r, _ratio(gpd, pd, epd))
        ok = ok and _outside_zero(gpd, lo, hi) and not gpd[pd == 0].any()
    return r if ok else np.inf


def check_bwd(i, defect=None):
    c, d, (dS, bound) = _case("bwd", i)
    g = emu_softmax_bwd(c, d, defect)
    ok = _outside_zero(g, d["lo"], d["hi"]) if c["onehot"] is None else not g[c["onehot"][0]].any()
    return _ratio(g, dS, bound) if ok else np.inf


def check_fwd(i, expf, defect=None):
    c, d, (ref, (ep, epd, ectx)) = _case("fwd", i)
    P, pd, ctx = emu_fwd(c, d, expf, defect)
    ok = _outside_zero(P, ref["lo"], ref["hi"]) and not pd[ref["pd"] == 0].any()
    r = max(_ratio(P, ref["P"], ep), _ratio(pd, ref["pd"], epd), _ratio(ctx, ref["ctx"], ectx))
    return r if ok else np.inf


# ------------------------------------------------------------------------------------------------------------------
# faithful emulation inside every bound
# ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("perturbed", [False, True])
def test_emulation_stays_inside_every_bound(perturbed):
    def expf():
        return Expf(np.random.RandomState(99) if perturbed else None)
    tag = "expf +-1 ulp" if perturbed else "expf correctly rounded"
    worst = {"softmax": max(check_softmax(i, expf()) for i in range(len(A.SOFTMAX_CASES))),
             "softmax_bwd": max(check_bwd(i) for i in range(len(A.SOFTMAX_BWD_CASES))),
             "fwd": max(check_fwd(i, expf()) for i in range(len(A.FWD_CASES)))}
    for what, r in worst.items():
        print("worst-ratio emulation %-12s (%s) %.4g" % (what, tag, r))
        assert r < 1.0, (what, r)
    for case in A.ARGMAX_CASES:
        row, want, _ = A.argmax_row(case)
        assert emu_argmax(row) == want == A.argmax_ref(row), case


# ------------------------------------------------------------------------------------------------------------------
# defect models
# ------------------------------------------------------------------------------------------------------------------
def _first_broken(check, n):
    for i in range(n):
        r = check(i)
        if not r < 1.0:
            return i, r
    return None, 0.0


SOFTMAX_DEFECTS = ["window_lo_off_by_one", "window_hi_off_by_one", "key_len_ignored_with_window", "window_against_key_len",
                   "mask_tight_stride", "keep_neighbour_row", "pd_scale_on_P", "pd_scale_dev_ignored", "sum_drops_64"]
BWD_DEFECTS = ["direct_left_out_of_dot", "drop_scale_on_dropped_only", "scale_dev_ignored"]
FWD_DEFECTS = ["odd_E_last_channel_dropped", "second_channel_batch_skipped", "second_key_batch_skipped", "c_tile_transposed",
               "sum_drops_8", "keep_neighbour_row", "pd_scale_on_P", "pd_scale_dev_ignored"]


@pytest.mark.parametrize("defect", SOFTMAX_DEFECTS)
def test_softmax_defect_breaks_a_case(defect):
    i, r = _first_broken(lambda i: check_softmax(i, Expf(), defect), len(A.SOFTMAX_CASES))
    assert i is not None, "no SOFTMAX_CASES entry notices " + defect
    print("defect %-30s caught by SOFTMAX_CASES[%d] %s (ratio %.3g)" % (defect, i, A.sm_name(A.SOFTMAX_CASES[i]), r))


@pytest.mark.parametrize("defect", BWD_DEFECTS)
def test_softmax_bwd_defect_breaks_a_case(defect):
    i, r = _first_broken(lambda i: check_bwd(i, defect), len(A.SOFTMAX_BWD_CASES))
    assert i is not None, "no SOFTMAX_BWD_CASES entry notices " + defect
    print("defect %-30s caught by SOFTMAX_BWD_CASES[%d] %s (ratio %.3g)" % (defect, i, A.bwd_name(A.SOFTMAX_BWD_CASES[i]), r))


@pytest.mark.parametrize("defect", FWD_DEFECTS)
def test_fwd_defect_breaks_a_case(defect):
    i, r = _first_broken(lambda i: check_fwd(i, Expf(), defect), len(A.FWD_CASES))
    assert i is not None, "no FWD_CASES entry notices " + defect
    print("defect %-30s caught by FWD_CASES[%d] %s (ratio %.3g)" % (defect, i, A.fwd_name(A.FWD_CASES[i]), r))


def test_argmax_defect_breaks_a_case():
    hit = [c for c in A.ARGMAX_CASES if emu_argmax(A.argmax_row(c)[0], "last_maximum") != A.argmax_row(c)[1]]
    assert hit, "no ARGMAX_CASES entry notices a last-maximum argmax"
    assert {c[2] for c in hit if c[0] == "tie"} == {(3, 4), (1, 66), (2, 130), (62, 63)} and ("equal", 64, None) in hit
    print("defect %-30s caught by ARGMAX_CASES %s" % ("last_maximum", hit))


# ------------------------------------------------------------------------------------------------------------------
# what the case lists claim
# ------------------------------------------------------------------------------------------------------------------
def test_the_reference_is_the_layer_core_in_float64():
    """softmax_ref against the reference's own sequence (deepvoice3.py:145-165) spelled with -inf fills, and
    softmax_bwd_ref against a central difference of it"""
    rs = np.random.RandomState(3)
    s = rs.standard_normal((2, 3, 11))
    x = s.copy()
    x[1, :, 7:] = -np.inf                       # :146-148
    x[:, :, :5 - 1] = -np.inf                   # :151-153, last_attended = 5
    x[:, :, 5 + 3:] = -np.inf                   # :154-156
    e = np.exp(x - x.max(axis=2, keepdims=True))
    P, pd, lo, hi = A.softmax_ref(s, [11, 7], 5, 1, 3, None, 1.0, 2.0)
    assert np.allclose(P, e / e.sum(axis=2, keepdims=True), rtol=1e-14, atol=0) and np.array_equal(pd, 2.0 * P)
    assert lo.tolist() == [4] * 6 and hi.tolist() == [8, 8, 8, 7, 7, 7]
    with pytest.raises(AssertionError):
        A.softmax_ref(s, [11, 4], 5, 1, 3, None, 1.0, 1.0)      # item 1: keys [0, 4) and window [4, 8): empty
    g = rs.standard_normal((2, 3, 11))
    dS = A.softmax_bwd_ref(P, g, None, None, 1.0)[0]
    h = 1e-6
    for idx in ((0, 1, 5), (1, 2, 6), (0, 0, 4)):
        sp, sm = s.copy(), s.copy()
        sp[idx] += h
        sm[idx] -= h
        num = ((A.softmax_ref(sp, [11, 7], 5, 1, 3, None, 1.0, 1.0)[0] - A.softmax_ref(sm, [11, 7], 5, 1, 3, None, 1.0, 1.0)[0])
               * g).sum() / (2 * h)
        assert abs(num - dS[idx]) < 1e-8


def test_softmax_cases_cover_what_they_claim():
    C = A.SOFTMAX_CASES
    assert {c["B"] * c["Tq"] for c in C} == {1, 3, 4, 5, 9} and max(c["B"] for c in C) <= 3
    assert {c["Tk"] for c in C} >= {1, 2, 33, 63, 64, 65, 130}
    assert {c["win"] for c in C if c["la"] is not None} == {(1, 3), (0, 1), (2, 5)}
    assert {c["mask"] for c in C} == {"none", "tight", "wide"} and {c["psd"] for c in C} == {None, 0.75}
    assert any(not c["pd"] for c in C) and any(c["la"] is None for c in C)
    assert {c["fam"] for c in C} == {"X", "R", "L"}
    las, clips, cross, kls = set(), set(), set(), set()
    for i, c in enumerate(C):
        Tk = c["Tk"]
        A.sm_ref(c, A.sm_data(c, i))                # asserts a non-empty [lo, hi) in every row
        for kl in c["key_len"] or ():
            kls.add("Tk" if kl == Tk else kl)
        if c["la"] is None:
            continue
        la, (wb, wa) = c["la"], c["win"]
        assert 0 <= la < Tk
        las.add("Tk-1" if la == Tk - 1 and Tk > 3 else "Tk-3" if la == Tk - 3 and Tk > 3 else la if la < 2 else "interior")
        clips.add(("lo", la - wb > 0))
        clips.add(("hi", la + wa < Tk))
        wlo, whi = attn_window(la, wb, wa, Tk)
        for kl in c["key_len"] or ():
            cross.add("== Tk" if kl == Tk else "inside" if whi < kl else "beyond" if whi > kl else "touching")
    assert las >= {0, 1, "interior", "Tk-3", "Tk-1"}, las
    assert clips == {("lo", True), ("lo", False), ("hi", True), ("hi", False)}
    assert cross >= {"== Tk", "inside", "beyond"}, cross
    assert kls >= {1, 2, "Tk"}, kls
    # a mask over a word boundary, with the wide stride, on more than one row
    assert any(c["mask"] == "wide" and c["Tk"] in (33, 65) and c["B"] * c["Tq"] > 1 for c in C)


def test_softmax_bwd_cases_cover_what_they_claim():
    C = A.SOFTMAX_BWD_CASES
    assert {c["B"] * c["Tq"] for c in C} >= {1, 3, 4, 5, 9} and max(c["B"] for c in C) <= 3
    assert {c["Tk"] for c in C} >= {1, 2, 63, 64, 65, 130}
    assert {c["form"] for c in C} == {"dpd", "direct", "both"}
    assert {c["mask"] for c in C} == {"none", "tight", "wide"} and {c["sdev"] for c in C} == {None, 0.75}
    assert any(c["onehot"] is not None for c in C)
    zeros = 0
    for i, c in enumerate(C):
        d = A.bwd_data(c, i)
        assert d["P"].dtype == np.float32
        zeros += int(any(d["lo"][r] > 0 or d["hi"][r] < c["Tk"] for r in range(len(d["lo"]))))
        if c["onehot"] is not None:
            row = d["P"][c["onehot"][0]]
            assert row.sum() == 1 and row[c["onehot"][1]] == 1
            assert not A.bwd_ref(c, d)[0][c["onehot"][0]].any()
    assert zeros >= 3


def test_fwd_cases_cover_what_they_claim():
    C = A.FWD_CASES
    assert {c["E"] for c in C} >= {1, 2, 31, 32, 33, 63, 64, 65, 97, 129}
    assert {c["Tk"] for c in C} >= {1, 7, 8, 9, 31, 32, 33, 64, 65, 97, 129, 511}
    assert {c["Tq"] for c in C} >= {1, 31, 32, 33, 65} and max(c["B"] for c in C) <= 3
    assert any((c["B"], c["E"], c["Tq"], c["Tk"]) == (1, 32, 33, 511) for c in C)
    kls = {("Tk" if kl == c["Tk"] else kl) for c in C for kl in (c["key_len"] or ())}
    assert kls >= {1, 5, "Tk"} and any(c["key_len"] is None for c in C)
    assert {c["mask"] for c in C} == {"none", "tight", "wide"} and {c["psd"] for c in C} == {None, 0.75}
    assert {c["fam"] for c in C} == {"X", "R", "L"}
    for c in C:
        assert A.fwd_lds_bytes(c["Tk"]) <= A.LDS_MAX, c
    assert A.fwd_lds_bytes(511) == A.LDS_MAX and A.fwd_lds_bytes(512) > A.LDS_MAX
    c = C[A.CONSISTENCY_CASE]
    assert (c["B"], c["E"], c["Tq"], c["Tk"], c["fam"]) == (2, 33, 33, 65, "X")


def _x_cap(s, P, ep, lo, hi, what):
    s, P = np.asarray(s, dtype=np.float64), np.asarray(P)
    B, Tq, Tk = s.shape
    for r in range(B * Tq):
        b, t = divmod(r, Tq)
        x = s[b, t, lo[r]:hi[r]]
        assert (x.max() - x).max() <= 32, what
    big = P > 1e-3
    assert (ep[big] / P[big]).max() <= 2.0 ** -16, (what, float((ep[big] / P[big]).max()))


def test_family_x_scores_are_exact_and_capped():
    """|s - max| <= 32 in every row and the relative bound on P above 1e-3 is below 2^-16 (Tk <= 511); the fp32
    contraction of the fused kernel's family X and L inputs is exact in any order"""
    for i, c in enumerate(A.SOFTMAX_CASES):
        if c["fam"] == "X":
            d = A.sm_data(c, i)
            P, pd, ep, epd, lo, hi = A.sm_ref(c, d)
            assert np.array_equal(d["s"] * 256, np.round(d["s"] * 256))
            _x_cap(d["s"], P, ep, lo, hi, A.sm_name(c))
    for i, c in enumerate(A.FWD_CASES):
        if c["fam"] == "R":
            continue
        d = A.fwd_data(c, i)
        ref, (ep, epd, ectx) = A.fwd_ref(c, d)
        s32 = np.zeros(ref["s"].shape, dtype=np.float32)
        for e in range(c["E"]):
            s32 = s32 + d["q"][:, e, :, None] * d["k"][:, e, None, :]
        assert np.array_equal(s32.astype(np.float64), ref["s"]), A.fwd_name(c)
        if c["fam"] == "X":
            _x_cap(ref["s"], ref["P"], ep, ref["lo"], ref["hi"], A.fwd_name(c))


def test_ladder_rows_hold_what_they_claim():
    """rows of family L: two keys within one fp32 ulp at the maximum, and keys 17 .. 200 below it whose probabilities
    cross 2^-126 (some normal, some subnormal, some 0 in fp32)"""
    c = A.SOFTMAX_CASES[[A.sm_name(x) for x in A.SOFTMAX_CASES].index(A.sm_name(A.sm_case(1, 1, 130, "L")))]
    d = A.sm_data(c, 0)
    row = np.sort(d["s"][0, 0].astype(np.float64))[::-1]
    assert row[0] == A.LADDER_TOP and 0 < row[0] - row[row < row[0]][0] <= 2.0 ** -22
    assert {17.0, 87.0, 88.5, 89.0, 104.0, 200.0} <= set((row[0] - row).tolist())
    P = A.sm_ref(c, d)[0][0, 0]
    assert ((P > 0) & (P < A.TINY)).any() and (P.astype(np.float32) == 0).any() and (P > 0.01).sum() >= 2
    cf = [x for x in A.FWD_CASES if x["fam"] == "L"][0]
    ref = A.fwd_ref(cf, A.fwd_data(cf, A.FWD_CASES.index(cf)))[0]
    assert ((ref["P"] > 0) & (ref["P"] < A.TINY)).any()


def test_argmax_cases_cover_what_they_claim():
    C = A.ARGMAX_CASES
    assert {c[1] for c in C} == {1, 63, 64, 65, 200}
    assert {c[2] for c in C if c[0] == "tie"} == {(3, 4), (1, 66), (2, 130), (62, 63)}
    assert {c[0] for c in C} == {"tie", "equal", "zero", "random"}
    for c in C:
        row, want, margin = A.argmax_row(c)
        assert row.dtype == np.float32 and row.shape == (c[1],) and want == A.argmax_ref(row)
        if c[0] == "random":
            assert margin > 0, c                     # every random row clears its gap: none is skipped
        if c[0] == "tie":
            assert want == c[2][0]

# coding: utf-8
"""float64 restatement of csrc/speaker_bias.hip's header comment (include/dv3hip.h: dv3_speaker_bias_fwd_f32 /
_bwd_f32), the input families the tests run and the per-element error bounds they hold the kernels to.  Plain numpy
from fp32 inputs, no import of the package; tests/test_cpu_speaker_bias_ref.py pins it against an fp32 emulation of the
kernels' dataflow and shows what its checks catch, tests/test_gpu_speaker_bias_elementwise.py holds the kernels to it.

    forward   out_l[b, c, t] = softsign(b_l[c] + sum_e W_l[c, e] emb[b, e, t]),   W_l = g_l v_l / ||v_l|| by rows (v_l: g NULL)
    backward  gp = dout_l (1 - |out_l|)^2;  db_l = sum_{b,t} gp;  dW_l = sum_{b,t} gp (x) emb;  d emb = sum_l W_l^T gp;
              dg_l = dW_l . v_l / ||v_l||,  dv_l = g_l / ||v_l|| (dW_l - v_l (dW_l . v_l) / ||v_l||^2)   (g NULL: dv = dW)

The backward takes `outs` as an INPUT -- the fp32 activations the kernel is handed -- so the cancellation of 1 - |out|
belongs to the forward and does not enter the backward's bounds: fl(1 - |y|) errs by u RELATIVE to 1 - |y|.

Bounds.  u = 2^-24, gamma(n) = n u / (1 - n u), first order with the common factor SLACK, as in weight_norm_ref.py.  A
fused multiply-add rounds once where the count assumes twice: the count is an upper limit either way.  What IS restated
from the kernels is the summation DEPTH (how many rounded operations a term passes through), never a measured error.

  W         W^ = fl(v * fl(g / sqrtf(ss^))), ss^ = the 16-term chain of v^2 (zero pads add exactly; all terms >= 0):
              ss^: 16 roundings per term at most (product + chain)   gamma(16), halved by the square root     8 u
              sqrtf: not assumed correctly rounded (csrc/Makefile sets no flag about it)                         2 u
              the division: likewise                                                                               2 u
              the product v * s                                                                                    1 u
            W_REL = 13 u of |W|;  g NULL: W^ = v exactly (1.0f * v), W_REL = 0.
  forward   z^: four chains of four products (product 1 + 3 additions), (p0 + p1) + (p2 + p3) (2), the bias add (1): a
            term passes through 7 roundings at most, and carries W's error:
                E_z = (W_REL + 7 u) (|b| + sum |W| |e|)
            out^ = fl(z^ * rcp(fl(1 + |z^|))): the addition 1 u, v_rcp_f32 1 ulp = 2 u, the product 1 u; softsign's slope
            is 1 / (1 + |z|)^2:
                E_out = E_z / (1 + |z|)^2 + 4 u |out|
  gp        fl(1 - |y|) (1 u of its value, doubled by the square), the square (1 u), the product with dout (1 u):
                |gp^ - gp| <= 4 u |gp|         (a c8 gradient: the same two products in the same association)
  dW, db    per workgroup (256 frames of one batch item) and wave (64 frames): a matrix-core sum whose internal order is
            taken as UNKNOWN: a term passes its product rounding (1) and at most one addition per valid frame of the wave
            (min(64, T); frames >= T hold exact zeros, and x + 0 is exact); then the four-wave sum (at most 3, fewer when
            T < 193), the serial sum of ceil(n_blocks / 4) partials per lane group and the 2 shuffle additions
            (fewer when n_blocks < 4), with gp's 4 u:
                D_sum = 4 + 1 + min(64, T) + min(3, ceil(min(T, 256) / 64) - 1) + ceil(n_blocks / 4) + min(2, ceil(log2(min(4, n_blocks))))
                E_dW = gamma(D_sum) sum |gp| |e|,     E_db = gamma(D_sum) sum |gp|
  d emb     accumulators live across the row tiles: one product (1) and at most C_l additions per layer (rows past C_l
            are exact zeros), W's and gp's errors, then the sum over L layers (L additions at most):
                E_de = sum_l gamma(W_REL_l / u + 4 + 1 + C_l + L) sum_c |W_l| |gp_l|
  finish    vv^ = sum v^2 and dot^ = sum dW^ v through a 16-lane shuffle tree: product 1 + 4 additions:
                E_dot = sum E_dW |v| + 5 u sum |dW| |v|
            rn^ = fl(1 / sqrtf(vv^)): 2.5 u (vv's 5 u halved) + 2 u (sqrtf) + 2 u (division) = 6.5 u
            dg^ = fl(dot^ rn^):                    E_dg = (E_dot + 7.5 u |dot|) / ||v||
            dv^ = fl(fl(g rn^) * fl(dW^ - fl(fl(v dot^) / vv^))),  q = v dot / ||v||^2,  c1 = g / ||v||:
              q^: product 1 u, division 2 u, vv 5 u = 8 u of |q|, and dot's error |v| E_dot / ||v||^2
              the subtraction 1 u of its result (<= |dW| + |q|); c1^: 6.5 u + 1 u; the last product 1 u
                E_dv = |c1| (E_dW + |v| E_dot / ||v||^2) + u |c1| (9.5 |dW| + 17.5 |q|)
            -- in terms of |dW| + |q| and the propagated error of the dot, NOT of the (possibly cancelled) difference.
  +=        out = fl(start + grad^): half an ulp of the total more (weight_norm_ref.accumulated).

EXACT families.  Inputs on dyadic grids such that every product and every partial sum, in ANY order, is an integer
number of grid units below 2^24: fp32 then computes every sum without rounding and the kernel must return the float64
value bit for bit.  The arithmetic is stated beside each builder, and assert_exact_premise() checks on the CPU that the
float64 result survives a round trip through fp32, so the premise is checked, not assumed."""
import numpy as np

from tests.weight_norm_ref import SLACK, U, accumulated, cdiv, gamma  # noqa: F401  (accumulated: re-exported)

EM, NT, CB = 16, 256, 32           # padded embedding width, frames per workgroup, rows per backward tile
W_REL_G = 13.0                     # units of u, see above
OUT_GRID = np.array([0.0, 0.5, -0.5, 0.75, -0.75])          # (1 - |out|)^2 in {1, 1/4, 1/16}
BF16_NAN = 0x7fc1


def _f64(a):
    a = np.asarray(a)
    assert a.dtype == np.float32, a.dtype
    return a.astype(np.float64)


def weight(layer):
    """W [C][E] float64 of a layer dict(v, g, bias)"""
    v = _f64(layer["v"])
    if layer.get("g") is None:
        return v
    return _f64(layer["g"]).reshape(-1, 1) * v / np.sqrt((v * v).sum(1, keepdims=True))


def w_rel(layer):
    return 0.0 if layer.get("g") is None else W_REL_G


# ------------------------------------------------------------------------------------------------------------------
# forward
# ------------------------------------------------------------------------------------------------------------------
def forward(e, layers):
    """e [B][E][T] fp32, layers [dict(v [C][E], g [C] | None, bias [C] | None)] -> per layer dict(out, z, chain, E_out):
    chain = |b| + sum |W| |e|, E_out the per-element bound of the header comment"""
    e64 = _f64(e)
    res = []
    for lay in layers:
        W = weight(lay)
        b = _f64(lay["bias"]) if lay.get("bias") is not None else np.zeros(W.shape[0])
        z = np.einsum("ce,bet->bct", W, e64) + b[None, :, None]
        chain = np.einsum("ce,bet->bct", np.abs(W), np.abs(e64)) + np.abs(b)[None, :, None]
        out = z / (1.0 + np.abs(z))
        E_z = (w_rel(lay) + 7.0) * U * chain
        E_out = (E_z / (1.0 + np.abs(z)) ** 2 + 4.0 * U * np.abs(out)) * SLACK
        res.append(dict(out=out, z=z, chain=chain, E_out=E_out))
    return res


# ------------------------------------------------------------------------------------------------------------------
# backward
# ------------------------------------------------------------------------------------------------------------------
def sum_depth(B, T):
    """D_sum of the header comment: roundings a term of dW / db passes through at most"""
    nb = B * cdiv(T, NT)
    waves = cdiv(min(T, NT), 64)
    groups = min(4, nb)
    return 4 + 1 + min(64, T) + min(3, waves - 1) + cdiv(nb, 4) + min(2, int(np.ceil(np.log2(groups))))


def backward(e, layers, outs, douts):
    """e [B][E][T], outs[l] / douts[l] [B][C_l][T] fp32 (the values the kernel reads: a c8 gradient as the fp32 values of
    its bf16 words) -> dict(de, E_de, A_de, layers=[dict(dW, db, dv, dg, A_dW, A_db, E_dW, E_db, E_dv, E_dg)])"""
    e64 = _f64(e)
    B, E, T = e64.shape
    L = len(layers)
    D = sum_depth(B, T)
    de, E_de, A_de = np.zeros_like(e64), np.zeros_like(e64), np.zeros_like(e64)
    res = []
    for lay, out, dout in zip(layers, outs, douts):
        W, v = weight(lay), _f64(lay["v"])
        C = W.shape[0]
        gp = _f64(dout) * (1.0 - np.abs(_f64(out))) ** 2
        dW = np.einsum("bct,bet->ce", gp, e64)
        A_dW = np.einsum("bct,bet->ce", np.abs(gp), np.abs(e64))              # sum |gp| |e|
        db, A_db = gp.sum((0, 2)), np.abs(gp).sum((0, 2))                      # sum |gp|
        a_de = np.einsum("ce,bct->bet", np.abs(W), np.abs(gp))                 # sum_c |W| |gp|
        de += np.einsum("ce,bct->bet", W, gp)
        A_de += a_de
        E_de += gamma(w_rel(lay) + 4 + 1 + C + L) * a_de * SLACK
        E_dW, E_db = gamma(D) * A_dW * SLACK, gamma(D) * A_db * SLACK
        r = dict(dW=dW, db=db, A_dW=A_dW, A_db=A_db, E_dW=E_dW, E_db=E_db, gp=gp)
        if lay.get("g") is None:
            r.update(dv=dW, E_dv=E_dW, dg=None, E_dg=None)
        else:
            g = _f64(lay["g"]).reshape(-1, 1)
            vv = (v * v).sum(1, keepdims=True)
            nrm = np.sqrt(vv)
            dot = (dW * v).sum(1, keepdims=True)
            E_dot = (E_dW * np.abs(v)).sum(1, keepdims=True) + 5.0 * U * (np.abs(dW) * np.abs(v)).sum(1, keepdims=True) * SLACK
            dg = dot / nrm
            E_dg = (E_dot + 7.5 * U * np.abs(dot)) / nrm * SLACK
            c1, q = g / nrm, v * dot / vv
            dv = c1 * (dW - q)
            E_dv = (np.abs(c1) * (E_dW + np.abs(v) * E_dot / vv) +
                    U * np.abs(c1) * (9.5 * np.abs(dW) + 17.5 * np.abs(q))) * SLACK
            r.update(dv=dv, E_dv=E_dv, dg=dg.reshape(-1), E_dg=E_dg.reshape(-1))
        res.append(r)
    return dict(de=de, E_de=E_de, A_de=A_de, layers=res)


# ------------------------------------------------------------------------------------------------------------------
# a c8 gradient: bf16 [B][ceil(2C/8)][T][8], the first C channels are the gradient of the bias
# ------------------------------------------------------------------------------------------------------------------
def bf16_round(x):
    """fp32 -> the fp32 value of its bf16 rounding (to nearest even)"""
    w = np.ascontiguousarray(x, dtype=np.float32).view(np.uint32).astype(np.uint64)
    w = ((w + 0x7fff + ((w >> 16) & 1)) >> 16) << 16
    return w.astype(np.uint32).view(np.float32)


def c8_words(dout, seed=0):
    """dout [B][C][T] fp32 of bf16-representable values -> uint16 [B][c8p][T][8], c8p = ceil(2 C / 8): channels C .. 2C - 1
    hold other finite values (the layer's second half), the padding channels of the last group NaN bit patterns"""
    B, C, T = dout.shape
    c8p = cdiv(2 * C, 8)
    full = np.random.RandomState(seed).standard_normal((B, c8p * 8, T)).astype(np.float32)
    full[:, :C] = dout
    words = (np.ascontiguousarray(bf16_round(full)).view(np.uint32) >> 16).astype(np.uint16)
    assert np.array_equal((words[:, :C].astype(np.uint32) << 16).view(np.float32), dout), "dout is not bf16-representable"
    words[:, 2 * C:] = BF16_NAN
    return np.ascontiguousarray(words.reshape(B, c8p, 8, T).transpose(0, 1, 3, 2)), c8p


# ------------------------------------------------------------------------------------------------------------------
# input families: -> dict(e, layers, outs, douts, exact)
# ------------------------------------------------------------------------------------------------------------------
EXACT_FAMILIES = ("dyadic", "dropped", "last", "coded", "wn")
BOUNDED_FAMILIES = ("normal", "wide", "saturated")


def _grid(rs, shape, lo, hi, step):
    return (rs.randint(lo, hi + 1, shape) * step).astype(np.float32)


def family(fam, B, E, T, Cs, seed=0, g=None, bias=True):
    """one case of an input family.  g: None = the family's default (wn: given; the other EXACT families: NULL; BOUNDED:
    given), True / False to force it where the family allows."""
    rs = np.random.RandomState(seed * 7919 + B * 131 + E * 17 + T + sum(Cs))
    if fam in EXACT_FAMILIES:
        assert not (g and fam != "wn"), "only the wn family is exact with g"
        return _exact(fam, rs, B, E, T, Cs, bias)
    assert fam in BOUNDED_FAMILIES, fam
    g = True if g is None else g
    e = rs.standard_normal((B, E, T)).astype(np.float32)
    e *= (rs.uniform(size=(B, 1, T)) > 0.05)                       # the per-frame speaker dropout
    layers, outs, douts = [], [], []
    for C in Cs:
        v = rs.standard_normal((C, E)).astype(np.float32)
        if fam == "saturated":
            v *= 100.0                                              # g NULL: |z| of hundreds; g given: rows renormalised
        lay = dict(v=v, g=(rs.uniform(0.5, 1.5, C) * (40.0 if fam == "saturated" else 1.0)).astype(np.float32) if g else None,
                   bias=(rs.standard_normal(C) * 0.1).astype(np.float32) if bias else None)
        layers.append(lay)
        d = rs.standard_normal((B, C, T))
        if fam == "wide":
            d *= 10.0 ** rs.uniform(-3, 3, (B, C, T))              # 1e-3 .. 1e3 on dout, element by element
        douts.append(d.astype(np.float32))
    if fam == "saturated":                                          # the backward is fed |out| in {1 - 2^-24, 1 - 2^-12, 1, 0} directly
        levels = np.array([1.0 - 2.0 ** -24, 1.0 - 2.0 ** -12, 1.0, 0.0], np.float32)
        outs = [(levels[rs.randint(0, 4, d.shape)] * rs.choice([-1.0, 1.0], d.shape)).astype(np.float32) for d in douts]
    else:
        outs = [r["out"].astype(np.float32) for r in forward(e, layers)]
    return dict(e=e, layers=layers, outs=outs, douts=douts, exact=False, fam=fam)


def _exact(fam, rs, B, E, T, Cs, bias):
    """dyadic / dropped / last / wn: e and v multiples of 1/4 with |.| <= 1, bias multiples of 1/16, dout multiples of 1/16
    with |.| <= 1 (five significant bits: bf16-representable, so a c8 gradient is exact as well), out in OUT_GRID.
      gp = dout (1 - |out|)^2: units of 1/256, |gp| <= 1;   gp e: units of 2^-10, at most 2^10 units each;
      dW, db: B T <= 3 * 515 = 1545 frames -> below 1545 * 2^10 = 2^20.6 units;
      d emb: |W| <= 4 (wn: W = sign(v) g, g in {1/4 .. 4}), units of 2^-10: rows * 2^12 units, rows <= 130 -> 2^19.1;
      dv of wn: dW times g / ||v|| in {1/2, 1, 2}: units of 2^-11, below 2 * 1545 * 2^11 = 2^22.6; with a prefill
      (multiples of 1/4, |.| <= 8) the same grid.   forward: 16 products of units 1/16 plus the bias: far below.
      (assert_exact_premise checks all of it in units of 2^-11.)
    wn: rows of v with ONE non-zero entry +-2^k: ||v|| = 2^k exactly, so sqrtf, both divisions and every product by a
    power of two are exact: W = v g / ||v|| exactly, dg = dW[c][j] sign(v) and dv = (g / ||v||) dW off the entry, exactly 0
    on it.  (A 3-4-0 row has the exact norm 5 2^k, but 1 / 5 is not a float: dg and dv would round.  Not used.)
    coded: see _coded."""
    if fam == "coded":
        return _coded(B, E, T, Cs)
    dmax = 16
    e = _grid(rs, (B, E, T), -4, 4, 0.25)
    if fam == "dropped":
        e *= (rs.uniform(size=(B, 1, T)) > 0.3)                    # whole frames zeroed, as the per-frame dropout does
    layers, outs, douts = [], [], []
    for C in Cs:
        if fam == "wn":
            v = np.zeros((C, E), np.float32)
            v[np.arange(C), rs.randint(0, E, C)] = rs.choice([-1.0, 1.0], C) * 2.0 ** rs.randint(-1, 2, C)
            gg = (np.abs(v).sum(1) * 2.0 ** rs.randint(-1, 2, C)).astype(np.float32)
        else:
            v, gg = _grid(rs, (C, E), -4, 4, 0.25), None
        layers.append(dict(v=v, g=gg, bias=_grid(rs, (C,), -16, 16, 1.0 / 16) if bias else None))
        outs.append(OUT_GRID[rs.randint(0, 5, (B, C, T))].astype(np.float32))
        d = _grid(rs, (B, C, T), -dmax, dmax, 1.0 / 16)
        if fam == "last":                                           # non-zero only in the last row's last valid frame
            keep = np.zeros_like(d)
            keep[:, C - 1, T - 1] = np.where(d[:, C - 1, T - 1] == 0, 0.5, d[:, C - 1, T - 1])
            d = keep
        douts.append(d)
    return dict(e=e, layers=layers, outs=outs, douts=douts, exact=True, fam=fam)


def _coded(B, E, T, Cs):
    """index-coded: every (layer, row, column) of dW (db = column 16) and every (item, e, frame) of d emb gets its own
    value, so any permutation of a register-to-element mapping changes some element.
      e[b][k][t] = v_l[c][k] = f_k / 4 with f = 1, 2, 3, 5, 6, .., 17 (4 is left to the column of ones: db = 4 / 4 times the
      row's sum),  gp_l[c][n] = (1 + 19 x[r][n]) / 16   (r: row over all layers, n: frame over all items),
      x[0][n] = n + R, x[r][0] = r + N, 0 elsewhere (R rows, N frames); out cycles through OUT_GRID and
      dout = gp / (1 - |out|)^2 (a power of two: exact).  Then
      dW_l[c][k] = f_k (N + 19 X_r) / 64, X_r the row sum of x;  de[n][k] = f_k (R + 19 Y_n) / 64, Y_n its column sum:
      f (N + 19 X) = f N (mod 19): with N and R no multiples of 19 and f in 1 .. 17 the residue gives the column, the
      quotient the row (frame), as the row (column) sums are distinct.  Largest sum, in units of 1 / 64:
      17 (N + 19 (N (N - 1) / 2 + R N + N)): N = 259, R = 66 -> 1.640e7 < 2^24 = 1.678e7 (asserted in
      assert_exact_premise).  All terms are positive: every partial sum is below the total.  bias = 0, so that db is an output."""
    R, N = sum(Cs), B * T
    assert N % 19 and R % 19 and E >= 1
    x = np.zeros((R, N), np.int64)
    x[0, :] = np.arange(N) + R
    x[:, 0] = np.arange(R) + N
    x[0, 0] = R + N
    assert len(set(x.sum(1))) == R and len(set(x.sum(0))) == N
    gp = ((1 + 19 * x) / 16.0).reshape(R, B, T).transpose(1, 0, 2)             # [B][R][T]
    f = np.array([1, 2, 3] + list(range(5, 18)), np.float64)[:E] / 4.0
    e = np.broadcast_to(f[None, :, None], (B, E, T)).astype(np.float32).copy()
    layers, outs, douts, r0 = [], [], [], 0
    for C in Cs:
        v = np.broadcast_to(f[None, :], (C, E)).astype(np.float32).copy()
        layers.append(dict(v=v, g=None, bias=np.zeros(C, np.float32)))
        idx = (np.arange(C)[None, :, None] + np.arange(T)[None, None, :] + np.arange(B)[:, None, None]) % 5
        out = OUT_GRID[idx]
        outs.append(out.astype(np.float32))
        d = gp[:, r0:r0 + C] / (1.0 - np.abs(out)) ** 2
        assert np.array_equal(d.astype(np.float32).astype(np.float64), d)
        douts.append(d.astype(np.float32))
        r0 += C
    return dict(e=e, layers=layers, outs=outs, douts=douts, exact=True, fam="coded")


def forward_exact_case(B, E, T, Cs, seed=0, bias=False, g=False):
    """the forward's EXACT family: z in {0, +-1, +-3}, so 1 + |z| is a power of two, v_rcp_f32 of it exact and out in
    OUT_GRID bit for bit.  Every frame of e is one-hot (+1) or zero (dropped); without a bias W[c][k] in {0, +-1, +-3};
    with one, b[c] in {0, +-1, +-3} and W[c][k] in {0, -2 b[c]}: z in {b, -b}.  g: rows scaled by g / ||v|| with ||v||
    a power of two is not available here (rows hold several entries): g stays NULL."""
    assert not g
    rs = np.random.RandomState(seed + B + E + T + sum(Cs))
    e = np.zeros((B, E, T), np.float32)
    hot = rs.randint(0, E, (B, T))
    on = rs.uniform(size=(B, T)) > 0.2
    for b in range(B):
        e[b, hot[b], np.arange(T)] = on[b]
    vals = np.array([0.0, 1.0, -1.0, 3.0, -3.0], np.float32)
    layers = []
    for C in Cs:
        if bias:
            bb = vals[rs.randint(0, 5, C)]
            v = (-2.0 * bb[:, None] * rs.randint(0, 2, (C, E))).astype(np.float32)
        else:
            bb, v = None, vals[rs.randint(0, 5, (C, E))]
        layers.append(dict(v=v, g=None, bias=bb))
    return dict(e=e, layers=layers, exact=True, fam="forward-exact")


def assert_exact_premise(case, prefill=None):
    """the float64 results of an EXACT case are fp32 values: every gradient (with its prefill, when given), so a kernel
    that sums without rounding returns exactly these"""
    ref = backward(case["e"], case["layers"], case["outs"], case["douts"])
    rt = lambda a: np.array_equal(np.asarray(a, np.float64).astype(np.float32).astype(np.float64), a)
    assert rt(ref["de"]), "de"
    B, T = case["e"].shape[0], case["e"].shape[2]
    for l, r in enumerate(ref["layers"]):
        # every partial sum in any order is bounded by the absolute sum: that one must stay below 2^24 units of the grid
        unit = 2.0 ** -11 if case["fam"] != "coded" else 2.0 ** -6
        assert r["A_dW"].max() / unit < 2.0 ** 24 and r["A_db"].max() / unit < 2.0 ** 24, (l, r["A_dW"].max() / unit)
        for name in ("dW", "db", "dv", "dg"):
            if r[name] is None:
                continue
            assert rt(r[name]), (l, name)
            if prefill is not None and name in ("dv", "dg", "db"):
                assert rt(r[name] + prefill[l][name].reshape(r[name].shape)), (l, name, "with prefill")
    assert ref["A_de"].max() / (2.0 ** -11 if case["fam"] != "coded" else 2.0 ** -6) < 2.0 ** 24
    return ref


def prefill_for(case, seed=0):
    """known dyadic starting values of the += gradients: multiples of 1/4 with |.| <= 8"""
    rs = np.random.RandomState(seed + 99)
    return [dict(dv=_grid(rs, lay["v"].shape, -32, 32, 0.25), dg=_grid(rs, (lay["v"].shape[0],), -32, 32, 0.25),
                 db=_grid(rs, (lay["v"].shape[0],), -32, 32, 0.25)) for lay in case["layers"]]

# coding: utf-8
"""-m gpu: the entry points of csrc/weight_norm.hip, each against the float64 references of tests/weight_norm_ref.py
computed from the same fp32 inputs, element by element (tests.util.assert_close_elementwise), through hand-built
dv3_wn_desc / dv3_wn_bwd_desc / dv3_wn_multi_entry structs -- buffers, leading dimensions, pads and alignment are the
test's.

  (a) dv3_weight_norm_pack_f32: scale and both operand images, every pad column exactly 0;
  (b) dv3_weight_norm_split_pack_bf16: the decoded (hi, lo) are the host split of (a)'s fp32 values bit for bit, the
      image is dv3_split_pack_bf16 of (a)'s images word for word, K pad rows zero, pad columns untouched;
      dv3_split_pack_bf16 on the transposed layers' images;
  (c) dv3_weight_norm_split_pack_multi: word-identical to (b) per layer over a whole arena, both orders of the table;
  (d) dv3_weight_norm_bwd_f32: dv, dg, dbias over the slab counts, both slab layouts, both gathers, both bias layouts,
      transposed layers, plain weights, accumulate, three input families;
  (e) dv3_weight_norm_bwd_multi: bit-identical to single calls; the documented refusals;
  (f) the refusals of the pack entry points.

Every output buffer starts as NaN (uint16 images: the sentinel word) and is followed by a guard that must be unchanged;
slab buffers carry NaN pad columns and a NaN tail.  The bounds are derived in weight_norm_ref.py -- none is measured;
tests/test_cpu_weight_norm_ref.py asserts the preconditions."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tests import weight_norm_ref as R  # noqa: E402
from tests.util import assert_close_elementwise  # noqa: E402

pytestmark = pytest.mark.gpu

NAN = float("nan")
GUARD = 1024                       # elements after every output buffer
DT = {"bf16": 0, "f16": 1}         # DV3_SPLIT_DTYPE_*


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


@pytest.fixture(autouse=True)
def _clear_range_counter():
    """the wide-range family leaves the fp16 range on purpose; the sticky device counter that notes it is read by
    trainers (ops.f16_range_events) and must not outlive the test"""
    yield
    if torch.cuda.is_available():
        from deepvoice3_pytorch_amd import ops
        ops._lib.call("dv3_f16_range_events", None, 1, ops._stream())
        torch.cuda.synchronize()


def _env():
    from deepvoice3_pytorch_amd import ops, _lib
    return ops, _lib.lib(), _lib.STRUCTS


def _report(what, ratio):
    print("worst-ratio %-72s %.4g" % (what, ratio))


def _up(dev, a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _nan(dev, n):
    return torch.full((n + GUARD,), NAN, device=dev)


def _words(dev, n):
    return torch.full((n + GUARD,), R.SENTINEL, dtype=torch.int16, device=dev)


def _f32_guard_ok(t, n):
    return bool(torch.isnan(t[n:]).all())


def _u16(t):
    return t.cpu().numpy().view(np.uint16)


def _refused(L, rc):
    msg = L.dv3_last_error()
    return rc != 0 and bool(msg) and len(msg) > 0


def _inputs(fam, O, I, J, transposed, seed):
    rows, inner = (I, (O, J)) if transposed else (O, (I, J))
    return R.family(fam, rows, inner, seed)


def _wn_desc(S, v, g, scale, lay, O, I, J, transposed, glu_cg, fwd=None, bwd=None, fwd_dtype=0):
    d = S["dv3_wn_desc"]()
    d.v, d.g, d.scale = v.data_ptr(), (g.data_ptr() if g is not None else None), scale.data_ptr()
    d.fwd_pack = fwd.data_ptr() if fwd is not None else None
    d.bwd_pack = bwd.data_ptr() if bwd is not None else None
    d.lda, d.a_half, d.ldb = lay["lda"], lay["a_half"], lay["ldb"]
    d.O, d.I, d.J, d.transposed, d.glu_cg, d.fwd_dtype = O, I, J, int(transposed), glu_cg, fwd_dtype
    return d


# ------------------------------------------------------------------------------------------------------------------
# (a) the fp32 pack
# ------------------------------------------------------------------------------------------------------------------
def _pack_f32(dev, v, g, O, I, J, glu_cg, transposed, with_bwd=True):
    """-> dict(scale, fwd, bwd (or None)) device tensors WITH their guards, and the sizes"""
    ops, L, S = _env()
    lay = R.layout(O, I, J, glu_cg, transposed, 0 if transposed else R.NT_LDA_PAD.get((O, I, J, glu_cg), 0))
    rows = I if transposed else O
    n_f, n_b = lay["Jp"] * lay["K"] * lay["lda"], lay["Jp"] * lay["Kb"] * lay["ldb"]
    vd, gd = _up(dev, v), (_up(dev, g) if g is not None else None)
    scale, fwd, bwd = _nan(dev, rows), _nan(dev, n_f), (_nan(dev, n_b) if with_bwd else None)
    d = _wn_desc(S, vd, gd, scale, lay, O, I, J, transposed, glu_cg, fwd, bwd)
    ops._lib.call("dv3_weight_norm_pack_f32", ctypes.byref(d), ops._stream())
    torch.cuda.synchronize()
    assert _f32_guard_ok(scale, rows) and _f32_guard_ok(fwd, n_f) and (bwd is None or _f32_guard_ok(bwd, n_b))
    return dict(scale=scale, fwd=fwd, bwd=bwd, n_f=n_f, n_b=n_b, rows=rows, lay=lay, v=vd, g=gd)


PACK_CASES = [(O, I, J, cg, False) for O, I, J, cg in R.NT_SHAPES] + [(O, I, J, 0, True) for I, O, J in R.T_SHAPES]


@pytest.mark.parametrize("g_given", [True, False])
@pytest.mark.parametrize("fam", R.FAMILIES)
@pytest.mark.parametrize("case", PACK_CASES)
def test_pack_f32_against_fp64(dev, case, fam, g_given):
    O, I, J, cg, tr = case
    v, g = _inputs(fam, O, I, J, tr, seed=O * 131 + I * 7 + J)
    g = g if g_given else None
    p = _pack_f32(dev, v, g, O, I, J, cg, tr)
    lay, length = p["lay"], v[0].size
    scale = p["scale"][:p["rows"]].cpu().numpy()
    if g_given:
        r0 = assert_close_elementwise(scale, R.scale_ref(v, g), R.scale_rel_bound(length), 0.0, "scale")
    else:
        assert np.array_equal(scale, np.ones(p["rows"], np.float32))
        r0 = 0.0
    w = R.weight_ref(v, g)
    rel = R.pack_rel_bound(length, g_given)
    want_f, _ = R.fwd_pack_of(w, lay["lda"], lay["a_half"], cg, tr, fill=0.0)     # pads: exactly 0 (bound 0 there)
    want_b, _ = R.bwd_pack_of(w, lay["ldb"], tr, fill=0.0)
    fwd = p["fwd"][:p["n_f"]].cpu().numpy().reshape(want_f.shape)
    bwd = p["bwd"][:p["n_b"]].cpu().numpy().reshape(want_b.shape)
    r1 = assert_close_elementwise(fwd, want_f, rel, 0.0, "fwd_pack")
    r2 = assert_close_elementwise(bwd, want_b, rel, 0.0, "bwd_pack")
    # bwd_pack NULL: the same scale and forward image, nothing else
    q = _pack_f32(dev, v, g, O, I, J, cg, tr, with_bwd=False)
    assert torch.equal(q["fwd"].view(torch.int32), p["fwd"].view(torch.int32))
    assert torch.equal(q["scale"].view(torch.int32), p["scale"].view(torch.int32))
    _report("(a) pack_f32 %s %s g=%s" % (case, fam, g_given), max(r0, r1, r2))


# ------------------------------------------------------------------------------------------------------------------
# (b) the fused split pack
# ------------------------------------------------------------------------------------------------------------------
def _split_of_f32(dev, img, n_j, K, lda, dtype):
    """dv3_split_pack_bf16 of a device fp32 image -> uint16 words [plane][j][Kp][lda] (host)"""
    ops, L, S = _env()
    n = R.split_words(n_j, K, lda)
    out = _words(dev, n)
    ops._lib.call("dv3_split_pack_bf16", img.data_ptr(), out.data_ptr(), n_j, K, lda, DT[dtype], ops._stream())
    torch.cuda.synchronize()
    o = _u16(out)
    assert np.all(o[n:] == R.SENTINEL)
    return R.decode_split_words(o[:n], n_j, K, lda)


def _check_split_image(words, f32_img, own, n_j, K, lda, dtype, what):
    """words [plane][j][Kp][lda] of a fused image against the fp32 image [j][K][lda] it must be the split of"""
    Kp = R.rup(K, 32)
    own_cols = own.any(axis=(0, 1))                                  # columns some weight owns
    hi, lo = R._from_bits(words[0], dtype), R._from_bits(words[1], dtype)
    eh, el = R.host_split(np.where(own, f32_img, 0).astype(np.float32), dtype)
    for got, want, nm in ((hi, eh, "hi"), (lo, el, "lo")):
        g_, w_ = got[:, :K][own], want[own]
        assert np.array_equal(g_, w_, equal_nan=True), "%s: %s plane differs from the host split at %d positions" % (
            what, nm, int((g_ != w_).sum()))
    assert np.all(words[:, :, K:Kp][..., own_cols] == 0), what + ": K pad rows are not zero"
    assert np.all(words[..., ~own_cols] == R.SENTINEL), what + ": a pad column was written"


@pytest.mark.parametrize("dtype", ["bf16", "f16"])
@pytest.mark.parametrize("fam", R.FAMILIES)
@pytest.mark.parametrize("shape", R.NT_SHAPES)
def test_split_pack_is_the_split_of_the_f32_pack(dev, shape, fam, dtype):
    ops, L, S = _env()
    O, I, J, cg = shape
    v, g = _inputs(fam, O, I, J, False, seed=O * 131 + I * 7 + J)
    p = _pack_f32(dev, v, g, O, I, J, cg, False)
    lay = p["lay"]
    lda, ldb = lay["lda"], lay["ldb"]
    n_f, n_b = R.split_words(J, I, lda), R.split_words(J, O, ldb)
    imgs = {}
    for with_bwd in (True, False):
        scale, fs, bs = _nan(dev, O), _words(dev, n_f), _words(dev, n_b)
        d = _wn_desc(S, p["v"], p["g"], scale, lay, O, I, J, False, cg, fwd_dtype=DT[dtype])
        ops._lib.call("dv3_weight_norm_split_pack_bf16", ctypes.byref(d), fs.data_ptr(),
                      bs.data_ptr() if with_bwd else None, ops._stream())
        torch.cuda.synchronize()
        assert torch.equal(scale.view(torch.int32), p["scale"].view(torch.int32))
        imgs[with_bwd] = (_u16(fs), _u16(bs))
        assert np.all(imgs[with_bwd][0][n_f:] == R.SENTINEL) and np.all(imgs[with_bwd][1][n_b:] == R.SENTINEL)
    assert np.array_equal(imgs[False][0], imgs[True][0])
    assert np.all(imgs[False][1] == R.SENTINEL), "bwd_split NULL, and the buffer was written"
    fw = R.decode_split_words(imgs[True][0][:n_f], J, I, lda)
    bw = R.decode_split_words(imgs[True][1][:n_b], J, O, ldb)
    w = R.weight_ref(v, g)
    _, own_f = R.fwd_pack_of(w, lda, lay["a_half"], cg)
    _, own_b = R.bwd_pack_of(w, ldb)
    f32_f = p["fwd"][:p["n_f"]].cpu().numpy().reshape(J, I, lda)
    f32_b = p["bwd"][:p["n_b"]].cpu().numpy().reshape(J, O, ldb)
    _check_split_image(fw, f32_f, own_f, J, I, lda, dtype, "fwd image")
    _check_split_image(bw, f32_b, own_b, J, O, ldb, "bf16", "bwd image")
    # the equivalence the kernel's comment claims: dv3_split_pack_bf16 of the fp32 images, word for word
    sf = _split_of_f32(dev, p["fwd"], J, I, lda, dtype)
    sb = _split_of_f32(dev, p["bwd"], J, O, ldb, "bf16")
    cf, cb = own_f.any(axis=(0, 1)), own_b.any(axis=(0, 1))
    assert np.array_equal(fw[..., cf], sf[..., cf]) and np.array_equal(bw[..., cb], sb[..., cb])


@pytest.mark.parametrize("dtype", ["bf16", "f16"])
@pytest.mark.parametrize("shape", R.T_SHAPES)
def test_split_pack_bf16_of_the_transposed_images(dev, shape, dtype):
    """dv3_split_pack_bf16 alone: K = I and K = J*O, neither a multiple of 32; the rows beyond K are zero"""
    I, O, J = shape
    v, g = _inputs("generic", O, I, J, True, seed=I * 31 + O)
    p = _pack_f32(dev, v, g, O, I, J, 0, True)
    lay = p["lay"]
    for img, n, K, ld in ((p["fwd"], p["n_f"], I, lay["lda"]), (p["bwd"], p["n_b"], J * O, lay["ldb"])):
        assert K % 32 != 0
        words = _split_of_f32(dev, img, 1, K, ld, dtype)
        f32 = img[:n].cpu().numpy().reshape(1, K, ld)
        eh, el = R.host_split(f32, dtype)
        assert np.array_equal(R._from_bits(words[0], dtype)[:, :K], eh)
        assert np.array_equal(R._from_bits(words[1], dtype)[:, :K], el)
        assert np.all(words[:, :, K:] == 0)
        assert np.array_equal(words.reshape(-1), R.decode_split_words(R.encode_split(f32, dtype), 1, K, ld).reshape(-1))


# ------------------------------------------------------------------------------------------------------------------
# (c) every layer in two launches
# ------------------------------------------------------------------------------------------------------------------
# (O, I, J, glu_cg, g given, forward dtype): a single block with one tap, the GLU column gap, the layer that sets max_taps,
# a plain weight, a 4-trip norm, a 1 x 1 x 1 layer
MULTI_LAYERS = [(33, 31, 3, 0, True, "f16"), (8, 8, 1, 0, True, "bf16"), (12, 36, 3, 6, True, "f16"),
                (64, 40, 5, 0, True, "bf16"), (66, 33, 2, 0, False, "f16"), (96, 257, 3, 0, True, "bf16"),
                (1, 1, 1, 0, True, "f16")]
ARENA_GAP = 16384                  # 4-byte words between any two buffers of the arena
ARENA_FILL = (R.SENTINEL << 16) | R.SENTINEL       # a NaN as fp32, the sentinel as either uint16 half


class _Arena(object):
    """one device allocation for every buffer of the table, so that `nothing else changed` is one comparison"""

    def __init__(self, dev, layers):
        self.off, n = [], ARENA_GAP
        for O, I, J, cg, gg, dt in layers:
            lay = R.layout(O, I, J, cg, lda_pad=R.NT_LDA_PAD.get((O, I, J, cg), 0))
            sizes = dict(v=O * I * J, g=O, scale=O, fwd=R.split_words(J, I, lay["lda"]) // 2,
                         bwd=R.split_words(J, O, lay["ldb"]) // 2)
            o = {}
            for k in ("v", "g", "scale", "fwd", "bwd"):
                o[k] = n
                n += R.rup(sizes[k], 4) + ARENA_GAP
            self.off.append((o, sizes, lay))
        self.buf = torch.full((n,), ARENA_FILL, dtype=torch.int32, device=dev)
        self.layers = layers
        self.inputs = []
        for (O, I, J, cg, gg, dt), (o, sizes, lay) in zip(layers, self.off):
            v, g = R.family("generic", O, (I, J), seed=O + I)
            self.buf[o["v"]:o["v"] + v.size] = _up(dev, v.reshape(-1)).view(torch.int32)
            self.buf[o["g"]:o["g"] + O] = _up(dev, g).view(torch.int32)
            self.inputs.append((v, g if gg else None))

    def ptr(self, l, k):
        return self.buf.data_ptr() + 4 * self.off[l][0][k]

    def desc(self, S, l):
        O, I, J, cg, gg, dt = self.layers[l]
        lay = self.off[l][2]
        d = S["dv3_wn_desc"]()
        d.v, d.g, d.scale = self.ptr(l, "v"), (self.ptr(l, "g") if gg else None), self.ptr(l, "scale")
        d.lda, d.a_half, d.ldb = lay["lda"], lay["a_half"], lay["ldb"]
        d.O, d.I, d.J, d.transposed, d.glu_cg, d.fwd_dtype = O, I, J, 0, cg, DT[dt]
        return d

    def reset_outputs(self):
        for o, sizes, lay in self.off:
            for k in ("scale", "fwd", "bwd"):
                self.buf[o[k]:o[k] + sizes[k]] = ARENA_FILL


def _run_multi(dev, arena, order):
    ops, L, S = _env()
    n = len(order)
    tab = (S["dv3_wn_multi_entry"] * n)()
    first_row, first_block, rows, blocks, taps = [], [], 0, 0, 0
    for k, l in enumerate(order):
        O, I, J = arena.layers[l][:3]
        tab[k].d = arena.desc(S, l)
        tab[k].fwd_split, tab[k].bwd_split = arena.ptr(l, "fwd"), arena.ptr(l, "bwd")
        first_row.append(rows)
        first_block.append(blocks)
        rows, blocks, taps = rows + O, blocks + R.cdiv(O, 32) * R.cdiv(I, 32), max(taps, J)
    tab_d = _up(dev, np.frombuffer(bytes(tab), dtype=np.uint8).copy())
    fr, fb = _up(dev, np.array(first_row, np.int32)), _up(dev, np.array(first_block, np.int32))
    ops._lib.call("dv3_weight_norm_split_pack_multi", tab_d.data_ptr(), fr.data_ptr(), fb.data_ptr(), n, rows, blocks,
                  taps, ops._stream())
    torch.cuda.synchronize()


@pytest.mark.parametrize("table", ["seven", "one"])
def test_split_pack_multi_is_the_per_layer_call(dev, table):
    ops, L, S = _env()
    layers = MULTI_LAYERS if table == "seven" else MULTI_LAYERS[:1]
    arena = _Arena(dev, layers)
    before = arena.buf.clone()
    for l in range(len(layers)):
        d = arena.desc(S, l)
        ops._lib.call("dv3_weight_norm_split_pack_bf16", ctypes.byref(d), arena.ptr(l, "fwd"), arena.ptr(l, "bwd"),
                      ops._stream())
    torch.cuda.synchronize()
    want = arena.buf.clone()
    # the per-layer calls wrote inside their own images only, and wrote them
    mask = torch.zeros_like(before, dtype=torch.bool)
    for o, sizes, lay in arena.off:
        for k in ("scale", "fwd", "bwd"):
            mask[o[k]:o[k] + sizes[k]] = True
    assert torch.equal(want[~mask], before[~mask])
    for l, (o, sizes, lay) in enumerate(arena.off):
        sc = want[o["scale"]:o["scale"] + sizes["scale"]].view(torch.float32).cpu().numpy()
        v, g = arena.inputs[l]
        if g is None:
            assert np.array_equal(sc, np.ones_like(sc))
        else:
            r = assert_close_elementwise(sc, R.scale_ref(v, g), R.scale_rel_bound(v[0].size), 0.0, "scale of layer %d" % l)
            _report("(c) scale of layer %d" % l, r)
    orders = [list(range(len(layers))), list(range(len(layers)))[::-1]]
    for order in orders[:len(layers)]:
        arena.reset_outputs()
        assert torch.equal(arena.buf, before)
        _run_multi(dev, arena, order)
        diff = arena.buf != want
        assert not bool(diff.any()), "order %s: %d words differ from the per-layer calls, first at word %d" % (
            order, int(diff.sum()), int(diff.nonzero()[0]))


# ------------------------------------------------------------------------------------------------------------------
# (d) the backward
# ------------------------------------------------------------------------------------------------------------------
def _bwd_setup(dev, c, seed):
    """host inputs, device buffers and the descriptor of one backward case -> dict"""
    ops, L, S = _env()
    O, I, J, tr = c["O"], c["I"], c["J"], c.get("tr", False)
    fam, n_slabs = c.get("fam", "generic"), c["n_slabs"]
    rows, length = (I if tr else O), (O * J if tr else I * J)
    v, g = _inputs(fam, O, I, J, tr, seed)
    g = g if c.get("g", True) else None
    scale = R.scale_ref(v, g).astype(np.float32)
    slabs = R.slabs_for(fam, v, n_slabs, O, I, J, tr, seed)
    ldo = c.get("ldo", R.rup(I, 4))
    flat, ss, rs = R.slab_buffer(slabs, c.get("rows_of_slabs", False), ldo)
    off = c.get("offset", 0)
    sb = torch.full((flat.size + 4,), NAN, device=dev)
    sb[off:off + flat.size] = _up(dev, flat)
    rng = np.random.RandomState(seed + 3)
    acc = c.get("acc", 0)
    k = dict(c=c, v=v, g=g, scale=scale, slabs=slabs, rows=rows, length=length, keep=[sb])
    d = S["dv3_wn_bwd_desc"]()
    d.slabs, d.slab_ss, d.ldo, d.n_slabs = sb.data_ptr() + 4 * off, ss, rs, n_slabs
    for name, arr in (("v", v), ("g", g), ("scale", scale if g is not None else None)):
        t = _up(dev, arr) if arr is not None else None
        setattr(d, name, t.data_ptr() if t is not None else None)
        k["keep"].append(t)

    def out(n, name):
        t = _nan(dev, n)
        start = None
        if acc:
            start = rng.standard_normal(n).astype(np.float32)
            t[:n] = _up(dev, start)
        k[name], k[name + "_start"], k[name + "_n"] = t, start, n
        return t.data_ptr()
    d.dv = out(rows * length, "dv")
    if g is not None:
        d.dg = out(rows, "dg")
    part = c.get("part")                       # (n_part, part_t) or None
    d.dbias = out(O, "dbias")                   # given even without partials: it must then stay untouched
    if part is not None:
        n_part, part_t = part
        k["part"] = (rng.standard_normal((O, n_part) if part_t else (n_part, O)) *
                     2.0 ** rng.uniform(-8, 8, (O, 1) if part_t else (1, O))).astype(np.float32)
        pb = torch.full((k["part"].size + GUARD,), NAN, device=dev)
        pb[:k["part"].size] = _up(dev, k["part"].reshape(-1))
        k["keep"].append(pb)
        d.bias_part, d.n_part, d.bias_part_t = pb.data_ptr(), n_part, int(part_t)
    d.O, d.I, d.J, d.transposed, d.accumulate = O, I, J, int(tr), acc
    k["d"] = d
    return k


def _bwd_outputs(k):
    torch.cuda.synchronize()
    out = {}
    for name in ("dv", "dg", "dbias"):
        if name in k:
            assert _f32_guard_ok(k[name], k[name + "_n"]), name + ": guard overwritten"
            out[name] = k[name][:k[name + "_n"]].cpu().numpy()
    return out


def _bwd_check(k, out, what):
    """every output of one backward call against the fp64 reference -> worst ratio"""
    c = k["c"]
    O, I, J, tr = c["O"], c["I"], c["J"], c.get("tr", False)
    ref = R.bwd_ref(k["slabs"], k["v"], k["g"], k["scale"], O, I, J, tr)
    worst = 0.0
    todo = [("dv", ref["dv"].reshape(-1), ref["E_dv"].reshape(-1))]
    if k["g"] is not None:
        todo.append(("dg", ref["dg"], ref["E_dg"]))
    if "part" in k:
        todo.append(("dbias",) + R.dbias_ref(k["part"], c["part"][1]))
    else:
        start = k["dbias_start"]
        assert np.array_equal(out["dbias"], start, equal_nan=True) if start is not None else np.all(np.isnan(out["dbias"]))
    for name, want, E in todo:
        if c.get("acc", 0):
            want, E = R.accumulated(k[name + "_start"], want, E)
        worst = max(worst, assert_close_elementwise(out[name], want, 0.0, E, "%s %s" % (what, name)))
    return worst


def _bwd_run(dev, c, seed, both_gathers=True):
    """one case through dv3_weight_norm_bwd_f32 (with the 16-byte and the 4-byte gather: the same bits) -> worst ratio"""
    ops, L, S = _env()
    outs = []
    for sw in ((1, 0) if both_gathers else (1,)):
        k = _bwd_setup(dev, c, seed)
        with ops._lib.switches({"DV3_SW_WN_BWD_VEC4": sw}):
            ops._lib.call("dv3_weight_norm_bwd_f32", ctypes.byref(k["d"]), ops._stream())
            outs.append(_bwd_outputs(k))
    if both_gathers:
        for name in outs[0]:
            assert np.array_equal(outs[0][name].view(np.int32), outs[1][name].view(np.int32)), name + ": gathers differ"
    return _bwd_check(k, outs[0], str(c))


SLAB_SHAPES = {"vec4": dict(O=24, I=40, J=3), "vec4_pad": dict(O=24, I=40, J=3, ldo=44), "vec4_off1": dict(O=24, I=40, J=3, offset=1),
               "scalar": dict(O=24, I=33, J=3), "vec4_2trips": dict(O=3, I=516, J=2)}


@pytest.mark.parametrize("kind", sorted(SLAB_SHAPES))
@pytest.mark.parametrize("n_slabs", R.N_SLABS)
def test_bwd_slab_counts(dev, n_slabs, kind):
    """every entry and exit of the 8-, 4- and 1-unrolled slab loops, both slab layouts, accumulate off and on; the
    16-byte-eligible shape also with NaN pad columns (ldo = I + 4) and with the slab pointer one float off, where the
    kernel is documented to fall back to the 4-byte gather: the test sees that the result is right, not which gather ran"""
    worst = 0.0
    for rows_of_slabs in (False, True):
        c = dict(SLAB_SHAPES[kind], n_slabs=n_slabs, rows_of_slabs=rows_of_slabs, acc=int(rows_of_slabs) ^ (n_slabs & 1))
        worst = max(worst, _bwd_run(dev, c, seed=n_slabs * 17 + len(kind)))
    _report("(d) slab counts %s S=%d" % (kind, n_slabs), worst)


BWD_CASES = [(O, I, J, False) for O, I, J, cg in R.NT_SHAPES] + [(O, I, J, True) for I, O, J in R.T_SHAPES]


@pytest.mark.parametrize("g_given", [True, False])
@pytest.mark.parametrize("fam", R.FAMILIES)
@pytest.mark.parametrize("idx", range(len(BWD_CASES)))
def test_bwd_families(dev, idx, fam, g_given):
    """all three input families over the pack shapes and the transposed layers, plain weights, accumulate off and on;
    no bias partials: dbias stays untouched.  The cancelling family is held to the absolute-sum bound."""
    O, I, J, tr = BWD_CASES[idx]
    n_slabs = R.N_SLABS[(idx * 3 + 1) % len(R.N_SLABS)]
    worst = 0.0
    for acc in (0, 1):
        c = dict(O=O, I=I, J=J, tr=tr, n_slabs=n_slabs, fam=fam, g=g_given, acc=acc, rows_of_slabs=bool(idx & 1))
        worst = max(worst, _bwd_run(dev, c, seed=idx * 101 + acc))
    _report("(d) families %s %s g=%s" % (BWD_CASES[idx], fam, g_given), worst)


@pytest.mark.parametrize("part_t", [False, True])
@pytest.mark.parametrize("n_part", R.N_PART)
def test_bwd_bias_partials(dev, n_part, part_t):
    """both bias-partial layouts over the partial counts at which the [O][n_part] loops change their trip counts, on a
    transposed layer with O > 2 rows (several trips of the channel loop per block)"""
    worst = 0.0
    for acc in (0, 1):
        c = dict(I=5, O=13, J=2, tr=True, n_slabs=3, part=(n_part, part_t), acc=acc)
        worst = max(worst, _bwd_run(dev, c, seed=n_part + acc, both_gathers=False))
    _report("(d) bias partials n_part=%d t=%s" % (n_part, part_t), worst)


@pytest.mark.parametrize("part_t", [False, True])
@pytest.mark.parametrize("case", R.ROWS_VS_O)
def test_bwd_rows_against_bias_channels(dev, case, part_t):
    I, O, J, tr = case
    c = dict(I=I, O=O, J=J, tr=tr, n_slabs=2, part=(257, part_t))
    _report("(d) rows vs O %s t=%s" % (case, part_t), _bwd_run(dev, c, seed=I * 5 + O, both_gathers=False))


# ------------------------------------------------------------------------------------------------------------------
# (e) several layers in one launch
# ------------------------------------------------------------------------------------------------------------------
# the longest row (the launch's LDS size) belongs to the third layer; one transposed layer; one plain weight
BWD_MULTI = [dict(O=8, I=8, J=1, n_slabs=1), dict(O=24, I=40, J=3, n_slabs=9, rows_of_slabs=True, part=(7, False)),
             dict(O=3, I=516, J=2, n_slabs=4, acc=1), dict(I=5, O=13, J=2, tr=True, n_slabs=3, part=(257, True)),
             dict(O=33, I=31, J=3, n_slabs=5, g=False), dict(O=24, I=33, J=3, n_slabs=13, fam="cancel"),
             dict(I=40, O=24, J=2, tr=True, n_slabs=2, part=(3, False), acc=1), dict(O=1, I=1, J=1, n_slabs=16)]


@pytest.mark.parametrize("n", [1, 3, 8])
def test_bwd_multi_is_the_single_calls(dev, n):
    ops, L, S = _env()
    single, worst = [], 0.0
    for l in range(n):
        k = _bwd_setup(dev, BWD_MULTI[l], seed=l)
        ops._lib.call("dv3_weight_norm_bwd_f32", ctypes.byref(k["d"]), ops._stream())
        single.append(_bwd_outputs(k))
        worst = max(worst, _bwd_check(k, single[-1], "single %d" % l))
    ks = [_bwd_setup(dev, BWD_MULTI[l], seed=l) for l in range(n)]
    arr = (S["dv3_wn_bwd_desc"] * n)(*[k["d"] for k in ks])
    ops._lib.call("dv3_weight_norm_bwd_multi", ctypes.byref(arr), n, ops._stream())
    for l, k in enumerate(ks):
        out = _bwd_outputs(k)
        for name in out:
            assert np.array_equal(out[name].view(np.int32), single[l][name].view(np.int32)), (l, name)
    _report("(e) bwd_multi n=%d" % n, worst)


def test_bwd_multi_refusals(dev):
    ops, L, S = _env()
    ks = [_bwd_setup(dev, dict(O=4 + l, I=8, J=1, n_slabs=2), seed=l) for l in range(9)]
    arr = (S["dv3_wn_bwd_desc"] * 9)(*[k["d"] for k in ks])
    assert _refused(L, L.dv3_weight_norm_bwd_multi(ctypes.byref(arr), 9, ops._stream())), "n = 9 was accepted"
    arr2 = (S["dv3_wn_bwd_desc"] * 3)(ks[0]["d"], ks[1]["d"], ks[2]["d"])
    arr2[2].dv = arr2[0].dv
    assert _refused(L, L.dv3_weight_norm_bwd_multi(ctypes.byref(arr2), 3, ops._stream())), "a shared dv was accepted"
    torch.cuda.synchronize()
    for k in ks:
        for name in ("dv", "dg", "dbias"):
            assert bool(torch.isnan(k[name]).all()), "a refused call wrote " + name


# ------------------------------------------------------------------------------------------------------------------
# (f) refusals of the pack entry points
# ------------------------------------------------------------------------------------------------------------------
def test_pack_refusals(dev):
    ops, L, S = _env()
    v = _up(dev, np.ones(16 * 16 * 16, np.float32))
    g = _up(dev, np.ones(16, np.float32))
    bufs = dict(scale=_nan(dev, 64), fwd=_nan(dev, 16 * 16 * 32), bwd=_nan(dev, 16 * 16 * 32))
    words = [_words(dev, 2 * 16 * 32 * 32), _words(dev, 2 * 16 * 32 * 32)]
    st = ops._stream()

    def desc(O, I, J, lda, a_half=0, cg=0, tr=0, ldb=None):
        lay = dict(lda=lda, a_half=a_half, ldb=ldb if ldb is not None else R.rup(I, 4))
        return _wn_desc(S, v, g, bufs["scale"], lay, O, I, J, tr, cg, bufs["fwd"], bufs["bwd"])

    def f32(d):
        return L.dv3_weight_norm_pack_f32(ctypes.byref(d), st)

    def fused(d):
        return L.dv3_weight_norm_split_pack_bf16(ctypes.byref(d), words[0].data_ptr(), words[1].data_ptr(), st)
    for entry in (f32, fused):
        assert _refused(L, entry(desc(6, 4, 1, lda=6))), "lda not a multiple of 4"
        assert _refused(L, entry(desc(8, 4, 1, lda=4))), "lda < O"
        assert _refused(L, entry(desc(10, 4, 1, lda=12, a_half=4, cg=4))), "GLU layout with 2 cg != O"
        assert _refused(L, entry(desc(8, 6, 1, lda=8, ldb=4))), "ldb < I"
    assert _refused(L, fused(desc(4, 4, 2, lda=8, tr=1))), "a transposed layer in the fused split pack"
    assert _refused(L, fused(desc(1, 1, 16, lda=4))), "16 taps: an LDS tile beyond 64 KB"
    torch.cuda.synchronize()
    for t in words:
        assert bool((t == R.SENTINEL).all()), "a refused call wrote an image"
    for t in bufs.values():
        assert bool(torch.isnan(t).all()), "a refused call wrote an output"
    # the accepted neighbours of the last two, so that the refusals are the stated ones
    assert f32(desc(4, 4, 2, lda=8, tr=1)) == 0
    torch.cuda.synchronize()
    bufs["fwd"].fill_(NAN)
    bufs["bwd"].fill_(NAN)
    assert fused(desc(1, 1, 15, lda=4)) == 0
    torch.cuda.synchronize()
    assert bool(torch.isnan(bufs["fwd"]).all()) and bool(torch.isnan(bufs["bwd"]).all())

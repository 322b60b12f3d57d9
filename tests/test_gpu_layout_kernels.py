# coding: utf-8
"""-m gpu: the layout and data-movement kernels of csrc/elementwise.hip that reach the rest of the suite only through
whole-model parity, each called directly and compared BIT FOR BIT (as int32) -- no tolerance anywhere in this file.

  pure moves      dv3_transpose_f32 (alpha = 1, no add), dv3_deinterleave2_f32 (both kernels), dv3_shift_append_f32,
                  dv3_dropout_apply_f32 (kept lanes, scale 1), dv3_zero_tail_b32 / dv3_zero_tail_items_b32, ops.zero_frames:
                  inputs are random BIT PATTERNS with -0.0, denormals, +-inf and NaN payloads planted; the output holds
                  the bits moved, and every output is surrounded by guard elements that must be unchanged.  transpose and
                  dropout_apply pass each value through one multiplication by 1.0f, which returns every value unchanged
                  but quiets a signalling NaN (IEEE 754): their patterns hold quiet NaN payloads only.
  with arithmetic the same expression in numpy float32, in the kernel's association, on finite inputs:
                  transpose   fl(fl(alpha x) + add): the kernel writes `v = alpha * x; if (add) v += add[..]` -- the addition
                              sits in its own conditional block, where -ffp-contract=fast (hipcc's default; csrc/Makefile
                              sets nothing else) does not reach it: a multiplication and an addition, each rounded.  Were
                              the two ever fused, the elements whose two roundings differ from one would fail here;
                  axpby       fl(alpha fl(a + b)) (b NULL: a + 0.0f);   ops.scaled_copy: the same with b NULL;
                  dropout     fl(x scale), +0.0 where dropped;
                  sum_scalars ((a + b) + c) + d, left to right.

Widths read from the kernels: transpose 32 x 32 tiles; axpby 256 threads, at most 4096 blocks (the grid-stride loop takes
a second pass above 1048576 elements); dropout_apply one wave per row, 64 frames per pass, 32 frames per mask word;
deinterleave2 16-byte loads of 4 samples / 8-byte stores (T even, both pointers 16-byte aligned) or one sample per
thread; shift_append one wave per row, 64 frames per pass; zero_tail* one 32-bit word per thread, 256 per block."""
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from oracle import dv3_oracle as O  # noqa: E402

pytestmark = pytest.mark.gpu

GUARD = 64
GUARD_WORD = 0x7fc0dead                      # a quiet NaN no kernel here can produce
F = np.float32
SPECIALS = [0x80000000, 0x00000000, 0x00000001, 0x807fffff, 0x7f800000, 0xff800000, 0x7fc12345, 0xffc00001, 0x7fffffff]
SIGNALLING = [0x7f800001, 0xffa00001, 0x7fbfffff]


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


def _env():
    from deepvoice3_pytorch_amd import ops, _lib
    return ops, _lib.lib()


def patterns(n, seed, signalling=True):
    """n uint32 words: random bit patterns with the special values planted.  signalling = False: every NaN is quiet"""
    rs = np.random.RandomState(seed)
    w = rs.randint(0, 2 ** 32, n, dtype=np.uint64).astype(np.uint32)
    sp = SPECIALS + (SIGNALLING if signalling else [])
    pos = rs.permutation(n)[:len(sp)]
    w[pos] = np.array(sp, np.uint32)[:len(pos)]
    if not signalling:
        nan = ((w & 0x7f800000) == 0x7f800000) & ((w & 0x007fffff) != 0)
        w = np.where(nan, w | 0x00400000, w).astype(np.uint32)
    return w


def finite(n, seed, scale_pow=20):
    """n fp32 values: normal, over 2^+-scale_pow in magnitude, no NaN / inf / denormal"""
    rs = np.random.RandomState(seed)
    return (rs.standard_normal(n) * 2.0 ** rs.uniform(-scale_pow, scale_pow, n)).astype(F)


class Buf(object):
    """a device buffer of 32-bit words [GUARD][n][GUARD] (+ `shift` leading words, to misalign the payload)"""

    def __init__(self, dev, words, shift=0):
        words = np.ascontiguousarray(words).reshape(-1)
        words = words.view(np.uint32) if words.dtype != np.uint32 else words
        self.n, self.pre = words.size, GUARD + shift
        host = np.full(self.pre + self.n + GUARD, GUARD_WORD, np.uint32)
        host[self.pre:self.pre + self.n] = words
        self.t = torch.from_numpy(host.view(np.int32)).to(dev)

    @property
    def ptr(self):
        return self.t.data_ptr() + 4 * self.pre

    def read(self):
        """-> the payload as uint32, after checking both guards"""
        h = self.t.cpu().numpy().view(np.uint32)
        assert np.all(h[:self.pre] == GUARD_WORD), "the words before the buffer were written"
        assert np.all(h[self.pre + self.n:] == GUARD_WORD), "the words after the buffer were written"
        return h[self.pre:self.pre + self.n].copy()


def out_buf(dev, n, shift=0):
    return Buf(dev, np.full(n, GUARD_WORD, np.uint32), shift)


def same_bits(got, want, what):
    want = np.ascontiguousarray(want).reshape(-1)
    want = want.view(np.uint32) if want.dtype != np.uint32 else want
    bad = np.nonzero(got != want)[0]
    assert bad.size == 0, "%s: %d of %d words differ, first at %d: got 0x%08x want 0x%08x" % (
        what, bad.size, got.size, bad[0], got[bad[0]], want[bad[0]])


# ------------------------------------------------------------------------------------------------------------------
# transpose
# ------------------------------------------------------------------------------------------------------------------
SIZES = (1, 31, 32, 33, 65)
ALPHAS = (1.0, 0.5, float(np.sqrt(F(0.5))))


@pytest.mark.parametrize("with_add", [False, True])
@pytest.mark.parametrize("B", [1, 3])
def test_transpose(dev, B, with_add):
    ops, L = _env()
    for R in SIZES:
        for C in SIZES:
            for alpha in ALPHAS:
                seed = R * 131 + C * 7 + B
                move = alpha == 1.0 and not with_add
                x = patterns(B * R * C, seed, signalling=False) if move else finite(B * R * C, seed).view(np.uint32)
                add = finite(B * R * C, seed + 1) if with_add else None
                xb, yb = Buf(dev, x), out_buf(dev, B * R * C)
                ab = Buf(dev, add) if with_add else None
                ops._lib.call("dv3_transpose_f32", xb.ptr, yb.ptr, ab.ptr if ab else None, B, R, C, float(alpha), ops._stream())
                torch.cuda.synchronize()
                if move:
                    want = x.reshape(B, R, C).transpose(0, 2, 1)
                else:
                    want = F(alpha) * x.view(F).reshape(B, R, C).transpose(0, 2, 1)            # rounded
                    if with_add:
                        want = want + add.reshape(B, C, R)                                        # rounded again
                what = "transpose B=%d R=%d C=%d alpha=%r add=%s" % (B, R, C, alpha, with_add)
                same_bits(yb.read(), np.ascontiguousarray(want), what)
                same_bits(xb.read(), x, what + ": the input")
                # the wrapper: the same bits
                xt = xb.t[xb.pre:xb.pre + xb.n].view(torch.float32).reshape(B, R, C)
                at = ab.t[ab.pre:ab.pre + ab.n].view(torch.float32).reshape(B, C, R) if ab else None
                y = ops.transpose(xt, at, alpha)
                assert y.shape == (B, C, R)
                same_bits(y.cpu().numpy().view(np.uint32).reshape(-1), np.ascontiguousarray(want), what + " (ops)")


# ------------------------------------------------------------------------------------------------------------------
# axpby, scaled_copy, sum_scalars
# ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("with_b", [False, True])
@pytest.mark.parametrize("n", [1, 255, 256, 257, 4096 * 256 + 257])
def test_axpby(dev, n, with_b):
    ops, L = _env()
    for alpha in ALPHAS:
        a, b = finite(n, n), (finite(n, n + 1) if with_b else None)
        ab_, bb, ob = Buf(dev, a), (Buf(dev, b) if with_b else None), out_buf(dev, n)
        ops._lib.call("dv3_axpby_f32", ab_.ptr, bb.ptr if bb else None, ob.ptr, n, float(alpha), ops._stream())
        torch.cuda.synchronize()
        want = F(alpha) * (a + (b if with_b else F(0)))
        same_bits(ob.read(), want, "axpby n=%d alpha=%r b=%s" % (n, alpha, with_b))
        at = ab_.t[ab_.pre:ab_.pre + n].view(torch.float32)
        if with_b:
            got = ops.axpby(at, bb.t[bb.pre:bb.pre + n].view(torch.float32), alpha)
        else:
            got = ops.scaled_copy(at, alpha)
        same_bits(got.cpu().numpy().view(np.uint32), want, "ops n=%d alpha=%r b=%s" % (n, alpha, with_b))


@pytest.mark.parametrize("k", [2, 3, 4])
def test_sum_scalars(dev, k):
    ops, L = _env()
    for seed in range(8):
        v = finite(4, 900 + seed, scale_pow=6)
        bufs = [Buf(dev, v[i:i + 1]) for i in range(k)]
        ob = out_buf(dev, 1)
        ptrs = [b.ptr for b in bufs] + [None] * (4 - k)
        ops._lib.call("dv3_sum_scalars_f32", ptrs[0], ptrs[1], ptrs[2], ptrs[3], ob.ptr, ops._stream())
        torch.cuda.synchronize()
        want = v[0] + v[1]
        for i in range(2, k):
            want = F(want + v[i])
        same_bits(ob.read(), np.array([want], F), "sum_scalars k=%d" % k)
        ts = [b.t[b.pre:b.pre + 1].view(torch.float32) for b in bufs] + [None] * (4 - k)
        same_bits(ops.sum_scalars(*ts).cpu().numpy().view(np.uint32), np.array([want], F), "ops.sum_scalars k=%d" % k)


# ------------------------------------------------------------------------------------------------------------------
# dropout_apply
# ------------------------------------------------------------------------------------------------------------------
def _bits_with_stride(bits, rows, rs, rs2, seed):
    """mask words [rows][rs] -> [rows][rs2] with random words in the surplus columns"""
    out = patterns(rows * rs2, seed).reshape(rows, rs2)
    out[:, :rs] = bits.reshape(rows, rs)
    return out


@pytest.mark.parametrize("rows", [1, 4, 5])
@pytest.mark.parametrize("T", [1, 31, 32, 33, 64, 65, 130])
def test_dropout_apply(dev, T, rows):
    ops, L = _env()
    rs = (T + 31) // 32
    masks = []
    saved = (ops.dropout_state.seed, ops.dropout_state.site)
    try:
        for p in (0.05, 0.5):
            ops.dropout_state.manual_seed(4000 + T * 8 + rows)
            bits, rs_ = ops.dropout_bits(rows, T, p, dev)
            assert rs_ == rs
            masks.append((bits.cpu().numpy().view(np.uint32), F(1.0 / (1.0 - p))))
    finally:
        ops.dropout_state.seed, ops.dropout_state.site = saved
    masks.append((np.full(rows * rs, 0xffffffff, np.uint32), F(1.0)))
    masks.append((np.zeros(rows * rs, np.uint32), F(1.0)))
    for m, (bits, scale) in enumerate(masks):
        for rs2 in (rs, rs + 2):
            keep = O.unpack_keep_bits(bits, rows, rs, T)
            for sc in (F(1.0), scale):
                move = sc == 1.0
                x = patterns(rows * T, T + rows + m, signalling=False) if move else finite(rows * T, T + rows + m).view(np.uint32)
                xb, ob = Buf(dev, x), out_buf(dev, rows * T)
                bb = Buf(dev, _bits_with_stride(bits, rows, rs, rs2, m))
                ops._lib.call("dv3_dropout_apply_f32", xb.ptr, bb.ptr, rs2, float(sc), ob.ptr, rows, T, ops._stream())
                torch.cuda.synchronize()
                if move:
                    want = np.where(keep.reshape(-1), x, np.uint32(0))
                else:
                    want = np.where(keep.reshape(-1), x.view(F) * sc, F(0)).astype(F)
                same_bits(ob.read(), want, "dropout_apply T=%d rows=%d mask %d bits_rs=%d scale=%r" % (T, rows, m, rs2, float(sc)))


# ------------------------------------------------------------------------------------------------------------------
# deinterleave2
# ------------------------------------------------------------------------------------------------------------------
def _deinterleave(dev, x, B, Oc, T, shift_in, shift_out):
    """-> (output words, whether the host's condition selects the 16-byte kernel)"""
    ops, L = _env()
    xb, ob = Buf(dev, x, shift_in), out_buf(dev, B * 2 * Oc * T, shift_out)
    vec = T % 2 == 0 and ((xb.ptr | ob.ptr) & 15) == 0           # the condition of dv3_deinterleave2_f32, restated
    ops._lib.call("dv3_deinterleave2_f32", xb.ptr, ob.ptr, B, Oc, T, ops._stream())
    torch.cuda.synchronize()
    same_bits(xb.read(), x, "deinterleave2: the input")
    return ob.read(), vec


@pytest.mark.parametrize("B", [1, 2])
@pytest.mark.parametrize("Oc", [1, 3, 80])
def test_deinterleave2(dev, Oc, B):
    assert GUARD % 4 == 0                 # torch allocations are 16-byte aligned: shift 0 keeps the payload so
    for T in (1, 2, 3, 4, 6, 129, 130):
        x = patterns(B * Oc * 2 * T, Oc * 1000 + T + B)
        want = x.reshape(B, Oc, T, 2).transpose(0, 3, 1, 2)          # out[b][j][o][t] = dy[b][o][2 t + j]
        got, vec = _deinterleave(dev, x, B, Oc, T, 0, 0)
        assert vec == (T % 2 == 0), "T=%d: the aligned call must take the %s kernel" % (T, "16-byte" if T % 2 == 0 else "scalar")
        same_bits(got, np.ascontiguousarray(want), "deinterleave2 B=%d O=%d T=%d (%s)" % (B, Oc, T, "16-byte" if vec else "scalar"))
        if T % 2 == 0:
            for si, so in ((1, 0), (0, 1), (1, 1)):
                got2, vec2 = _deinterleave(dev, x, B, Oc, T, si, so)
                assert not vec2, "a pointer one element off 16-byte alignment must take the scalar kernel"
                same_bits(got2, got, "deinterleave2 B=%d O=%d T=%d: scalar kernel (input +%d, output +%d) against the 16-byte one" % (B, Oc, T, si, so))


# ------------------------------------------------------------------------------------------------------------------
# shift_append
# ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("x_stride", [1, 7])
@pytest.mark.parametrize("rows", [1, 4, 5, 9])
def test_shift_append_three_steps(dev, rows, x_stride):
    """the decode loop's use: three steps in succession; L > 64 takes the kernel's second pass, where lane 63 of the first
    pass must have read element 64 before the second pass overwrites it"""
    ops, L_ = _env()
    for L in (1, 2, 3, 63, 64, 65, 128, 130):
        buf = patterns(rows * L, rows * 977 + L)
        bb = Buf(dev, buf)
        want = buf.reshape(rows, L).copy()
        for step in range(3):
            x = patterns(rows * x_stride, rows + L + step)
            xb = Buf(dev, x)
            ops._lib.call("dv3_shift_append_f32", bb.ptr, xb.ptr, rows, L, x_stride, ops._stream())
            torch.cuda.synchronize()
            want = np.concatenate([want[:, 1:], x[::x_stride][:rows, None]], axis=1)
            same_bits(bb.read(), np.ascontiguousarray(want), "shift_append rows=%d L=%d x_stride=%d step %d" % (rows, L, x_stride, step))
            same_bits(xb.read(), x, "shift_append: x")


# ------------------------------------------------------------------------------------------------------------------
# zero tails
# ------------------------------------------------------------------------------------------------------------------
def _lengths(T, mult):
    top = T // mult
    return sorted(set(l for l in (0, 1, top - 1, top) if 0 <= l <= top))


@pytest.mark.parametrize("mult", [1, 4])
@pytest.mark.parametrize("words", [1, 4])
def test_zero_tail_items(dev, words, mult):
    """per item: columns t >= len[b] * mult of the item's rows to zero words, every other word untouched; lengths 0, 1,
    T / mult - 1 and T / mult, one item each; max_tail the exact promise and a larger one (clamped to T by the host)"""
    ops, L = _env()
    for T in (1, 3, 4, 5, 8, 63, 64, 65, 257):
        lens = _lengths(T, mult)
        B = len(lens)
        for rpi in (1, 3):
            x = patterns(B * rpi * T * words, T * 31 + words + mult + rpi)
            x = np.where(x == 0, np.uint32(1), x)                      # a zero word in the input would hide a missed write
            col = np.arange(T)[None, None, :, None]
            lim = (np.array(lens) * mult)[:, None, None, None]
            want = np.where(col >= lim, np.uint32(0), x.reshape(B, rpi, T, words))
            lb = torch.tensor(lens, dtype=torch.int32, device=dev)
            for max_tail in (T - min(lens) * mult, T + 5):
                xb = Buf(dev, x)
                ops._lib.call("dv3_zero_tail_items_b32", xb.ptr, B, rpi, T, words, lb.data_ptr(), mult, max_tail, ops._stream())
                torch.cuda.synchronize()
                same_bits(xb.read(), np.ascontiguousarray(want), "zero_tail_items T=%d words=%d mult=%d rows/item=%d max_tail=%d" % (
                    T, words, mult, rpi, max_tail))
            # a promise of zero surplus columns launches nothing
            xb = Buf(dev, x)
            ops._lib.call("dv3_zero_tail_items_b32", xb.ptr, B, rpi, T, words, lb.data_ptr(), mult, 0, ops._stream())
            torch.cuda.synchronize()
            same_bits(xb.read(), x, "zero_tail_items max_tail = 0")


@pytest.mark.parametrize("mult", [1, 4])
@pytest.mark.parametrize("D", [1, 4, 5])
def test_zero_frames(dev, D, mult):
    """ops.zero_frames: x (B, T, D) in place, frames t >= lengths[b] * mult to zero"""
    ops, L = _env()
    for T in (1, 4, 5, 64, 65):
        lens = _lengths(T, mult)
        B = len(lens)
        x = patterns(B * T * D, T * 17 + D + mult)
        x = np.where(x == 0, np.uint32(1), x)
        xb = Buf(dev, x)
        xt = xb.t[xb.pre:xb.pre + xb.n].view(torch.float32).reshape(B, T, D)
        lb = torch.tensor(lens, dtype=torch.int32, device=dev)
        ret = ops.zero_frames(xt, lb, min(lens), mult)
        torch.cuda.synchronize()
        assert ret.data_ptr() == xt.data_ptr()
        lim = (np.array(lens) * mult)[:, None, None]
        want = np.where(np.arange(T)[None, :, None] >= lim, np.uint32(0), x.reshape(B, T, D))
        same_bits(xb.read(), np.ascontiguousarray(want), "zero_frames T=%d D=%d mult=%d" % (T, D, mult))


@pytest.mark.parametrize("words", [1, 4])
def test_zero_tail_of_the_batch(dev, words):
    """dv3_zero_tail_b32: one device scalar for every row"""
    ops, L = _env()
    for T in (1, 5, 64, 65):
        for mult in (1, 4):
            for tv in _lengths(T, mult):
                rows = 5
                x = patterns(rows * T * words, T + words + tv)
                x = np.where(x == 0, np.uint32(1), x)
                xb = Buf(dev, x)
                tvb = torch.tensor([tv], dtype=torch.int32, device=dev)
                ops._lib.call("dv3_zero_tail_b32", xb.ptr, rows, T, words, tvb.data_ptr(), mult, T - tv * mult, ops._stream())
                torch.cuda.synchronize()
                want = np.where(np.arange(T)[None, :, None] >= tv * mult, np.uint32(0), x.reshape(rows, T, words))
                same_bits(xb.read(), np.ascontiguousarray(want), "zero_tail T=%d words=%d mult=%d t_valid=%d" % (T, words, mult, tv))


# ------------------------------------------------------------------------------------------------------------------
# the head of a c8 tensor as fp32 (the per-frame speaker-bias gradient of the per-layer path)
# ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("C,c8p", [(1, 1), (7, 2), (8, 2), (9, 3), (40, 10)])
def test_from_c8_head(dev, C, c8p):
    """dv3_from_c8_head_f32: out[b][c][t] = the fp32 value of bf16 word x[b][c >> 3][t][c & 7], c < C, of a tensor with c8p
    groups per item: a pure move of 16 bits into the upper half of a word (random bf16 patterns, specials included)"""
    ops, L = _env()
    for B in (1, 3):
        for T in (1, 5, 64, 65):
            w = (patterns(B * c8p * T * 8, C * 100 + T + B) >> 16).astype(np.uint16)
            xb = Buf(dev, np.ascontiguousarray(w).view(np.uint32))
            ob = out_buf(dev, B * C * T)
            ops._lib.call("dv3_from_c8_head_f32", xb.ptr, c8p, ob.ptr, C * T, T, B, C, T, ops._stream())
            torch.cuda.synchronize()
            full = w.reshape(B, c8p, T, 8).transpose(0, 1, 3, 2).reshape(B, c8p * 8, T)
            want = full[:, :C].astype(np.uint32) << 16
            same_bits(ob.read(), np.ascontiguousarray(want), "from_c8_head B=%d C=%d c8p=%d T=%d" % (B, C, c8p, T))

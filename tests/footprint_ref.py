# coding: utf-8
"""Placements and guard bands for the GEMM kernels' memory footprint (host code; runs on CPU tensors too).

A PLACEMENT puts a logical fp32 tensor -- (B, R, T) activations, or weight-gradient slabs [S][J][M][Cin] /
[J][M][S][Cin] with row stride ldo -- inside a larger flat fp32 buffer the test owns.  Every word of the buffer that is
not a logical element holds SENTINEL = 0x7fc0dead, the quiet NaN of tests/test_gpu_layout_kernels.py: as POISON around
an input it propagates through any arithmetic that touches it (a load that is multiplied by a zero mask instead of
selected shows as a NaN in the output), as a GUARD around an output no kernel here can produce it, so a word that no
longer holds it was stored to.

    name        base pointer                         row stride                 batch stride
    banded      16-byte aligned                      T                          R T   (dense: bands before / after only)
    strided4    16-byte aligned                      T + p, rs % 4 == 0         R rs + 4 q  (bs % 4 == 0)
    strided1    16-byte aligned                      rs % 4 == 1                bs % 4 != 0
    offset1..3  1, 2, 3 floats past such a boundary  dense                      dense

Slabs take the same names: the row stride is ldo = Cin (banded, offset*), the next multiple of four above Cin + 4
(strided4: ldo % 4 == 0, at least four floats of slack) or the first ldo > Cin with ldo % 4 == 1 (strided1); the outer
strides are those ops.wgrad_gemm derives from ldo (the kernels take one slab stride and one row stride, nothing else).

BAND RULE: the bands before and after the tensor hold at least 256 * row_stride + 256 elements each -- one whole
256-row tile of the widest kernel plus a 256-column tile -- so a store that is wrong by a whole tile still lands inside
the test's own allocation, where violations() finds it, and not in a neighbouring tensor of the allocator.

place(t, placement, device) -> (buf, view); violations(buf, layout) -> the non-logical words that changed, each with the
band or gap it lies in, the nearest logical element and the distance to it; poisoned(view) / unwritten(view) say whether
a NaN or the sentinel sits in a logical output.  tests/test_cpu_footprint_ref.py proves what these catch.
"""
import numpy as np
import torch

SENTINEL = 0x7fc0dead
PLACEMENTS = ("banded", "strided4", "strided1", "offset1", "offset2", "offset3")
BAND_ROWS, BAND_EXTRA = 256, 256
_NAMES3 = ("b", "row", "t")


def band_elems(row_stride):
    """the band rule (module docstring)"""
    return BAND_ROWS * int(row_stride) + BAND_EXTRA


def strides3(shape, placement):
    """(bs, rs) of a (B, R, T) tensor under `placement`, in elements (the table of the module docstring)"""
    B, R, T = shape
    if placement == "strided4":
        rs = (T + 4) // 4 * 4 + 4                 # p = 5 .. 8: rs % 4 == 0, at least five floats of gap
        return R * rs + 8, rs                     # q = 2
    if placement == "strided1":
        rs = T + 1
        while rs % 4 != 1:
            rs += 1
        bs = R * rs + 1
        while bs % 4 == 0:
            bs += 1
        return bs, rs
    assert placement == "banded" or placement in ("offset1", "offset2", "offset3"), placement
    return R * T, T


def slab_ldo(Cin, placement):
    """row stride of weight-gradient slabs under `placement`"""
    if placement == "strided4":
        return (Cin + 4) // 4 * 4 + 4
    if placement == "strided1":
        ldo = Cin + 1
        while ldo % 4 != 1:
            ldo += 1
        return ldo
    return Cin


def base_offset(placement):
    return int(placement[6:]) if placement.startswith("offset") else 0


class Layout(object):
    """where the logical elements of one placed tensor lie in its flat buffer: element (i0, i1, ...) at
    base + sum(i_k * strides[k]), all in fp32 elements"""

    def __init__(self, shape, strides, base, n, placement, names=None):
        self.shape, self.strides = tuple(int(v) for v in shape), tuple(int(v) for v in strides)
        self.base, self.n, self.placement = int(base), int(n), placement
        self.names = tuple(names) if names is not None else (_NAMES3 if len(self.shape) == 3 else
                                                                tuple("i%d" % k for k in range(len(self.shape))))
        self.sentinel, self.int_dtype = SENTINEL, torch.int32        # place_c8: 16-bit elements
        self._offsets = None
        self._mask = {}

    @property
    def row_stride(self):
        return self.strides[-2]

    @property
    def span(self):
        """elements from the first logical element to one past the last"""
        return sum((s - 1) * st for s, st in zip(self.shape, self.strides)) + 1

    def offsets(self):
        """flat offsets of the logical elements, in logical (row-major) order, int64 numpy"""
        if self._offsets is None:
            off = np.zeros((), np.int64) + self.base
            for s, st in zip(self.shape, self.strides):
                off = off[..., None] + np.arange(s, dtype=np.int64) * st
            self._offsets = off.reshape(-1)
        return self._offsets

    def guard_mask(self, device):
        """bool [n] on `device`: True at every non-logical word"""
        key = str(device)
        if key not in self._mask:
            m = torch.ones(self.n, dtype=torch.bool)
            m[torch.from_numpy(self.offsets())] = False
            self._mask[key] = m.to(device)
        return self._mask[key]

    def view(self, buf):
        return torch.as_strided(buf, self.shape, self.strides, self.base)


def _make(shape, strides, placement, device, names=None):
    """allocate the sentinel-filled buffer and fix the base so that it sits base_offset(placement) floats past a 16-byte
    boundary of the ACTUAL address"""
    span = sum((s - 1) * st for s, st in zip(shape, strides)) + 1
    band = band_elems(strides[-2])
    n = band + 4 + span + band + 4
    buf = torch.full((n,), SENTINEL, dtype=torch.int32, device=device).view(torch.float32)
    word = buf.data_ptr() // 4
    assert buf.data_ptr() % 4 == 0
    base = band + (-(word + band)) % 4 + base_offset(placement)
    return buf, Layout(shape, strides, base, n, placement, names)


def place(t, placement, device):
    """t: an fp32 (B, R, T) tensor / array (an INPUT: its values are written into the view, everything around them is
    poison) or a shape (an OUTPUT: the whole buffer holds the sentinel).  -> (buf, view); buf.fp_layout is the Layout."""
    shape = tuple(t) if isinstance(t, (tuple, list, torch.Size)) else tuple(t.shape)
    assert len(shape) == 3, shape
    bs, rs = strides3(shape, placement)
    buf, lay = _make(shape, (bs, rs, 1), placement, device)
    buf.fp_layout = lay
    view = lay.view(buf)
    if not isinstance(t, (tuple, list, torch.Size)):
        src = torch.from_numpy(np.ascontiguousarray(t)) if isinstance(t, np.ndarray) else t
        assert src.dtype == torch.float32, src.dtype
        view.copy_(src.to(device))
    return buf, view


def place_slabs(S, J, M, Cin, placement, device, rows_of_slabs=False):
    """the output of ops.wgrad_gemm under `placement`: -> (buf, view (S, J, M, ldo) or (J, M, S, ldo) as the kernel is
    handed it, ldo); the LOGICAL elements are the first Cin of every row (buf.fp_layout)"""
    ldo = slab_ldo(Cin, placement)
    if rows_of_slabs:
        shape, names = (J, M, S, Cin), ("j", "m", "s", "c")
        strides = (M * S * ldo, S * ldo, ldo, 1)
    else:
        shape, names = (S, J, M, Cin), ("s", "j", "m", "c")
        strides = (J * M * ldo, M * ldo, ldo, 1)
    buf, lay = _make(shape, strides, placement, device, names)
    buf.fp_layout = lay
    return buf, lay.view(buf), ldo


class Violation(object):
    """one non-logical word that no longer holds the sentinel"""
    __slots__ = ("offset", "where", "nearest", "distance", "bits", "names")

    def __init__(self, offset, where, nearest, distance, bits, names):
        self.offset, self.where, self.nearest, self.distance, self.bits, self.names = offset, where, nearest, distance, bits, names

    def __repr__(self):
        at = ", ".join("%s=%d" % (n, v) for n, v in zip(self.names, self.nearest))
        return "word %d (%s) holds 0x%08x: %+d elements from logical (%s)" % (self.offset, self.where, self.bits, self.distance, at)


def violations(buf, layout=None):
    """-> [Violation]: every non-logical word of `buf` whose int32 bits differ from SENTINEL (the comparison is made
    where the buffer lives; only the offending offsets travel to the host).  where: "band before" / "band after" / "gap
    between <axis> items" (the outermost axis on which the two logical neighbours differ: "row" = the slack of a padded
    row stride, "b" = the batch gap); nearest: the closest logical element, distance: offset - its offset (negative =
    the stray word lies before it)."""
    lay = layout if layout is not None else buf.fp_layout
    words = buf.view(lay.int_dtype)
    assert words.numel() == lay.n, (words.numel(), lay.n)
    bad = ((words != lay.sentinel) & lay.guard_mask(buf.device)).nonzero().reshape(-1)
    if bad.numel() == 0:
        return []
    off = bad.cpu().numpy().astype(np.int64)
    bits = words[bad].cpu().numpy().astype(np.int64) & (0xffffffff if lay.int_dtype == torch.int32 else 0xffff)
    logical = lay.offsets()
    order = np.argsort(logical, kind="stable")
    srt = logical[order]
    hi = np.searchsorted(srt, off)                            # first logical offset above the word
    lo = hi - 1
    out = []
    for k in range(off.size):
        o = int(off[k])
        if lo[k] < 0:
            where, near = "band before", int(order[0])
        elif hi[k] >= srt.size:
            where, near = "band after", int(order[-1])
        else:
            a, b = int(order[lo[k]]), int(order[hi[k]])
            ca, cb = np.unravel_index(a, lay.shape), np.unravel_index(b, lay.shape)
            axis = next(i for i in range(len(lay.shape)) if ca[i] != cb[i])
            where = "gap between %s items" % lay.names[axis]
            near = a if o - int(logical[a]) <= int(logical[b]) - o else b
        coords = tuple(int(v) for v in np.unravel_index(near, lay.shape))
        out.append(Violation(o, where, coords, o - int(logical[near]), int(bits[k]), lay.names))
    return out


C8_SENTINEL = SENTINEL >> 16          # 0x7fc0: the sentinel's upper half, a quiet NaN as bf16 -- every ELEMENT around a c8 tensor


def place_c8(bits, C, device):
    """A c8 tensor (include/dv3hip.h: bf16 [B][round_up(C, 32) / 8][T][8]; dense only, 16-byte aligned) inside a buffer of
    16-bit sentinels.  bits: its uint16 image (gemm_split_ref.c8_pack) -- an input -- or the shape (B, G, T, 8) of an output,
    whose valid groups then hold the sentinel and whose groups from the first one with a padding channel on are zero, as the
    format requires of a tensor handed to a kernel (the kernels keep the padding zero, they do not write it).
    -> (buf int16, view bf16 (B, G, T, 8)); the band rule with one group row (8 T elements) as the row."""
    shape = tuple(bits) if isinstance(bits, (tuple, list)) else tuple(bits.shape)
    B, G, T, e = shape
    assert e == 8 and G == (C + 31) // 32 * 4, (shape, C)
    band = band_elems(8 * T)
    numel = B * G * T * 8
    n = band + 8 + numel + band + 8
    buf = torch.full((n,), C8_SENTINEL, dtype=torch.int16, device=device)
    assert buf.data_ptr() % 2 == 0
    base = band + (-(buf.data_ptr() // 2 + band)) % 8
    lay = Layout(shape, (G * T * 8, T * 8, 8, 1), base, n, "banded", ("b", "group", "t", "e"))
    lay.sentinel, lay.int_dtype = C8_SENTINEL, torch.int16
    buf.fp_layout = lay
    view16 = lay.view(buf)
    if isinstance(bits, (tuple, list)):
        if C % 32:
            view16[:, C // 8:] = 0
    else:
        view16.copy_(torch.from_numpy(np.ascontiguousarray(bits).view(np.int16)).to(device))
    view = view16.view(torch.bfloat16)
    assert view.data_ptr() % 16 == 0 and view.is_contiguous()
    return buf, view


def describe(viol, limit=6):
    return "%d stray words: %s%s" % (len(viol), "; ".join(repr(v) for v in viol[:limit]), " ..." if len(viol) > limit else "")


def poisoned(view):
    """did a NaN reach a logical output?"""
    return bool(torch.isnan(view).any())


def unwritten(view):
    """how many logical words still hold the sentinel (an output element the kernel never stored)"""
    return int((view.contiguous().view(torch.int32) == SENTINEL).sum())

# coding: utf-8
"""-m gpu: the dropout masks, every form, BIT FOR BIT against the independent Philox4x32-10 of tests/philox_ref.py (itself
pinned to the published known answers by tests/test_cpu_philox_ref.py).  No tolerance anywhere: whole buffers are compared
with np.array_equal.  Every output is prefilled with 0xA5 bytes (the keep-byte forms a second time with 0x5A, so that an
unwritten byte can not pass for a drawn one) and stands between guard bytes that must come back unchanged.

  dv3_dropout_bits           one thread per word, 256 per block: 1, 255, 256, 257, 1025 words; every threshold edge of
                             thr = trunc(p 65536 + 0.5); seeds and sites with high words; the device step offset with the
                             carry into the high key word, the wrap mod 2^64 and a negative int64
  dv3_dropout_keep_c8,       one thread per (entry, channel), 32 entries (b, group, 32-frame word) per block, a byte tail at
  dv3_dropout_bits_keep      T % 32 and T % 4: pad channels of the last group, whole pad groups (written, zero), nothing past
                             byte T of a row; the bits form [B*C][ceil(T/32)] with the bits past T drawn like any others
  dv3_dropout_keep_c8_multi  the six sites of tests/test_gpu_model.py and a table of exactly DV3_DROPOUT_MULTI_MAX sites
                             (keep, both, bits-only; one block and several); MAX + 1 sites: DV3_EINVAL, nothing written
  ops                        the k-th call after dropout_state.manual_seed takes site k in all three wrappers; a plan of 50
                             signatures is drawn in 2 launches and every planned mask is the reference's

Not covered: the high word of the WORD counter (c1) is non-zero only beyond 2^30 mask words (4 GiB of mask), and the entry
points take no word offset, so no test-sized call reaches it; the reference's own c1 handling is pinned by the known-answer
vectors on the CPU."""
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tests import philox_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu

GUARD = 64                                   # bytes on either side
FILL = 0xA5
U64 = 1 << 64
P_EDGES = [0.0, 1e-5, 0.3, 100.5 / 65536, (100.5 - 2.0 ** -10) / 65536, 0.99999, 1 - 2.0 ** -24]
SEED_SITE = [(0, 0), (777, 1), (2 ** 32 - 1, 1), (2 ** 32, 2 ** 32 + 3), (2 ** 64 - 1, 2 ** 64 - 1)]


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


def _env():
    from deepvoice3_pytorch_amd import ops, _lib
    return ops, _lib


class Out(object):
    """a device output of n bytes between two guards, all of it prefilled: [GUARD][n][GUARD] bytes of `fill`"""

    def __init__(self, dev, n, fill=FILL):
        self.n, self.fill = int(n), fill
        self.t = torch.full((GUARD + self.n + GUARD,), fill, dtype=torch.uint8, device=dev)

    @property
    def ptr(self):
        return self.t.data_ptr() + GUARD

    def read(self, dtype=np.uint8):
        """-> the payload, after checking both guards"""
        h = self.t.cpu().numpy()
        assert np.all(h[:GUARD] == self.fill), "the bytes before the buffer were written"
        assert np.all(h[GUARD + self.n:] == self.fill), "the bytes after the buffer were written"
        return h[GUARD:GUARD + self.n].copy().view(dtype)

    def untouched(self):
        return bool(np.all(self.t.cpu().numpy() == self.fill))


def _offset(dev, value):
    """a device step counter holding `value` mod 2^64 (stored as the int64 of the same bits), or None"""
    if value is None:
        return None
    v = int(value) % U64
    return torch.tensor([v - U64 if v >= 1 << 63 else v], dtype=torch.int64, device=dev)


def _p(t):
    return t.data_ptr() if t is not None else None


def same(got, want, what):
    want = np.ascontiguousarray(want).reshape(-1)
    assert got.dtype == want.dtype and got.shape == want.shape, (what, got.shape, want.shape)
    if not np.array_equal(got, want):
        bad = np.nonzero(got != want)[0]
        raise AssertionError("%s: %d of %d differ, first at %d: got 0x%x want 0x%x" % (
            what, bad.size, got.size, bad[0], got[bad[0]], want[bad[0]]))


# ------------------------------------------------------------------------------------------------------------------
# dv3_dropout_bits
# ------------------------------------------------------------------------------------------------------------------
def draw_bits(dev, n_words, p, seed, site, offset=None):
    ops, _lib = _env()
    out, off = Out(dev, 4 * n_words), _offset(dev, offset)
    _lib.call("dv3_dropout_bits", out.ptr, n_words, float(p), seed, site, _p(off), ops._stream())
    return out.read(np.uint32)


@pytest.mark.parametrize("p", P_EDGES)
def test_bits_sizes_seeds_sites_and_threshold_edges(dev, p):
    thr = R.threshold(p)
    for n_words in (1, 255, 256, 257, 1025):
        for seed, site in SEED_SITE:
            got = draw_bits(dev, n_words, p, seed, site)
            same(got, R.keep_words(n_words, p, seed, site), "p %r n %d seed %d site %d" % (p, n_words, seed, site))
            if thr == 0:
                assert np.all(got == 0xFFFFFFFF)
            if thr == 65536:
                assert np.all(got == 0)


OFFSETS = [                                   # (seed, the device word; None = a NULL pointer)
    (777, None), (777, 0), (777, 1), (777, 12345),
    (2 ** 32 - 1, 1),                         # the carry into the high key word
    (2 ** 64 - 1, 2),                         # wraps mod 2^64
    (777, -3),                                # a negative int64 is the uint64 of the same bits
    (5, -(2 ** 63)), (2 ** 40 + 17, 2 ** 33 + 5),
]


@pytest.mark.parametrize("seed,offset", OFFSETS)
def test_bits_device_step_offset(dev, seed, offset):
    for p in (0.3, 0.05):
        for n_words in (257, 1025):
            got = draw_bits(dev, n_words, p, seed, 2 ** 32 + 3, offset)
            same(got, R.keep_words(n_words, p, seed, 2 ** 32 + 3, offset or 0), "seed %d offset %r" % (seed, offset))


def test_bits_offset_k_draws_the_masks_of_seed_plus_k(dev):
    for seed, k in ((777, 1), (777, 12345), (2 ** 32 - 1, 1), (2 ** 32 - 7, 2 ** 32 + 9)):
        a = draw_bits(dev, 1025, 0.3, seed, 4, k)
        same(a, draw_bits(dev, 1025, 0.3, seed + k, 4), "device: seed %d offset %d" % (seed, k))
        same(a, R.keep_words(1025, 0.3, seed + k, 4, 0), "reference: seed %d offset %d" % (seed, k))
    assert not np.array_equal(draw_bits(dev, 1025, 0.3, 777, 4, 1), draw_bits(dev, 1025, 0.3, 777, 4, 2))
    assert not np.array_equal(draw_bits(dev, 1025, 0.3, 777, 4, 2 ** 32), draw_bits(dev, 1025, 0.3, 777, 4))


def test_bits_sites_differ(dev):
    """sites 1 and 2 of one step, and two sites that differ in the high word only: different masks, each the reference's,
    and agreeing in about q^2 + (1 - q)^2 of the decisions as independent masks do (p = 0.5, 32800 decisions: 6 sigma)"""
    n, p = 1025, 0.5
    m = {site: draw_bits(dev, n, p, 777, site) for site in (1, 2, 2 ** 32 + 1)}
    for site, got in m.items():
        same(got, R.keep_words(n, p, 777, site), "site %d" % site)
    for a, b in ((1, 2), (1, 2 ** 32 + 1)):
        assert not np.array_equal(m[a], m[b])
        agree = 32 * n - int(np.unpackbits((m[a] ^ m[b]).view(np.uint8)).sum())
        assert abs(agree - 16 * n) <= 6 * np.sqrt(8 * n), (a, b, agree)


# ------------------------------------------------------------------------------------------------------------------
# dv3_dropout_keep_c8 and dv3_dropout_bits_keep
# ------------------------------------------------------------------------------------------------------------------
SHAPES = [(1, 8, 1), (2, 3, 70), (3, 40, 37), (1, 37, 130), (2, 513, 33), (4, 256, 32), (1, 64, 31)]
# per shape a stream of its own: high words in seed and site, offsets with and without the carry
STREAM = [(777, 1, None), (2 ** 32 - 1, 2, 1), (2 ** 32, 2 ** 32 + 3, 12345), (2 ** 64 - 1, 2 ** 64 - 1, 2), (0, 0, 0),
          (12345678901234567, 7, -3), (777, 2 ** 40, 2 ** 33)]


def _groups(C):
    return (C + 31) // 32 * 4


def check_keep(got, B, C, T, want, what):
    """the keep bytes against the reference, and what the reference's zeros mean, spelled out"""
    same(got, want, what)
    g = got.reshape(B, _groups(C), T)
    full, rest = C // 8, C % 8
    assert not g[:, full + (1 if rest else 0):].any(), "%s: a pad group is not zero" % what
    if rest:
        assert not (g[:, full] >> rest).any(), "%s: a pad channel of the last group is kept" % what


@pytest.mark.parametrize("p", [0.3, 0.05, 0.0])
@pytest.mark.parametrize("case", range(len(SHAPES)))
def test_keep_c8(dev, case, p):
    ops, _lib = _env()
    (B, C, T), (seed, site, offset) = SHAPES[case], STREAM[case]
    want = R.keep_bytes(B, C, T, p, seed, site, offset or 0)
    assert want.shape == (B, _groups(C), T)
    for fill in (FILL, 0x5A):
        out, off = Out(dev, B * _groups(C) * T, fill), _offset(dev, offset)
        _lib.call("dv3_dropout_keep_c8", out.ptr, B, C, T, float(p), seed, site, _p(off), ops._stream())
        check_keep(out.read(), B, C, T, want, "keep_c8 %r p %r fill %x" % ((B, C, T), p, fill))
    if p == 0.0:                              # everything kept: every real channel's bit set, frame by frame
        chans = np.unpackbits(want.reshape(B, _groups(C), 1, T), axis=2, bitorder="little").reshape(B, -1, T)
        assert chans[:, :C].all() and not chans[:, C:].any()


@pytest.mark.parametrize("p", [0.3, 0.05, 0.0])
@pytest.mark.parametrize("case", range(len(SHAPES)))
def test_bits_keep(dev, case, p):
    ops, _lib = _env()
    (B, C, T), (seed, site, offset) = SHAPES[case], STREAM[case]
    rs = (T + 31) // 32
    want_keep = R.keep_bytes(B, C, T, p, seed, site, offset or 0)
    want_bits = R.keep_words(B * C * rs, p, seed, site, offset or 0)
    for fill in (FILL, 0x5A):
        keep, bits, off = Out(dev, B * _groups(C) * T, fill), Out(dev, 4 * B * C * rs, fill), _offset(dev, offset)
        _lib.call("dv3_dropout_bits_keep", bits.ptr, keep.ptr, B, C, T, float(p), seed, site, _p(off), ops._stream())
        what = "bits_keep %r p %r fill %x" % ((B, C, T), p, fill)
        same(bits.read(np.uint32), want_bits, what + " (bits)")
        check_keep(keep.read(), B, C, T, want_keep, what + " (keep)")
    # the same words dv3_dropout_bits draws over the rows
    same(draw_bits(dev, B * C * rs, p, seed, site, offset), want_bits, "dropout_bits over the same rows")


# ------------------------------------------------------------------------------------------------------------------
# dv3_dropout_keep_c8_multi
# ------------------------------------------------------------------------------------------------------------------
SIX = [("both", 3, 64, 77, 0.05, 11), ("keep", 2, 72, 150, 0.1, 12), ("both", 4, 256, 33, 0.05, 14), ("keep", 1, 8, 5, 0.5, 20),
       ("bits", 1, 300, 77, 0.05, 21), ("bits", 1, 37, 130, 0.2, 23)]


def _blocks(B, C, T):
    return (B * _groups(C) * ((T + 31) // 32) + 31) // 32


def _table(n):
    """n sites of tiny, mixed shapes and kinds: sites of one block and of several in turn, the last one of several"""
    shapes = [(1, 8, 5), (3, 40, 37), (2, 3, 70), (1, 37, 130), (2, 40, 33), (2, 72, 70), (1, 64, 31), (1, 513, 33)]
    kinds = ("keep", "both", "bits")
    ps = (0.05, 0.3, 0.5, 0.0, 0.99999)
    out = []
    for i in range(n):
        B, C, T = shapes[(i * 3 + i // 8) % len(shapes)] if i < n - 1 else (2, 72, 70)
        kind = kinds[i % 3]
        if kind == "bits":
            B, C = 1, B * C                      # rows
        out.append((kind, B, C, T, ps[i % len(ps)], (2 ** 32 - 2 + i) if i % 2 else 3 * i + 1))
    return out


def launch_multi(dev, sites, seed, offset, fill=FILL):
    """-> (return code, [(keep Out or None, bits Out or None)]) of ONE dv3_dropout_keep_c8_multi call"""
    ops, _lib = _env()
    arr, outs = (ops.STRUCTS["dv3_dropout_site"] * len(sites))(), []
    for e, (kind, B, C, T, p, site) in zip(arr, sites):
        keep = Out(dev, B * _groups(C) * T, fill) if kind != "bits" else None
        bits = Out(dev, 4 * B * C * ((T + 31) // 32), fill) if kind != "keep" else None
        e.keep, e.bits = (keep.ptr if keep else None), (bits.ptr if bits else None)
        e.B, e.C, e.T, e.p, e.site = B, C, T, p, site
        outs.append((keep, bits))
    off = _offset(dev, offset)
    rc = _lib.lib().dv3_dropout_keep_c8_multi(arr, len(sites), seed, _p(off), ops._stream())
    torch.cuda.synchronize()
    return rc, outs


def check_multi(sites, outs, seed, offset, what):
    for l, ((kind, B, C, T, p, site), (keep, bits)) in enumerate(zip(sites, outs)):
        w = "%s: site %d of the table %r" % (what, l, (kind, B, C, T, p, site))
        if bits is not None:
            same(bits.read(np.uint32), R.keep_words(B * C * ((T + 31) // 32), p, seed, site, offset or 0), w + " (bits)")
        if keep is not None:
            check_keep(keep.read(), B, C, T, R.keep_bytes(B, C, T, p, seed, site, offset or 0), w + " (keep)")


def test_multi_six_sites(dev):
    for fill in (FILL, 0x5A):
        rc, outs = launch_multi(dev, SIX, 777, 12345, fill)
        assert rc == 0
        check_multi(SIX, outs, 777, 12345, "six sites, fill %x" % fill)


def test_multi_full_table(dev):
    _, _lib = _env()
    MAX = _lib.CONSTS["DV3_DROPOUT_MULTI_MAX"]
    sites = _table(MAX)
    assert len(sites) == MAX and {s[0] for s in sites} == {"keep", "both", "bits"}
    nb = [_blocks(B, C, T) for _, B, C, T, _, _ in sites]
    assert 1 in nb and max(nb) > 2 and nb[-1] > 1 and nb[0] == 1        # one block and several; the last of several
    for kind in ("keep", "both", "bits"):                                # every kind in both sizes
        sizes = {min(b, 2) for s, b in zip(sites, nb) if s[0] == kind}
        assert sizes == {1, 2}, (kind, sizes)
    for fill, seed, offset in ((FILL, 2 ** 32 - 1, 1), (0x5A, 12345678901234567, None)):
        rc, outs = launch_multi(dev, sites, seed, offset, fill)
        assert rc == 0
        check_multi(sites, outs, seed, offset, "%d sites, fill %x" % (MAX, fill))


def test_multi_refuses_more_than_the_table_holds(dev):
    _, _lib = _env()
    MAX = _lib.CONSTS["DV3_DROPOUT_MULTI_MAX"]
    rc, outs = launch_multi(dev, _table(MAX + 1), 777, 5)
    assert rc == _lib.CONSTS["DV3_EINVAL"] == -1
    assert b"dropout_keep_c8_multi" in _lib.lib().dv3_last_error()
    for keep, bits in outs:
        assert (keep is None or keep.untouched()) and (bits is None or bits.untouched())


# ------------------------------------------------------------------------------------------------------------------
# ops: site numbers, the plan
# ------------------------------------------------------------------------------------------------------------------
def _np(t, dtype=np.uint8):
    return t.cpu().numpy().reshape(-1).view(dtype)


def _call_and_check(ops, dev, kind, B, C, T, p, seed, site, offset, what):
    """one ops call of `kind` over (B, C, T); what it returns against the reference of (seed, site, offset)"""
    rs = (T + 31) // 32
    if kind == "bits":
        bits, got_rs = ops.dropout_bits(B * C, T, p, dev)
        keep = None
    elif kind == "keep":
        keep, bits, got_rs = ops.dropout_keep_c8(B, C, T, p, dev), None, rs
    else:
        bits, got_rs, keep = ops.dropout_bits_keep(B, C, T, p, dev)
    assert got_rs == rs
    if bits is not None:
        assert bits.dtype == torch.int32 and bits.numel() == B * C * rs
        same(_np(bits, np.uint32), R.keep_words(B * C * rs, p, seed, site, offset), what + " (bits)")
    if keep is not None:
        assert keep.dtype == torch.uint8 and tuple(keep.shape) == (B, _groups(C), T)
        check_keep(_np(keep), B, C, T, R.keep_bytes(B, C, T, p, seed, site, offset), what + " (keep)")


class _saved_state(object):
    """ops.dropout_state and ops.mask_plan as they were, put back on exit"""

    def __enter__(self):
        ops, _ = _env()
        self.ops = ops
        self.state = dict(vars(ops.dropout_state))
        self.plan, self.enabled = ops.mask_plan, ops.MaskPlan.enabled
        return ops

    def __exit__(self, *exc):
        ops = self.ops
        vars(ops.dropout_state).clear()
        vars(ops.dropout_state).update(self.state)
        ops.mask_plan, ops.MaskPlan.enabled = self.plan, self.enabled
        return False


def test_ops_the_kth_call_takes_site_k(dev):
    calls = [("bits", 1, 37, 130), ("keep", 2, 3, 70), ("both", 3, 40, 37), ("bits", 2, 8, 33), ("both", 1, 64, 31),
             ("keep", 1, 8, 1), ("keep", 2, 40, 33), ("bits", 1, 5, 1)]
    with _saved_state() as ops:
        ops.mask_plan = ops.MaskPlan()
        for seed in (2 ** 32 - 1, 12345678901234567, 2 ** 64 + 777):
            ops.dropout_state.manual_seed(seed)
            ops.dropout_state.dev_offset, ops.dropout_state.record = None, None
            assert ops.dropout_state.seed == seed % U64 and ops.dropout_state.site == 0
            for k, (kind, B, C, T) in enumerate(calls, 1):
                _call_and_check(ops, dev, kind, B, C, T, 0.3, seed % U64, k, 0, "seed %d call %d" % (seed, k))
                assert ops.dropout_state.site == k
        # with a device step counter: the same site numbers, the counter added to the seed
        ops.dropout_state.manual_seed(2 ** 32 - 5)
        ops.dropout_state.dev_offset = _offset(dev, 9)
        for k, (kind, B, C, T) in enumerate(calls[:3], 1):
            _call_and_check(ops, dev, kind, B, C, T, 0.05, 2 ** 32 - 5, k, 9, "step counter, call %d" % k)


def test_ops_a_plan_of_50_sites_is_drawn_in_two_launches(dev):
    shapes = [(1, 8, 5), (3, 40, 37), (2, 3, 70), (1, 37, 130), (2, 40, 33), (1, 64, 31)]
    kinds = ("keep", "both", "bits")
    sigs = []
    for i in range(50):
        B, C, T = shapes[(i + i // 6) % len(shapes)]
        kind = kinds[i % 3]
        if kind == "bits":
            B, C = 1, B * C
        sigs.append((i + 1, kind, B, C, T, float((0.05, 0.3, 0.5)[i % 3])))
    seed, step = 2 ** 32 - 3, 7
    with _saved_state() as ops:
        MAX = ops.CONSTS["DV3_DROPOUT_MULTI_MAX"]
        assert MAX < len(sigs) <= 2 * MAX
        plan = ops.mask_plan = ops.MaskPlan()
        ops.MaskPlan.enabled = True
        st = ops.dropout_state
        st.manual_seed(seed)
        st.dev_offset, st.record = _offset(dev, step), None
        for k in (1, 2, 3):                       # three sites before the step: the plan starts at s0 = 3
            _call_and_check(ops, dev, "bits", 1, 9, 40, 0.3, seed, k, step, "before the step, call %d" % k)
        assert plan.stats == dict(batched_launches=0, planned=0, single=0)
        plan.plan = tuple(sigs)
        plan.begin_step(dev)
        s0 = plan.s0
        assert s0 == 3 and len(plan.ready) == 50
        assert plan.stats == dict(batched_launches=2, planned=0, single=0)
        for off, kind, B, C, T, p in sigs:
            _call_and_check(ops, dev, kind, B, C, T, p, seed, s0 + off, step, "planned site %d" % off)
        assert plan.stats == dict(batched_launches=2, planned=50, single=0) and not plan.ready
        # a 51st call the plan does not hold: its own launch, its own site number
        _call_and_check(ops, dev, "both", 2, 8, 33, 0.25, seed, s0 + 51, step, "the 51st call")
        assert plan.stats == dict(batched_launches=2, planned=50, single=1)
        assert st.site == s0 + 51
        plan.end_step()
        assert plan.plan is None and len(plan.last) == 51


def test_ops_a_call_that_differs_from_the_plan_draws_its_own_mask(dev):
    """same position, another shape: the planned mask is dropped, the call launches for itself at the same site"""
    with _saved_state() as ops:
        plan = ops.mask_plan = ops.MaskPlan()
        ops.MaskPlan.enabled = True
        st = ops.dropout_state
        st.manual_seed(4242)
        st.dev_offset, st.record = None, None
        plan.plan = ((1, "keep", 2, 40, 33, 0.05), (2, "both", 1, 8, 5, 0.05))
        plan.begin_step(dev)
        _call_and_check(ops, dev, "keep", 2, 40, 37, 0.05, 4242, 1, 0, "a shape the plan does not hold")
        _call_and_check(ops, dev, "both", 1, 8, 5, 0.05, 4242, 2, 0, "the planned one after it")
        assert plan.stats == dict(batched_launches=1, planned=1, single=1)
        plan.end_step()

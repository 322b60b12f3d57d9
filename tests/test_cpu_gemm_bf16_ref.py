# coding: utf-8
"""No GPU: proves the single-term ("bf16") and c8 parts of tests/gemm_split_ref.py, on which tests/test_gpu_gemm_bf16.py
rests, and shows that its checks are not vacuous.

  * c8 pack / unpack, keep-bytes and keep-bits against a per-element loop of the header's statement (include/dv3hip.h);
  * bf16_rn against round-to-nearest-even done in integer arithmetic, on the E5 values among others;
  * a single-term kernel emulated on the host (exact products added in fp32 in a random order) stays inside `bound`;
  * every exact family is exact on every shape the GPU test uses (all partial sums below 2^24 quanta, masks, the
    dropout scale 2 and the addends included);
  * the outputs of E1 / E3 are mostly NOT bf16 values and E1 produces exact bf16 ties: the "stored value == bf16_rn(exact)"
    check of the c8 outputs can catch a wrong output rounding;
  * eight defect models (operand truncation, round-half-away, a three-term result, output truncation, a product lost at a
    sequence end, a frame lost at a slab boundary, a keep-byte ignored, an empty slab left unwritten) each break
    exactness on an exact family and leave the bound by at least 2 x on a bounded one where the defect has a size.
"""
import numpy as np
import pytest
import torch

from tests import gemm_split_ref as R
from tests.test_cpu_gemm_split_ref import EMU_SHAPES

GEMMS = ("fwd", "dgrad", "wgrad")
MODE = "bf16"
FA, FW = R.forms("fwd", MODE)


def _setup(fam, gemm, shape, c8):
    """operands of a case as the tensor holds them (c8: rounded to bf16 on the host), the GEMM and its depth"""
    B, C, T, k, d, causal = shape[:6]
    M = R.c8_shape_M(shape)
    padL = R.pad_left(k, d, causal)
    f = R.family(fam, gemm, MODE, shape)
    act, wgt = f["act"], f["wgt"]
    if c8:
        act = R.bf16_rn(act).astype(np.float32)
        if gemm == "wgrad":
            wgt = R.bf16_rn(wgt).astype(np.float32)
    mm = R.make_mm(gemm, d, padL, k)
    n = R.n_products(gemm, MODE, J=k, K=(C if gemm == "fwd" else M), B=B, T=T)
    return f, act, wgt, mm, n, R.bias_bcast(f["addend"]), dict(J=k, dil=d, padL=padL)


def _rne_bits(v32):
    """round-to-nearest-even of fp32 to bf16 in integer arithmetic (finite values)"""
    b = np.ascontiguousarray(v32, dtype=np.float32).view(np.uint32).astype(np.uint64)
    r = (b + 0x7fff + ((b >> 16) & 1)) >> 16
    return (r.astype(np.uint32) << 16).view(np.float32).astype(np.float64)


def _trunc(v):
    b = np.ascontiguousarray(np.asarray(v, np.float32)).view(np.uint32) & np.uint32(0xffff0000)
    return b.view(np.float32).astype(np.float64)


def _half_away(v):
    b = np.ascontiguousarray(np.asarray(v, np.float32)).view(np.uint32).astype(np.uint64)
    return (((b + 0x8000) >> 16).astype(np.uint32) << 16).view(np.float32).astype(np.float64)


def test_forms_of_the_single_term_mode():
    for gemm in GEMMS:
        assert R.forms(gemm, MODE) == (("bf16_1",), ("bf16_1",))
    v = np.float32([1.0 + 2.0 ** -8, 1.0 + 3 * 2.0 ** -8, -3.0, 0.0])
    hi, lo, s = R.split(v, FA)
    assert hi.tolist() == [1.0, 1.0 + 2.0 ** -6, -3.0, 0.0] and not lo.any() and s == 0
    assert not R.delta(v, FA).any()
    assert R.n_products("fwd", MODE, J=3, K=40, B=2, T=9) == 3 * 64
    assert R.n_products("wgrad", MODE, J=3, K=40, B=4, T=9, n_slabs=2) == 2 * 9
    assert R.n_products("wgrad", MODE, J=3, K=40, B=4, T=40, n_slabs=3, k_split=True) == 3 * 32


def test_bf16_rn_is_round_to_nearest_even():
    rng = np.random.RandomState(0)
    exps = np.arange(-100, 100)
    v = (rng.uniform(1, 2, size=(exps.size, 512)) * 2.0 ** exps[:, None]).astype(np.float32).ravel()
    e5 = np.concatenate([R.family("E5", g, MODE, s)[k].ravel() for g in GEMMS for s in R.EDGE_SHAPES[:3] for k in ("act", "wgt")])
    v = np.concatenate([v, -v, e5])
    assert np.array_equal(R.bf16_rn(v), _rne_bits(v))
    nz = e5[e5 != 0]
    # E5 is where the three roundings part: ties (truncation != RNE on odd h, half-away != RNE on even h) and neighbours
    assert np.any(_trunc(nz) != R.bf16_rn(nz)) and np.any(_half_away(nz) != R.bf16_rn(nz))
    tie = (np.ascontiguousarray(nz, dtype=np.float32).view(np.uint32) & 0xffff) == 0x8000
    assert 0.3 < tie.mean() < 0.7, tie.mean()
    up = R.bf16_rn(nz[tie]) != _trunc(nz[tie])
    assert 0.3 < up.mean() < 0.7, "both parities of h"
    assert len(set(np.frexp(nz)[1].tolist())) >= 3, "several binades"


@pytest.mark.parametrize("B,C,T", [(2, 40, 5), (1, 8, 1), (2, 513, 3), (3, 3, 33), (1, 64, 2)])
def test_c8_layout_and_keep_bytes_against_a_per_element_loop(B, C, T):
    rng = np.random.RandomState(B + C + T)
    v = R.bf16_rn(rng.standard_normal((B, C, T)).astype(np.float32))
    bits = R.c8_pack(v)
    G = (C + 31) // 32 * 32 // 8
    assert bits.shape == (B, G, T, 8) and bits.dtype == np.uint16
    keep = rng.rand(B, C, T) < 0.5
    kb = R.keep_bytes(keep)
    words, rs = R.keep_bits_words(keep)
    assert kb.shape == (B, G, T) and words.shape == (B * C, rs) and rs == (T + 31) // 32
    tv = torch.from_numpy(bits.view(np.int16)).view(torch.bfloat16).double().numpy()
    seen = np.zeros(bits.shape, bool)
    for b in range(B):
        for c in range(C):
            for t in range(T):
                assert tv[b, c // 8, t, c % 8] == v[b, c, t]
                seen[b, c // 8, t, c % 8] = True
                assert bool((kb[b, c // 8, t] >> (c % 8)) & 1) == bool(keep[b, c, t])
                assert bool((int(words[b * C + c, t // 32]) >> (t % 32)) & 1) == bool(keep[b, c, t])
    assert not bits[~seen].any(), "channels >= C are zero"
    for b in range(B):
        for g in range(G):
            for e in range(8):
                if 8 * g + e >= C:
                    assert not ((kb[b, g] >> e) & 1).any(), "padding channels are not kept"
    back, pad = R.c8_unpack(bits, C)
    assert np.array_equal(back, v) and pad == 0.0
    if G * 8 > C:
        dirty = bits.copy()
        dirty[0, G - 1, 0, 7] = 0x3f80
        assert R.c8_unpack(dirty, C)[1] == 1.0


def test_bf16_output_bound_and_ulp():
    assert R.ulp_bf16(np.float64([1.0, 1.99, 2.0, 0.75, 3e-5])).tolist() == [2.0 ** -7, 2.0 ** -7, 2.0 ** -6, 2.0 ** -8, 2.0 ** -23]
    rng = np.random.RandomState(3)
    ref = rng.standard_normal(200000) * 2.0 ** rng.randint(-20, 20, size=200000)
    bnd = np.abs(ref) * 2.0 ** -20
    tail = (ref + bnd * rng.uniform(-1, 1, size=ref.shape)).astype(np.float32)       # fp32 tail within bnd (up to its own ulp)
    got = R.bf16_rn(tail)
    lim = R.bf16_out_bound(ref, bnd + np.abs(ref) * 2.0 ** -24)
    assert np.all(np.abs(got - ref) <= lim)
    assert float((np.abs(got - ref) / lim).max()) > 0.95, "half an ulp is reached: nothing smaller would do"
    # the torch form inside check_bf16 is the same function
    t, b = torch.from_numpy(ref), torch.from_numpy(bnd)
    a = (t.abs() + b).clamp_min(2.0 ** -126)
    assert np.array_equal((b + 0.5 * torch.ldexp(torch.ones_like(a), torch.frexp(a)[1] - 8)).numpy(), R.bf16_out_bound(ref, bnd))
    assert torch.equal(R.bf16_out_bound(t, b), torch.from_numpy(R.bf16_out_bound(ref, bnd)))


def test_slab_partition_of_the_c8_k_split():
    for (B, T, S) in [(3, 200, 1), (3, 200, 3), (3, 200, 7), (3, 200, 22), (1, 1, 3), (2, 33, 7), (5, 37, 11)]:
        own = R.c8_slabs(B, T, S)
        assert own.shape == (S, B, T) and np.array_equal(own.sum(0), np.ones((B, T))), "every frame in exactly one slab"
        n_tc = (T + 31) // 32
        q = -(-(B * n_tc) // S)
        for s in range(S):
            steps = sorted({(b, t // 32) for b, t in zip(*np.nonzero(own[s]))})
            assert steps == [divmod(gs, n_tc) for gs in range(s * q, min((s + 1) * q, B * n_tc))]
        assert R.c8_slab_frames(B, T, S) <= min(B * T, q * 32)
        if S > B * n_tc:
            assert not own[B * n_tc:].any(), "trailing slabs are empty"


def test_c8_shape_set_reaches_what_it_was_chosen_for():
    wanted = ["(3, 64, 200, 3, 1, False)", "(3, 96, 150, 3, 27, True)", "(2, 128, 513, 3, 9, True)", "(1, 8, 1, 3, 1, True)",
              "(1, 16, 3, 3, 2, False)", "(2, 8, 33, 1, 1, False)", "(2, 40, 50, 3, 4, True)", "(5, 24, 37, 3, 3, False)"]
    assert [str(s) for s in R.C8_SHAPES[:8]] == wanted     # the edge shapes, the 2- and 5-tap ones with the 3 taps c8 serves
    for s in R.C8_SHAPES:
        assert s[3] in (1, 3) and (s[3] - 1) * s[4] <= R.C8_HALO_MAX
    reach = {str(s): R.c8_reach(s) for s in R.C8_SHAPES}
    # each shape still reaches the item it is in the set for
    for s, items in {"(3, 64, 200, 3, 1, False)": ["spans_items", "ragged_chunk", "wgrad_narrow"],
                     "(3, 96, 150, 3, 27, True)": ["spans_items", "wgrad_wide", "wgrad_row_tiles"],
                     "(2, 128, 513, 3, 9, True)": ["spans_items", "ragged_chunk", "wgrad_row_tiles"],
                     "(1, 8, 1, 3, 1, True)": ["one_frame", "short", "ragged_channels"],
                     "(1, 16, 3, 3, 2, False)": ["short", "ragged_channels"],
                     "(2, 8, 33, 1, 1, False)": ["spans_items", "ragged_chunk", "ragged_channels"],
                     "(2, 40, 50, 3, 4, True)": ["ragged_channels", "spans_items"],
                     "(5, 24, 37, 3, 3, False)": ["ragged_channels", "spans_items"],
                     "(2, 32, 70, 3, 32, True)": ["halo_limit", "wgrad_wide"],
                     "(2, 513, 40, 1, 1, False, 64)": ["ragged_channels", "wgrad_col_tiles"],
                     "(2, 64, 40, 1, 1, False, 513)": ["ragged_channels", "wgrad_row_tiles"]}.items():
        for it in items:
            assert reach[s][it], (s, it)
    for it in next(iter(reach.values())):
        assert any(r[it] for r in reach.values()), it
    assert sum(r["gated_ok"] for r in reach.values()) == 9 and not reach["(2, 513, 40, 1, 1, False, 64)"]["gated_ok"]


@pytest.mark.parametrize("gemm", GEMMS)
def test_single_term_emulation_stays_inside_the_bound(gemm):
    for fam in R.EXACT_BF16 + R.BOUNDED:
        worst = 0.0
        for si, shape in enumerate(EMU_SHAPES):
            f, act, wgt, mm, n, bias, kw = _setup(fam, gemm, shape, False)
            tail, bnd = R.expect_bf16(mm, act, wgt, n, addend=bias)
            assert torch.equal(tail, R.three_term(mm, act, wgt, FA, FW, bias))
            assert torch.equal(tail, R.reference(mm, act, wgt, bias, form_a=FA, form_w=FW)), "the same-rounding reference"
            assert torch.equal(bnd, R.bound(mm, act, wgt, FA, FW, n, bias)[0]) and not R.bound(mm, act, wgt, FA, FW, n, bias)[1].any()
            got = R.emulate(gemm, act, wgt, FA, FW, addend=bias, seed=si, **kw)
            worst = max(worst, R.check_bf16(fam[0] == "E", got, tail, bnd, "%s %s %s" % (fam, gemm, shape)))
            if fam[0] == "B":        # ... and its bf16 store inside the bf16-output bound, which half an ulp nearly fills
                stored = torch.from_numpy(R.bf16_rn(got.numpy().astype(np.float32)))
                R.check_bf16(False, stored, tail, bnd, "stored", out_bf16=True)
        assert worst < 1.0
        print("%s %s: emulated worst ratio %.3f" % (fam, gemm, worst))


def _exact_cases():
    for shape in R.EDGE_SHAPES:
        yield shape, False
    for shape in R.C8_SHAPES:
        yield shape, True


@pytest.mark.parametrize("gemm", GEMMS)
@pytest.mark.parametrize("fam", R.EXACT_BF16)
def test_exact_families_are_exact_on_every_shape_used(fam, gemm):
    """every product and every partial sum -- with the dropout scale 2 on the accumulators and an addend of the operands'
    size -- is a whole number of quanta below 2^24: fp32 adds them exactly in any order"""
    worst = 0.0
    for shape, c8 in _exact_cases():
        f, act, wgt, mm, n, bias, kw = _setup(fam, gemm, shape, c8)
        tail, _ = R.expect_bf16(mm, act, wgt, n, addend=bias)
        q = f["quantum"]
        a, w = np.abs(R.bf16_rn(act)), np.abs(R.bf16_rn(wgt))
        tot = 2.0 * mm(R._t64(a), R._t64(w))
        tot = tot + (float(np.abs(f["addend"]).max()) if bias is not None else 15 * q)   # bias / the input gradient's r: |m| <= 15 quanta
        quanta = float(tot.max()) / q
        worst = max(worst, quanta)
        assert quanta < 2.0 ** 24, (shape, quanta)
        tq = (tail / q).numpy()
        assert np.array_equal(tq, np.round(tq)) and torch.equal(tail.float().double(), tail), shape
        if fam in ("E4", "E5"):
            nz = mm(R._t64((act != 0).astype(np.float64)), R._t64((wgt != 0).astype(np.float64)))
            assert float(nz.max()) <= 8, (shape, float(nz.max()))
        if fam in ("E4", "E5") and not c8:      # the rounding is live: the fp32 operands are not bf16 values
            assert np.any(R.bf16_rn(act) != act) and np.any(R.bf16_rn(wgt) != wgt)
            assert not torch.equal(tail, R.reference(mm, act, wgt, bias)), shape
    print("%s %s: largest sum of |terms| = 2^%.1f quanta" % (fam, gemm, np.log2(max(worst, 1.0))))


def _is_bf16(t):
    return t.float().to(torch.bfloat16).double() == t


def _is_tie(t):
    a = t.abs().numpy()
    ulp = R.ulp_bf16(a)
    return torch.from_numpy((a - np.floor(a / ulp) * ulp) == 0.5 * ulp)


@pytest.mark.parametrize("gemm", ["fwd", "dgrad"])
def test_rounding_checks_of_the_c8_outputs_are_not_vacuous(gemm):
    n_all = n_nb = n_tie = n_e1 = 0
    for fam in ("E1", "E3"):
        for shape in R.C8_SHAPES:
            f, act, wgt, mm, n, bias, kw = _setup(fam, gemm, shape, True)
            tail, _ = R.expect_bf16(mm, act, wgt, n, addend=bias)
            n_all += tail.numel()
            n_nb += int(((tail != 0) & ~_is_bf16(tail)).sum())
            if fam == "E1":
                n_e1 += tail.numel()
                n_tie += int(_is_tie(tail).sum())
    print("%s: %d of %d E1 / E3 outputs are nonzero and not bf16 values (%.0f %%); %d of %d E1 outputs are exact bf16 ties"
          % (gemm, n_nb, n_all, 100.0 * n_nb / n_all, n_tie, n_e1))
    assert n_nb >= 0.5 * n_all
    assert n_tie > 0


# ---------------------------------------------------------------------------------------------------------------
# defect models
# ---------------------------------------------------------------------------------------------------------------
def _fails(exact, got, tail, bnd, out_bf16=False):
    try:
        R.check_bf16(exact, got, tail, bnd, "defect", out_bf16=out_bf16)
    except AssertionError:
        return True
    return False


def _ratio(got, tail, bnd):
    err = (got - tail).abs()
    return float(torch.where(err == 0, torch.zeros_like(err), err / bnd).max())


@pytest.mark.parametrize("gemm", GEMMS)
@pytest.mark.parametrize("defect", ["truncation", "half_away", "three_term"])
def test_a_wrong_operand_rounding_breaks_e5(gemm, defect):
    for shape in R.EDGE_SHAPES:
        f, act, wgt, mm, n, bias, kw = _setup("E5", gemm, shape, False)
        tail, bnd = R.expect_bf16(mm, act, wgt, n)
        if defect == "three_term":
            bad = R.three_term(mm, act, wgt, ("bf16",), ("bf16",))
        else:
            rnd = _trunc if defect == "truncation" else _half_away
            bad = mm(R._t64(rnd(act)), R._t64(rnd(wgt)))
        assert torch.equal(bad.float().double(), bad), "the defective kernel's value is an fp32 value too: only exactness tells"
        assert _fails(True, bad, tail, bnd), (defect, gemm, shape)


@pytest.mark.parametrize("gemm", ["fwd", "dgrad"])
def test_output_truncation_breaks_e1(gemm):
    for shape in R.C8_SHAPES:
        f, act, wgt, mm, n, bias, kw = _setup("E1", gemm, shape, True)
        tail, bnd = R.expect_bf16(mm, act, wgt, n, addend=bias)
        good = torch.from_numpy(R.bf16_rn(tail.numpy().astype(np.float32)))
        bad = torch.from_numpy(_trunc(tail.numpy().astype(np.float32)))
        assert not _fails(True, good, tail, bnd, out_bf16=True)
        if shape[0] * shape[2] >= 33:          # (a frame or three of small integers can all be bf16 values)
            assert _fails(True, bad, tail, bnd, out_bf16=True), (gemm, shape)


def _lost_product(gemm, act, wgt, shape, kw, fam):
    """what one lost product at a sequence end takes from the output: the LAST frame of the last batch item does not reach
    the tap that reads it at the output's last frame (fwd / dgrad: one input channel, all output rows)"""
    B, C, T, k, d, causal = shape[:6]
    a, w = R.bf16_rn(act), R.bf16_rn(wgt)
    out = torch.zeros(B, w.shape[1] if gemm == "dgrad" else w.shape[0], T, dtype=torch.float64)
    padL = kw["padL"] if gemm == "fwd" else (k - 1) * d - kw["padL"]
    # taps that read frame T - 1 for output frame T - 1: j d - padL == 0
    taps = [j for j in range(k) if j * d - padL == 0]
    assert taps, shape
    j = taps[0]
    c = int(np.argmax(np.abs(a[B - 1, :, T - 1])))
    col = w[:, c, j] if gemm == "fwd" else w[c, :, k - 1 - j]
    out[B - 1, :, T - 1] = torch.from_numpy(col * a[B - 1, c, T - 1])
    return out


@pytest.mark.parametrize("gemm", ["fwd", "dgrad"])
def test_a_product_lost_at_a_sequence_end_is_caught(gemm):
    for shape in R.C8_SHAPES:
        for fam in ("E1", "B1"):
            f, act, wgt, mm, n, bias, kw = _setup(fam, gemm, shape, True)
            tail, bnd = R.expect_bf16(mm, act, wgt, n, addend=bias)
            lost = _lost_product(gemm, act, wgt, shape, kw, fam)
            assert bool((lost != 0).any()), (fam, shape)
            if fam == "E1":
                assert _fails(True, tail - lost, tail, bnd), (gemm, shape)
                stored = torch.from_numpy(R.bf16_rn((tail - lost).numpy().astype(np.float32)))
                assert _fails(True, stored, tail, bnd, out_bf16=True), (gemm, shape)
            else:
                r = _ratio(tail - lost, tail, bnd)
                assert r >= 2.0, (gemm, shape, r)
                # through the bf16 store as well: the lost product is far above half a bf16 ulp of the output
                stored = torch.from_numpy(R.bf16_rn((tail - lost).numpy().astype(np.float32)))
                lim = R.bf16_out_bound(tail, bnd)
                r8 = _ratio(stored, tail, lim)
                print("%s %s: lost product %.3g x the fp32 bound, %.3g x the bf16-output bound" % (gemm, shape, r, r8))
                assert r8 >= 2.0, (gemm, shape, r8)


WGRAD_S = (1, 3, 7)


def _slab_expect(g, x, keep, shape, S, kw):
    """per-slab expectation of wgrad_c8: (S, J, M, C) tails and bounds"""
    B, C, T, k, d, causal = shape[:6]
    own = R.c8_slabs(B, T, S)
    n = R.c8_slab_frames(B, T, S)
    tails, bnds = [], []
    for s in range(S):
        t, b = R.expect_bf16(R.make_mm("wgrad", d, kw["padL"], k), g, x, n, act_keep=own[s][:, None, :], wgt_keep=keep,
                             scale=2.0 if keep is not None else 1.0, ops=1)
        tails.append(t)
        bnds.append(b)
    return torch.stack(tails), torch.stack(bnds), own


def test_a_frame_lost_at_a_slab_boundary_and_an_unwritten_empty_slab_are_caught():
    for shape in R.C8_SHAPES:
        B, C, T, k, d, causal = shape[:6]
        chunks = B * ((T + 31) // 32)
        for fam in ("E1", "B1"):
            f, g, x, mm, n, bias, kw = _setup(fam, "wgrad", shape, True)
            for S in WGRAD_S + (chunks + 2,):
                tails, bnds, own = _slab_expect(g, x, None, shape, S, kw)
                assert torch.equal(tails.sum(0), R.expect_bf16(mm, g, x, n)[0]) or fam == "B1"
                assert not _fails(fam == "E1", tails.clone(), tails, bnds)
                if S > chunks:
                    assert not tails[chunks:].any() and not bnds[chunks:].any()
                    stale = tails.clone()
                    stale[S - 1] = 1.0          # the slab keeps what the buffer held
                    assert _fails(fam == "E1", stale, tails, bnds), (shape, S)
                    assert _ratio(stale, tails, bnds) == float("inf")
                if S == 1 or S > chunks or fam == "B1" and T < 2:
                    continue
                # the first frame of slab 1 (a slab boundary) is lost from slab 1: tap j reads x at t + j d - padL
                b, t = (int(v[0]) for v in np.nonzero(own[1]))
                a, w = torch.from_numpy(R.bf16_rn(g)), torch.from_numpy(R.bf16_rn(x))
                lost = torch.zeros_like(tails)
                for j in range(k):
                    tx = t + j * d - kw["padL"]
                    if 0 <= tx < T:
                        lost[1, j] = a[b, :, t, None] * w[b, None, :, tx]
                if not bool((lost != 0).any()):
                    continue
                if fam == "E1":
                    assert _fails(True, tails - lost, tails, bnds), (shape, S)
                else:
                    r = _ratio(tails - lost, tails, bnds)
                    assert r >= 2.0, (shape, S, r)


def test_an_ignored_keep_byte_is_caught():
    for shape in R.C8_SHAPES:
        B, C, T, k, d, causal = shape[:6]
        keep = np.random.RandomState(7).rand(B, C, T) < 0.5
        kb = R.keep_bytes(keep)
        b, g, t = (int(v[0]) for v in np.nonzero(kb != 0xff if C >= 8 else kb != (1 << C) - 1))
        ignored = keep.copy()
        ignored[b, 8 * g: 8 * g + 8, t] = True          # the kernel stages the whole unit
        for gemm in ("fwd", "wgrad"):
            for fam in ("E1", "B1"):
                f, act, wgt, mm, n, bias, kw = _setup(fam, gemm, shape, True)
                kws = [dict(act_keep=keep), dict(act_keep=ignored)] if gemm == "fwd" else [dict(wgt_keep=keep), dict(wgt_keep=ignored)]
                tail, bnd = R.expect_bf16(mm, act, wgt, n, scale=2.0, addend=bias, ops=3, **kws[0])
                bad, _ = R.expect_bf16(mm, act, wgt, n, scale=2.0, addend=bias, ops=3, **kws[1])
                x = R.bf16_rn(act if gemm == "fwd" else wgt)
                if not np.any(x[b, 8 * g: 8 * g + 8, t][~keep[b, 8 * g: 8 * g + 8, t]]):
                    continue                            # (E1 holds zeros: the dropped channels may all be zero here)
                if fam == "E1":
                    assert _fails(True, bad, tail, bnd), (gemm, shape)
                else:
                    r = _ratio(bad, tail, bnd)
                    assert r >= 2.0, (gemm, shape, r)

# coding: utf-8
"""The dropout-mask reference without a GPU: tests/philox_ref.py pinned to the three published Random123 known-answer
vectors of philox4x32-10, the float32 threshold at its edges, and the properties a mask generator is built for -- shown
here for the integer restatement alone; tests/test_gpu_dropout_masks.py then holds the device to it bit for bit, so what
is shown here holds for the kernels' masks too."""
import inspect
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tests import philox_ref as R  # noqa: E402


# ----------------------------------------------------------------------------------------------------------------------
# known answers (Random123, kat_vectors: philox4x32 10)
# ----------------------------------------------------------------------------------------------------------------------
KAT = [
    ((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
    ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
    ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0),
     (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1)),
]


@pytest.mark.parametrize("counter,key,want", KAT)
def test_known_answer_vectors(counter, key, want):
    got = R.philox4x32(counter, key)
    assert got.dtype == np.uint32 and got.shape == (4,)
    assert tuple(int(v) for v in got) == want, [hex(int(v)) for v in got]


def test_the_core_is_vectorised_over_the_counter():
    """the three vectors share no key, so: one key, a counter array holding every word of the three counters in every
    position against the same calls one at a time -- and the counter's high words (c1, c3) matter"""
    vals = sorted({v for c, _, _ in KAT for v in c})
    c = np.array(np.meshgrid(vals, vals, vals, vals, indexing="ij")).reshape(4, -1)
    key = KAT[2][1]
    got = R.philox4x32(tuple(c), key)
    assert got.shape == (c.shape[1], 4)
    for i in range(0, c.shape[1], 37):
        assert np.array_equal(got[i], R.philox4x32(tuple(int(v) for v in c[:, i]), key))
    i = int(np.nonzero((c.T == np.array(KAT[2][0])).all(axis=1))[0][0])
    assert tuple(int(v) for v in got[i]) == KAT[2][2]
    assert len({tuple(r) for r in got.tolist()}) == c.shape[1]          # a bijection of the counter: no two rows alike


def test_constants_as_published():
    assert (R.M0, R.M1, R.W0, R.W1, R.ROUNDS) == (0xD2511F53, 0xCD9E8D57, 0x9E3779B9, 0xBB67AE85, 10)


# ----------------------------------------------------------------------------------------------------------------------
# the threshold
# ----------------------------------------------------------------------------------------------------------------------
THRESHOLDS = [
    (0.0, 0),                                   # everything kept
    (1e-5, 1),
    (0.3, 19661),
    (100.5 / 65536, 101),                       # the tie rounds up
    ((100.5 - 2.0 ** -10) / 65536, 100),
    (0.99999, 65535),
    (1 - 2.0 ** -24, 65536),                    # the contract's edge: p < 1 is accepted, and nothing is ever kept
]


@pytest.mark.parametrize("p,thr", THRESHOLDS)
def test_threshold_edges(p, thr):
    """thr = trunc(p 65536 + 0.5) in float32.  A uniform is one of 0 .. 65535 and kept when >= thr: thr = 0 keeps every
    element, and thr = 65536 -- reached from p = 1 - 2^-17 on, where p 65536 + 0.5 >= 65536 -- keeps none although the
    entry points accept every p < 1: the contract's edge.  (Consumers scale by 1 / (1 - p), finite there.)"""
    assert R.threshold(p) == thr
    assert R.threshold(np.float32(p)) == thr
    w = R.keep_words(64, p, 777, 1)
    if thr == 0:
        assert np.all(w == 0xFFFFFFFF)
    if thr == 65536:
        assert np.all(w == 0)


def test_the_edge_starts_at_one_minus_two_to_the_minus_17():
    assert R.threshold(1 - 2.0 ** -17) == 65536
    assert R.threshold(float(np.nextafter(np.float32(1 - 2.0 ** -17), np.float32(0)))) == 65535


def _preset_probabilities():
    from deepvoice3_pytorch_amd import builder
    ps = set()
    for name, fn in inspect.getmembers(builder, inspect.isfunction):
        par = inspect.signature(fn).parameters.get("dropout")
        if not name.startswith("_") and par is not None and par.default is not inspect.Parameter.empty:
            ps.add(float(par.default))
    return sorted(ps)


def test_quantisation_bias_of_the_presets():
    """The drop rate the masks realise is thr / 65536, the consumers scale the kept elements by 1 / (1 - p): the
    expectation of a dropped-and-scaled activation is (1 - thr / 65536) / (1 - p) times the activation, so
    |thr / 65536 - p| <= 2^-17 (half a quantum of the 16-bit uniforms) is the WHOLE bias of the expectation --
    a relative 2^-17 / (1 - p), 8e-6 at the presets' p = 0.05."""
    ps = _preset_probabilities()
    assert ps and all(0.0 < p < 1.0 for p in ps)
    for p in ps:
        assert abs(R.threshold(p) / 65536.0 - p) <= 2.0 ** -17, p


# ----------------------------------------------------------------------------------------------------------------------
# design properties: conditions on the generator, checked on the reference (2^15 words = 2^20 decisions each)
# ----------------------------------------------------------------------------------------------------------------------
N_WORDS = 1 << 15
PS = (0.05, 0.25, 0.5, 0.95)
STREAMS = [(777, 1), (777, 2), (778, 1), (2 ** 32 - 1, 1), (2 ** 32, 1), (12345678901234567, 2 ** 32 + 3)]
PAIRS = {
    "neighbouring site": ((777, 1), (777, 2)),
    "neighbouring step": ((777, 1), (778, 1)),
    "site high word only": ((777, 1), (777, 2 ** 32 + 1)),
    "across the seed carry": ((2 ** 32 - 1, 1), (2 ** 32, 1)),
    "diagonal": ((777, 5), (778, 4)),
}
_uniforms = {}


def _kept(seed, site, p):
    """[2^20] booleans; the uniforms of a stream are drawn once and shared by every p"""
    if (seed, site) not in _uniforms:
        u = R.uniforms(N_WORDS, seed, site)
        u.setflags(write=False)
        _uniforms[(seed, site)] = u
    return (_uniforms[(seed, site)] >= R.threshold(p)).reshape(-1)


def _z(count, n, prob):
    return (count - n * prob) / np.sqrt(n * prob * (1.0 - prob))


def test_uniforms_and_words_are_the_same_decisions():
    for p in PS:
        k = _kept(777, 1, p).reshape(N_WORDS, 32)[:256]
        w = R.keep_words(256, p, 777, 1)
        assert np.array_equal(((w[:, None] >> np.arange(32, dtype=np.uint32)) & 1).astype(bool), k)


@pytest.mark.parametrize("p", PS)
@pytest.mark.parametrize("seed,site", STREAMS)
def test_keep_rate(seed, site, p):
    """the keep rate of 2^20 decisions against 1 - thr / 65536: |z| <= 5 (worst over the 24 cases: 3.30)"""
    k = _kept(seed, site, p)
    z = _z(int(k.sum()), k.size, 1.0 - R.threshold(p) / 65536.0)
    assert abs(z) <= 5.0, z


@pytest.mark.parametrize("p", PS)
@pytest.mark.parametrize("which", sorted(PAIRS))
def test_two_masks_agree_as_independent_ones_do(which, p):
    """two independent masks of keep rate q agree at a rate q^2 + (1 - q)^2: |z| <= 5 (worst over the 20 cases: 2.11).
    Were the site missing from the counter, or the step offset from the key, the agreement would be 1."""
    a, b = PAIRS[which]
    ka, kb = _kept(a[0], a[1], p), _kept(b[0], b[1], p)
    q = 1.0 - R.threshold(p) / 65536.0
    z = _z(int((ka == kb).sum()), ka.size, q * q + (1.0 - q) * (1.0 - q))
    assert abs(z) <= 5.0, z


@pytest.mark.parametrize("lag", [1, 2, 16, 32, 128])
def test_lagged_agreement_within_one_stream(lag):
    """p = 0.5: decisions `lag` apart in one stream (neighbouring halves, outputs, calls, words) agree half the time:
    |z| <= 5 (worst over the lags: 1.12)"""
    k = _kept(777, 1, 0.5)
    assert R.threshold(0.5) == 32768
    z = _z(int((k[lag:] == k[:-lag]).sum()), k.size - lag, 0.5)
    assert abs(z) <= 5.0, z


# ----------------------------------------------------------------------------------------------------------------------
# the layouts built on the words
# ----------------------------------------------------------------------------------------------------------------------
def test_offset_is_added_to_the_whole_seed():
    assert np.array_equal(R.keep_words(64, 0.3, 777, 1, offset=12345), R.keep_words(64, 0.3, 777 + 12345, 1))
    assert np.array_equal(R.keep_words(64, 0.3, 2 ** 32 - 1, 1, offset=1), R.keep_words(64, 0.3, 2 ** 32, 1))
    assert np.array_equal(R.keep_words(64, 0.3, 2 ** 64 - 1, 1, offset=2), R.keep_words(64, 0.3, 1, 1))
    assert np.array_equal(R.keep_words(64, 0.3, 777, 1, offset=-5), R.keep_words(64, 0.3, 777, 1, offset=2 ** 64 - 5))
    assert not np.array_equal(R.keep_words(64, 0.3, 2 ** 32, 1), R.keep_words(64, 0.3, 0, 1))           # the high key word
    assert not np.array_equal(R.keep_words(64, 0.3, 777, 2 ** 32 + 1), R.keep_words(64, 0.3, 777, 1))  # ... counter word


@pytest.mark.parametrize("B,C,T", [(1, 8, 1), (2, 3, 70), (3, 40, 37), (1, 64, 31)])
def test_keep_bytes_hold_the_words_decisions(B, C, T):
    """byte (b, g, t) bit e = bit t % 32 of word t // 32 of row b C + 8g + e, spelled out element by element"""
    p, seed, site = 0.3, 777, 9
    rs, G = (T + 31) // 32, (C + 31) // 32 * 4
    words = R.keep_words(B * C * rs, p, seed, site).reshape(B * C, rs)
    got = R.keep_bytes(B, C, T, p, seed, site)
    assert got.shape == (B, G, T) and got.dtype == np.uint8
    for b in range(B):
        for g in range(G):
            for t in range(T):
                want = 0
                for e in range(8):
                    ch = 8 * g + e
                    if ch < C:
                        want |= ((int(words[b * C + ch, t // 32]) >> (t % 32)) & 1) << e
                assert int(got[b, g, t]) == want, (b, g, t)
    kept, w2 = R.keep_rows(B * C, T, p, seed, site)
    assert np.array_equal(w2, words) and kept.shape == (B * C, T)

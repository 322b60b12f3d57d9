# coding: utf-8
"""The dropout masks restated in numpy, integer arithmetic only -- the independent reference the device kernels of
csrc/elementwise.hip (dropout_bits_kernel, dropout_keep_c8_kernel, dropout_keep_c8_multi_kernel) are compared with bit
for bit (tests/test_gpu_dropout_masks.py); tests/test_cpu_philox_ref.py pins this file to the published known answers.

Philox4x32-10 as published (Salmon, Moraes, Dror, Shaw: "Parallel random numbers: as easy as 1, 2, 3", SC'11; the
Random123 library): a 128-bit counter (c0, c1, c2, c3), a 64-bit key (k0, k1), ten rounds of

    (c0, c1, c2, c3) -> (hi(M1 c2) ^ c1 ^ k0,  lo(M1 c2),  hi(M0 c0) ^ c3 ^ k1,  lo(M0 c0))

hi / lo the halves of the 64-bit product, the key bumped by (W0, W1) between rounds.

The mask contract of include/dv3hip.h ("Dropout keep-bit generator"): mask word w of a site is four calls with
counter (lo32(4w + q), hi32(4w + q), lo32(site), hi32(site)), q = 0..3, and key (lo32(s), hi32(s)), s = (seed + offset)
mod 2^64; each of the four 32-bit outputs of a call gives two 16-bit uniforms, the low half first; bit 8q + 2e + h of the
word (e the output, h the half) is set -- the element is KEPT -- when the uniform is >= thr, thr = trunc(p 65536 + 0.5)
in float32.  Bit i of word w of a row is element 32 w + i of that row."""
import numpy as np

M0, M1 = 0xD2511F53, 0xCD9E8D57              # the round multipliers
W0, W1 = 0x9E3779B9, 0xBB67AE85              # the key increments (golden ratio, sqrt(3) - 1)
ROUNDS = 10
LO32 = 0xFFFFFFFF
U64 = 1 << 64


def philox4x32(counter, key, rounds=ROUNDS):
    """counter: four integers or integer arrays (broadcast against each other), each < 2^32; key: two integers < 2^32.
    -> uint32 array [..., 4]"""
    c0, c1, c2, c3 = np.broadcast_arrays(*[np.asarray(c, dtype=np.uint64) for c in counter])
    assert all(int(c.max()) <= LO32 for c in (c0, c1, c2, c3))
    k0, k1 = int(key[0]), int(key[1])
    assert 0 <= k0 <= LO32 and 0 <= k1 <= LO32
    lo32 = np.uint64(LO32)
    s32 = np.uint64(32)
    for _ in range(rounds):
        p0 = np.uint64(M0) * c0               # 32 x 32 -> 64 bits: no overflow in uint64
        p1 = np.uint64(M1) * c2
        c0, c1, c2, c3 = (p1 >> s32) ^ c1 ^ np.uint64(k0), p1 & lo32, (p0 >> s32) ^ c3 ^ np.uint64(k1), p0 & lo32
        k0 = (k0 + W0) & LO32
        k1 = (k1 + W1) & LO32
    return np.stack([c0, c1, c2, c3], axis=-1).astype(np.uint32)


def threshold(p):
    """thr of the contract: p * 65536 + 0.5 evaluated in float32, truncated.  A uniform u in [0, 65536) is kept when
    u >= thr: the keep rate is exactly 1 - thr / 65536, and thr = 65536 (p >= 1 - 2^-17) keeps nothing."""
    f = np.float32
    return int(f(f(f(p) * f(65536.0)) + f(0.5)))


def uniforms(n_words, seed, site, offset=0):
    """the 32 sixteen-bit uniforms behind every mask word, in bit order -> int64 [n_words][32]"""
    s = (int(seed) + int(offset)) % U64
    site = int(site) % U64
    ci = 4 * np.arange(n_words, dtype=np.uint64)[:, None] + np.arange(4, dtype=np.uint64)[None, :]      # [w][q]
    out = philox4x32((ci & np.uint64(LO32), ci >> np.uint64(32), site & LO32, site >> 32), (s & LO32, s >> 32))
    out = out.astype(np.int64)                                                                           # [w][q][e]
    halves = np.stack([out & 0xFFFF, out >> 16], axis=-1)                                                # [w][q][e][h]
    return halves.reshape(n_words, 32)


def keep_words(n_words, p, seed, site, offset=0):
    """-> uint32 [n_words]: bit 8q + 2e + h of word w set = kept"""
    kept = (uniforms(n_words, seed, site, offset) >= threshold(p)).astype(np.uint64)
    return (kept << np.arange(32, dtype=np.uint64)[None, :]).sum(axis=1).astype(np.uint32)


def keep_rows(rows, T, p, seed, site, offset=0):
    """the keep decisions of a site over [rows][T] elements -> (uint8 [rows][T] of 0 / 1, uint32 [rows][ceil(T/32)]);
    the words hold drawn bits past T in each row's last word too"""
    rs = (T + 31) // 32
    words = keep_words(rows * rs, p, seed, site, offset).reshape(rows, rs)
    t = np.arange(T)
    return ((words[:, t // 32] >> (t % 32).astype(np.uint32)) & 1).astype(np.uint8), words


def keep_bytes(B, C, T, p, seed, site, offset=0):
    """the keep-byte form [B][ceil(C/32)*4][T] (uint8): bit e of byte (b, g, t) = channel 8g + e of item b kept at frame
    t; zero for channels >= C (the pad channels of the last group and the whole pad groups)"""
    G = (C + 31) // 32 * 4
    kept, _ = keep_rows(B * C, T, p, seed, site, offset)
    full = np.zeros((B, G * 8, T), np.uint8)
    full[:, :C] = kept.reshape(B, C, T)
    full = full.reshape(B, G, 8, T)
    return (full << np.arange(8, dtype=np.uint8)[None, None, :, None]).sum(axis=2).astype(np.uint8)

# coding: utf-8
"""No GPU: tests/audio_kernels_ref.py's references agree with oracle/audio_oracle.py, its bounds hold for a plain float32
numpy emulation of every audio kernel, and they BREAK for emulations mutated the way a kernel could be wrong.

The emulations restate the arithmetic of csrc/audio.hip in float32 (Stockham radix-4 passes closed by a radix-2 pass,
float32 twiddles and windows rounded from float64, the packed two-frame projection, both de-emphasis forms); they share no
code with the float64 references but the frame index table (which the oracle comparison pins).  Inputs are the families the
GPU test uses, at all three sizes.  The mutants:
    hann_symmetric   a symmetric instead of a periodic Hann on the torch framing          -> spectrum, family W
    twiddle_fp16     one twiddle of the last pass rounded to fp16                           -> spectrum, family I (per bin)
    reflect_off      the right-edge reflection index off by one                              -> spectrum, family W
    two_thirds_edge  the 2/3 normaliser on an edge sample                                    -> iSTFT, family W
    dc_pair          the packed separation reading Z[N - k] at k = 0 as Z[N - 1]              -> projection, family T
    nyquist_sign     the packed separation with a sign error at Nyquist (second frame)        -> projection, family T
    phantom_frame    the unpaired last frame taken for a real one                             -> projection, family T
    carry_pow15      a chunked de-emphasis carry with coef^15 for coef^16                     -> de-emphasis
    no_clip          gl_prepare without its clip                                              -> gl_prepare grid
phantom_frame: not zeroing the phantom partner's spectrum alone cannot show in the real frame (in exact arithmetic the
packing keeps the two frames apart, and the rounding it adds is what a real partner adds), so the mutant is the whole
fault -- the phantom is framed, projected AND written, one frame past the item's last; the projection is therefore
judged on a buffer with one guard frame behind it, which must come back untouched (bound zero)."""
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tests import audio_kernels_ref as R  # noqa: E402
from oracle import audio_oracle as A  # noqa: E402

F32, C64 = np.float32, np.complex64
GUARD = F32(7.0)


def _report(what, ratio):
    print("worst-ratio %-72s %.4g" % (what, ratio))


# ----------------------------------------------------------------------------------------------------------------------
# float32 emulations
# ----------------------------------------------------------------------------------------------------------------------
def _twiddles(n):
    j = np.arange(n) * 2.0 / n
    return (np.cos(np.pi * j).astype(F32) + 1j * np.sin(np.pi * j).astype(F32)).astype(C64)


def _cx(re, im):
    out = np.empty(re.shape, dtype=C64)
    out.real, out.imag = re, im
    return out


def _fp16(w):
    return _cx(w.real.astype(np.float16).astype(F32), w.imag.astype(np.float16).astype(F32))


def emu_fft(a, sign, mut=None):
    """fft_lds<n, sign>: a complex64 [..., n]"""
    n = a.shape[-1]
    W = _twiddles(n) if sign > 0 else np.conj(_twiddles(n))
    src = a.astype(C64)
    ns = 1
    while ns * 4 <= n:
        j = np.arange(n // 4)
        k = j & (ns - 1)
        v = [src[..., j]]
        for r in (1, 2, 3):
            w = W[k * r * (n // 4 // ns)].copy()
            if mut == "twiddle_fp16" and n == 1024 and ns * 4 == n and r == 1:
                w[5] = _fp16(w[5:6])[0]
            v.append(src[..., j + r * (n // 4)] * w)
        s02, d02, s13, d13 = v[0] + v[2], v[0] - v[2], v[1] + v[3], v[1] - v[3]
        jd = _cx(d13.imag, -d13.real) if sign < 0 else _cx(-d13.imag, d13.real)
        j0 = ((j - k) << 2) + k
        dst = np.empty_like(src)
        dst[..., j0], dst[..., j0 + ns], dst[..., j0 + 2 * ns], dst[..., j0 + 3 * ns] = s02 + s13, d02 + jd, s02 - s13, d02 - jd
        src, ns = dst, ns * 4
    if n != 1024:
        j = np.arange(n // 2)
        w = W[j].copy()
        if mut == "twiddle_fp16":
            w[5] = _fp16(w[5:6])[0]
        u, v = src[..., j], src[..., j + n // 2] * w
        src = np.concatenate([u + v, u - v], axis=-1)
    return src


def emu_windows(n, hop, framing, mut=None):
    """(analysis, synthesis) float32"""
    if framing == "lws":
        aw, sw = A.lws_windows(n, hop)
        return aw.astype(F32), sw.astype(F32)
    c = np.cos(2.0 * np.pi * np.arange(n) / ((n - 1) if mut == "hann_symmetric" else n)).astype(F32)
    h = F32(0.5) - F32(0.5) * c
    return h, h


def emu_framed(y32, T, n, hop, framing, mut=None):
    idx = R.gather_index(y32.shape[1], T, n, hop, framing, reflect_shift=1 if mut == "reflect_off" else 0)
    ys = np.where(idx >= 0, y32[:, np.maximum(idx, 0)], F32(0))
    return (ys * emu_windows(n, hop, framing, mut)[0]).astype(F32)


def emu_stft(y32, n, hop, framing, mut=None):
    T = R.num_frames(y32.shape[1], n, hop, framing)
    a = emu_framed(y32, T, n, hop, framing, mut)
    return emu_fft(a.astype(C64), -1, mut)[..., :n // 2 + 1]


def _unit(x, y):
    inv = F32(1) / np.maximum(np.sqrt(x * x + y * y), F32(1e-8))
    return x * inv, y * inv


def emu_phasor(spec_c64):
    px, py = _unit(spec_c64.real, spec_c64.imag)
    return np.stack([px, py], axis=-1)


def _hermitian(half, n):
    """[..., n/2+1] -> [..., n]; the imaginary parts at DC and Nyquist are the caller's business"""
    return np.concatenate([half, np.conj(half[..., 1:n // 2][..., ::-1])], axis=-1)


def emu_frames(mag32, ph32, n, hop, framing):
    zx = mag32 if ph32 is None else mag32 * ph32[..., 0]
    zy = np.zeros_like(mag32) if ph32 is None else mag32 * ph32[..., 1]
    zy = zy.copy()
    zy[..., 0] = zy[..., -1] = 0
    v = emu_fft(_hermitian(_cx(zx, zy), n), +1).real
    return v * F32(1.0 / n) * emu_windows(n, hop, framing)[1]


def emu_ola(fr32, n, hop, framing, mut=None):
    B, T, _ = fr32.shape
    L = R.num_samples(T, n, hop, framing)
    off = n - hop if framing == "lws" else n // 2
    h = emu_windows(n, hop, "torch")[0]
    acc, wsum = np.zeros((B, (T - 1) * hop + n), dtype=F32), np.zeros((T - 1) * hop + n, dtype=F32)
    for t in range(T):
        s = slice(t * hop, t * hop + n)
        acc[:, s] = acc[:, s] + fr32[:, t]
        wsum[s] = wsum[s] + h * h
    acc, wsum = acc[:, off:off + L], wsum[off:off + L]
    if framing == "lws":
        return acc, np.ones(L, dtype=bool)
    p = np.arange(L) + off
    t_hi = np.minimum(p // hop, T - 1)
    t_lo = np.where(p - n + 1 <= 0, 0, (p - n + hop) // hop)
    interior = (hop * 4 == n) & (t_hi - t_lo == 3) & (p - t_lo * hop < n) & (p - t_hi * hop >= 0)
    pick = interior.copy()
    if mut == "two_thirds_edge":
        pick[0] = True
    return np.where(pick, acc * F32(2.0 / 3.0), acc / wsum), interior


def emu_project(y32, mag32, n, hop, framing, mut=None):
    """gl_project2_kernel -> flat [B * T + 1, n]: the frames and one guard frame behind them"""
    B, T, F = mag32.shape
    TP = (T + 1) // 2
    a = emu_framed(y32, T, n, hop, framing)
    m = mag32
    if T % 2:
        ghost = mut == "phantom_frame"       # the phantom takes a real frame's samples and the real frame's magnitudes
        a = np.concatenate([a, a[:, -2:-1] if ghost else np.zeros_like(a[:, :1])], axis=1)
        m = np.concatenate([m, m[:, -1:] if ghost else np.zeros_like(m[:, :1])], axis=1)
    a, m = a.reshape(B, TP, 2, n), m.reshape(B, TP, 2, F)
    Z = emu_fft(_cx(a[:, :, 0], a[:, :, 1]), -1)
    k = np.arange(F)
    kn = (n - k) & (n - 1)
    if mut == "dc_pair":
        kn[0] = n - 1
    zk, zn = Z[..., k], Z[..., kn]
    x1x, x1y = F32(0.5) * (zk.real + zn.real), F32(0.5) * (zk.imag - zn.imag)
    x2x, x2y = F32(0.5) * (zk.imag + zn.imag), F32(-0.5) * (zk.real - zn.real)
    if mut == "nyquist_sign":
        x2x[..., -1] = -x2x[..., -1]
    p1x, p1y = _unit(x1x, x1y)
    p2x, p2y = _unit(x2x, x2y)
    w1x, w1y, w2x, w2y = m[:, :, 0] * p1x, m[:, :, 0] * p1y, m[:, :, 1] * p2x, m[:, :, 1] * p2y
    for w in (w1y, w2y):
        w[..., 0] = w[..., -1] = 0
    V = np.concatenate([_cx(w1x - w2y, w1y + w2x), _cx(w1x + w2y, -w1y + w2x)[..., 1:n // 2][..., ::-1]], axis=-1)
    v = emu_fft(V, +1)
    h = emu_windows(n, hop, framing)[1] * F32(1.0 / n)
    out = np.stack([v.real * h, v.imag * h], axis=2).reshape(B, 2 * TP, n)
    flat = np.full((B * T + 1, n), GUARD, dtype=F32)
    if T % 2 and mut == "phantom_frame":
        flat[np.arange(B) * T + T] = out[:, T]        # one frame past the item's last; the real frames land afterwards
    flat[:B * T] = out[:, :T].reshape(B * T, n)
    return flat


def judge_project_flat(flat, y, mag, n, hop, framing, ref=None):
    B, T, _ = mag.shape
    out = R.judge_project(flat[:B * T].reshape(B, T, n), y, mag, n, hop, framing, ref)
    out["guard"] = 0.0 if (flat[B * T] == GUARD).all() else float("inf")
    return out


def emu_gl_prepare(lin32, min_db=-100.0, ref_db=20.0, power=1.4, mut=None):
    x = lin32 if mut == "no_clip" else np.clip(lin32, F32(0), F32(1))
    db = x * F32(-min_db) + F32(min_db) + F32(ref_db)
    e = db * F32(0.05) * F32(power) * F32(3.32192809488736234787)
    with np.errstate(over="ignore"):
        return np.exp2(e.astype(np.float64)).astype(F32)


def emu_db_norm(x32, min_db=-100.0, ref_db=20.0):
    ml = F32(np.exp2(np.float64(F32(min_db) * F32(0.05) * F32(3.32192809488736234787))))
    lg = np.log10(np.maximum(ml, x32).astype(np.float64)).astype(F32)
    db = (20.0 * lg.astype(np.float64) - ref_db).astype(F32)
    return np.clip((db - F32(min_db)) / F32(-min_db), F32(0), F32(1))


def emu_preemph(x32, coef):
    s = x32.astype(np.float64)
    s[:, 1:] = s[:, 1:] - float(F32(coef)) * x32[:, :-1].astype(np.float64)
    return s.astype(F32)


def emu_deemph_serial(x32, coef, lens=None):
    c = F32(coef)
    y = x32.copy()
    for b in range(y.shape[0]):
        L = y.shape[1] if lens is None else min(max(int(lens[b]), 0), y.shape[1])
        y[b, L:] = 0
        if L == 0:
            continue
        ln = -(-L // 256)
        pad = np.zeros(256 * ln, dtype=F32)
        pad[:L] = y[b, :L]
        seg = pad.reshape(256, ln)
        cnt = np.clip(L - np.arange(256) * ln, 0, ln)
        v = np.zeros(256, dtype=F32)
        for i in range(ln):
            v = np.where(i < cnt, seg[:, i] + c * v, v)
            seg[:, i] = v
        carry, cc = np.zeros(256, dtype=F32), F32(0)
        for s in range(256):
            carry[s] = cc
            cc = v[s] + F32(np.float64(c) ** float(cnt[s])) * cc
        g = c
        for i in range(ln):
            seg[:, i] = np.where(carry != 0, seg[:, i] + g * carry, seg[:, i])
            g = g * c
        y[b, :L] = seg.reshape(-1)[:L]
    return y


def emu_deemph_chunked(x32, coef, lens=None, mut=None):
    c = F32(coef)
    W, CH, E = R.DEEMPH_W, R.DEEMPH_CH, R.DEEMPH_E
    y = np.zeros_like(x32)
    cE = c
    for _ in range(E - (2 if mut == "carry_pow15" else 1)):
        cE = cE * c
    for b in range(x32.shape[0]):
        L = x32.shape[1] if lens is None else min(max(int(lens[b]), 0), x32.shape[1])
        for out0 in range(0, L, CH):
            i = out0 - W + np.arange(256 * E)
            v = np.where((i >= 0) & (i < L), x32[b, np.clip(i, 0, L - 1)], F32(0)).reshape(256, E).astype(F32)
            acc = np.zeros(256, dtype=F32)
            for j in range(E):
                acc = v[:, j] + c * acc
                v[:, j] = acc
            carry, cc = np.zeros(256, dtype=F32), F32(0)
            for s in range(256):
                carry[s] = cc
                cc = acc[s] + cE * cc
            g = c
            for j in range(E):
                v[:, j] = v[:, j] + g * carry
                g = g * c
            keep = (i >= out0) & (i < L)
            y[b, i[keep]] = v.reshape(-1)[keep]
    return y


def emu_deemph(x32, coef, lens, inplace, mut=None):
    if R.deemph_form(coef, inplace) == "serial":
        return emu_deemph_serial(x32, coef, lens)
    return emu_deemph_chunked(x32, coef, lens, mut)


# ----------------------------------------------------------------------------------------------------------------------
# the references against the oracle
# ----------------------------------------------------------------------------------------------------------------------
def _configs(n):
    return [(fr, hop) for fr in R.FRAMINGS for hop in R.hops(n)]


@pytest.mark.parametrize("n", R.SIZES)
def test_references_match_the_oracle(n):
    """spectrum, inverse and one projection against oracle/audio_oracle.py; the impulse family against its analytic
    answer w[m] exp(-2 pi i k m / n); the emulated transform against numpy's"""
    rng = np.random.RandomState(n)
    z = (rng.randn(3, n) + 1j * rng.randn(3, n)).astype(C64)
    for sign in (-1, 1):
        want = np.fft.fft(z.astype(np.complex128)) if sign < 0 else np.fft.ifft(z.astype(np.complex128)) * n
        assert np.abs(emu_fft(z, sign) - want).max() < 1e-5 * np.abs(want).max()
    for fr, hop in _configs(n):
        y = R.family_W(n, hop, fr, B=2, T=9)
        Z = R.spectrum_ref(y, n, hop, fr)[0]
        Zo = A.lws_stft(y.astype(np.float64), n, hop) if fr == "lws" else A.stft(torch.from_numpy(y).double(), hop, n).numpy()
        assert Z.shape == Zo.shape and np.abs(Z - Zo).max() < 1e-11 * np.abs(Zo).max()
        mag = np.abs(Z).astype(F32)
        f = R.project_ref(y, mag, n, hop, fr)[0]
        back = R.ola_ref(f, np.zeros_like(f), n, hop, fr)[0]
        S = mag.astype(np.float64) * Z / np.abs(Z)
        want = A.lws_istft(S, hop) if fr == "lws" else A.istft(torch.from_numpy(S), hop, n).numpy()
        assert back.shape == want.shape and np.abs(back - want).max() < 1e-11 * np.abs(want).max()
        ph = np.stack([np.cos(np.angle(Z)), np.sin(np.angle(Z))], axis=-1).astype(F32)
        f2 = R.frames_ref(mag, ph, n, hop, fr)[0]
        assert np.abs(f2 - f).max() < 1e-6 * np.abs(f).max()                 # the fp32 phasors round
        # impulses: frames with a single non-zero sample
        x = R.family_I(n, hop, fr)
        a = R.frames_in(x, n, hop, fr)[0]
        Zi = R.spectrum_ref(x, n, hop, fr)[0]
        w = R.windows(n, hop, fr)[0]
        one = (a != 0).sum(-1) == 1
        assert (one | ((a != 0).sum(-1) == 0)).all()                         # no frame holds an impulse twice
        m = np.abs(a).argmax(-1)
        seen = np.unique(m[one])
        assert set(range(1, n - 1)) <= set(seen.tolist())                    # every offset (w[0] = 0: no sample there)
        k = np.arange(n // 2 + 1)
        want = w[m[one]][:, None] * np.exp(-2j * np.pi * k[None, :] * m[one][:, None] / n)
        assert np.abs(Zi[one] - want).max() < 1e-12


# ----------------------------------------------------------------------------------------------------------------------
# the emulation stays inside every bound; every mutant breaks one
# ----------------------------------------------------------------------------------------------------------------------
def _spectrum_ratios(n, fam, mut=None):
    out = {}
    for fr, hop in _configs(n):
        if mut == "twiddle_fp16" and hop * 4 != n:
            continue
        y = {"W": R.family_W, "S": R.family_S, "I": R.family_I}[fam](n, hop, fr)
        got = emu_stft(y, n, hop, fr, mut)
        for k, v in R.judge_spectrum(got, y, n, hop, fr).items():
            out["%s %s hop %d %s" % (fam, fr, hop, k)] = v
        if mut is None and fam != "I":
            spec = np.stack([got.real, got.imag], -1)
            out["%s %s hop %d phasor" % (fam, fr, hop)] = R.judge_phasor(emu_phasor(got), spec)["phasor"]
    return out


def _inverse_inputs(n, hop, fam, B=3, T=12):
    """family W: random magnitudes and phasors; family S: the staircase across frames, items at 2^12, 1, 2^-12"""
    rng = np.random.RandomState(n + hop + (fam == "S"))
    F = n // 2 + 1
    mag = rng.rand(B, T, F)
    if fam == "S":
        mag = mag * (4.0 ** -np.arange(T))[None, :, None] * np.array([2.0 ** 12, 1.0, 2.0 ** -12])[:, None, None]
    phz = rng.uniform(-np.pi, np.pi, (B, T, F))
    return mag.astype(F32), np.stack([np.cos(phz), np.sin(phz)], axis=-1).astype(F32)


def _istft_ratios(n, fam, mut=None):
    out = {}
    for fr, hop in _configs(n):
        mag, ph = _inverse_inputs(n, hop, fam)
        y, interior = emu_ola(emu_frames(mag, ph, n, hop, fr), n, hop, fr, mut)
        assert (interior == R.ola_ref(np.zeros((1, 12, n)), np.zeros((1, 12, n)), n, hop, fr)[2]).all()
        j = R.judge_istft(y, mag, ph, n, hop, fr)
        assert j.pop("n_switch") == (4 if (fr == "torch" and hop * 4 == n) else 0)
        for k, v in j.items():
            out["%s %s hop %d %s" % (fam, fr, hop, k)] = v
    return out


def _single_bin_ratios(n):
    mag, ph, phi = R.family_K(n)
    out = {}
    for fr in R.FRAMINGS:
        hop = n // 4
        out["K %s" % fr] = R.judge_frames(emu_frames(mag, ph, n, hop, fr), mag, ph, n, hop, fr)["frames"]
    # the reference of this family is the closed form (c / n) cos(2 pi k m / n + phi) w[m], c = 2 inside, 1 (and the real
    # part of the phasor alone) at DC and Nyquist
    f = R.frames_ref(mag, ph, n, n // 4, "torch")[0][0]
    w = R.windows(n, n // 4, "torch")[1]
    m = np.arange(n)
    for k in (0, 1, n // 4 + 1, n // 2):
        p = ph[0, k, k].astype(np.float64)
        c = 2.0 if 0 < k < n // 2 else 1.0
        want = c / n * (p[0] * np.cos(2 * np.pi * k * m / n) - (p[1] * np.sin(2 * np.pi * k * m / n) if c == 2 else 0)) * w
        assert np.abs(f[k] - want).max() < 1e-15
    return out


_tone_cache = {}


def _tone_case(n, fr, hop, T, bins, q):
    """the inputs and the reference of one launch, shared by the emulation and the mutants"""
    key = (n, fr, hop, T, q)
    if key not in _tone_cache:
        y, mag = R.family_T(n, hop, fr, T, bins, q)
        _tone_cache[key] = (y, mag, R.project_ref(y, mag, n, hop, fr))
    return _tone_cache[key]


@pytest.fixture(scope="module", autouse=True)
def _release_cache():
    yield
    _tone_cache.clear()


def _project_ratios(n, mut=None, quiet=True):
    """every launch of the tone family; a mutant: the two launches at hop n/4 (T even and odd)"""
    out = {}
    for fr in R.FRAMINGS:
        for hop, T, bins, q in R.tone_launches(n, fr):
            if (q and not quiet) or (mut is not None and hop * 4 != n):
                continue
            y, mag, ref = _tone_case(n, fr, hop, T, bins, q)
            j = judge_project_flat(emu_project(y, mag, n, hop, fr, mut), y, mag, n, hop, fr, ref)
            tag = "T%s %s hop %d T %d" % ("q" if q else "", fr, hop, T)
            out[tag], out[tag + " guard"] = j["all"], j["guard"]
            if q:
                out[tag + " quiet frames"] = j["odd"]
                print("%s: error / own peak: loud frames %.3g, quiet frames %.3g" % (tag, j["rel_even"], j["rel_odd"]))
    return out


def _show(tag, ratios):
    for k in sorted(ratios):
        _report("%s %s" % (tag, k), ratios[k])
    return max(ratios.values())


@pytest.mark.parametrize("n", R.SIZES)
def test_emulation_stays_inside_every_bound(n):
    worst = 0.0
    for fam in ("W", "S", "I"):
        worst = max(worst, _show("emu n %d spectrum" % n, _spectrum_ratios(n, fam)))
    for fam in ("W", "S"):
        worst = max(worst, _show("emu n %d istft" % n, _istft_ratios(n, fam)))
    worst = max(worst, _show("emu n %d frames" % n, _single_bin_ratios(n)))
    worst = max(worst, _show("emu n %d project" % n, _project_ratios(n)))
    assert worst <= 1.0, worst


@pytest.mark.parametrize("n", R.SIZES)
def test_silence(n):
    """a silent item: exact zeros, everything finite, and the emulation's neighbours unchanged (they share nothing)"""
    for fr, hop in _configs(n):
        y = R.family_W(n, hop, fr)
        y[1] = 0
        Z = emu_stft(y, n, hop, fr)
        assert (Z[1] == 0).all() and (emu_phasor(Z)[1] == 0).all() and np.isfinite(emu_phasor(Z)).all()
        ref, b = R.phasor_ref(np.zeros((1, 2, 3, 2), dtype=F32))
        assert (ref == 0).all()
        mag = np.zeros((2, 5, n // 2 + 1), dtype=F32)
        f, b = R.project_ref(y[:2, :R.signal_len(5, n, hop, fr)], mag, n, hop, fr)
        assert (f == 0).all() and (b == 0).all()


@pytest.mark.parametrize("n", R.SIZES)
def test_tone_bounds_stay_below_the_cap(n):
    """the condition on family T: every per-sample projection bound is below 1e-3 of its frame's peak reference amplitude
    (the 2^-16 variant: its loud frames; its quiet frames' bound is their partner's and is reported)"""
    for fr in R.FRAMINGS:
        for hop, T, bins, q in R.tone_launches(n, fr):
            y, mag, (f, b) = _tone_case(n, fr, hop, T, bins, q)
            peak = np.abs(f).max(-1)
            assert (b.max(-1)[peak == 0] == 0).all()
            r = np.where(peak > 0, b.max(-1) / np.where(peak > 0, peak, 1.0), 0.0)
            loud = r[:, 0::2] if q else r
            print("n %d %s hop %d T %d%s: bound / peak <= %.3g%s"
                  % (n, fr, hop, T, " (2^-16 variant)" if q else "", loud.max(), ", quiet frames %.3g" % r[:, 1::2].max() if q else ""))
            assert loud.max() < 1e-3, (n, fr, hop, T, float(loud.max()))
            assert (mag > 0).any(-1).all() or fr == "lws"


MUTANTS = {"hann_symmetric": lambda n, m: _spectrum_ratios(n, "W", m), "twiddle_fp16": lambda n, m: _spectrum_ratios(n, "I", m),
           "reflect_off": lambda n, m: _spectrum_ratios(n, "W", m), "two_thirds_edge": lambda n, m: _istft_ratios(n, "W", m),
           "dc_pair": lambda n, m: _project_ratios(n, m, quiet=False), "nyquist_sign": lambda n, m: _project_ratios(n, m, quiet=False),
           "phantom_frame": lambda n, m: _project_ratios(n, m, quiet=False)}


@pytest.mark.parametrize("n", R.SIZES)
@pytest.mark.parametrize("mutant", sorted(MUTANTS))
def test_mutant_breaks_a_bound(mutant, n):
    ratios = MUTANTS[mutant](n, mutant)
    broken = {k: v for k, v in ratios.items() if v > 1.0}
    _report("mutant %s n %d (%d of %d checks broken)" % (mutant, n, len(broken), len(ratios)), max(ratios.values()))
    assert broken, (mutant, n, max(ratios.values()))


# ----------------------------------------------------------------------------------------------------------------------
# point-wise kernels and de-emphasis
# ----------------------------------------------------------------------------------------------------------------------
def test_pointwise_emulations_and_the_clip_mutant():
    lin = R.grid_gl_prepare()
    for power in (1.4, 1.0):
        mag, rb = R.gl_prepare_ref(lin, power=power)
        r = R.worst(np.abs(emu_gl_prepare(lin, power=power) / mag - 1), rb)
        _report("emu gl_prepare power %.1f (bound at x = 0: %.0f u)" % (power, rb[lin == 0][0] / R.U), r)
        assert r <= 1.0
        assert R.worst(np.abs(emu_gl_prepare(lin, power=power, mut="no_clip") / mag - 1), rb) > 1.0
    assert 95 < R.gl_prepare_ref(np.zeros(1))[1][0] / R.U < 105
    for ref_db in (20.0, -20.0):
        x = R.grid_db_norm(ref_db=ref_db)
        out, b = R.db_norm_ref(x, ref_db=ref_db)
        r = R.worst(np.abs(emu_db_norm(x, ref_db=ref_db) - out), b)
        _report("emu amp_to_db_norm ref_db %.0f (largest bound %.1f u)" % (ref_db, b.max() / R.U), r)
        assert r <= 1.0 and out.min() == (0 if ref_db > 0 else 0.2) or abs(out.min() - 0.2) < 1e-12
        assert out.max() == 1
    x = R.deemph_input(3073)
    for coef in (0.97, -0.5, 0.0):
        s, b = R.preemph_ref(x, coef)
        got = emu_preemph(x, coef)
        r = R.worst(np.abs(got[:, 1:] - s[:, 1:]), b[:, 1:])
        _report("emu preemphasis coef %g" % coef, r)
        assert r <= 1.0 and (got[:, 0] == x[:, 0]).all()


@pytest.mark.parametrize("coef", R.DEEMPH_COEFS)
def test_deemphasis_emulations_and_the_carry_mutant(coef):
    worst, bit = 0.0, False
    for L in R.DEEMPH_LENGTHS:
        x = R.deemph_input(L)
        for inplace in (False, True):
            for lens in R.deemph_lens(L):
                r = R.judge_deemph(emu_deemph(x, coef, lens, inplace), x, coef, lens, inplace)["deemph"]
                worst = max(worst, r)
                assert r <= 1.0, (coef, L, inplace, lens, r)
                # coef^16 first meets a non-zero carry at the third 16-sample segment
                if R.deemph_form(coef, inplace) == "chunked" and coef != 0 and L > 32 and lens is None:
                    m = R.judge_deemph(emu_deemph(x, coef, lens, inplace, "carry_pow15"), x, coef, lens, inplace)["deemph"]
                    assert m > 1.0, (coef, L, m)
                    bit = True
    _report("emu deemphasis coef %g (%s)" % (coef, R.deemph_form(coef, False)), worst)
    assert bit or coef in (0.0, 0.9995)

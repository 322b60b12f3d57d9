# coding: utf-8
"""float64 references and DERIVED element-wise error bounds for the audio kernels of csrc/audio.hip.  numpy only, no GPU.

tests/test_gpu_audio_elementwise.py holds the kernels to these; tests/test_cpu_audio_kernels_ref.py shows on fp32
emulations that the bounds hold for a correct implementation and break for mutated ones.  Framing, windows, STFT / iSTFT
and the filters are oracle/audio_oracle.py's wherever it restates the operation; this file adds the per-frame windowed
input a[n], one Griffin-Lim projection, and the bounds.  Nothing below is tuned to what a kernel returns: every constant
is counted from the source.  u = 2^-24 (fp32 unit roundoff).  SLACK = 1.001 multiplies every first-order bound and
swallows the second-order terms (the largest first-order relative error used here is ~ 1e-4).

ASSUMED (no accuracy table of the device math library is at hand): the OpenCL full-profile limits it is written to --
sinpi / cospi 4 ulp, log10 3 ulp, exp2 3 ulp, pow 16 ulp; division and sqrtf correctly rounded (the build has no
fast-math flag).  k ulp of a result r is at most 2 k u |r|.  The compiler may or may not contract a * b + c into an
fma: a bound counts the roundings of the uncontracted form, which the contracted one never exceeds.

WINDOWS.  torch framing: hann(n) = 0.5 - 0.5 cospif(2 n / N) (also hann_t from the W table: same function).  2 n / N is
exact; cospif errs by <= 8 u |c|; 0.5 c is exact; the subtraction rounds once:  dh[n] = 4 u |cos(2 pi n / N)| + u h[n].
NOTE this is absolute, not relative to h[n] (near n = 0, h ~ (pi n / N)^2 is far below 4 u): a single constant c_win
times sum |a| cannot state it, so the window term enters per sample.
lws framing: aw / sw are fp32 tables of the float64 windows: dh[n] = u |w[n]|.

FRAMED INPUT.  a[n] = rn(y[i(n)] h^[n]):  da[n] = |y[i(n)]| dh[n] + u |a[n]|.

ONE FFT PASS (fft_lds).  A radix-4 butterfly forms out_q = sum_r s_qr (w_r v_r), s in {1, -1, i, -i} (exact), w_0 = 1.
  * twiddle: the argument (k r / (4 ns), or the index of the W table) is exact; sincospif errs by <= 8 u per component
    relative, so |w^ - w| <= 8 u;
  * the complex product: |fl(v w) - v w| <= sqrt(5) u |v| |w| (Brent, Percival & Zimmermann 2007; 2 u with fma);
  * two levels of complex additions, each relative u of its own result.
Let an element carry the mass M (the sum of |a_n| over the inputs it combines, which bounds its modulus).  An output of
mass M_out = M_0 + .. + M_3 gets (8 + sqrt 5) u (M_1 + M_2 + M_3) + u M_out (level 1: each half its own mass) + u M_out
(level 2):  C4 = 10 + sqrt 5 = 12.24 per radix-4 pass, and for the radix-2 pass u + w v: C2 = 9 + sqrt 5 = 11.24.
Errors of earlier passes pass through with |w^| <= 1 + 8 u.
Per bin, P4 radix-4 and P2 radix-2 passes:    |Z^_k - Z_k| <= SLACK [sum_n da[n] + (C4 P4 + C2 P2) u sum_n |a[n]|].
Norm-wise (Higham, Accuracy and Stability, Thm 24.2 form): a butterfly is sqrt(radix) times a unitary map, so the same
local errors in the 2-norm are C u ||out||_2 per pass and later passes keep them (scaled like the data):
    ||Z^ - Z||_2 <= SLACK [sqrt(N) ||da||_2 + (C4 P4 + C2 P2) u ||Z||_2]    over all N bins.
The kernel returns N/2 + 1 bins and its computed spectrum need not be exactly Hermitian, so the left side is taken over
the returned bins UNWEIGHTED (a subset of the N) and the right side is the Hermitian-weighted norm of the reference (=
its N-bin norm): rigorous, and tighter than weighting both sides.
P4, P2 = 5, 0 at 1024; 4, 1 at 512; 5, 1 at 2048.

PHASOR, mag_bct (functions of the kernel's OWN returned spectrum z, which the bounds above pin to float64).
mag_bct = sqrtf(rn(x^2) + rn(y^2)), contraction off: reproduced in numpy float32 BIT FOR BIT.  phasor = z * inv, inv =
1 / fmaxf(|z|^, 1e-8f): the squares and their sum err by 2 u relative, the root halves that and adds its own u, so
|z|^ is 2 u off; the division adds u, the product u:  per component 4 u relative (+ 2^-149, the
subnormal spacing).  |z|^ < 1e-8 gives z * rn(1 / 1e-8f); a zero z gives exact zeros.

INVERSE FRAMES (istft_frames_kernel).  A_k = m_k (p_k.x, p_k.y): one rounding per component, dA_k = u |A_k|; the imaginary
part at DC / Nyquist is dropped and the Hermitian fill copies.  The inverse transform's per-sample bound over all N
bins: ev = SLACK [sum_k dA_k + Cfft u sum_k |A_k|].  out = rn(Bf.x (1/N) h^[n]) (1/N exact):
    |out[n] - f[n]| <= SLACK [(ev (h[n] + dh[n]) + |v[n]| dh[n]) / N + u |f[n]|],   v = N irfft(A).
OVERLAP-ADD (ola_kernel), J frames cover a sample, added in ascending t: sum of the frame bounds + (J - 1) u sum_t |f_t|.
Normaliser, torch framing: interior (hop = N/4, four whole frames): acc * rn(2/3): 2 u relative.  Edge: acc / wsum, wsum
= sum rn(h^2): dW = sum (2 h dh + u h^2) + (J - 1) u W;  |y^ - y| <= SLACK [num / (W - dW) + |y| (dW / (W - dW) + u)].
lws framing: the synthesis window carries the normaliser; no further rounding.

PROJECTION (gl_project2_kernel: frames 2q, 2q+1 ride one complex transform).  a = a1 + i a2, so per bin
    E = SLACK [sum da1 + sum da2 + Cfft u (sum |a1| + sum |a2|)]   bounds |Z^_k - Z_k| at EVERY k: both frames' sums
enter each frame's bound.  X1 = (Z_k + conj Z_{N-k}) / 2: (E + E) / 2 plus one rounding per component of the sum (the
halving is exact): dX_k = E + u |X_k|.  Unit phase: |a/|a| - b/|b|| <= 2 |a - b| / (|a| + |b|) gives rho_k = dX_k /
(|X_k| - dX_k / 2); sqrtf / division / two products add 5 u:  dw_k = m_k (rho_k + 5 u) (bins with m_k = 0 give exact
zeros whatever the phase; where dX_k reaches |X_k| the phase is not determined and rho_k = 2, the distance of two unit
vectors at most -- the tone family keeps away from that by construction, except the quiet frames of its 2^-16 variant).
V_k = w1^_k + i w2^_k and V_{N-k} = conj w1^_k + i conj w2^_k are formed from the SAME computed w^, so the exact inverse
transform of the exact V keeps the frames apart whatever the phase errors are: its real part is the inverse of w1^ alone.
Frame 1 therefore takes its own sum dw1, the packing's one rounding u (|w1^_k| + |w2^_k|) and the transform's Cfft u sum
|V_k|, with |w^_k| <= m_k:      ev1 = SLACK [sum dw1 + (1 + Cfft) u sum_k (m1_k + m2_k)]    over all N bins,
then the window and 1/N as for the inverse frames.  (The partner's phase error dw2 does NOT enter: adding it would make
the bound of a loud frame next to a quiet one vacuous for no reason.)  A frame carries its partner twice: Cfft u sum
|a_partner| in its phase, and (1 + Cfft) u sum m_partner in its samples.  That is the cost of the packing, stated here
and measured by the tests on a frame 2^-16 below its partner.  An unpaired last frame has a zero partner.

gl_prepare (relative).  x = clip(lin, 0, 1) exact; db = x (-min_db) + min_db + ref_db: ddb = u (|x min_db| + |x (-min_db) +
min_db| + |db|); e = db * 0.05f * power * log2(10)f: three products and two rounded constants (0.05f, log2(10)f; `power`
is the kernel's float argument, the reference uses that float): de = 5 u |e| + ddb |e / db|; exp2f: 6 u:
    |mag^ / mag - 1| <= SLACK [ln2 de + 6 u]      (100 u at x = 0 with the presets -100 / 20 / 1.4: ln2 (93 + 42) + 6).
amp_to_db_norm (absolute).  min_level^ = exp2f(rn(rn(min_db 0.05f) log2(10)f)): relative dml = ln2 3 u |e| + 6 u, only
felt where x <= min_level (1 + dml).  L = log10f(m): dL = dm / ln 10 + 6 u |L|; db = fmaf(20, L, -ref): 20 dL + u |db|;
(db - min_db): u; the division: u;  clip is 1-Lipschitz:
    |out^ - out| <= SLACK [(20 dL + u |db| + u |db - min_db|) / |min_db| + u |q|].
preemphasis.  One fmaf: |got - s| <= (1/2) ulp32(s) (1 + 2^-28), s = x[i] - coef32 x[i-1] in float64 (the product is
exact there); y[0] = x[0] exactly.

DE-EMPHASIS y[i] = x[i] + c y[i-1].  Both forms scan segments locally from zero state, chain the segment carries through
one thread, then add g_j * carry with g_j = c^(j+1) by repeated products.  Magnitudes Y[i] = |x[i]| + |c| Y[i-1] bound
the true values.  Local scan (two roundings a step): el[i] = |c| el[i-1] + u (|c| Yl[i-1] + Yl[i]).  Carry: ec' = el[end]
+ |c|^n ec + (rp + u) |c|^n Yc + u Yc', rp = 32 u (powf, serial form) or 15 u (c^16 by fifteen products, chunked form).
Output: e[i] = el[i] + |c|^(j+1) ec + (j + 1) u |c|^(j+1) Yc + u Y[i].  Chunked form, chunks after the first: the warm-up
starts W = 1024 samples early from zero state: + |c|^W / (1 - |c|) max |x|.  Which form runs is dv3_deemphasis_f32's own
rule, restated in deemph_form.
"""
import numpy as np

from oracle import audio_oracle as A

U = 2.0 ** -24
SLACK = 1.001
ULP_SINCOSPI, ULP_LOG10, ULP_EXP2, ULP_POW = 4, 3, 3, 16
C4 = 2 * ULP_SINCOSPI + np.sqrt(5.0) + 2.0
C2 = 2 * ULP_SINCOSPI + np.sqrt(5.0) + 1.0
SIZES = (512, 1024, 2048)
FRAMINGS = ("torch", "lws")
DEEMPH_W, DEEMPH_CH, DEEMPH_E = 1024, 3072, 16


def hops(n):
    return (n // 4, 3 * n // 16)


def passes(n):
    """(radix-4 passes, radix-2 passes) of fft_lds<n>"""
    return {512: (4, 1), 1024: (5, 0), 2048: (5, 1)}[n]


def c_fft(n):
    p4, p2 = passes(n)
    return C4 * p4 + C2 * p2


# ----------------------------------------------------------------------------------------------------------------------
# windows and framing
# ----------------------------------------------------------------------------------------------------------------------
def windows(n, hop, framing):
    """-> (analysis window, synthesis window, d analysis, d synthesis) as float64 [n]"""
    if framing == "lws":
        aw, sw = A.lws_windows(n, hop)
        return aw, sw, U * np.abs(aw), U * np.abs(sw)
    k = np.arange(n, dtype=np.float64)
    c = np.cos(2.0 * np.pi * k / n)
    h = 0.5 - 0.5 * c
    dh = 2 * ULP_SINCOSPI * U * 0.5 * np.abs(c) + U * h
    return h, h, dh, dh


def num_frames(L, n, hop, framing):
    return A.lws_num_frames(L, n, hop) if framing == "lws" else L // hop + 1


def num_samples(T, n, hop, framing):
    return (T + 1) * hop - n if framing == "lws" else hop * (T - 1)


def gather_index(L, T, n, hop, framing, reflect_shift=0):
    """index [T, n] into the signal of every frame sample, -1 where the framing puts a zero.  reflect_shift: the CPU
    test's mutant (right-edge reflection off by one)"""
    i = np.arange(T)[:, None] * hop + np.arange(n)[None, :]
    if framing == "lws":
        i = i - (n - hop)
        return np.where((i >= 0) & (i < L), i, -1)
    i = np.abs(i - n // 2)
    return np.where(i >= L, 2 * (L - 1) - i + reflect_shift, i)


def frames_in(y, n, hop, framing):
    """y [B, L] -> (a, da): the windowed frames a[b, t, n] in float64 and the bound on the kernel's own"""
    y = np.asarray(y, dtype=np.float64)
    L = y.shape[1]
    T = num_frames(L, n, hop, framing)
    idx = gather_index(L, T, n, hop, framing)
    ys = np.where(idx >= 0, y[:, np.maximum(idx, 0)], 0.0)
    w, _, dw, _ = windows(n, hop, framing)
    a = ys * w
    return a, np.abs(ys) * dw + U * np.abs(a)


def spectrum_ref(y, n, hop, framing):
    """-> Z [B, T, n/2+1] complex128, per-bin bound [B, T, 1], l2 bound [B, T] (see the docstring: left side unweighted
    over the returned bins)"""
    a, da = frames_in(y, n, hop, framing)
    Z = np.fft.rfft(a, axis=-1)
    bin_bound = SLACK * (da.sum(-1) + c_fft(n) * U * np.abs(a).sum(-1))[..., None]
    znorm = np.sqrt(n) * np.linalg.norm(a, axis=-1)              # Parseval: the N-bin norm of Z
    l2_bound = SLACK * (np.sqrt(n) * np.linalg.norm(da, axis=-1) + c_fft(n) * U * znorm)
    return Z, bin_bound, l2_bound


# ----------------------------------------------------------------------------------------------------------------------
# phasor and mag_bct from the kernel's own spectrum
# ----------------------------------------------------------------------------------------------------------------------
def mag_bct_exact(spec32):
    """spec32 [B, T, F, 2] float32 -> [B, F, T] float32, the bits cabs_f returns"""
    x, y = spec32[..., 0].astype(np.float32), spec32[..., 1].astype(np.float32)
    return np.sqrt((x * x).astype(np.float32) + (y * y).astype(np.float32), dtype=np.float32).transpose(0, 2, 1)


def phasor_ref(spec32):
    """-> (phasor [B, T, F, 2] float64, bound per component)"""
    z = spec32.astype(np.float64)
    inv = 1.0 / np.maximum(np.hypot(z[..., 0], z[..., 1]), float(np.float32(1e-8)))
    ph = z * inv[..., None]
    return ph, SLACK * 4 * U * np.abs(ph) + 2.0 ** -149


# ----------------------------------------------------------------------------------------------------------------------
# inverse frames, overlap-add
# ----------------------------------------------------------------------------------------------------------------------
def _window_out(v, ev, n, hop, framing):
    """v = N * (the inverse transform's real output), ev its bound -> (frames, bound)"""
    _, sw, _, dsw = windows(n, hop, framing)
    f = v * sw / n
    return f, SLACK * ((ev * (np.abs(sw) + dsw) + np.abs(v) * dsw) / n + U * np.abs(f))


def frames_ref(mag, phasor, n, hop, framing):
    """mag [B, T, F], phasor [B, T, F, 2] (the fp32 values; None: zero phase) -> (frames [B, T, n], bound)"""
    mag = np.asarray(mag, dtype=np.float64)
    S = mag.astype(np.complex128) if phasor is None else mag * (phasor[..., 0].astype(np.float64) + 1j * phasor[..., 1])
    S[..., 0] = S[..., 0].real
    S[..., -1] = S[..., -1].real
    absA = 2 * np.abs(S).sum(-1) - np.abs(S[..., 0]) - np.abs(S[..., -1])          # over all N bins
    ev = SLACK * ((0.0 if phasor is None else U) + c_fft(n) * U) * absA
    return _window_out(np.fft.irfft(S, n=n, axis=-1) * n, ev[..., None], n, hop, framing)


def ola_ref(frames, fbound, n, hop, framing):
    """frames / fbound [B, T, n] -> (y [B, L], bound, interior [L] bool: the samples that take the 2/3 shortcut)"""
    B, T, _ = frames.shape
    L = num_samples(T, n, hop, framing)
    off = n - hop if framing == "lws" else n // 2
    h, _, dh, _ = windows(n, hop, "torch")
    tot = (T - 1) * hop + n
    acc, eacc, aabs, W, dW, J = (np.zeros((B, tot)), np.zeros((B, tot)), np.zeros((B, tot)), np.zeros(tot),
                                 np.zeros(tot), np.zeros(tot))
    for t in range(T):
        s = slice(t * hop, t * hop + n)
        acc[:, s] += frames[:, t]
        eacc[:, s] += fbound[:, t]
        aabs[:, s] += np.abs(frames[:, t])
        W[s] += h * h
        dW[s] += 2 * h * dh + U * h * h
        J[s] += 1
    cut = slice(off, off + L)
    acc, eacc, aabs, W, dW, J = acc[:, cut], eacc[:, cut], aabs[:, cut], W[cut], dW[cut], J[cut]
    num = eacc + (J - 1) * U * aabs
    if framing == "lws":
        return acc, SLACK * num, np.ones(L, dtype=bool)
    p = np.arange(L) + off
    interior = (hop * 4 == n) & (p >= n - hop) & (p // hop <= T - 1)                 # four whole frames: t_lo .. t_lo + 3
    y = acc / W
    dW = dW + (J - 1) * U * W
    edge = SLACK * (num / (W - dW) + np.abs(y) * (dW / (W - dW) + U))
    inner = SLACK * (num / 1.5 + 2 * U * np.abs(y))
    return y, np.where(interior, inner, edge), interior


# ----------------------------------------------------------------------------------------------------------------------
# one Griffin-Lim projection: stft -> unit phase -> x mag -> istft frames
# ----------------------------------------------------------------------------------------------------------------------
def project_ref(y, mag, n, hop, framing):
    """y [B, L], mag [B, T, F] -> (frames [B, T, n], bound [B, T, n]); frames (2q, 2q+1) share a transform"""
    a, da = frames_in(y, n, hop, framing)
    B, T, _ = a.shape
    mag = np.asarray(mag, dtype=np.float64)
    assert mag.shape == (B, T, n // 2 + 1)
    X = np.fft.rfft(a, axis=-1)
    absX = np.abs(X)
    ph = X / np.maximum(absX, 1e-300)
    S = mag * ph
    S[..., 0] = S[..., 0].real
    S[..., -1] = S[..., -1].real
    v = np.fft.irfft(S, n=n, axis=-1) * n
    sda, sa = da.sum(-1), np.abs(a).sum(-1)                                          # [B, T]
    partner = np.arange(T) ^ 1
    has = partner < T
    pz = np.where(has, partner, 0)
    E = SLACK * (sda + np.where(has, sda[:, pz], 0.0) + c_fft(n) * U * (sa + np.where(has, sa[:, pz], 0.0)))
    dX = E[..., None] + U * absX
    rho = np.where(absX > dX, dX / np.maximum(absX - 0.5 * dX, 1e-300), 2.0)         # two unit vectors differ by <= 2
    rho = np.where(mag > 0, np.minimum(rho, 2.0), 0.0)
    dw = mag * (rho + 5 * U)
    full = lambda q: 2 * q.sum(-1) - q[..., 0] - q[..., -1]                          # noqa: E731  (one-sided -> N bins)
    sdw, sm = full(dw), full(mag)
    smp = np.where(has, sm[:, pz], 0.0)
    ev = SLACK * (sdw + (1.0 + c_fft(n)) * U * (sm + smp))
    return _window_out(v, ev[..., None], n, hop, framing)


# ----------------------------------------------------------------------------------------------------------------------
# point-wise kernels
# ----------------------------------------------------------------------------------------------------------------------
def gl_prepare_ref(lin, min_db=-100.0, ref_db=20.0, power=1.4):
    """-> (mag float64, relative bound)"""
    p32 = float(np.float32(power))
    lin = np.asarray(lin, dtype=np.float64)
    mag = A.magnitudes(lin, min_db, ref_db, p32)
    x = np.clip(lin, 0, 1)
    db = x * -min_db + min_db + ref_db
    ddb = U * (np.abs(x * min_db) + np.abs(x * -min_db + min_db) + np.abs(db))
    scale = 0.05 * p32 * np.log2(10.0)
    de = 5 * U * np.abs(db * scale) + ddb * scale
    return mag, SLACK * (np.log(2.0) * de + 2 * ULP_EXP2 * U)


def db_norm_ref(x, min_db=-100.0, ref_db=20.0):
    """-> (out float64, absolute bound)"""
    x = np.asarray(x, dtype=np.float64)
    out = A.normalize(A.amp_to_db(x, min_db) - ref_db, min_db)
    ml = 10.0 ** (min_db / 20.0)
    e = abs(min_db * 0.05 * np.log2(10.0))
    dml = np.log(2.0) * 3 * U * e + 2 * ULP_EXP2 * U
    m = np.maximum(ml, x)
    dm = np.where(x <= ml * (1 + 2 * dml), 2 * dml, 0.0)         # relative; 2 x: either side of the floor's own error
    Lg = np.log10(m)
    dL = dm / np.log(10.0) + 2 * ULP_LOG10 * U * np.abs(Lg)
    db = 20 * Lg - ref_db
    q = (db - min_db) / -min_db
    return out, SLACK * ((20 * dL + U * np.abs(db) + U * np.abs(db - min_db)) / abs(min_db) + U * np.abs(q))


def ulp32(s):
    s = np.abs(np.asarray(s, dtype=np.float64))
    e = np.floor(np.log2(np.maximum(s, 2.0 ** -126)))
    return 2.0 ** (e - 23)


def preemph_ref(x32, coef):
    """x32 [B, L] float32 -> (s float64, bound); bound[:, 0] = 0"""
    c = float(np.float32(coef))
    s = A.preemphasis(x32.astype(np.float64), c)
    b = 0.5 * ulp32(s) * (1 + 2.0 ** -28)
    b[..., 0] = 0.0
    return s, b


# ----------------------------------------------------------------------------------------------------------------------
# de-emphasis
# ----------------------------------------------------------------------------------------------------------------------
def deemph_form(coef, inplace):
    """dv3_deemphasis_f32's rule, in its own float arithmetic"""
    a = np.float32(abs(np.float32(coef)))
    ok = a < 1 and (a == 0 or np.float32(DEEMPH_W) * np.log(a, dtype=np.float32) <=
                    np.log(np.float32(1e-9) * (np.float32(1) - a), dtype=np.float32))
    return "chunked" if ok and not inplace else "serial"


def _scan(x, c):
    """y[i] = x[i] + c y[i-1] along the last axis from zero state (scipy's lfilter through the oracle)"""
    return A.inv_preemphasis(x, c) if x.shape[-1] else x


def _deemph_bound_span(ax, c, seg, rp, e_tail):
    """|x| of one row over one span that starts from zero state, segments of `seg` samples -> bound per sample"""
    n = ax.shape[0]
    nseg = -(-n // seg)
    pad = np.zeros(nseg * seg)
    pad[:n] = ax
    Y = _scan(ax[None], c)[0]                                     # global magnitudes of the span
    Yl = _scan(pad.reshape(nseg, seg), c)                         # segment-local magnitudes
    Ylp = np.concatenate([np.zeros((nseg, 1)), Yl[:, :-1]], axis=1)
    el = _scan(U * (c * Ylp + Yl), c)                             # the local scan's error
    g = c ** np.arange(1, seg + 1)
    out = np.zeros(nseg * seg)
    ec, Yc = 0.0, 0.0
    for s in range(nseg):
        cnt = min(seg, n - s * seg)
        out[s * seg:(s + 1) * seg] = el[s] + g * ec + np.arange(1, seg + 1) * U * g * Yc
        Yn = Y[s * seg + cnt - 1]
        ec = el[s, cnt - 1] + g[cnt - 1] * ec + (rp + U) * g[cnt - 1] * Yc + U * Yn
        Yc = Yn
    return SLACK * (out[:n] + U * Y) + e_tail


def deemph_ref(x32, coef, lens=None, inplace=False):
    """x32 [B, L] float32 -> (y float64, bound).  lens: row b filters its first clamp(lens[b], 0, L) samples, zeros after"""
    c32 = float(np.float32(coef))
    c = abs(c32)
    x = x32.astype(np.float64)
    B, L = x.shape
    y, bound = np.zeros((B, L)), np.zeros((B, L))
    form = deemph_form(coef, inplace)
    for b in range(B):
        Lb = L if lens is None else min(max(int(lens[b]), 0), L)
        if Lb == 0:
            continue
        y[b, :Lb] = A.inv_preemphasis(x[b, :Lb], c32)
        ax = np.abs(x[b, :Lb])
        if form == "serial":
            bound[b, :Lb] = _deemph_bound_span(ax, c, -(-Lb // 256), 2 * ULP_POW * U, 0.0)
        else:
            tail = c ** DEEMPH_W / (1 - c) * ax.max()
            for out0 in range(0, Lb, DEEMPH_CH):
                lo, hi = max(out0 - DEEMPH_W, 0), min(out0 + DEEMPH_CH, Lb)
                e = _deemph_bound_span(ax[lo:hi], c, DEEMPH_E, (DEEMPH_E - 1) * U, tail if out0 else 0.0)
                bound[b, out0:hi] = e[out0 - lo:]
    return y, bound


# ----------------------------------------------------------------------------------------------------------------------
# input families (float32 arrays, as the kernels receive them)
# ----------------------------------------------------------------------------------------------------------------------
def signal_len(T, n, hop, framing):
    return num_samples(T, n, hop, framing)


def family_W(n, hop, framing, B=3, T=12, seed=0):
    """unit white noise"""
    rng = np.random.RandomState(seed + n + hop)
    return rng.randn(B, signal_len(T, n, hop, framing)).astype(np.float32)


def family_S(n, hop, framing, T=12, seed=1):
    """staircase: the level falls by 2^-2 per hop; items at 2^12, 1, 2^-12"""
    L = signal_len(T, n, hop, framing)
    rng = np.random.RandomState(seed + n + hop)
    env = 4.0 ** -(np.arange(L) // hop).astype(np.float64)
    x = rng.randn(3, L) * env * np.array([2.0 ** 12, 1.0, 2.0 ** -12])[:, None]
    return x.astype(np.float32)


def family_I(n, hop, framing):
    """one unit sample per item, at every position of one hop: every frame offset is hit in some frame.  torch framing:
    the positions start at n/2 + 1 and the signal ends more than n/2 behind them, so no reflection doubles an impulse"""
    if framing == "lws":
        L, p0 = 5 * hop, 2 * hop
    else:
        L, p0 = hop * -(-(n + hop + 2) // hop), n // 2 + 1
    x = np.zeros((hop, L), dtype=np.float32)
    x[np.arange(hop), p0 + np.arange(hop)] = 1.0
    return x


def family_K(n, seed=2):
    """mag = 1 at bin t of frame t alone, T = n/2 + 1 frames of one item, arbitrary phasors (also at DC and Nyquist)"""
    F = n // 2 + 1
    rng = np.random.RandomState(seed + n)
    mag = np.eye(F, dtype=np.float32)[None]
    phi = rng.uniform(-np.pi, np.pi, (1, F, F))
    phi[0, 0, 0], phi[0, -1, -1] = 0.7, 2.4                       # a non-zero imaginary part where c2r must ignore it
    ph = np.stack([np.cos(phi), np.sin(phi)], axis=-1).astype(np.float32)
    return mag, ph, phi


def family_T(n, hop, framing, T, bins, quiet_odd=False, seed=3):
    """one bin-centred cosine per item (bin bins[b], arbitrary phase); mag random in [0.5, 1] where the REFERENCE has
    |Z_k| >= max_k |Z_k| / 4 of that frame, 0 elsewhere.  quiet_odd (torch framing at hop = n, where frames share no
    sample but the one reflected at the left edge): the odd frames' input is 2^-16 of the even frames'."""
    L = signal_len(T, n, hop, framing)
    rng = np.random.RandomState(seed + n + hop + T)
    bins = np.asarray(bins)
    phi = rng.uniform(-np.pi, np.pi, (len(bins), 1))
    y = np.cos(2 * np.pi * bins[:, None] * np.arange(L)[None, :] / n + phi)
    if quiet_odd:
        assert framing == "torch" and hop == n
        y = y * np.where(((np.arange(L) + n // 2) // n) % 2 == 0, 1.0, 2.0 ** -16)[None, :]
    y = y.astype(np.float32)
    Z = np.abs(spectrum_ref(y, n, hop, framing)[0])
    mag = np.where(Z >= 0.25 * Z.max(-1, keepdims=True), rng.uniform(0.5, 1.0, Z.shape), 0.0)
    mag[Z.max(-1) == 0] = 0.0
    return y, mag.astype(np.float32)


def tone_launches(n, framing):
    """[(hop, T, bins, quiet_odd)]: four launches -- both hops, even and odd T (an unpaired last frame) -- that between
    them put a tone on every bin 0 .. n/2 (launch j takes the bins = j mod 4; the bins at and next to DC and Nyquist ride
    in every launch), and on the torch framing the 2^-16 variant at hop = n"""
    edge = [0, 1, n // 2 - 1, n // 2]
    out = []
    for j, (hop, T) in enumerate([(n // 4, 6), (n // 4, 7), (3 * n // 16, 7), (3 * n // 16, 6)]):
        out.append((hop, T, sorted(set(edge) | set(range(j, n // 2 + 1, 4))), False))
    if framing == "torch":
        out.append((n, 5, edge + [n // 8 + 1, n // 3], True))
    return out


def worst(err, bound):
    """max of err / bound; an error where the bound is zero counts as infinite"""
    err, bound = np.asarray(err, dtype=np.float64), np.broadcast_to(np.asarray(bound, dtype=np.float64), np.shape(err))
    if not np.isfinite(err).all():
        return float("inf")
    r = np.where(bound > 0, err / np.where(bound > 0, bound, 1.0), np.where(err > 0, np.inf, 0.0))
    return float(r.max()) if r.size else 0.0


# ----------------------------------------------------------------------------------------------------------------------
# judgements: the same code holds the fp32 emulations (CPU test) and the kernels (GPU test) to the bounds.  Each returns
# {name: worst ratio}; a ratio above 1 is a broken bound.
# ----------------------------------------------------------------------------------------------------------------------
def to_complex(t):
    t = np.asarray(t)
    return t if np.iscomplexobj(t) else t[..., 0].astype(np.float64) + 1j * t[..., 1].astype(np.float64)


def judge_spectrum(got, y, n, hop, framing):
    """got [B, T, F] complex or [B, T, F, 2]: every bin against its frame's per-bin bound, every frame in the 2-norm"""
    got = to_complex(got).astype(np.complex128)
    Z, bb, l2 = spectrum_ref(y, n, hop, framing)
    assert got.shape == Z.shape, (got.shape, Z.shape)
    err = np.abs(got - Z)
    return {"bin": worst(err, bb), "l2": worst(np.linalg.norm(err, axis=-1), l2)}


def judge_phasor(got_ph, spec32):
    ref, b = phasor_ref(np.asarray(spec32))
    return {"phasor": worst(np.abs(np.asarray(got_ph, dtype=np.float64) - ref), b)}


def judge_frames(got, mag, phasor, n, hop, framing):
    f, b = frames_ref(mag, phasor, n, hop, framing)
    return {"frames": worst(np.abs(np.asarray(got, dtype=np.float64) - f), b)}


def judge_istft(got, mag, phasor, n, hop, framing):
    """through the overlap-add: all samples, the first and last n, and both sides of every interior / edge switch"""
    f, fb = frames_ref(mag, phasor, n, hop, framing)
    y, b, interior = ola_ref(f, fb, n, hop, framing)
    got = np.asarray(got, dtype=np.float64)
    assert got.shape == y.shape, (got.shape, y.shape)
    err = np.abs(got - y)
    sw = np.flatnonzero(interior[1:] != interior[:-1])
    sw = np.unique(np.concatenate([sw, sw + 1])).astype(int)
    return {"all": worst(err, b), "head": worst(err[:, :n], b[:, :n]), "tail": worst(err[:, -n:], b[:, -n:]),
            "switch": worst(err[:, sw], b[:, sw]), "n_switch": len(sw)}


def judge_project(got, y, mag, n, hop, framing, ref=None):
    """got [B, T, n] -> worst ratio, and per frame parity (the 2^-16 variant reports its quiet frames apart).  ref: what
    project_ref returns for these inputs, where the caller judges several results against it"""
    f, b = ref if ref is not None else project_ref(y, mag, n, hop, framing)
    err = np.abs(np.asarray(got, dtype=np.float64) - f)
    peak = np.abs(f).max(-1)
    rel = np.where(peak > 0, err.max(-1) / np.where(peak > 0, peak, 1.0), 0.0)    # error / the frame's own peak
    return {"all": worst(err, b), "even": worst(err[:, 0::2], b[:, 0::2]), "odd": worst(err[:, 1::2], b[:, 1::2]),
            "rel_even": float(rel[:, 0::2].max()), "rel_odd": float(rel[:, 1::2].max())}


# grids of the point-wise kernels: the edge values and both neighbours of each
def _around(vals):
    v = np.asarray(vals, dtype=np.float32)
    return np.concatenate([v, np.nextafter(v, np.float32(-np.inf)), np.nextafter(v, np.float32(np.inf))])


def grid_gl_prepare():
    """[0, 1] densely, the clip ends and their neighbours, values outside the clip"""
    rng = np.random.RandomState(5)
    return np.concatenate([np.linspace(0, 1, 1001).astype(np.float32), _around([0.0, 1.0]), rng.rand(1000).astype(np.float32),
                           np.float32([-0.5, -1e-30, -0.0, 1.5, 1e30, -1e30])])


def grid_db_norm(min_db=-100.0, ref_db=20.0):
    """140 dB of amplitudes, 0 and below, the floor and the two clip ends with their neighbours"""
    rng = np.random.RandomState(6)
    ml = 10.0 ** (min_db / 20.0)
    lo, hi = 10.0 ** ((min_db + ref_db) / 20.0), 10.0 ** (ref_db / 20.0)             # where the result meets 0 and 1
    return np.concatenate([(10.0 ** rng.uniform(-7, 2, 3000)).astype(np.float32), _around([0.0, ml, lo, hi, 1.0]),
                           np.float32([-1.0, -0.0, 1e-30, 1e-45, 1e30])])


DEEMPH_LENGTHS = (1, 15, 16, 17, 3071, 3072, 3073, 6145, 20481)
DEEMPH_COEFS = (0.97, 0.5, 0.0, -0.97, 0.9995)


def deemph_input(L, seed=7):
    """B = 2 rows (odd L: the second row starts misaligned), noise on a DC offset of 0.5"""
    rng = np.random.RandomState(seed + L)
    return (0.5 + rng.randn(2, L)).astype(np.float32)


def deemph_lens(L):
    return [None, (0, L + 5), (1, L)]


def judge_deemph(got, x32, coef, lens, inplace):
    y, b = deemph_ref(x32, coef, lens, inplace)
    got = np.asarray(got, dtype=np.float64)
    out = {"deemph": worst(np.abs(got - y), b)}
    if lens is not None:                                        # exact zeros after the item's own samples
        for r, lb in enumerate(lens):
            if not (got[r, min(max(lb, 0), got.shape[1]):] == 0).all():
                out["deemph"] = float("inf")
    return out

// Audio inverse on the GPU: what synthesis.py does on the host after the model,
// audio.inv_spectrogram (audio.py:37-43): _denormalize -> _db_to_amp (audio.py:84-93) -> magnitude
// ** power -> phase reconstruction -> istft -> inv_preemphasis (audio.py:26-28).
//
// The reference delegates phase reconstruction to the third-party `lws` package (not vendored,
// "parity unpinned"); the north-star asks for Griffin-Lim as FFT + reduction kernels.
// These kernels implement Griffin-Lim with torch.stft / torch.istft conventions (periodic Hann
// window of n_fft points, hop as given, center=True with reflect padding, onesided n_fft/2 + 1 bins,
// istft normalised by the overlap-added squared window) so the CPU oracle (oracle/audio_oracle.py)
// can be an independent restatement on torch-CPU FFTs.
//
// One workgroup (256 threads) transforms one N-point frame in LDS, N = 512, 1024 or 2048 (a template
// parameter of every kernel that frames): Stockham auto-sort radix-4 passes, at 512 and 2048 closed
// by one radix-2 pass (fft_lds), twiddles from sincospif or a table.  Frames are independent, so the
// grid is B*T workgroups; the only cross-frame step is the overlap-add, a gather over the frames
// that cover a sample (<= 4 at hop = N/4; deterministic, no atomics).  The preset's size, 1024 / 256,
// is what the entry points without an n_fft argument run.
#include "common.h"

#include <type_traits>

namespace {

constexpr float PI_F = 3.14159265358979323846f;

struct cplx {
  float x, y;
};
__device__ __forceinline__ cplx cmul(cplx a, cplx b) { return {a.x * b.x - a.y * b.y, a.x * b.y + a.y * b.x}; }
__device__ __forceinline__ cplx cadd(cplx a, cplx b) { return {a.x + b.x, a.y + b.y}; }
__device__ __forceinline__ cplx csub(cplx a, cplx b) { return {a.x - b.x, a.y - b.y}; }

// per-item frame count (the *_items entry points): tlen[b] clamped to [tlo, T], tlo = the fewest frames the framing takes
// at this hop (the host's bound: no read outside the item's own signal whatever the device array holds); NULL: T
__device__ __forceinline__ int item_frames(const int32_t* tlen, int b, int T, int tlo) {
  return tlen ? min(max(tlen[b], tlo), T) : T;
}
template <int NFFT, bool LWS>
__device__ __forceinline__ int item_samples(int Tb, int hop) { return LWS ? (Tb + 1) * hop - NFFT : hop * (Tb - 1); }

template <int NFFT>
__device__ __forceinline__ float hann(int n) { return 0.5f - 0.5f * cospif(2.0f * (float)n / (float)NFFT); }

// ---- forward-analysis steps shared by the batch path (preemphasis_kernel, stft_phase_kernel<true>,
// amp_to_db_norm_kernel) and the ragged one (analysis_items_kernel).  Each states its roundings explicitly (fmaf, or
// contraction off): whether the compiler contracts a * b + c depends on the code around it, and the two paths must round
// alike.  The forms are the ones the batch kernels compiled to before they shared them. ----
// y[i] = x[i] - coef * x[i-1] (one rounding), y[0] = x[0]   (nnmnkwii.preprocessing.preemphasis, audio.py:21-23)
__device__ __forceinline__ float preemph(float cur, float prev, float coef) { return fmaf(-coef, prev, cur); }
__device__ __forceinline__ float preemph_at(const float* x, int i, float coef) { return i ? preemph(x[i], x[i - 1], coef) : x[0]; }
// x * gain rounded on its own (never contracted into the preemphasis that reads it): the product a host computes
// in fp32 before it hands the rescaled signal to the batch path
__device__ __forceinline__ float gain_mul(float x, float g) {
#pragma clang fp contract(off)
  return x * g;
}
// the lws framing of frame t into A: aw[n] * sample(t * hop + n - (NFFT - hop)) inside [0, L), zeros outside
template <int NFFT, class Sample>
__device__ __forceinline__ void lws_frame(cplx* A, int t, int hop, int L, const float* aw, int tid, Sample sample) {
  for (int n = tid; n < NFFT; n += 256) {
    const int i = t * hop + n - (NFFT - hop);
    A[n] = cplx{(i >= 0 && i < L) ? sample(i) * aw[n] : 0.f, 0.f};
  }
}
// |z| = sqrt(rn(x^2) + rn(y^2)): both squares rounded, no fused multiply-add
__device__ __forceinline__ float cabs_f(cplx z) {
#pragma clang fp contract(off)
  return sqrtf(z.x * z.x + z.y * z.y);
}
// amp_to_db_norm: clip((20*log10(max(min_level, x)) - ref_db - min_db) / -min_db, 0, 1)   audio.py:34-35,79-89
__device__ __forceinline__ float db_min_level(float min_db) { return exp2f(min_db * 0.05f * 3.32192809488736234787f); }
__device__ __forceinline__ float db_norm(float x, float min_level, float min_db, float ref_db) {
  const float db = fmaf(20.0f, log10f(fmaxf(min_level, x)), -ref_db);
  return fminf(fmaxf((db - min_db) / (-min_db), 0.f), 1.f);
}

// W[j] = exp(+2 pi i j / NFFT), filled once per workgroup (4 sincospif per thread instead of 3 per butterfly and
// pass: the transcendental calls were most of a frame's instructions).  hann(n) = 0.5 - 0.5 * Re W[n].
template <int NFFT>
__device__ __forceinline__ void fill_twiddles(cplx* W, int tid) {
  for (int j = tid; j < NFFT; j += 256) {
    float s, c;
    sincospif(2.0f * (float)j / (float)NFFT, &s, &c);
    W[j] = cplx{c, s};
  }
}
__device__ __forceinline__ float hann_t(const cplx* W, int n) { return 0.5f - 0.5f * W[n].x; }

// In-LDS N-point complex FFT, N = 512, 1024 or 2048 (SIGN = -1 forward, +1 inverse, unnormalised).  `a` holds the
// input in natural order; the result ends in `b`.  256 threads.  Stockham auto-sort: radix-4 passes at strides ns = 1,
// 4, ... while 4 ns <= N (five at 1024 and 2048, four at 512; a->b->a->...), each of the N/4 butterflies of a pass by
// thread j mod 256: one per thread at 1024, two at 2048, and at 512 only threads 0..127 -- waves 0 and 1 whole, waves 2
// and 3 idle, so the predicate is wave-uniform.  512 = 2 * 4^4 and 2048 = 2 * 4^5 leave one radix-2 pass, taken LAST
// (ns = N/2): there butterfly j reads and writes the same two elements j and j + N/2, so it may run in place.  At 2048
// the radix-4 passes end in `b` and the radix-2 pass stays there; at 512 they end in `a` and it moves the result to `b`.
// Its twiddle is exp(SIGN 2 pi i j / N) = W[j] itself.  One barrier per pass (in front of it) and one after the last.
template <int N, int SIGN>
__device__ __forceinline__ void fft_lds(cplx* a, cplx* b, int tid, const cplx* W = nullptr) {
  static_assert(N == 512 || N == 1024 || N == 2048, "fft_lds: 512, 1024 or 2048 points");
  cplx* src = a;
  cplx* dst = b;
#pragma unroll
  for (int ns = 1; ns * 4 <= N; ns *= 4) {
    __syncthreads();
#pragma unroll
    for (int u = 0; u < (N == 2048 ? 2 : 1); ++u) {
      const int j = tid + 256 * u;                    // this thread's butterfly
      if (N == 512 && j >= N / 4) continue;           // 128 butterflies: waves 0 and 1
      const int k = j & (ns - 1);
      const float ang = (float)SIGN * 2.0f * (float)k / (float)(ns * 4);  // in units of pi
      cplx v[4];
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        v[r] = src[j + r * (N / 4)];
        if (r) {
          if (W) {       // exp(SIGN * 2 pi i k r / (4 ns)) = W[k r (N/4)/ns] (conjugated for SIGN < 0); k r / (4 ns) < 3/4
            const cplx w = W[k * r * (N / 4 / ns)];
            v[r] = cmul(v[r], cplx{w.x, SIGN < 0 ? -w.y : w.y});
          } else {
            float s, c;
            sincospif(ang * (float)r, &s, &c);
            v[r] = cmul(v[r], cplx{c, s});
          }
        }
      }
      // radix-4 DFT, natural order: X[q] = sum_m v[m] * w^(q*m), w = exp(SIGN * i*pi/2)
      const cplx s02 = cadd(v[0], v[2]), d02 = csub(v[0], v[2]);
      const cplx s13 = cadd(v[1], v[3]), d13 = csub(v[1], v[3]);
      const cplx jd13 = (SIGN < 0) ? cplx{d13.y, -d13.x} : cplx{-d13.y, d13.x};  // w * d13
      const int j0 = ((j - k) << 2) + k;  // (j / ns) * ns * 4 + k
      dst[j0] = cadd(s02, s13);
      dst[j0 + ns] = cadd(d02, jd13);
      dst[j0 + 2 * ns] = csub(s02, s13);
      dst[j0 + 3 * ns] = csub(d02, jd13);
    }
    cplx* t = src; src = dst; dst = t;
  }
  if constexpr (N != 1024) {   // the radix-2 pass at ns = N/2: X[j] = u + w v, X[j + N/2] = u - w v, into `b` (src == b: in place)
    __syncthreads();
#pragma unroll
    for (int j = tid; j < N / 2; j += 256) {
      const cplx u = src[j];
      cplx v = src[j + N / 2];
      if (W) {
        const cplx w = W[j];
        v = cmul(v, cplx{w.x, SIGN < 0 ? -w.y : w.y});
      } else {
        float s, c;
        sincospif((float)SIGN * 2.0f * (float)j / (float)N, &s, &c);
        v = cmul(v, cplx{c, s});
      }
      b[j] = cadd(u, v);
      b[j + N / 2] = csub(u, v);
    }
  }
  __syncthreads();
}

// mag[b][t][k] = (10^((clip(x,0,1)*(-min_db) + min_db + ref_db) / 20)) ^ power      audio.py:39-41,84-93
__global__ void gl_prepare_kernel(const float* __restrict__ lin, float* __restrict__ mag, int64_t n,
                                  float min_db, float ref_db, float power) {
  int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (; i < n; i += stride) {
    const float x = fminf(fmaxf(lin[i], 0.f), 1.f);
    const float db = x * (-min_db) + min_db + ref_db;
    mag[i] = exp2f(db * 0.05f * power * 3.32192809488736234787f);  // 10^(db/20*power)
  }
}

// frames[b][t][n] = hann[n] * irfft(mag[b][t][:] * phasor[b][t][:])[n]   (phasor NULL: zero phase)
// LWS: the conventions of lws.lws(NFFT, hop) (audio.py:54-55; oracle/audio_oracle.py: lws_windows): `sw` = the
// perfect-reconstruction synthesis window (the overlap-add normaliser is folded into it)
template <int NFFT, bool LWS>
__global__ __launch_bounds__(256) void istft_frames_kernel(const float* __restrict__ mag,
                                                           const float* __restrict__ phasor,
                                                           float* __restrict__ frames, const float* __restrict__ sw,
                                                           const int32_t* __restrict__ tlen, int T, int tlo) {
  constexpr int NBIN = NFFT / 2 + 1;
  __shared__ cplx A[NFFT], Bf[NFFT];
  const int tid = threadIdx.x;
  const int64_t fr = blockIdx.x;
  if (tlen && (int)(fr % T) >= item_frames(tlen, (int)(fr / T), T, tlo)) return;   // past the item's own frames
  const float* m = mag + fr * NBIN;
  const float* ph = phasor ? phasor + fr * NBIN * 2 : nullptr;
  for (int k = tid; k <= NFFT / 2; k += 256) {
    cplx z{m[k], 0.f};
    if (ph) z = cplx{m[k] * ph[2 * k], m[k] * ph[2 * k + 1]};
    if (k == 0 || k == NFFT / 2) z.y = 0.f;  // c2r ignores the imaginary part of DC / Nyquist
    A[k] = z;
    if (k > 0 && k < NFFT / 2) A[NFFT - k] = cplx{z.x, -z.y};
  }
  fft_lds<NFFT, +1>(A, Bf, tid);
  float* out = frames + fr * NFFT;
  for (int n = tid; n < NFFT; n += 256) out[n] = Bf[n].x * (1.0f / NFFT) * (LWS ? sw[n] : hann<NFFT>(n));
}

// y[b][i] = sum_t frames[b][t][p - t*hop] / sum_t hann^2[p - t*hop],  p = i + NFFT/2, i < hop*(T-1)
// LWS: p = i + (NFFT - hop) (the zero padding lws strips), no division (the synthesis window carries the normaliser)
// tlen (per item): item b overlap-adds its own Tb frames into its own item_samples(Tb) samples, zeros after them
template <int NFFT, bool LWS>
__global__ void ola_kernel(const float* __restrict__ frames, float* __restrict__ y, int T, int hop,
                           int L, const int32_t* __restrict__ tlen, int tlo) {
  const int b = blockIdx.y;
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= L) return;
  const int Tb = item_frames(tlen, b, T, tlo);
  if (tlen && i >= item_samples<NFFT, LWS>(Tb, hop)) {
    y[(int64_t)b * L + i] = 0.f;
    return;
  }
  const int p = i + (LWS ? NFFT - hop : NFFT / 2);
  int t_hi = p / hop;
  if (t_hi > Tb - 1) t_hi = Tb - 1;
  int t_lo = (p - NFFT + hop) / hop;  // smallest t with p - t*hop <= NFFT-1  (ceil((p-NFFT+1)/hop))
  if (p - NFFT + 1 <= 0) t_lo = 0;
  float acc = 0.f, wsum = 0.f;
  const float* fb = frames + (int64_t)b * T * NFFT;
  // interior samples of the hop = N/4 periodic-Hann framing meet four frames whose squared windows sum to exactly 3/2
  // (sum_j sin^4(x + j pi/4) = 3/2): no transcendental per tap there; the edges keep the general form
  const bool interior = LWS || (hop * 4 == NFFT && t_hi - t_lo == 3 && p - t_lo * hop < NFFT && p - t_hi * hop >= 0);
  for (int t = t_lo; t <= t_hi; ++t) {
    const int n = p - t * hop;
    if (n < 0 || n >= NFFT) continue;
    acc += fb[(int64_t)t * NFFT + n];
    if (!interior) {
      const float w = hann<NFFT>(n);
      wsum += w * w;
    }
  }
  y[(int64_t)b * L + i] = LWS ? acc : (interior ? acc * (2.0f / 3.0f) : acc / wsum);
}

// phasor[b][t][k] = Z / max(|Z|, 1e-8), Z = rfft(hann * reflect_pad(y[b])[t*hop : t*hop + NFFT])[k]
// (spec, optional: Z itself, for tests / spectral convergence)
// LWS: Z = rfft(aw * zero_pad(y[b], NFFT - hop)[t*hop : t*hop + NFFT]) -- lws.lws(NFFT, hop).stft (sqrt-Hann analysis window
// `aw`, zeros instead of reflection)
template <int NFFT, bool LWS>
__global__ __launch_bounds__(256) void stft_phase_kernel(const float* __restrict__ y,
                                                         float* __restrict__ phasor,
                                                         float* __restrict__ spec,
                                                         float* __restrict__ mag_bct, int T, int hop, int L,
                                                         const float* __restrict__ aw) {
  constexpr int NBIN = NFFT / 2 + 1;
  __shared__ cplx A[NFFT], Bf[NFFT];
  const int tid = threadIdx.x;
  const int b = blockIdx.x / T, t = blockIdx.x - b * T;
  const float* yb = y + (int64_t)b * L;
  if constexpr (LWS) {
    lws_frame<NFFT>(A, t, hop, L, aw, tid, [=](int i) { return yb[i]; });
  } else {
    for (int n = tid; n < NFFT; n += 256) {
      int i = t * hop + n - NFFT / 2;  // index into the un-padded signal
      if (i < 0) i = -i;
      if (i >= L) i = 2 * (L - 1) - i;
      A[n] = cplx{yb[i] * hann<NFFT>(n), 0.f};
    }
  }
  fft_lds<NFFT, -1>(A, Bf, tid);
  const int64_t fr = blockIdx.x;
  for (int k = tid; k <= NFFT / 2; k += 256) {
    const cplx z = Bf[k];
    if (spec) {
      spec[(fr * NBIN + k) * 2] = z.x;
      spec[(fr * NBIN + k) * 2 + 1] = z.y;
    }
    if (mag_bct) mag_bct[((int64_t)b * NBIN + k) * T + t] = cabs_f(z);
    if (phasor) {
      const float inv = 1.0f / fmaxf(cabs_f(z), 1e-8f);
      phasor[(fr * NBIN + k) * 2] = z.x * inv;
      phasor[(fr * NBIN + k) * 2 + 1] = z.y * inv;
    }
  }
}

// One Griffin-Lim projection without leaving LDS: STFT of the current signal estimate -> unit phase -> times the target
// magnitude -> inverse FFT -> synthesis window.  Equals stft_phase_kernel followed by istft_frames_kernel (same
// arithmetic, same order) minus the phasor round trip through HBM (8 KB per frame at 1024), for TWO frames per
// workgroup: both input frames are real, so they ride one complex FFT as
// z = x1 + i x2 (X1[k] = (Z[k] + conj Z[N-k]) / 2, X2[k] = (Z[k] - conj Z[N-k]) / 2i), and the two Hermitian target
// spectra ride one inverse FFT as V = Y1 + i Y2 (y1 = Re v, y2 = Im v): half the FFT passes -- the LDS traffic that
// bounds this kernel -- per frame.  Frames (2q, 2q+1) of one batch item; an odd last frame pairs with nothing.
//
// MOM (fast Griffin-Lim, Perraudin, Balazs & Sondergaard 2013): the phase is taken from t = c + alpha (c - c_prev)
// instead of the consistent spectrum c itself.  cprev [B][T][NBIN] float2 in the frame order of `mag` holds c_prev; every
// (frame, bin) belongs to one thread of one workgroup, which reads c_prev, stores c in its place and normalises t.  The
// reads are issued before the forward FFT and held in registers (at most 5 bins x 2 frames x 2 floats per thread at
// 2048), so their latency lies under the FFT's LDS passes.  `first` (uniform): cprev holds nothing yet -- it is not read
// (t = c) and still written.  The phantom partner of an unpaired last frame and the frames from Tb on are neither read
// nor written.  MOM = false is the instruction stream of the kernel without the option.
template <int NFFT, bool LWS, bool MOM>
__global__ __launch_bounds__(256) void gl_project2_kernel(const float* __restrict__ y, const float* __restrict__ mag,
                                                          float* __restrict__ frames, int T, int hop, int L, int TP,
                                                          const float* __restrict__ aw, const float* __restrict__ sw,
                                                          const int32_t* __restrict__ tlen, int tlo,
                                                          float2* __restrict__ cprev, float alpha, int first) {
  constexpr int NBIN = NFFT / 2 + 1;
  constexpr int KPT = NFFT / 512 + 1;        // bins k = tid + 256 q <= NFFT/2 of one thread (the last one: thread 0 alone)
  __shared__ cplx A[NFFT], Bf[NFFT], W[NFFT];
  const int tid = threadIdx.x;
  const int b = blockIdx.x / TP, t1 = 2 * (blockIdx.x - b * TP);
  const float* yb = y + (int64_t)b * L;      // rows L apart; item b's own signal is its first Lb samples
  const int Tb = item_frames(tlen, b, T, tlo);
  if (t1 >= Tb) return;                      // a pair past the item's own frames (workgroup-uniform, before any barrier)
  const bool two = t1 + 1 < Tb;
  L = tlen ? item_samples<NFFT, LWS>(Tb, hop) : L;
  fill_twiddles<NFFT>(W, tid);
  __syncthreads();
  for (int n = tid; n < NFFT; n += 256) {
    if constexpr (LWS) {      // lws framing: zeros outside the signal, sqrt-Hann analysis window from the table
      const int i1 = t1 * hop + n - (NFFT - hop), i2 = i1 + hop;
      const float h = aw[n];
      A[n] = cplx{(i1 >= 0 && i1 < L) ? yb[i1] * h : 0.f, (two && i2 >= 0 && i2 < L) ? yb[i2] * h : 0.f};
    } else {
      int i1 = t1 * hop + n - NFFT / 2, i2 = i1 + hop;
      if (i1 < 0) i1 = -i1;
      if (i1 >= L) i1 = 2 * (L - 1) - i1;
      if (i2 < 0) i2 = -i2;
      if (i2 >= L) i2 = 2 * (L - 1) - i2;
      const float h = hann_t(W, n);
      A[n] = cplx{yb[i1] * h, two ? yb[i2] * h : 0.f};
    }
  }
  // c_prev of this thread's bins, in flight under the forward transform.  Unconditional per lane (a lane-dependent
  // branch would make the compiler wait for the loads where it ends): a lane past the last bin re-reads bin NFFT/2, and
  // an unpaired last frame, which has no partner row, reads its own row twice -- neither value is used.
  float2 p1[KPT], p2[KPT];
  if constexpr (MOM) {
    if (!first) {
      const float2* c1 = cprev + ((int64_t)b * T + t1) * NBIN;
      const float2* c2 = c1 + (two ? NBIN : 0);
#pragma unroll
      for (int q = 0; q < KPT; ++q) {
        const int k = min(tid + 256 * q, NFFT / 2);
        p1[q] = c1[k];
        p2[q] = c2[k];
      }
    }
  }
  fft_lds<NFFT, -1>(A, Bf, tid, W);
  const int64_t fr = (int64_t)b * T + t1;
  const float* m1 = mag + fr * NBIN;
  const float* m2 = m1 + (two ? NBIN : 0);
  if constexpr (!MOM) {
    for (int k = tid; k <= NFFT / 2; k += 256) {
      const cplx zk = Bf[k], zn = Bf[(NFFT - k) & (NFFT - 1)];
      // X1 = (zk + conj zn) / 2, X2 = (zk - conj zn) / (2i) = ((zk.y + zn.y) - i (zk.x - zn.x)) / 2
      const cplx x1{0.5f * (zk.x + zn.x), 0.5f * (zk.y - zn.y)};
      const cplx x2{0.5f * (zk.y + zn.y), -0.5f * (zk.x - zn.x)};
      const float inv1 = 1.0f / fmaxf(sqrtf(x1.x * x1.x + x1.y * x1.y), 1e-8f);
      const float inv2 = 1.0f / fmaxf(sqrtf(x2.x * x2.x + x2.y * x2.y), 1e-8f);
      cplx w1{m1[k] * (x1.x * inv1), m1[k] * (x1.y * inv1)};
      cplx w2{m2[k] * (x2.x * inv2), m2[k] * (x2.y * inv2)};
      if (k == 0 || k == NFFT / 2) w1.y = w2.y = 0.f;
      if (!two) w2 = cplx{0.f, 0.f};
      // V[k] = w1 + i w2 ; V[N-k] = conj(w1) + i conj(w2)
      A[k] = cplx{w1.x - w2.y, w1.y + w2.x};
      if (k > 0 && k < NFFT / 2) A[NFFT - k] = cplx{w1.x + w2.y, -w1.y + w2.x};
    }
  } else {
    // the same loop, unrolled so that p1 / p2 stay in registers: c = (x1, x2) goes to cprev, the phase comes from t
    float2* c1 = cprev + fr * NBIN;
#pragma unroll
    for (int q = 0; q < KPT; ++q) {
      const int k = tid + 256 * q;
      if (k > NFFT / 2) continue;
      const cplx zk = Bf[k], zn = Bf[(NFFT - k) & (NFFT - 1)];
      const cplx x1{0.5f * (zk.x + zn.x), 0.5f * (zk.y - zn.y)};
      const cplx x2{0.5f * (zk.y + zn.y), -0.5f * (zk.x - zn.x)};
      c1[k] = float2{x1.x, x1.y};
      if (two) c1[NBIN + k] = float2{x2.x, x2.y};
      cplx u1 = x1, u2 = x2;
      if (!first) {                            // t = c + alpha (c - c_prev)
        u1 = cplx{x1.x + alpha * (x1.x - p1[q].x), x1.y + alpha * (x1.y - p1[q].y)};
        u2 = cplx{x2.x + alpha * (x2.x - p2[q].x), x2.y + alpha * (x2.y - p2[q].y)};
      }
      const float inv1 = 1.0f / fmaxf(sqrtf(u1.x * u1.x + u1.y * u1.y), 1e-8f);
      const float inv2 = 1.0f / fmaxf(sqrtf(u2.x * u2.x + u2.y * u2.y), 1e-8f);
      cplx w1{m1[k] * (u1.x * inv1), m1[k] * (u1.y * inv1)};
      cplx w2{m2[k] * (u2.x * inv2), m2[k] * (u2.y * inv2)};
      if (k == 0 || k == NFFT / 2) w1.y = w2.y = 0.f;
      if (!two) w2 = cplx{0.f, 0.f};
      A[k] = cplx{w1.x - w2.y, w1.y + w2.x};
      if (k > 0 && k < NFFT / 2) A[NFFT - k] = cplx{w1.x + w2.y, -w1.y + w2.x};
    }
  }
  fft_lds<NFFT, +1>(A, Bf, tid, W);
  float* out = frames + fr * NFFT;
  for (int n = tid; n < NFFT; n += 256) {
    const float h = (LWS ? sw[n] : hann_t(W, n)) * (1.0f / NFFT);
    out[n] = Bf[n].x * h;
    if (two) out[NFFT + n] = Bf[n].y * h;
  }
}

// y[n] = x[n] + coef * y[n-1] per row (scipy.signal.lfilter([1], [1, -coef]); audio.py:26-28), in
// place.  One workgroup per row: 256 contiguous segments scanned locally, carries chained in LDS.
// lens (per item): row b filters its own first lens[b] samples and is zero after them
__global__ __launch_bounds__(256) void deemphasis_kernel(float* __restrict__ y, int L, float coef,
                                                         const int32_t* __restrict__ lens) {
  __shared__ float seg_end[256];
  __shared__ float carry[256];
  const int tid = threadIdx.x;
  float* row = y + (int64_t)blockIdx.x * L;
  if (lens) {
    const int Lb = min(max(lens[blockIdx.x], 0), L);
    for (int i = Lb + tid; i < L; i += 256) row[i] = 0.f;
    L = Lb;
  }
  const int len = (L + 255) / 256;
  const int lo = min(tid * len, L), hi = min(lo + len, L);
  float v = 0.f;
  for (int i = lo; i < hi; ++i) {
    v = row[i] + coef * v;
    row[i] = v;
  }
  seg_end[tid] = v;
  __syncthreads();
  if (tid == 0) {
    float c = 0.f;  // value of y just before segment s
    for (int s = 0; s < 256; ++s) {
      carry[s] = c;
      const int n = min((s + 1) * len, L) - min(s * len, L);
      c = seg_end[s] + powf(coef, (float)n) * c;
    }
  }
  __syncthreads();
  const float c = carry[tid];
  if (c != 0.f) {
    float g = coef;
    for (int i = lo; i < hi; ++i) {
      row[i] += g * c;
      g *= coef;
    }
  }
}

// y[n] = x[n] - coef * x[n-1], y[0] = x[0]   (nnmnkwii.preprocessing.preemphasis, audio.py:21-23)
__global__ void preemphasis_kernel(const float* __restrict__ x, float* __restrict__ y, int L, float coef) {
  const int b = blockIdx.y;
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= L) return;
  y[(int64_t)b * L + i] = preemph_at(x + (int64_t)b * L, i, coef);
}

// out = clip((20*log10(max(min_level, x)) - ref_db - min_db) / -min_db, 0, 1)   audio.py:34-35,79-89
__global__ void amp_to_db_norm_kernel(const float* __restrict__ x, float* __restrict__ out, int64_t n,
                                      float min_db, float ref_db) {
  int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  const float min_level = db_min_level(min_db);
  for (; i < n; i += stride) out[i] = db_norm(x[i], min_level, min_db, ref_db);
}

// ---- ragged forward analysis (ABI 45, include/dv3hip.h: dv3_analysis_items_f32) ----
// gain[b] = rescaling_max / max|x_b| over item b's own samples, 1 for a silent item.  One workgroup per item; fmaxf is
// exact, so the reduction order does not show in the result.
__global__ __launch_bounds__(256) void item_gain_kernel(const float* __restrict__ x, const int64_t* __restrict__ soff,
                                                        float rescaling_max, float* __restrict__ gain) {
  __shared__ float red[256];
  const int tid = threadIdx.x;
  const int64_t lo = soff[blockIdx.x], hi = soff[blockIdx.x + 1];
  float m = 0.f;
  for (int64_t i = lo + tid; i < hi; i += 256) m = fmaxf(m, fabsf(x[i]));
  red[tid] = m;
  for (int s = 128; s > 0; s >>= 1) {
    __syncthreads();
    if (tid < s) red[tid] = fmaxf(red[tid], red[tid + s]);
  }
  if (tid == 0) gain[blockIdx.x] = red[0] > 0.f ? rescaling_max / red[0] : 1.f;
}

// One workgroup per OUTPUT ROW g of the packed result: frame t = g - foff[b] of item b (foff[b] <= g < foff[b+1]).
// preemphasis (optionally of gain[b] * x) inline -> lws framing of item b's own samples [0, L_b) -> NFFT-point FFT in
// LDS -> |X| -> lin row (dB-normalised) and, from the magnitudes left in LDS, the mel row: one lane per filter, a
// fixed-order fmaf chain over the filter's ascending nonzero bins [band[2m], band[2m+1]).  Nothing of the row depends
// on another item, on B or on the grid: the row is what item b alone gives.  The linear row takes the same steps, in
// the same expressions, as preemphasis_kernel -> stft_phase_kernel<true> -> amp_to_db_norm_kernel.
template <int NFFT, bool GAIN>
__global__ __launch_bounds__(256) void analysis_items_kernel(
    const float* __restrict__ x, const int64_t* __restrict__ soff, const int32_t* __restrict__ foff, int B, int hop,
    float coef, const float* __restrict__ aw, const float* __restrict__ gain, const float* __restrict__ basis,
    const int32_t* __restrict__ band, int n_mels, float min_db, float ref_db, float* __restrict__ lin,
    float* __restrict__ mel) {
  constexpr int NBIN = NFFT / 2 + 1;
  __shared__ cplx A[NFFT], Bf[NFFT];
  const int tid = threadIdx.x;
  const int g = blockIdx.x;
  int lo = 0, hi = B;                                 // the item: largest b with foff[b] <= g
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if (foff[mid] <= g) lo = mid; else hi = mid;
  }
  const int b = lo, t = g - foff[b];
  const float* xb = x + soff[b];
  const int L = (int)(soff[b + 1] - soff[b]);
  if constexpr (GAIN) {
    const float gb = gain[b];
    lws_frame<NFFT>(A, t, hop, L, aw, tid, [=](int i) {
      return i ? preemph(gain_mul(xb[i], gb), gain_mul(xb[i - 1], gb), coef) : gain_mul(xb[0], gb);
    });
  } else {
    lws_frame<NFFT>(A, t, hop, L, aw, tid, [=](int i) { return preemph_at(xb, i, coef); });
  }
  fft_lds<NFFT, -1>(A, Bf, tid);                      // ends with a barrier; the spectrum is in Bf, A is free
  float* Ms = reinterpret_cast<float*>(A);
  const float min_level = db_min_level(min_db);
  for (int k = tid; k < NBIN; k += 256) {
    const float m = cabs_f(Bf[k]);
    Ms[k] = m;
    if (lin) lin[(int64_t)g * NBIN + k] = db_norm(m, min_level, min_db, ref_db);
  }
  if (!mel) return;                                   // workgroup-uniform
  __syncthreads();
  for (int m = tid; m < n_mels; m += 256) {
    const float* w = basis + (int64_t)m * NBIN;
    const int k0 = band ? max(band[2 * m], 0) : 0, k1 = band ? min(band[2 * m + 1], NBIN) : NBIN;
    float acc = 0.f;
    for (int k = k0; k < k1; ++k) acc = fmaf(w[k], Ms[k], acc);
    mel[(int64_t)g * n_mels + m] = db_norm(acc, min_level, min_db, ref_db);
  }
}

}  // namespace

extern "C" int dv3_preemphasis_f32(const float* x, float* y, int32_t B, int32_t L, float coef,
                                   void* stream) {
  DV3_REQUIRE(x && y && B > 0 && L > 0, "preemphasis: bad arguments");
  hipLaunchKernelGGL(preemphasis_kernel, dim3(dv3_cdiv(L, 256), B), dim3(256), 0, (hipStream_t)stream, x, y,
                     L, coef);
  return dv3_check_launch("preemphasis");
}

extern "C" int dv3_amp_to_db_norm_f32(const float* x, float* out, int64_t n, float min_level_db,
                                      float ref_level_db, void* stream) {
  DV3_REQUIRE(x && out && n > 0, "amp_to_db_norm: bad arguments");
  const int blocks = (int)(dv3_cdiv64(n, 256) < 4096 ? dv3_cdiv64(n, 256) : 4096);
  hipLaunchKernelGGL(amp_to_db_norm_kernel, dim3(blocks), dim3(256), 0, (hipStream_t)stream, x, out, n,
                     min_level_db, ref_level_db);
  return dv3_check_launch("amp_to_db_norm");
}

extern "C" int dv3_gl_prepare_f32(const float* lin, float* mag, int64_t n, float min_level_db,
                                  float ref_level_db, float power, void* stream) {
  DV3_REQUIRE(lin && mag && n > 0, "gl_prepare: bad arguments");
  const int blocks = (int)(dv3_cdiv64(n, 256) < 4096 ? dv3_cdiv64(n, 256) : 4096);
  hipLaunchKernelGGL(gl_prepare_kernel, dim3(blocks), dim3(256), 0, (hipStream_t)stream, lin, mag, n,
                     min_level_db, ref_level_db, power);
  return dv3_check_launch("gl_prepare");
}

// ---- the entry points that frame: one host function per entry point, templated on the frame size N.  The entry
// points of ABI <= 48 (no n_fft argument) are the N = 1024 instantiation; their `_n` siblings (ABI 49) pick the
// instantiation from n_fft.  3 * N * 8 bytes of static LDS (A, Bf, W) is 48 KB at 2048; 4096 would need 96 KB, past the
// 64 KB a workgroup may declare, so the siblings take 512, 1024 and 2048 and refuse everything else. ----
template <class F>
static int with_fft_size(const char* what, int32_t n_fft, F f) {
  switch (n_fft) {
    case 512: return f(std::integral_constant<int, 512>{});
    case 1024: return f(std::integral_constant<int, 1024>{});
    case 2048: return f(std::integral_constant<int, 2048>{});
  }
  dv3_set_error("%s: n_fft = %d is not supported: the FFT kernels are built for 512, 1024 and 2048", what, (int)n_fft);
  return DV3_EINVAL;
}

// lws framing: T frames cover (T + 1) * hop - N samples (a signal padded with N - hop zeros on both sides)
template <int N>
static inline int lws_len(int T, int hop) { return (T + 1) * hop - N; }
// the sample counts above and hop * (T - 1) are ints: T and hop are checked with this before either is formed
static inline bool samples_fit(int T, int hop) { return (int64_t)(T + 1LL) * hop <= INT32_MAX; }

template <int N>
static int istft_frames(const float* mag, const float* phasor, float* frames, int32_t B, int32_t T, void* stream) {
  DV3_REQUIRE(mag && frames && B > 0 && T > 0, "istft_frames: bad arguments");
  hipLaunchKernelGGL((istft_frames_kernel<N, false>), dim3((unsigned)((int64_t)B * T)), dim3(256), 0,
                     (hipStream_t)stream, mag, phasor, frames, (const float*)nullptr, (const int32_t*)nullptr, (int)T, 1);
  return dv3_check_launch("istft_frames");
}
template <int N>
static int lws_istft_frames(const float* mag, const float* phasor, const float* swin, float* frames, int32_t B, int32_t T,
                            void* stream) {
  DV3_REQUIRE(mag && frames && swin && B > 0 && T > 0, "lws_istft_frames: bad arguments");
  hipLaunchKernelGGL((istft_frames_kernel<N, true>), dim3((unsigned)((int64_t)B * T)), dim3(256), 0,
                     (hipStream_t)stream, mag, phasor, frames, swin, (const int32_t*)nullptr, (int)T, 1);
  return dv3_check_launch("lws_istft_frames");
}

template <int N>
static int overlap_add(const float* frames, float* y, int32_t B, int32_t T, int32_t hop, void* stream) {
  DV3_REQUIRE(frames && y && B > 0 && T > 1 && hop > 0 && hop <= N && samples_fit(T, hop), "overlap_add: bad arguments");
  const int L = hop * (T - 1);
  hipLaunchKernelGGL((ola_kernel<N, false>), dim3(dv3_cdiv(L, 256), B), dim3(256), 0, (hipStream_t)stream, frames, y,
                     T, hop, L, (const int32_t*)nullptr, 1);
  return dv3_check_launch("overlap_add");
}
template <int N>
static int lws_overlap_add(const float* frames, float* y, int32_t B, int32_t T, int32_t hop, void* stream) {
  DV3_REQUIRE(frames && y && B > 0 && T > 1 && hop > 0 && hop <= N && samples_fit(T, hop) && lws_len<N>(T, hop) > 0,
              "lws_overlap_add: bad arguments");
  const int L = lws_len<N>(T, hop);
  hipLaunchKernelGGL((ola_kernel<N, true>), dim3(dv3_cdiv(L, 256), B), dim3(256), 0, (hipStream_t)stream, frames, y, T, hop, L,
                     (const int32_t*)nullptr, 1);
  return dv3_check_launch("lws_overlap_add");
}
template <int N>
static int lws_stft(const float* y, const float* awin, float* phasor, float* spec, float* mag_bct, int32_t B, int32_t T,
                    int32_t hop, int32_t L, void* stream) {
  DV3_REQUIRE(y && awin && (phasor || spec || mag_bct) && B > 0 && T > 1 && hop > 0 && hop <= N && L > 0 &&
              samples_fit(T, hop), "lws_stft: bad arguments");
  DV3_REQUIRE(L <= lws_len<N>(T, hop) && L > lws_len<N>(T - 1, hop), "lws_stft: %d frames do not frame %d samples at hop %d", T, L, hop);
  hipLaunchKernelGGL((stft_phase_kernel<N, true>), dim3((unsigned)((int64_t)B * T)), dim3(256), 0, (hipStream_t)stream, y, phasor,
                     spec, mag_bct, T, hop, L, awin);
  return dv3_check_launch("lws_stft");
}
template <int N>
static int lws_gl_project(const float* y, const float* mag, const float* awin, const float* swin, float* frames, int32_t B,
                          int32_t T, int32_t hop, void* stream) {
  DV3_REQUIRE(y && mag && frames && awin && swin && B > 0 && T > 1 && hop > 0 && hop <= N && samples_fit(T, hop) &&
              lws_len<N>(T, hop) > 0, "lws_gl_project: bad arguments");
  const int TP = (T + 1) / 2;
  hipLaunchKernelGGL((gl_project2_kernel<N, true, false>), dim3((unsigned)((int64_t)B * TP)), dim3(256), 0, (hipStream_t)stream, y, mag,
                     frames, T, hop, lws_len<N>(T, hop), TP, awin, swin, (const int32_t*)nullptr, 1, (float2*)nullptr, 0.f, 0);
  return dv3_check_launch("lws_gl_project");
}

template <int N>
static int stft_phase(const float* y, float* phasor, float* spec, float* mag_bct, int32_t B, int32_t T, int32_t hop,
                      void* stream) {
  DV3_REQUIRE(y && (phasor || spec || mag_bct) && B > 0 && T > 1 && hop > 0 && samples_fit(T, hop), "stft_phase: bad arguments");
  const int L = hop * (T - 1);
  DV3_REQUIRE(L > N / 2, "stft_phase: signal shorter than the reflect padding");
  hipLaunchKernelGGL((stft_phase_kernel<N, false>), dim3((unsigned)((int64_t)B * T)), dim3(256), 0,
                     (hipStream_t)stream, y, phasor, spec, mag_bct, T, hop, L, (const float*)nullptr);
  return dv3_check_launch("stft_phase");
}

template <int N>
static int gl_project(const float* y, const float* mag, float* frames, int32_t B, int32_t T, int32_t hop, void* stream) {
  DV3_REQUIRE(y && mag && frames && B > 0 && T > 1 && hop > 0 && samples_fit(T, hop), "gl_project: bad arguments");
  const int L = hop * (T - 1);
  DV3_REQUIRE(L > N / 2, "gl_project: signal shorter than the reflect padding");
  const int TP = (T + 1) / 2;     // two real frames per complex FFT
  hipLaunchKernelGGL((gl_project2_kernel<N, false, false>), dim3((unsigned)((int64_t)B * TP)), dim3(256), 0, (hipStream_t)stream, y, mag,
                     frames, T, hop, L, TP, (const float*)nullptr, (const float*)nullptr, (const int32_t*)nullptr, 1, (float2*)nullptr, 0.f, 0);
  return dv3_check_launch("gl_project");
}

extern "C" int dv3_istft_frames_f32(const float* mag, const float* phasor, float* frames, int32_t B,
                                    int32_t T, void* stream) {
  return istft_frames<1024>(mag, phasor, frames, B, T, stream);
}
extern "C" int dv3_istft_frames_f32_n(const float* mag, const float* phasor, float* frames, int32_t B, int32_t T,
                                      int32_t n_fft, void* stream) {
  return with_fft_size("istft_frames", n_fft, [&](auto n) { return istft_frames<decltype(n)::value>(mag, phasor, frames, B, T, stream); });
}
extern "C" int dv3_lws_istft_frames_f32(const float* mag, const float* phasor, const float* swin, float* frames, int32_t B,
                                        int32_t T, void* stream) {
  return lws_istft_frames<1024>(mag, phasor, swin, frames, B, T, stream);
}
extern "C" int dv3_lws_istft_frames_f32_n(const float* mag, const float* phasor, const float* swin, float* frames, int32_t B,
                                          int32_t T, int32_t n_fft, void* stream) {
  return with_fft_size("lws_istft_frames", n_fft,
                       [&](auto n) { return lws_istft_frames<decltype(n)::value>(mag, phasor, swin, frames, B, T, stream); });
}

extern "C" int dv3_overlap_add_f32(const float* frames, float* y, int32_t B, int32_t T, int32_t hop,
                                   void* stream) {
  return overlap_add<1024>(frames, y, B, T, hop, stream);
}
extern "C" int dv3_overlap_add_f32_n(const float* frames, float* y, int32_t B, int32_t T, int32_t hop, int32_t n_fft,
                                     void* stream) {
  return with_fft_size("overlap_add", n_fft, [&](auto n) { return overlap_add<decltype(n)::value>(frames, y, B, T, hop, stream); });
}
extern "C" int dv3_lws_overlap_add_f32(const float* frames, float* y, int32_t B, int32_t T, int32_t hop, void* stream) {
  return lws_overlap_add<1024>(frames, y, B, T, hop, stream);
}
extern "C" int dv3_lws_overlap_add_f32_n(const float* frames, float* y, int32_t B, int32_t T, int32_t hop, int32_t n_fft,
                                         void* stream) {
  return with_fft_size("lws_overlap_add", n_fft, [&](auto n) { return lws_overlap_add<decltype(n)::value>(frames, y, B, T, hop, stream); });
}
extern "C" int dv3_lws_stft_f32(const float* y, const float* awin, float* phasor, float* spec, float* mag_bct, int32_t B,
                                int32_t T, int32_t hop, int32_t L, void* stream) {
  return lws_stft<1024>(y, awin, phasor, spec, mag_bct, B, T, hop, L, stream);
}
extern "C" int dv3_lws_stft_f32_n(const float* y, const float* awin, float* phasor, float* spec, float* mag_bct, int32_t B,
                                  int32_t T, int32_t hop, int32_t L, int32_t n_fft, void* stream) {
  return with_fft_size("lws_stft", n_fft,
                       [&](auto n) { return lws_stft<decltype(n)::value>(y, awin, phasor, spec, mag_bct, B, T, hop, L, stream); });
}
extern "C" int dv3_lws_gl_project_f32(const float* y, const float* mag, const float* awin, const float* swin, float* frames,
                                      int32_t B, int32_t T, int32_t hop, void* stream) {
  return lws_gl_project<1024>(y, mag, awin, swin, frames, B, T, hop, stream);
}
extern "C" int dv3_lws_gl_project_f32_n(const float* y, const float* mag, const float* awin, const float* swin, float* frames,
                                        int32_t B, int32_t T, int32_t hop, int32_t n_fft, void* stream) {
  return with_fft_size("lws_gl_project", n_fft,
                       [&](auto n) { return lws_gl_project<decltype(n)::value>(y, mag, awin, swin, frames, B, T, hop, stream); });
}

extern "C" int dv3_stft_phase_f32(const float* y, float* phasor, float* spec, float* mag_bct, int32_t B,
                                  int32_t T, int32_t hop, void* stream) {
  return stft_phase<1024>(y, phasor, spec, mag_bct, B, T, hop, stream);
}
extern "C" int dv3_stft_phase_f32_n(const float* y, float* phasor, float* spec, float* mag_bct, int32_t B, int32_t T,
                                    int32_t hop, int32_t n_fft, void* stream) {
  return with_fft_size("stft_phase", n_fft, [&](auto n) { return stft_phase<decltype(n)::value>(y, phasor, spec, mag_bct, B, T, hop, stream); });
}

extern "C" int dv3_gl_project_f32(const float* y, const float* mag, float* frames, int32_t B, int32_t T, int32_t hop,
                                  void* stream) {
  return gl_project<1024>(y, mag, frames, B, T, hop, stream);
}
extern "C" int dv3_gl_project_f32_n(const float* y, const float* mag, float* frames, int32_t B, int32_t T, int32_t hop,
                                    int32_t n_fft, void* stream) {
  return with_fft_size("gl_project", n_fft, [&](auto n) { return gl_project<decltype(n)::value>(y, mag, frames, B, T, hop, stream); });
}

// The same filter in parallel over the row.  |coef| < 1, so the response to a sample dies off geometrically: a chunk of
// DEEMPH_CH outputs is exact to fp32 rounding when its recursion starts DEEMPH_W samples earlier from zero state (what is
// dropped is bounded by coef^W / (1 - coef) * max|x|: 1e-12 * max|x| at the presets' 0.97) -- no carry crosses a
// workgroup.  One workgroup = one chunk of one row: every thread scans 16 contiguous samples in registers (four 16-byte
// loads), the 256 segment carries are chained through LDS, outputs leave as 16-byte stores.  64 rows x 206 k samples:
// 4288 workgroups instead of the 64 of the serial form (938 us, round 2).
constexpr int DEEMPH_W = 1024, DEEMPH_CH = 3072, DEEMPH_E = (DEEMPH_W + DEEMPH_CH) / 256;
static_assert(DEEMPH_E == 16, "sixteen samples per thread");
__global__ __launch_bounds__(256) void deemphasis_chunk_kernel(const float* __restrict__ x, float* __restrict__ y, int L,
                                                               float coef, const int32_t* __restrict__ lens) {
  __shared__ float seg_end[256];
  __shared__ float carry[256];
  const int tid = threadIdx.x;
  const float* xr = x + (int64_t)blockIdx.y * L;
  float* yr = y + (int64_t)blockIdx.y * L;
  const int out0 = blockIdx.x * DEEMPH_CH;                    // first output of the chunk
  if (lens) {                                                 // per item: its own first lens[b] samples, zeros after them
    const int Lb = min(max(lens[blockIdx.y], 0), L);
    for (int i = max(out0, Lb) + tid; i < min(out0 + DEEMPH_CH, L); i += 256) yr[i] = 0.f;
    L = Lb;
  }
  const int i0 = out0 - DEEMPH_W + tid * DEEMPH_E;            // this thread's first sample (may lie before the row)
  float v[DEEMPH_E];
  const bool vec = i0 >= 0 && i0 + DEEMPH_E <= L && ((((uintptr_t)(xr + i0)) & 15) == 0);
  if (vec) {
#pragma unroll
    for (int q = 0; q < DEEMPH_E / 4; ++q) {
      const f32x4 t4 = *reinterpret_cast<const f32x4*>(xr + i0 + 4 * q);
      v[4 * q] = t4[0]; v[4 * q + 1] = t4[1]; v[4 * q + 2] = t4[2]; v[4 * q + 3] = t4[3];
    }
  } else {
#pragma unroll
    for (int j = 0; j < DEEMPH_E; ++j) v[j] = (i0 + j >= 0 && i0 + j < L) ? xr[i0 + j] : 0.f;
  }
  float acc = 0.f;
#pragma unroll
  for (int j = 0; j < DEEMPH_E; ++j) {
    acc = v[j] + coef * acc;
    v[j] = acc;
  }
  seg_end[tid] = acc;
  __syncthreads();
  if (tid == 0) {
    float cE = coef;
#pragma unroll
    for (int j = 1; j < DEEMPH_E; ++j) cE *= coef;            // coef^16
    float c = 0.f;                                            // filter state just before segment s
    for (int s = 0; s < 256; ++s) {
      carry[s] = c;
      c = seg_end[s] + cE * c;
    }
  }
  __syncthreads();
  if (i0 + DEEMPH_E <= out0 || i0 >= L) return;               // warm-up segments and segments past the row write nothing
  const float c = carry[tid];
  float g = coef;
#pragma unroll
  for (int j = 0; j < DEEMPH_E; ++j) {
    v[j] += g * c;
    g *= coef;
  }
  if (vec && i0 >= out0 && ((((uintptr_t)(yr + i0)) & 15) == 0)) {
#pragma unroll
    for (int q = 0; q < DEEMPH_E / 4; ++q)
      *reinterpret_cast<f32x4*>(yr + i0 + 4 * q) = f32x4{v[4 * q], v[4 * q + 1], v[4 * q + 2], v[4 * q + 3]};
  } else {
#pragma unroll
    for (int j = 0; j < DEEMPH_E; ++j)
      if (i0 + j >= out0 && i0 + j < L) yr[i0 + j] = v[j];
  }
}

extern "C" int dv3_deemphasis_f32(const float* x, float* y, int32_t B, int32_t L, float coef, void* stream) {
  DV3_REQUIRE(x && y && B > 0 && L > 0, "deemphasis: bad arguments");
  // the chunked form needs the warm-up to swallow the filter's memory; a coefficient too close to 1 (or >= 1) runs
  // the serial-per-row form, which is in place
  const float a = fabsf(coef);
  const bool chunked = a < 1.f && (a == 0.f || DEEMPH_W * logf(a) <= logf(1e-9f * (1.f - a))) && x != y;
  if (chunked) {
    hipLaunchKernelGGL(deemphasis_chunk_kernel, dim3(dv3_cdiv(L, DEEMPH_CH), B), dim3(256), 0, (hipStream_t)stream, x, y, L, coef,
                       (const int32_t*)nullptr);
    return dv3_check_launch("deemphasis");
  }
  if (x != y) {
    hipError_t e = hipMemcpyAsync(y, x, (size_t)B * L * sizeof(float), hipMemcpyDeviceToDevice, (hipStream_t)stream);
    if (e != hipSuccess) {
      dv3_set_error("deemphasis: %s", hipGetErrorString(e));
      return DV3_ELAUNCH;
    }
  }
  hipLaunchKernelGGL(deemphasis_kernel, dim3(B), dim3(256), 0, (hipStream_t)stream, y, L, coef, (const int32_t*)nullptr);
  return dv3_check_launch("deemphasis");
}

// ---- per-item frame counts (ABI 44, include/dv3hip.h: dv3_gl_istft_items_f32 ...): a batch of utterances of different
// lengths, each item's inverse exactly its B = 1 call on its own trimmed spectrogram ----
// the fewest frames a framing takes at this hop: lws needs a positive signal length, torch one longer than the reflect pad
template <int N>
static int items_tlo(int lws, int hop) {
  int t = 2;
  while (lws ? lws_len<N>(t, hop) <= 0 : hop * (t - 1) <= N / 2) ++t;
  return t;
}
template <int N>
static int gl_istft_items(const float* mag, const float* phasor, const float* swin, float* frames, int32_t B, int32_t T,
                          int32_t hop, const int32_t* tlen, int32_t lws, void* stream) {
  DV3_REQUIRE(mag && frames && tlen && (!lws || swin) && B > 0 && T > 1 && hop > 0 && hop <= N &&
              samples_fit(T, hop) && T >= items_tlo<N>(lws, hop), "gl_istft_items: bad arguments");
  if (lws)
    hipLaunchKernelGGL((istft_frames_kernel<N, true>), dim3((unsigned)((int64_t)B * T)), dim3(256), 0, (hipStream_t)stream, mag,
                       phasor, frames, swin, tlen, (int)T, items_tlo<N>(lws, hop));
  else
    hipLaunchKernelGGL((istft_frames_kernel<N, false>), dim3((unsigned)((int64_t)B * T)), dim3(256), 0, (hipStream_t)stream, mag,
                       phasor, frames, (const float*)nullptr, tlen, (int)T, items_tlo<N>(lws, hop));
  return dv3_check_launch("gl_istft_items");
}
template <int N>
static int overlap_add_items(const float* frames, float* y, int32_t B, int32_t T, int32_t hop, const int32_t* tlen,
                             int32_t lws, void* stream) {
  DV3_REQUIRE(frames && y && tlen && B > 0 && T > 1 && hop > 0 && hop <= N && samples_fit(T, hop) &&
              T >= items_tlo<N>(lws, hop), "overlap_add_items: bad arguments");
  const int L = lws ? lws_len<N>(T, hop) : hop * (T - 1);
  if (lws)
    hipLaunchKernelGGL((ola_kernel<N, true>), dim3(dv3_cdiv(L, 256), B), dim3(256), 0, (hipStream_t)stream, frames, y, T, hop, L,
                       tlen, items_tlo<N>(lws, hop));
  else
    hipLaunchKernelGGL((ola_kernel<N, false>), dim3(dv3_cdiv(L, 256), B), dim3(256), 0, (hipStream_t)stream, frames, y, T, hop, L,
                       tlen, items_tlo<N>(lws, hop));
  return dv3_check_launch("overlap_add_items");
}
template <int N>
static int gl_project_items(const float* y, const float* mag, const float* awin, const float* swin, float* frames, int32_t B,
                            int32_t T, int32_t hop, const int32_t* tlen, int32_t lws, void* stream) {
  DV3_REQUIRE(y && mag && frames && tlen && (!lws || (awin && swin)) && B > 0 && T > 1 && hop > 0 && hop <= N &&
              samples_fit(T, hop) && T >= items_tlo<N>(lws, hop), "gl_project_items: bad arguments");
  const int TP = (T + 1) / 2;
  const int L = lws ? lws_len<N>(T, hop) : hop * (T - 1);
  if (lws)
    hipLaunchKernelGGL((gl_project2_kernel<N, true, false>), dim3((unsigned)((int64_t)B * TP)), dim3(256), 0, (hipStream_t)stream, y, mag,
                       frames, T, hop, L, TP, awin, swin, tlen, items_tlo<N>(lws, hop), (float2*)nullptr, 0.f, 0);
  else
    hipLaunchKernelGGL((gl_project2_kernel<N, false, false>), dim3((unsigned)((int64_t)B * TP)), dim3(256), 0, (hipStream_t)stream, y, mag,
                       frames, T, hop, L, TP, (const float*)nullptr, (const float*)nullptr, tlen, items_tlo<N>(lws, hop), (float2*)nullptr, 0.f,
                       0);
  return dv3_check_launch("gl_project_items");
}
// fast Griffin-Lim: gl_project / lws_gl_project (tlen NULL) or gl_project_items with the momentum term of
// gl_project2_kernel<N, LWS, true>.  T >= items_tlo is the bound of all three (a positive signal length on the lws
// framing, a signal longer than the reflect padding on the torch one).
template <int N>
static int gl_project_momentum(const float* y, const float* mag, const float* awin, const float* swin, float* cprev,
                               float* frames, int32_t B, int32_t T, int32_t hop, const int32_t* tlen, int32_t lws, float alpha,
                               int32_t first, void* stream) {
  DV3_REQUIRE(y && mag && frames && (!lws || (awin && swin)) && B > 0 && T > 1 && hop > 0 && hop <= N && samples_fit(T, hop),
              "gl_project_momentum: bad arguments");
  DV3_REQUIRE(cprev && ((uintptr_t)cprev & 7) == 0, "gl_project_momentum: cprev must be a buffer of B * T * (n_fft/2 + 1) float pairs, 8-byte aligned");
  DV3_REQUIRE(alpha >= 0.f && alpha < 1.f, "gl_project_momentum: alpha = %g must lie in [0, 1)", (double)alpha);
  const int tlo = items_tlo<N>(lws, hop);
  DV3_REQUIRE(T >= tlo, "gl_project_momentum: %d frames at hop %d are fewer than the %d the framing takes", (int)T, (int)hop, tlo);
  const int TP = (T + 1) / 2;
  const int L = lws ? lws_len<N>(T, hop) : hop * (T - 1);
  if (lws)
    hipLaunchKernelGGL((gl_project2_kernel<N, true, true>), dim3((unsigned)((int64_t)B * TP)), dim3(256), 0, (hipStream_t)stream, y, mag,
                       frames, T, hop, L, TP, awin, swin, tlen, tlo, reinterpret_cast<float2*>(cprev), alpha, (int)(first != 0));
  else
    hipLaunchKernelGGL((gl_project2_kernel<N, false, true>), dim3((unsigned)((int64_t)B * TP)), dim3(256), 0, (hipStream_t)stream, y, mag,
                       frames, T, hop, L, TP, (const float*)nullptr, (const float*)nullptr, tlen, tlo,
                       reinterpret_cast<float2*>(cprev), alpha, (int)(first != 0));
  return dv3_check_launch("gl_project_momentum");
}
extern "C" int dv3_gl_project_momentum_f32(const float* y, const float* mag, const float* awin, const float* swin, float* cprev,
                                           float* frames, int32_t B, int32_t T, int32_t hop, const int32_t* tlen, int32_t lws,
                                           int32_t n_fft, float alpha, int32_t first, void* stream) {
  return with_fft_size("gl_project_momentum", n_fft, [&](auto n) {
    return gl_project_momentum<decltype(n)::value>(y, mag, awin, swin, cprev, frames, B, T, hop, tlen, lws, alpha, first, stream);
  });
}

extern "C" int dv3_gl_istft_items_f32(const float* mag, const float* phasor, const float* swin, float* frames, int32_t B,
                                      int32_t T, int32_t hop, const int32_t* tlen, int32_t lws, void* stream) {
  return gl_istft_items<1024>(mag, phasor, swin, frames, B, T, hop, tlen, lws, stream);
}
extern "C" int dv3_gl_istft_items_f32_n(const float* mag, const float* phasor, const float* swin, float* frames, int32_t B,
                                        int32_t T, int32_t hop, const int32_t* tlen, int32_t lws, int32_t n_fft, void* stream) {
  return with_fft_size("gl_istft_items", n_fft,
                       [&](auto n) { return gl_istft_items<decltype(n)::value>(mag, phasor, swin, frames, B, T, hop, tlen, lws, stream); });
}
extern "C" int dv3_overlap_add_items_f32(const float* frames, float* y, int32_t B, int32_t T, int32_t hop, const int32_t* tlen,
                                         int32_t lws, void* stream) {
  return overlap_add_items<1024>(frames, y, B, T, hop, tlen, lws, stream);
}
extern "C" int dv3_overlap_add_items_f32_n(const float* frames, float* y, int32_t B, int32_t T, int32_t hop,
                                           const int32_t* tlen, int32_t lws, int32_t n_fft, void* stream) {
  return with_fft_size("overlap_add_items", n_fft,
                       [&](auto n) { return overlap_add_items<decltype(n)::value>(frames, y, B, T, hop, tlen, lws, stream); });
}
extern "C" int dv3_gl_project_items_f32(const float* y, const float* mag, const float* awin, const float* swin, float* frames,
                                        int32_t B, int32_t T, int32_t hop, const int32_t* tlen, int32_t lws, void* stream) {
  return gl_project_items<1024>(y, mag, awin, swin, frames, B, T, hop, tlen, lws, stream);
}
extern "C" int dv3_gl_project_items_f32_n(const float* y, const float* mag, const float* awin, const float* swin,
                                          float* frames, int32_t B, int32_t T, int32_t hop, const int32_t* tlen, int32_t lws,
                                          int32_t n_fft, void* stream) {
  return with_fft_size("gl_project_items", n_fft, [&](auto n) {
    return gl_project_items<decltype(n)::value>(y, mag, awin, swin, frames, B, T, hop, tlen, lws, stream);
  });
}
extern "C" int dv3_deemphasis_items_f32(const float* x, float* y, int32_t B, int32_t L, const int32_t* lens, float coef,
                                        void* stream) {
  DV3_REQUIRE(x && y && lens && B > 0 && L > 0, "deemphasis_items: bad arguments");
  const float a = fabsf(coef);
  const bool chunked = a < 1.f && (a == 0.f || DEEMPH_W * logf(a) <= logf(1e-9f * (1.f - a))) && x != y;
  if (chunked) {
    hipLaunchKernelGGL(deemphasis_chunk_kernel, dim3(dv3_cdiv(L, DEEMPH_CH), B), dim3(256), 0, (hipStream_t)stream, x, y, L,
                       coef, lens);
    return dv3_check_launch("deemphasis_items");
  }
  if (x != y) {
    hipError_t e = hipMemcpyAsync(y, x, (size_t)B * L * sizeof(float), hipMemcpyDeviceToDevice, (hipStream_t)stream);
    if (e != hipSuccess) {
      dv3_set_error("deemphasis_items: %s", hipGetErrorString(e));
      return DV3_ELAUNCH;
    }
  }
  hipLaunchKernelGGL(deemphasis_kernel, dim3(B), dim3(256), 0, (hipStream_t)stream, y, L, coef, lens);
  return dv3_check_launch("deemphasis_items");
}

extern "C" int dv3_item_gain_f32(const float* x, const int64_t* soff, int32_t B, float rescaling_max, float* gain,
                                 void* stream) {
  DV3_REQUIRE(x && soff && gain && B > 0 && rescaling_max > 0.f, "item_gain: bad arguments");
  hipLaunchKernelGGL(item_gain_kernel, dim3(B), dim3(256), 0, (hipStream_t)stream, x, soff, rescaling_max, gain);
  return dv3_check_launch("item_gain");
}

template <int N>
static int analysis_items(const float* x, const int64_t* soff, const int32_t* foff, int32_t B, int32_t n_frames, int32_t hop,
                          float preemphasis, const float* awin, const float* gain, const float* mel_basis,
                          const int32_t* mel_band, int32_t n_mels, float min_level_db, float ref_level_db, float* lin,
                          float* mel, void* stream) {
  DV3_REQUIRE(x && soff && foff && awin && B > 0 && n_frames > 0 && hop > 0 && hop <= N && (lin || mel) &&
              (!mel || (mel_basis && n_mels > 0)) && min_level_db < 0.f, "analysis_items: bad arguments");
  if (gain)
    hipLaunchKernelGGL((analysis_items_kernel<N, true>), dim3(n_frames), dim3(256), 0, (hipStream_t)stream, x, soff, foff, B,
                       hop, preemphasis, awin, gain, mel_basis, mel_band, n_mels, min_level_db, ref_level_db, lin, mel);
  else
    hipLaunchKernelGGL((analysis_items_kernel<N, false>), dim3(n_frames), dim3(256), 0, (hipStream_t)stream, x, soff, foff, B,
                       hop, preemphasis, awin, gain, mel_basis, mel_band, n_mels, min_level_db, ref_level_db, lin, mel);
  return dv3_check_launch("analysis_items");
}
extern "C" int dv3_analysis_items_f32(const float* x, const int64_t* soff, const int32_t* foff, int32_t B,
                                      int32_t n_frames, int32_t hop, float preemphasis, const float* awin,
                                      const float* gain, const float* mel_basis, const int32_t* mel_band, int32_t n_mels,
                                      float min_level_db, float ref_level_db, float* lin, float* mel, void* stream) {
  return analysis_items<1024>(x, soff, foff, B, n_frames, hop, preemphasis, awin, gain, mel_basis, mel_band, n_mels,
                              min_level_db, ref_level_db, lin, mel, stream);
}
extern "C" int dv3_analysis_items_f32_n(const float* x, const int64_t* soff, const int32_t* foff, int32_t B,
                                        int32_t n_frames, int32_t hop, float preemphasis, const float* awin,
                                        const float* gain, const float* mel_basis, const int32_t* mel_band, int32_t n_mels,
                                        float min_level_db, float ref_level_db, float* lin, float* mel, int32_t n_fft,
                                        void* stream) {
  return with_fft_size("analysis_items", n_fft, [&](auto n) {
    return analysis_items<decltype(n)::value>(x, soff, foff, B, n_frames, hop, preemphasis, awin, gain, mel_basis, mel_band, n_mels,
                               min_level_db, ref_level_db, lin, mel, stream);
  });
}

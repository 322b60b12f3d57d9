// YIN pitch tracking per frame of B utterances packed back to back (include/dv3hip.h: dv3_yin_items_f32, where the
// definition, the summation orders and the bounds are stated).  de Cheveigne & Kawahara 2002, steps 2-5, in the direct
// difference form.  One workgroup of 256 threads per output row (frame t of item b, the lws framing of
// analysis_items_kernel: csrc/audio.hip).
//
// Shape: the frame is staged once in LDS (N + 16 floats, the tail zero).  d(tau) is N - tau_max terms for each of up to
// 1025 lags: a thread owns a QUAD of lags 4q .. 4q+3 (lag 0 is computed and unused) and one SLICE of the j range, so a
// wave's window reads s[j + 4q ..] are consecutive 16-byte words (conflict-free ds_read_b128) and s[j ..] is one
// broadcast word; the window slides, so four j cost two 16-byte reads for 16 difference-square terms.  The slices'
// partial sums meet in LDS and are added in slice order.  The prefix over the lags, d', and the search run in wave 0:
// lane l owns the CH consecutive lags from 1 + l * CH (CH odd, so the lanes' words fall on distinct banks).
#include "common.h"
#include <limits.h>
#include <math.h>

namespace {

constexpr int YIN_THREADS = 256;
constexpr int YIN_MAX_N = 2048;
constexpr int YIN_PAD = 16;                      // zeros behind the frame: a quad's window may run 7 words past N - 1

__global__ __launch_bounds__(YIN_THREADS) void yin_items_kernel(
    const float* __restrict__ x, const int64_t* __restrict__ soff, const int32_t* __restrict__ foff, int B, int hop, int N,
    int tau_min, int tau_max, float threshold, float sample_rate, float* __restrict__ f0, float* __restrict__ ap,
    float* __restrict__ power, int32_t* __restrict__ lag_out) {
  __shared__ __attribute__((aligned(16))) float S[YIN_MAX_N + YIN_PAD];
  __shared__ __attribute__((aligned(16))) float P[DV3_YIN_MAX_LAG + 8];   // [slice][4 * nq] partial sums of d
  __shared__ float Dd[DV3_YIN_MAX_LAG + 4];                               // d(tau), then unused
  __shared__ float Dp[DV3_YIN_MAX_LAG + 4];                               // d'(tau)
  __shared__ float red[4];
  __shared__ int pick[1];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int g = blockIdx.x;
  int lo = 0, hi = B;                                 // the item: largest b with foff[b] <= g
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if (foff[mid] <= g) lo = mid; else hi = mid;
  }
  const int b = lo, t = g - foff[b];
  const float* xb = x + soff[b];
  const int L = (int)(soff[b + 1] - soff[b]);

  // ---- stage the frame; power: per thread a chain over n = tid, tid + 256, ..., then the xor tree of a wave, then the
  // four waves in order ----
  float pw = 0.f;
  for (int n = tid; n < N; n += YIN_THREADS) {
    const int i = t * hop + n - (N - hop);
    const float v = (i >= 0 && i < L) ? xb[i] : 0.f;
    S[n] = v;
    pw = fmaf(v, v, pw);
  }
  if (tid < YIN_PAD) S[N + tid] = 0.f;
  pw = dv3_wave_sum(pw);
  if (lane == 0) red[wave] = pw;
  __syncthreads();

  // ---- d(tau): quads of lags x slices of j ----
  const int W = N - tau_max;                          // terms of every d(tau)
  const int nq = tau_max / 4 + 1;                     // quads: lags 0 .. 4 nq - 1 cover 0 .. tau_max
  const int qthreads = nq < YIN_THREADS ? nq : YIN_THREADS;
  const int nsl = YIN_THREADS / qthreads;             // slices of the j range (1 when nq > 128)
  const int Wc = ((W + nsl - 1) / nsl + 3) & ~3;      // j per slice, a multiple of 4
  const int sl = tid / qthreads;
  if (sl < nsl) {
    const int j0 = sl * Wc, j1 = min(W, j0 + Wc);
    for (int q = tid - sl * qthreads; q < nq; q += qthreads) {
      const float* w = S + 4 * q;
      float a0 = 0.f, a1 = 0.f, a2 = 0.f, a3 = 0.f;
      int j = j0;
      if (j + 4 <= j1) {
        f32x4 wl = *reinterpret_cast<const f32x4*>(w + j);
        for (; j + 4 <= j1; j += 4) {
          const f32x4 wh = *reinterpret_cast<const f32x4*>(w + j + 4);
          const f32x4 sj = *reinterpret_cast<const f32x4*>(S + j);
          const float v[8] = {wl[0], wl[1], wl[2], wl[3], wh[0], wh[1], wh[2], wh[3]};
#pragma unroll
          for (int jj = 0; jj < 4; ++jj) {
            const float e0 = sj[jj] - v[jj], e1 = sj[jj] - v[jj + 1], e2 = sj[jj] - v[jj + 2], e3 = sj[jj] - v[jj + 3];
            a0 = fmaf(e0, e0, a0);
            a1 = fmaf(e1, e1, a1);
            a2 = fmaf(e2, e2, a2);
            a3 = fmaf(e3, e3, a3);
          }
          wl = wh;
        }
      }
      for (; j < j1; ++j) {                           // at most 3 terms
        const float s = S[j];
        const float e0 = s - w[j], e1 = s - w[j + 1], e2 = s - w[j + 2], e3 = s - w[j + 3];
        a0 = fmaf(e0, e0, a0);
        a1 = fmaf(e1, e1, a1);
        a2 = fmaf(e2, e2, a2);
        a3 = fmaf(e3, e3, a3);
      }
      *reinterpret_cast<f32x4*>(P + sl * 4 * nq + 4 * q) = f32x4{a0, a1, a2, a3};
    }
  }
  __syncthreads();
  for (int tau = tid; tau <= tau_max; tau += YIN_THREADS) {
    float d = P[tau];
    for (int k = 1; k < nsl; ++k) d += P[k * 4 * nq + tau];
    Dd[tau] = d;
  }
  __syncthreads();

  // ---- wave 0: c(tau) (lane-local chains joined by a scan over the lanes), d', and each lane's part of the search ----
  if (wave == 0) {
    const int CH = ((tau_max + 63) / 64) | 1;
    const int t0 = 1 + lane * CH, t1 = min(t0 + CH, tau_max + 1);
    float tot = 0.f;
    for (int tau = t0; tau < t1; ++tau) tot += Dd[tau];
    float inc = tot;                                  // inclusive scan of the lanes' totals
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
      const float up = __shfl_up(inc, off, 64);
      if (lane >= off) inc += up;
    }
    float c = __shfl_up(inc, 1, 64);
    if (lane == 0) c = 0.f;
    int first = INT_MAX, argmin = INT_MAX;
    float vmin = INFINITY;
    for (int tau = t0; tau < t1; ++tau) {
      const float d = Dd[tau];
      c += d;
      const float dp = c > 0.f ? (d * (float)tau) / c : 1.f;
      Dp[tau] = dp;
      if (tau >= tau_min && tau < tau_max) {
        if (first == INT_MAX && dp < threshold) first = tau;
        if (dp < vmin) {
          vmin = dp;
          argmin = tau;
        }
      }
    }
    if (lane == 0) Dp[0] = 1.f;
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
      first = min(first, __shfl_xor(first, off, 64));
      const float ov = __shfl_xor(vmin, off, 64);
      const int oa = __shfl_xor(argmin, off, 64);
      if (ov < vmin || (ov == vmin && oa < argmin)) {
        vmin = ov;
        argmin = oa;
      }
    }
    if (argmin == INT_MAX) argmin = tau_min;          // every d' a NaN (non-finite samples): still a lag in the range
    if (lane == 0) pick[0] = first != INT_MAX ? first : -argmin;   // negative: no lag under the threshold
  }
  __syncthreads();

  if (tid == 0) {
    int lag = pick[0];
    if (lag > 0) {
      while (lag + 1 < tau_max && Dp[lag + 1] < Dp[lag]) ++lag;
    } else {
      lag = -lag;
    }
    const float pa = Dp[lag - 1], pb = Dp[lag], pc = Dp[lag + 1];
    const float D = (pa - 2.f * pb) + pc;
    float delta = 0.f;
    if (D > 0.f) delta = fminf(fmaxf(0.5f * (pa - pc) / D, -1.f), 1.f);
    f0[g] = sample_rate / ((float)lag + delta);
    ap[g] = pb;
    power[g] = (((red[0] + red[1]) + red[2]) + red[3]) * (1.f / (float)N);
    if (lag_out) lag_out[g] = lag;
  }
}

}  // namespace

extern "C" int dv3_yin_items_f32(const float* x, const int64_t* soff, const int32_t* foff, int32_t B, int32_t n_frames,
                                 int32_t hop, int32_t n_fft, int32_t tau_min, int32_t tau_max, float threshold,
                                 float sample_rate, float* f0, float* ap, float* power, int32_t* lag, void* stream) {
  DV3_REQUIRE(x, "yin_items: x is null");
  DV3_REQUIRE(soff, "yin_items: soff is null");
  DV3_REQUIRE(foff, "yin_items: foff is null");
  DV3_REQUIRE(f0, "yin_items: f0 is null");
  DV3_REQUIRE(ap, "yin_items: ap is null");
  DV3_REQUIRE(power, "yin_items: power is null");
  DV3_REQUIRE(B >= 1, "yin_items: B = %d < 1", (int)B);
  DV3_REQUIRE(n_frames >= 1, "yin_items: n_frames = %d < 1", (int)n_frames);
  DV3_REQUIRE(n_fft == 512 || n_fft == 1024 || n_fft == 2048, "yin_items: n_fft = %d is none of 512, 1024, 2048", (int)n_fft);
  DV3_REQUIRE(hop >= 1 && hop <= n_fft, "yin_items: hop = %d outside [1, n_fft = %d]", (int)hop, (int)n_fft);
  DV3_REQUIRE(tau_min >= 2, "yin_items: tau_min = %d < 2", (int)tau_min);
  DV3_REQUIRE(tau_max <= n_fft / 2 && tau_max <= DV3_YIN_MAX_LAG, "yin_items: tau_max = %d above n_fft / 2 = %d",
              (int)tau_max, (int)n_fft / 2);
  DV3_REQUIRE(tau_min + 1 < tau_max, "yin_items: tau_min + 1 = %d is not below tau_max = %d", (int)tau_min + 1, (int)tau_max);
  DV3_REQUIRE(threshold > 0.f && threshold <= 1.f, "yin_items: threshold = %g outside (0, 1]", (double)threshold);
  DV3_REQUIRE(isfinite(sample_rate) && sample_rate > 0.f, "yin_items: sample_rate = %g is not finite and positive",
              (double)sample_rate);
  hipLaunchKernelGGL(yin_items_kernel, dim3(n_frames), dim3(YIN_THREADS), 0, (hipStream_t)stream, x, soff, foff, (int)B,
                     (int)hop, (int)n_fft, (int)tau_min, (int)tau_max, threshold, sample_rate, f0, ap, power, lag);
  return dv3_check_launch("yin_items");
}

// Mel-to-linear inversion: a non-negative least-squares estimate of the linear magnitudes under a mel frame, by
// multiplicative updates with the filterbank fixed (include/dv3hip.h: dv3_mel_to_linear_f32).
//
//   staging   once per workgroup (kWaves waves): the band of every filter and the filter range of every bin are clamped
//             to the arrays and prefix-summed (one wave each, a shuffle scan), and when both compact images fit
//             (kCap floats each; 1024 bins x 2 filters is 2050) the nonzero part of W is copied to LDS twice: filter-major
//             (filter m's band contiguous, for r = W s) and bin-major (bin k's filters contiguous, for d = W^T r; an
//             entry whose bin lies outside its filter's band is stored as 0).  A denser basis is read from global
//             memory through the same two accessors: same values, same order, same bits.
//   frames    one 64-lane wave per output frame, the workgroup's waves striding over the frames.  Bin k lives in lane
//             k % 64, register k / 64 (the register count NJ is a template parameter); filter m is computed by lane
//             m % 64.  s and r (and the amplitudes a, in r's place, at the start) are in the wave's LDS.  The wave's own
//             LDS traffic is ordered by wave_sync() -- a wavefront-scope fence, no instruction --: there is NO
//             workgroup barrier after the staging.
//   roundings every sum over bins is one fmaf chain in ascending bin order from 0, every sum over filters one fmaf chain
//             in ascending filter order from 0; the frame's amplitude sum is each lane's ascending sum, then a xor
//             butterfly; the update is s * (b / max(d, FLOOR)) with the IEEE division; 10^e is exp2f of a two-term
//             product e * log2(10); the output is audio.hip's db_norm.
#include "common.h"

namespace {

constexpr int kWaves = 4;                       // frames in flight per workgroup
constexpr int kCap = 3072;                      // floats of each compact image of W in LDS
constexpr int kMaxBins = 1025;
constexpr float kFloor = 1e-30f;

__device__ __forceinline__ void wave_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

__device__ __forceinline__ int clamp_i(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

// the two expressions of csrc/audio.hip (amp_to_db_norm), restated: this file's output is that kernel's format
__device__ __forceinline__ float db_min_level(float min_db) { return exp2f(min_db * 0.05f * 3.32192809488736234787f); }
__device__ __forceinline__ float db_norm(float x, float min_level, float min_db, float ref_db) {
  const float db = fmaf(20.0f, log10f(fmaxf(min_level, x)), -ref_db);
  return fminf(fmaxf((db - min_db) / (-min_db), 0.f), 1.f);
}

// 10^e: e * log2(10) as a two-term product (hi + lo exact to ~2^-48 relative), exp2f of each part
__device__ __forceinline__ float exp10_f(float e) {
  const float l2hi = 3.3219280242919921875f, l2lo = 7.059536955e-08f;      // log2(10) = l2hi + l2lo
  const float hi = e * l2hi;
  const float lo = fmaf(e, l2lo, fmaf(e, l2hi, -hi));
  return exp2f(hi) * exp2f(lo);
}

// exclusive prefix sum of in[0 .. n) into out[0 .. n) by one wave -> the total
__device__ __forceinline__ int wave_scan(const int* in, int* out, int n, int lane) {
  int carry = 0;
  for (int i0 = 0; i0 < n; i0 += 64) {
    const int i = i0 + lane;
    const int v = i < n ? in[i] : 0;
    int inc = v;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
      const int o = __shfl_up(inc, off, 64);
      if (lane >= off) inc += o;
    }
    if (i < n) out[i] = carry + inc - v;
    carry += __shfl(inc, 63, 64);
  }
  return carry;
}

struct Tables {                                 // the workgroup's LDS image of the two band tables
  int fk0[DV3_MELINV_MAX_MELS], fw[DV3_MELINV_MAX_MELS], foff[DV3_MELINV_MAX_MELS];      // filter m: first bin, width, offset
  int bm0[kMaxBins], bcnt[kMaxBins], boff[kMaxBins];                                    // bin k: first filter, count, offset
};

// The frames of one wave.  STAGED: W comes from the two compact LDS images, else from `basis` in global memory.
template <int NJ, bool STAGED>
__device__ __forceinline__ void melinv_frames(const float* __restrict__ mel, const int32_t* __restrict__ tlen,
                                              const float* __restrict__ basis, float inv_basis_sum,
                                              float* __restrict__ lin, int T, int M, int F, int u, int iters, float min_db,
                                              float ref_db, int64_t n_frames, const Tables& tb, const float* wf,
                                              const float* wb, float* sv, float* rv, int lane, int64_t first,
                                              int64_t stride) {
  // W[m][fk0[m] + i], i < fw[m]
  auto w_filter = [&](int m, int off, int k0, int i) -> float {
    return STAGED ? wf[off + i] : basis[(int64_t)m * F + k0 + i];
  };
  // W[bm0[k] + j][k], j < bcnt[k]; 0 where bin k lies outside that filter's band
  auto w_bin = [&](int k, int off, int m0, int j) -> float {
    if (STAGED) return wb[off + j];
    const int m = m0 + j;
    return (unsigned)(k - tb.fk0[m]) < (unsigned)tb.fw[m] ? basis[(int64_t)m * F + k] : 0.f;
  };
  // v_k = sum over the filters of bin k, ascending, of W[m][k] * vec[m] (the bin's range is read from the tables each
  // time: three LDS words per bin, instead of 3 NJ registers)
  auto apply_t = [&](const float* vec, float (&out)[NJ]) {
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
      const int k = lane + 64 * j;
      const bool in = k < F;
      const int m0 = in ? tb.bm0[k] : 0, cnt = in ? tb.bcnt[k] : 0, off = in ? tb.boff[k] : 0;
      float acc = 0.f;
      for (int q = 0; q < cnt; ++q) acc = fmaf(w_bin(k, off, m0, q), vec[m0 + q], acc);
      out[j] = acc;
    }
  };
  uint32_t covered = 0;                         // bit j: the column of bin lane + 64 j has a positive sum
#pragma unroll
  for (int j = 0; j < NJ; ++j) {
    const int k = lane + 64 * j;
    const int cnt = k < F ? tb.bcnt[k] : 0;
    float col = 0.f;
    for (int q = 0; q < cnt; ++q) col += w_bin(k, tb.boff[k], tb.bm0[k], q);
    covered |= (uint32_t)(col > 0.f) << j;
  }
  const float min_level = db_min_level(min_db);
  const float fu = (float)u;
  const int Tu = T * u;
  for (int64_t g = first; g < n_frames; g += stride) {      // wave-uniform
    const int b = (int)(g / Tu), t = (int)(g % Tu);
    const int Tb = tlen ? clamp_i(tlen[b], 0, T) : T;
    float* __restrict__ row = lin + g * F;
    if (t >= Tb * u) {
      for (int k = lane; k < F; k += 64) row[k] = 0.f;
      continue;
    }
    const int i0 = t / u, i1 = min(i0 + 1, Tb - 1);
    const float f = (float)(t % u) / fu, f0 = 1.0f - f;
    const float* __restrict__ x0 = mel + ((int64_t)b * T + i0) * M;
    const float* __restrict__ x1 = mel + ((int64_t)b * T + i1) * M;
    wave_sync();                                // the frame before is done with rv
    float asum = 0.f;
    for (int m = lane; m < M; m += 64) {
      const float c0 = fminf(fmaxf(x0[m], 0.f), 1.f), c1 = fminf(fmaxf(x1[m], 0.f), 1.f);
      const float x = fmaf(f, c1, f0 * c0);
      const float a = exp10_f(fmaf(x, -min_db, min_db + ref_db) / 20.0f);
      rv[m] = a;
      asum += a;
    }
    asum = dv3_wave_sum(asum);
    wave_sync();
    float bk[NJ], s[NJ];
    apply_t(rv, bk);
    const float s0 = asum * inv_basis_sum;
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
      s[j] = (covered >> j & 1u) ? s0 : 0.f;
      if (lane + 64 * j < F) sv[lane + 64 * j] = s[j];
    }
    for (int it = 0; it < iters; ++it) {
      wave_sync();                              // sv is written, rv is read
      for (int m = lane; m < M; m += 64) {
        const int k0 = tb.fk0[m], w = tb.fw[m], o = tb.foff[m];
        float acc = 0.f;
        for (int i = 0; i < w; ++i) acc = fmaf(w_filter(m, o, k0, i), sv[k0 + i], acc);
        rv[m] = acc;
      }
      wave_sync();                              // rv is written, sv is read
      float d[NJ];
      apply_t(rv, d);
#pragma unroll
      for (int j = 0; j < NJ; ++j) {
        s[j] = s[j] * (bk[j] / fmaxf(d[j], kFloor));
        if (lane + 64 * j < F) sv[lane + 64 * j] = s[j];
      }
    }
#pragma unroll
    for (int j = 0; j < NJ; ++j)
      if (lane + 64 * j < F) row[lane + 64 * j] = db_norm(s[j], min_level, min_db, ref_db);
  }
}

template <int NJ>
__global__ __launch_bounds__(64 * kWaves) void mel_to_linear_kernel(const float* __restrict__ mel,
                                                                    const int32_t* __restrict__ tlen,
                                                                    const float* __restrict__ basis,
                                                                    const int32_t* __restrict__ mel_band,
                                                                    const int32_t* __restrict__ bin_band,
                                                                    float inv_basis_sum, float* __restrict__ lin, int T,
                                                                    int M, int F, int u, int iters, float min_db,
                                                                    float ref_db, int64_t n_frames) {
  __shared__ Tables tb;
  __shared__ float wf[kCap], wb[kCap];
  __shared__ float sv[kWaves][NJ * 64], rv[kWaves][DV3_MELINV_MAX_MELS];
  __shared__ int totals[2];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  for (int m = tid; m < M; m += 64 * kWaves) {
    const int k0 = clamp_i(mel_band[2 * m], 0, F), k1 = clamp_i(mel_band[2 * m + 1], k0, F);
    tb.fk0[m] = k0;
    tb.fw[m] = k1 - k0;
  }
  for (int k = tid; k < F; k += 64 * kWaves) {
    const int a = clamp_i(bin_band[2 * k], 0, M), e = clamp_i(bin_band[2 * k + 1], a, M);
    tb.bm0[k] = a;
    tb.bcnt[k] = e - a;
  }
  __syncthreads();
  if (wave == 0) {
    const int n = wave_scan(tb.fw, tb.foff, M, lane);
    if (lane == 0) totals[0] = n;
  } else if (wave == 1) {
    const int n = wave_scan(tb.bcnt, tb.boff, F, lane);
    if (lane == 0) totals[1] = n;
  }
  __syncthreads();
  const bool staged = totals[0] <= kCap && totals[1] <= kCap;      // workgroup-uniform
  if (staged) {
    for (int m = wave; m < M; m += kWaves) {
      const int k0 = tb.fk0[m], w = tb.fw[m], o = tb.foff[m];
      for (int i = lane; i < w; i += 64) wf[o + i] = basis[(int64_t)m * F + k0 + i];
    }
    for (int k = tid; k < F; k += 64 * kWaves) {
      const int a = tb.bm0[k], c = tb.bcnt[k], o = tb.boff[k];
      for (int q = 0; q < c; ++q) {
        const int m = a + q;
        wb[o + q] = (unsigned)(k - tb.fk0[m]) < (unsigned)tb.fw[m] ? basis[(int64_t)m * F + k] : 0.f;
      }
    }
  }
  __syncthreads();
  const int64_t first = (int64_t)blockIdx.x * kWaves + wave, stride = (int64_t)gridDim.x * kWaves;
  if (staged)
    melinv_frames<NJ, true>(mel, tlen, basis, inv_basis_sum, lin, T, M, F, u, iters, min_db, ref_db, n_frames, tb, wf,
                            wb, sv[wave], rv[wave], lane, first, stride);
  else
    melinv_frames<NJ, false>(mel, tlen, basis, inv_basis_sum, lin, T, M, F, u, iters, min_db, ref_db, n_frames, tb, wf,
                             wb, sv[wave], rv[wave], lane, first, stride);
}

}  // namespace

extern "C" int dv3_mel_to_linear_f32(const float* mel, const int32_t* tlen, const float* basis, const int32_t* mel_band,
                                     const int32_t* bin_band, float inv_basis_sum, float* lin, int32_t B, int32_t T,
                                     int32_t n_mels, int32_t n_bins, int32_t upsample, int32_t iters, float min_level_db,
                                     float ref_level_db, void* stream) {
  DV3_REQUIRE(mel, "mel_to_linear: mel is null");
  DV3_REQUIRE(basis, "mel_to_linear: basis is null");
  DV3_REQUIRE(mel_band, "mel_to_linear: mel_band is null");
  DV3_REQUIRE(bin_band, "mel_to_linear: bin_band is null");
  DV3_REQUIRE(lin, "mel_to_linear: lin is null");
  DV3_REQUIRE(B >= 1, "mel_to_linear: B = %d < 1", (int)B);
  DV3_REQUIRE(T >= 1, "mel_to_linear: T = %d < 1", (int)T);
  DV3_REQUIRE(n_mels >= 1 && n_mels <= DV3_MELINV_MAX_MELS, "mel_to_linear: n_mels = %d outside [1, %d]", (int)n_mels,
              DV3_MELINV_MAX_MELS);
  DV3_REQUIRE(n_bins >= 1 && n_bins <= kMaxBins, "mel_to_linear: n_bins = %d outside [1, %d]", (int)n_bins, kMaxBins);
  DV3_REQUIRE(upsample >= 1 && upsample <= 16, "mel_to_linear: upsample = %d outside [1, 16]", (int)upsample);
  DV3_REQUIRE(iters >= 0 && iters <= DV3_MELINV_MAX_ITERS, "mel_to_linear: iters = %d outside [0, %d]", (int)iters,
              DV3_MELINV_MAX_ITERS);
  DV3_REQUIRE(min_level_db < 0.f, "mel_to_linear: min_level_db = %g is not negative", (double)min_level_db);
  DV3_REQUIRE(inv_basis_sum > 0.f && inv_basis_sum <= 3.4e38f, "mel_to_linear: inv_basis_sum = %g is not positive and finite",
              (double)inv_basis_sum);
  const int64_t n_frames = (int64_t)B * T * upsample;
  DV3_REQUIRE(n_frames < ((int64_t)1 << 31), "mel_to_linear: B * T * upsample = %lld frames, 2^31 or more",
              (long long)n_frames);
  const int grid = (int)(dv3_cdiv64(n_frames, kWaves) < 1024 ? dv3_cdiv64(n_frames, kWaves) : 1024);
  hipStream_t st = (hipStream_t)stream;
#define DV3_MELINV(NJ)                                                                                              \
  hipLaunchKernelGGL(mel_to_linear_kernel<NJ>, dim3(grid), dim3(64 * kWaves), 0, st, mel, tlen, basis, mel_band,   \
                     bin_band, inv_basis_sum, lin, (int)T, (int)n_mels, (int)n_bins, (int)upsample, (int)iters,    \
                     min_level_db, ref_level_db, n_frames)
  if (n_bins <= 5 * 64) DV3_MELINV(5);
  else if (n_bins <= 9 * 64) DV3_MELINV(9);
  else DV3_MELINV(17);
#undef DV3_MELINV
  return dv3_check_launch("mel_to_linear_f32");
}

// Deliverable audio: per-item levels, levels -> gains, and ONE launch that places, scales, fades and quantises the
// utterances of a document (include/dv3hip.h: dv3_wave_levels_f32, dv3_wave_gains_f32, dv3_wave_master_f32, where every
// step is stated).  The reference's counterpart is audio.save_wav (audio.py:16-18), one file per line of
// text on the host; it joins nothing.
//
//   levels   grid (chunks, B): a workgroup of 256 owns DV3_LEVELS_CHUNK samples of one item, counted from the item's own
//            first sample, and reads them as dwords (256 contiguous bytes per wave, whatever the span's alignment); fp64
//            accumulators per lane, a fixed LDS tree, one partial row per chunk; a second launch adds an item's chunks in
//            ascending order.  No atomics, and nothing depends on B or on where the span lies.
//   gains    one thread per group: a handful of fp64 operations.
//   master   a streaming kernel: a lane owns V consecutive output samples (4 floats or 8 int16: one 16-byte store), a wave
//            64 V of them, and walks kMasterChunks such chunks in a row.  The segments that cover a chunk are a contiguous
//            index range [lo, hi) because starts AND ends ascend: one binary search per wave, then both cursors only move
//            forward, all of it on wave-uniform values (scalar loads).  A segment's source offset is arbitrary relative
//            to its destination, so the source is read with 4-byte-aligned vector loads (legal on gfx950 for global
//            memory); lanes at a segment's edges fall back to clamped dword loads.  Lanes outside every fade skip the
//            weight (fmul(g, 1) == g).
#include "common.h"

namespace {

constexpr int kThreads = 256;
constexpr int kMasterChunks = 4;

// ---- levels ---------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kThreads) void wave_levels_chunk_kernel(const float* __restrict__ x,
                                                                     const int64_t* __restrict__ starts,
                                                                     const int64_t* __restrict__ lengths, int64_t max_len,
                                                                     int nchunk, double* __restrict__ part) {
  __shared__ double s_sq[kThreads], s_sum[kThreads];
  __shared__ float s_peak[kThreads];
  __shared__ uint32_t s_over[kThreads], s_bad[kThreads];
  const int b = blockIdx.y, c = blockIdx.x, tid = threadIdx.x;
  const int64_t n = min(max(lengths[b], (int64_t)0), max_len);
  const int64_t i0 = (int64_t)c * DV3_LEVELS_CHUNK;
  if (i0 >= n) return;                               // block-uniform: the second launch reads ceil(n / chunk) rows only
  const int64_t i1 = min(n, i0 + DV3_LEVELS_CHUNK);
  const float* __restrict__ xs = x + starts[b];
  float peak = 0.0f;
  double sq = 0.0, sum = 0.0;
  uint32_t over = 0, bad = 0;
  for (int64_t i = i0 + tid; i < i1; i += kThreads) {
    const float v = xs[i];
    const float a = fabsf(v);
    if (a < INFINITY) {                              // finite (a NaN fails the comparison)
      const double d = (double)v;
      peak = fmaxf(peak, a);
      sq += d * d;                                   // the square of an fp32 is exact in fp64
      sum += d;
    } else {
      ++bad;
    }
    over += a >= 1.0f;
  }
  s_sq[tid] = sq; s_sum[tid] = sum; s_peak[tid] = peak; s_over[tid] = over; s_bad[tid] = bad;
  for (int st = kThreads / 2; st > 0; st >>= 1) {
    __syncthreads();
    if (tid < st) {
      s_sq[tid] = s_sq[tid] + s_sq[tid + st];
      s_sum[tid] = s_sum[tid] + s_sum[tid + st];
      s_peak[tid] = fmaxf(s_peak[tid], s_peak[tid + st]);
      s_over[tid] += s_over[tid + st];
      s_bad[tid] += s_bad[tid + st];
    }
  }
  if (tid == 0) {
    double* row = part + ((int64_t)b * nchunk + c) * DV3_LEVEL_COLUMNS;
    row[0] = (double)s_peak[0]; row[1] = s_sq[0]; row[2] = s_sum[0]; row[3] = (double)s_over[0]; row[4] = (double)s_bad[0];
  }
}

__global__ __launch_bounds__(64) void wave_levels_final_kernel(const int64_t* __restrict__ lengths, int64_t max_len, int B,
                                                               int nchunk, const double* __restrict__ part,
                                                               double* __restrict__ levels) {
  const int b = blockIdx.x * 64 + threadIdx.x;
  if (b >= B) return;
  const int64_t n = min(max(lengths[b], (int64_t)0), max_len);
  const int nc = (int)((n + DV3_LEVELS_CHUNK - 1) / DV3_LEVELS_CHUNK);
  double peak = 0.0, sq = 0.0, sum = 0.0, over = 0.0, bad = 0.0;
  for (int c = 0; c < nc; ++c) {
    const double* row = part + ((int64_t)b * nchunk + c) * DV3_LEVEL_COLUMNS;
    peak = fmax(peak, row[0]); sq += row[1]; sum += row[2]; over += row[3]; bad += row[4];
  }
  double* out = levels + (int64_t)b * DV3_LEVEL_COLUMNS;
  out[0] = peak; out[1] = sq; out[2] = sum; out[3] = over; out[4] = bad;
}

// ---- gains ----------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(64) void wave_gains_kernel(const double* __restrict__ levels, const int64_t* __restrict__ lengths,
                                                        const int32_t* __restrict__ goff, int B, int G, int policy,
                                                        double target, double ceiling, double max_gain,
                                                        float* __restrict__ gain) {
#pragma clang fp contract(off)
  const int g = blockIdx.x * 64 + threadIdx.x;
  if (g >= G) return;
  const int b0 = min(max(goff[g], 0), B), b1 = min(max(goff[g + 1], b0), B);
  double P = 0.0, Q = 0.0;
  int64_t n = 0;
  for (int b = b0; b < b1; ++b) {
    P = fmax(P, levels[(int64_t)b * DV3_LEVEL_COLUMNS]);
    Q += levels[(int64_t)b * DV3_LEVEL_COLUMNS + 1];
    n += max(lengths[b], (int64_t)0);
  }
  float v;
  if (policy == DV3_GAIN_REFERENCE) {
    v = fmaxf((float)P, 0.01f);
  } else {
    double q = 1.0;
    if (P > 0.0 && n > 0 && (policy == DV3_GAIN_PEAK || Q > 0.0)) {
      q = policy == DV3_GAIN_PEAK ? target / P : fmin(target / sqrt(Q / (double)n), ceiling / P);
      q = fmin(q, max_gain);
    }
    v = (float)q;
  }
  for (int b = b0; b < b1; ++b) gain[b] = v;
}

// ---- master ---------------------------------------------------------------------------------------------------------
typedef int16_t i16x8 __attribute__((ext_vector_type(8)));

// One rounding per operation, never an fma: the operators below are compiled with contraction off, so the instructions
// they inline to carry no licence to fuse.  (The __fmul_rn / __fadd_rn of the HIP headers are plain operators compiled
// under the headers' own contraction mode: a product of theirs feeding a sum of theirs may still become one fma.)
__device__ __forceinline__ float mul_rn(float a, float b) {
#pragma clang fp contract(off)
  return a * b;
}
__device__ __forceinline__ float add_rn(float a, float b) {
#pragma clang fp contract(off)
  return a + b;
}
__device__ __forceinline__ float div_rn(float a, float b) {   // IEEE division (hipcc's default for fp32)
#pragma clang fp contract(off)
  return a / b;
}

__device__ __forceinline__ float master_dither(int64_t n, uint32_t k0, uint32_t k1) {
  uint32_t r[4];
  dv3_philox4x32_10((uint32_t)(uint64_t)n, (uint32_t)((uint64_t)n >> 32), 0u, 0u, k0, k1, r);
  return add_rn(mul_rn((float)(r[0] >> 8), 0x1p-24f), -mul_rn((float)(r[1] >> 8), 0x1p-24f));   // all exact
}

__device__ __forceinline__ int16_t master_clamp_i16(float r) {   // r integral or non-finite: saturate, NaN -> 0
  if (r != r) return 0;
  return (int16_t)(int)fminf(fmaxf(r, -32768.0f), 32767.0f);
}

template <int MODE, bool DITHER>
__global__ __launch_bounds__(kThreads) void wave_master_kernel(const float* __restrict__ x, const int64_t* __restrict__ src,
                                                               const int64_t* __restrict__ len,
                                                               const int64_t* __restrict__ dst,
                                                               const float* __restrict__ gain,
                                                               const int32_t* __restrict__ flags, int S,
                                                               const float* __restrict__ fade, int F, uint32_t k0,
                                                               uint32_t k1, void* __restrict__ out, int64_t N) {
#pragma clang fp contract(off)
  constexpr int V = MODE == DV3_MASTER_F32 ? 4 : 8;
  constexpr int64_t CH = 64 * V;
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int64_t w0 = ((int64_t)blockIdx.x * (kThreads / 64) + wave) * (kMasterChunks * CH);
  if (w0 >= N) return;
  int lo = 0;                                         // the first segment that ends past w0 (ends ascend)
  for (int hi_ = S; lo < hi_;) {
    const int m = (lo + hi_) >> 1;
    if (dst[m] + len[m] > w0) hi_ = m; else lo = m + 1;
  }
  int hi = lo;
  for (int j = 0; j < kMasterChunks; ++j) {
    const int64_t c0 = w0 + j * CH;
    if (c0 >= N) break;
    const int64_t c1 = min(c0 + CH, N);
    while (lo < S && dst[lo] + len[lo] <= c0) ++lo;
    hi = max(hi, lo);
    while (hi < S && dst[hi] < c1) ++hi;
    const int64_t n0 = c0 + (int64_t)lane * V;
    float y[V];
    bool any[V];
#pragma unroll
    for (int v = 0; v < V; ++v) { y[v] = 0.0f; any[v] = false; }
    for (int s = lo; s < hi; ++s) {                   // wave-uniform bounds and segment fields
      const int64_t d = dst[s], L = len[s];
      const float g = gain[s];
      const int fl = MODE == DV3_MASTER_I16_REFERENCE ? 0 : flags[s];
      const int64_t i0 = n0 - d;
      if (L <= 0 || i0 + V <= 0 || i0 >= L) continue;
      const float* __restrict__ xs = x + src[s];
      const bool inside = i0 >= 0 && i0 + V <= L;
      float xv[V];
      if (inside) {
#pragma unroll
        for (int q = 0; q < V / 4; ++q) {
          f32x4 t;                                    // 16 bytes from a 4-byte-aligned address
          __builtin_memcpy(&t, xs + i0 + 4 * q, sizeof(t));
          xv[4 * q] = t[0]; xv[4 * q + 1] = t[1]; xv[4 * q + 2] = t[2]; xv[4 * q + 3] = t[3];
        }
      } else {
#pragma unroll
        for (int v = 0; v < V; ++v) xv[v] = xs[min(max(i0 + v, (int64_t)0), L - 1)];
      }
      const bool plain = inside && !((fl & DV3_MASTER_FADE_IN) && i0 < F) &&
                         !((fl & DV3_MASTER_FADE_OUT) && i0 + V > L - F);
#pragma unroll
      for (int v = 0; v < V; ++v) {
        const int64_t i = i0 + v;
        if (i < 0 || i >= L) continue;
        float t;
        if (MODE == DV3_MASTER_I16_REFERENCE) {
          t = div_rn(mul_rn(xv[v], 32767.0f), g);
        } else {
          float w = 1.0f;
          if (!plain) {
            if ((fl & DV3_MASTER_FADE_IN) && i < F) w = fade[i];
            if ((fl & DV3_MASTER_FADE_OUT) && i >= L - F) w = mul_rn(w, fade[L - 1 - i]);
          }
          t = mul_rn(mul_rn(g, w), xv[v]);
        }
        y[v] = any[v] ? add_rn(y[v], t) : t;
        any[v] = true;
      }
    }
    if (MODE == DV3_MASTER_F32) {
      float* o = reinterpret_cast<float*>(out) + n0;
      if (n0 + V <= N) {
        *reinterpret_cast<f32x4*>(o) = f32x4{y[0], y[1], y[2], y[3]};
      } else {
#pragma unroll
        for (int v = 0; v < V; ++v)
          if (n0 + v < N) o[v] = y[v];
      }
    } else {
      i16x8 q8;
#pragma unroll
      for (int v = 0; v < V; ++v) {
        if (MODE == DV3_MASTER_I16_REFERENCE) {
          q8[v] = master_clamp_i16(truncf(y[v]));
        } else {
          float r = mul_rn(y[v], 32767.0f);
          if (DITHER) r = add_rn(r, master_dither(n0 + v, k0, k1));
          q8[v] = master_clamp_i16(rintf(r));
        }
      }
      int16_t* o = reinterpret_cast<int16_t*>(out) + n0;
      if (n0 + V <= N) {
        *reinterpret_cast<i16x8*>(o) = q8;
      } else {
#pragma unroll
        for (int v = 0; v < V; ++v)
          if (n0 + v < N) o[v] = q8[v];
      }
    }
  }
}

constexpr int64_t kMaxSamples = (int64_t)1 << 40;

}  // namespace

extern "C" int dv3_wave_levels_f32(const float* x, const int64_t* starts, const int64_t* lengths, int32_t B, int64_t max_len,
                                   double* scratch, double* levels, void* stream) {
  DV3_REQUIRE(x, "wave_levels: x is null");
  DV3_REQUIRE(starts, "wave_levels: starts is null");
  DV3_REQUIRE(lengths, "wave_levels: lengths is null");
  DV3_REQUIRE(levels, "wave_levels: levels is null");
  DV3_REQUIRE(B >= 1 && B <= 65535, "wave_levels: B = %d outside [1, 65535]", (int)B);
  DV3_REQUIRE(max_len >= 0 && max_len <= kMaxSamples, "wave_levels: max_len = %lld outside [0, 2^40]", (long long)max_len);
  DV3_REQUIRE(scratch || max_len == 0, "wave_levels: scratch is null with max_len = %lld", (long long)max_len);
  DV3_REQUIRE(((uintptr_t)levels & 7) == 0 && ((uintptr_t)scratch & 7) == 0 && ((uintptr_t)x & 3) == 0,
              "wave_levels: levels or scratch is not 8-byte aligned, or x not 4-byte aligned");
  const int nchunk = (int)dv3_cdiv64(max_len, DV3_LEVELS_CHUNK);
  if (nchunk > 0) {
    hipLaunchKernelGGL(wave_levels_chunk_kernel, dim3(nchunk, B), dim3(kThreads), 0, (hipStream_t)stream, x, starts, lengths,
                       max_len, nchunk, scratch);
    const int rc = dv3_check_launch("wave_levels (chunks)");
    if (rc != DV3_OK) return rc;
  }
  hipLaunchKernelGGL(wave_levels_final_kernel, dim3(dv3_cdiv(B, 64)), dim3(64), 0, (hipStream_t)stream, lengths, max_len,
                     (int)B, nchunk, scratch, levels);
  return dv3_check_launch("wave_levels");
}

extern "C" int dv3_wave_gains_f32(const double* levels, const int64_t* lengths, const int32_t* goff, int32_t B, int32_t G,
                                  int32_t policy, double target, double ceiling, double max_gain, float* gain,
                                  void* stream) {
  DV3_REQUIRE(levels, "wave_gains: levels is null");
  DV3_REQUIRE(lengths, "wave_gains: lengths is null");
  DV3_REQUIRE(goff, "wave_gains: goff is null");
  DV3_REQUIRE(gain, "wave_gains: gain is null");
  DV3_REQUIRE(B >= 1 && B <= 65535, "wave_gains: B = %d outside [1, 65535]", (int)B);
  DV3_REQUIRE(G >= 1 && G <= B, "wave_gains: G = %d outside [1, B = %d]", (int)G, (int)B);
  DV3_REQUIRE(policy == DV3_GAIN_PEAK || policy == DV3_GAIN_RMS || policy == DV3_GAIN_REFERENCE,
              "wave_gains: policy = %d is none of PEAK, RMS, REFERENCE", (int)policy);
  if (policy != DV3_GAIN_REFERENCE) {
    const bool ok = target > 0.0 && target < (double)INFINITY && ceiling > 0.0 && ceiling < (double)INFINITY &&
                    max_gain > 0.0 && max_gain < (double)INFINITY;
    DV3_REQUIRE(ok, "wave_gains: target = %g, ceiling = %g, max_gain = %g must be positive finite linear values", target,
                ceiling, max_gain);
  }
  hipLaunchKernelGGL(wave_gains_kernel, dim3(dv3_cdiv(G, 64)), dim3(64), 0, (hipStream_t)stream, levels, lengths, goff,
                     (int)B, (int)G, (int)policy, target, ceiling, max_gain, gain);
  return dv3_check_launch("wave_gains");
}

extern "C" int dv3_wave_master_f32(const float* x, const int64_t* src, const int64_t* len, const int64_t* dst,
                                   const float* gain, const int32_t* flags, int32_t S, const float* fade, int32_t F,
                                   int32_t mode, int32_t dither, uint64_t seed, void* out, int64_t N, void* stream) {
  DV3_REQUIRE(x, "wave_master: x is null");
  DV3_REQUIRE(src && len && dst, "wave_master: src, len or dst is null");
  DV3_REQUIRE(gain, "wave_master: gain is null");
  DV3_REQUIRE(flags, "wave_master: flags is null");
  DV3_REQUIRE(out, "wave_master: out is null");
  DV3_REQUIRE(S >= 1 && S <= DV3_MASTER_MAX_SEGMENTS, "wave_master: S = %d outside [1, %d]", (int)S, DV3_MASTER_MAX_SEGMENTS);
  DV3_REQUIRE(F >= 0 && F <= DV3_MASTER_MAX_FADE, "wave_master: F = %d outside [0, %d]", (int)F, DV3_MASTER_MAX_FADE);
  DV3_REQUIRE(fade || F == 0, "wave_master: fade is null with F = %d", (int)F);
  DV3_REQUIRE(N >= 0 && N <= kMaxSamples, "wave_master: N = %lld outside [0, 2^40]", (long long)N);
  DV3_REQUIRE(mode == DV3_MASTER_F32 || mode == DV3_MASTER_I16 || mode == DV3_MASTER_I16_REFERENCE,
              "wave_master: mode = %d is none of F32, I16, I16_REFERENCE", (int)mode);
  DV3_REQUIRE(dither == 0 || dither == 1, "wave_master: dither = %d is neither 0 nor 1", (int)dither);
  DV3_REQUIRE(mode != DV3_MASTER_I16_REFERENCE || (F == 0 && dither == 0),
              "wave_master: the reference mode takes no fades (F = %d) and no dither (%d)", (int)F, (int)dither);
  DV3_REQUIRE(mode != DV3_MASTER_F32 || dither == 0, "wave_master: dither needs an int16 mode");
  DV3_REQUIRE(((uintptr_t)out & 15) == 0 && ((uintptr_t)x & 3) == 0, "wave_master: out is not 16-byte aligned, or x not 4-byte aligned");
  DV3_REQUIRE((const void*)x != (const void*)out, "wave_master: out must not be x");
  if (N == 0) return DV3_OK;
  const int V = mode == DV3_MASTER_F32 ? 4 : 8;
  const int64_t blocks = dv3_cdiv64(N, (int64_t)kThreads * V * kMasterChunks);
  const uint32_t k0 = (uint32_t)seed, k1 = (uint32_t)(seed >> 32);
#define DV3_MASTER_LAUNCH(M, D)                                                                                          \
  hipLaunchKernelGGL((wave_master_kernel<M, D>), dim3((unsigned)blocks), dim3(kThreads), 0, (hipStream_t)stream, x, src, \
                     len, dst, gain, flags, (int)S, fade, (int)F, k0, k1, out, N)
  if (mode == DV3_MASTER_F32) DV3_MASTER_LAUNCH(DV3_MASTER_F32, false);
  else if (mode == DV3_MASTER_I16_REFERENCE) DV3_MASTER_LAUNCH(DV3_MASTER_I16_REFERENCE, false);
  else if (dither) DV3_MASTER_LAUNCH(DV3_MASTER_I16, true);
  else DV3_MASTER_LAUNCH(DV3_MASTER_I16, false);
#undef DV3_MASTER_LAUNCH
  return dv3_check_launch("wave_master");
}

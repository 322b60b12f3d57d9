// Alignment diagnostics for free-running synthesis (include/dv3hip.h: dv3_alignment_stats_f32).
//
// The step kernels store one probability row per decoder step; here every row is reduced to the key it attended
// (path: first-maximum argmax, the rule of attn_step_item and attn_argmax_kernel, deepvoice3.py:445) and to the share of
// its mass on that key (peak), and a finishing pass scans each item's path into DV3_ALIGN_COLS fp32 columns.
//
//   rows pass    grid (slices, B), 4 waves per workgroup, one wave per row: item b's OWN steps t < steps[b] are cut into
//                gridDim.x slices (the per-item loss kernels' cut), lanes read n = lane, lane + 64, ... < key_len[b]
//                (coalesced dwords, any row stride), a shuffle reduction carries (value, index) and the row sum.
//                path / peak go to scratch; nothing outside t < steps[b], n < key_len[b] is read.
//   finish pass  one wave per item: 64 steps per trip, the neighbour path[t - 1] re-read from scratch, run boundaries
//                as a ballot mask (the stall length of a run is the distance of two set bits), distinct keys in an LDS
//                bitmap.  Integer LDS atomics only; every floating-point sum has a fixed order: two calls agree bit for bit.
#include "common.h"

namespace {

constexpr int kRowWaves = 4;                    // rows in flight per workgroup
constexpr int kSliceRows = 16, kMaxSlices = 64;
constexpr int kMaxKeys = 4096;                  // the finishing pass's bitmap: kMaxKeys / 32 LDS words

inline int row_slices(int T) {
  const int s = dv3_cdiv(T, kSliceRows);
  return s < 1 ? 1 : (s > kMaxSlices ? kMaxSlices : s);
}

__device__ __forceinline__ int clamp_i(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

// scratch: path int32 [B][T] | peak fp32 [B][T]; a bad row is stored as peak = -1 (a good row's peak is > 0)
__global__ __launch_bounds__(64 * kRowWaves) void align_rows_kernel(const float* __restrict__ attn, int64_t item_stride,
                                                                    int64_t step_stride, int T, int Tk,
                                                                    const int32_t* __restrict__ steps,
                                                                    const int32_t* __restrict__ key_len,
                                                                    int32_t* __restrict__ path, float* __restrict__ peak) {
  const int b = blockIdx.y, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int Tb = clamp_i(steps[b], 0, T), Nb = clamp_i(key_len[b], 1, Tk);
  const int per = (Tb + (int)gridDim.x - 1) / (int)gridDim.x;
  const int t0 = min((int)blockIdx.x * per, Tb), t1 = min(t0 + per, Tb);
  const float* __restrict__ item = attn + (int64_t)b * item_stride;
  for (int t = t0 + wave; t < t1; t += kRowWaves) {      // wave-uniform
    const float* __restrict__ row = item + (int64_t)t * step_stride;
    float best = -INFINITY, sum = 0.f;
    int bi = 0x7fffffff;
    for (int n = lane; n < Nb; n += 64) {
      const float v = row[n];
      sum += v;
      if (v > best) { best = v; bi = n; }                // a NaN never wins
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
      const float ov = __shfl_xor(best, off, 64);
      const int oi = __shfl_xor(bi, off, 64);
      sum += __shfl_xor(sum, off, 64);
      if (ov > best || (ov == best && oi < bi)) { best = ov; bi = oi; }
    }
    if (lane == 0) {
      const bool bad = !(sum > 0.f) || !(sum < INFINITY) || bi == 0x7fffffff;
      path[(int64_t)b * T + t] = bad ? 0 : bi;
      peak[(int64_t)b * T + t] = bad ? -1.f : best / sum;
    }
  }
}

__device__ __forceinline__ int wave_max_i(int v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v = max(v, __shfl_xor(v, off, 64));
  return v;
}
__device__ __forceinline__ int wave_sum_i(int v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
  return v;
}

__global__ __launch_bounds__(64) void align_finish_kernel(const int32_t* __restrict__ path, const float* __restrict__ peak,
                                                          int T, int Tk, const int32_t* __restrict__ steps,
                                                          const int32_t* __restrict__ key_len, float* __restrict__ out) {
  __shared__ uint32_t seen[kMaxKeys / 32];
  const int b = blockIdx.x, lane = threadIdx.x;
  const int Tb = clamp_i(steps[b], 0, T), Nb = clamp_i(key_len[b], 1, Tk);
  const int words = (Nb + 31) >> 5;
  for (int w = lane; w < words; w += 64) seen[w] = 0u;
  __syncthreads();
  const int32_t* __restrict__ pb = path + (int64_t)b * T;
  const float* __restrict__ kb = peak + (int64_t)b * T;
  double fsum = 0.0;
  float fmin = INFINITY;
  int furthest = 0, end_step = 0x7fffffff, back = 0, jump = 0, stall = 0, bad = 0;
  int run_start = 0;                       // first step of the run that is open at the trip's first step
  for (int c = 0; c < Tb; c += 64) {       // wave-uniform
    const int t = c + lane;
    const bool on = t < Tb;
    const int p = on ? pb[t] : 0;
    const int q = (on && t > 0) ? pb[t - 1] : 0;          // path[-1] = 0
    float f = on ? kb[t] : 0.f;
    if (on) {
      if (f < 0.f) { f = 0.f; ++bad; }
      fsum += (double)f;
      fmin = fminf(fmin, f);
      furthest = max(furthest, p);
      if (p >= Nb - 1) end_step = min(end_step, t);
      if (t > 0 && p < q) ++back;
      jump = max(jump, p - q);
      atomicOr(&seen[p >> 5], 1u << (p & 31));
    }
    // a run starts where the path changes; the run before a start at t began at the nearest start below t
    const bool start = on && t > 0 && p != q;
    const unsigned long long m = __ballot(start);
    if (start) {
      const unsigned long long below = m & ((1ull << lane) - 1ull);
      const int prev = below ? c + 63 - __clzll((long long)below) : run_start;
      stall = max(stall, t - prev);
    }
    if (m) run_start = c + 63 - __clzll((long long)m);
  }
  if (Tb > 0) stall = max(stall, Tb - run_start);          // the run that is open at the end
  __syncthreads();
  int covered = 0;
  for (int w = lane; w < words; w += 64) covered += __popc(seen[w]);
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    fsum += __shfl_xor(fsum, off, 64);
    fmin = fminf(fmin, __shfl_xor(fmin, off, 64));
    end_step = min(end_step, __shfl_xor(end_step, off, 64));
  }
  furthest = wave_max_i(furthest);
  jump = wave_max_i(jump);
  stall = wave_max_i(stall);
  back = wave_sum_i(back);
  bad = wave_sum_i(bad);
  covered = wave_sum_i(covered);
  if (end_step == 0x7fffffff) end_step = -1;
  if (lane < DV3_ALIGN_COLS) {
    float v = 0.f;
    switch (lane) {
      case 0: v = (float)Tb; break;
      case 1: v = (float)Nb; break;
      case 2: v = Tb > 0 ? (float)(fsum / (double)Tb) : 0.f; break;
      case 3: v = Tb > 0 ? fmin : 0.f; break;
      case 4: v = Tb > 0 ? (float)pb[Tb - 1] : 0.f; break;
      case 5: v = (float)furthest; break;
      case 6: v = (float)end_step; break;
      case 7: v = end_step >= 0 ? (float)(Tb - 1 - end_step) : 0.f; break;
      case 8: v = (float)covered; break;
      case 9: v = (float)back; break;
      case 10: v = (float)jump; break;
      case 11: v = (float)stall; break;
      default: v = (float)bad; break;
    }
    out[(int64_t)b * DV3_ALIGN_COLS + lane] = v;
  }
}

}  // namespace

extern "C" int dv3_alignment_stats_scratch_bytes(int32_t B, int32_t T) {
  if (B <= 0 || T <= 0 || (int64_t)B * T * 8 >= (1ll << 31)) return 0;
  return (int)((int64_t)B * T * 8);
}

extern "C" int dv3_alignment_stats_f32(const float* attn, int64_t item_stride, int64_t step_stride, int32_t B, int32_t T,
                                       int32_t Tk, const int32_t* steps, const int32_t* key_len, float* out,
                                       void* scratch, void* stream) {
  DV3_REQUIRE(attn, "alignment_stats: attn is null");
  DV3_REQUIRE(steps, "alignment_stats: steps is null");
  DV3_REQUIRE(key_len, "alignment_stats: key_len is null");
  DV3_REQUIRE(out, "alignment_stats: out is null");
  DV3_REQUIRE(scratch, "alignment_stats: scratch is null");
  DV3_REQUIRE(B >= 1 && B <= 65535, "alignment_stats: B = %d outside [1, 65535]", (int)B);
  DV3_REQUIRE(T >= 1, "alignment_stats: T = %d < 1", (int)T);
  DV3_REQUIRE(Tk >= 1, "alignment_stats: Tk = %d < 1", (int)Tk);
  DV3_REQUIRE(Tk <= kMaxKeys, "alignment_stats: Tk = %d > %d (the distinct-key bitmap)", (int)Tk, kMaxKeys);
  DV3_REQUIRE(dv3_alignment_stats_scratch_bytes(B, T) > 0, "alignment_stats: B * T = %lld rows do not fit the scratch query",
              (long long)B * T);
  DV3_REQUIRE(((uintptr_t)out & 3) == 0, "alignment_stats: out is not 4-byte aligned");
  DV3_REQUIRE(((uintptr_t)scratch & 3) == 0, "alignment_stats: scratch is not 4-byte aligned");
  hipStream_t st = (hipStream_t)stream;
  int32_t* path = (int32_t*)scratch;
  float* peak = (float*)scratch + (int64_t)B * T;
  hipLaunchKernelGGL(align_rows_kernel, dim3(row_slices(T), B), dim3(64 * kRowWaves), 0, st, attn, item_stride,
                     step_stride, (int)T, (int)Tk, steps, key_len, path, peak);
  hipLaunchKernelGGL(align_finish_kernel, dim3(B), dim3(64), 0, st, (const int32_t*)path, (const float*)peak, (int)T,
                     (int)Tk, steps, key_len, out);
  return dv3_check_launch("alignment_stats_f32");
}

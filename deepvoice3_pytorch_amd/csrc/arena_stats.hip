// Per-tensor statistics of the flat arenas: a segmented reduction over the parameter, gradient and
// moment arenas, on demand, in two launches and without atomics -- the same data gives the same table bit for bit.
//   stage 1   one workgroup per CHUNK of a host-built table (element offset, length <= 4096, tensor index): a chunk
//             lies inside one tensor and covers none of the 0-3 padding elements between tensors; 16 bytes per lane
//             where the chunk starts on a 16-byte boundary (arena offsets are multiples of 4: every chunk does), one
//             element at a time for the last length % 4.  Six fp32 partials per chunk go to a scratch row.
//   stage 2   one wave per tensor over its contiguous run of scratch rows: sums and the count in fp64, maxima in fp32
//             (exact), one float64 row of the table.
// HBM-bound: 16 B per parameter (8 B when the last pass was skipped: the moments are not read then).
#include "common.h"
#include <float.h>

namespace {

constexpr int STAT_COLS = DV3_TENSOR_STAT_COLS;
constexpr int CHUNK_MAX = DV3_ARENA_CHUNK_MAX;

struct stat_acc {
  float g_sumsq, g_absmax, g_bad, p_sumsq, p_absmax, u_sumsq;
};

// gradient: NaN / +-Inf elements are counted and left out of the sum and the maximum
__device__ __forceinline__ void acc_grad_param(stat_acc& a, float gi, float pi, float prescale) {
  const float ag = fabsf(gi);
  if (ag <= FLT_MAX) {
    const float x = prescale * ag;
    a.g_sumsq += x * x;
    a.g_absmax = fmaxf(a.g_absmax, x);
  } else {
    a.g_bad += 1.0f;
  }
  a.p_sumsq += pi * pi;
  a.p_absmax = fmaxf(a.p_absmax, fabsf(pi));
}

// the update the last pass applied, from the moments it left: step_size * m / (sqrt(v) / bc2s + eps)
__device__ __forceinline__ void acc_update(stat_acc& a, float mi, float vi, float step_size, float bc2s, float eps) {
  const float d = step_size * (mi / (sqrtf(vi) / bc2s + eps));
  a.u_sumsq += d * d;
}

__global__ __launch_bounds__(256) void arena_stats_chunk_kernel(
    const float* __restrict__ p, const float* __restrict__ g, const float* __restrict__ m, const float* __restrict__ v,
    const float* __restrict__ hyper, const float* __restrict__ health, const int64_t* __restrict__ chunks, int64_t n,
    float prescale, float eps, float* __restrict__ scratch) {
  const int64_t c = blockIdx.x;
  const int64_t off = chunks[3 * c];
  int64_t len = chunks[3 * c + 1];
  // a row that does not lie inside the arena is read as empty (the table is built by the host: train_step.arena_chunks)
  if (off < 0 || len < 0 || len > CHUNK_MAX || off > n - len) len = 0;
  const bool skipped = health != nullptr && health[1] != 0.0f;        // a skipped pass moved nothing: column 5 is 0
  const float step_size = hyper[0] / hyper[1], bc2s = hyper[2];
  stat_acc a = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  const int tid = threadIdx.x;
  const int64_t len4 = (off & 3) == 0 ? (len & ~(int64_t)3) : 0;
  for (int64_t i = (int64_t)tid * 4; i < len4; i += 256 * 4) {
    const f32x4 gv = *reinterpret_cast<const f32x4*>(g + off + i);
    const f32x4 pv = *reinterpret_cast<const f32x4*>(p + off + i);
#pragma unroll
    for (int k = 0; k < 4; ++k) acc_grad_param(a, gv[k], pv[k], prescale);
    if (!skipped) {
      const f32x4 mv = *reinterpret_cast<const f32x4*>(m + off + i);
      const f32x4 vv = *reinterpret_cast<const f32x4*>(v + off + i);
#pragma unroll
      for (int k = 0; k < 4; ++k) acc_update(a, mv[k], vv[k], step_size, bc2s, eps);
    }
  }
  for (int64_t i = len4 + tid; i < len; i += 256) {
    acc_grad_param(a, g[off + i], p[off + i], prescale);
    if (!skipped) acc_update(a, m[off + i], v[off + i], step_size, bc2s, eps);
  }
  __shared__ float red[STAT_COLS][4];
  a.g_sumsq = dv3_wave_sum(a.g_sumsq);
  a.g_absmax = dv3_wave_max(a.g_absmax);
  a.g_bad = dv3_wave_sum(a.g_bad);
  a.p_sumsq = dv3_wave_sum(a.p_sumsq);
  a.p_absmax = dv3_wave_max(a.p_absmax);
  a.u_sumsq = dv3_wave_sum(a.u_sumsq);
  if ((tid & 63) == 0) {
    const int w = tid >> 6;
    red[0][w] = a.g_sumsq, red[1][w] = a.g_absmax, red[2][w] = a.g_bad;
    red[3][w] = a.p_sumsq, red[4][w] = a.p_absmax, red[5][w] = a.u_sumsq;
  }
  __syncthreads();
  if (tid < STAT_COLS) {
    const float* r = red[tid];
    const bool is_max = tid == 1 || tid == 4;
    scratch[c * STAT_COLS + tid] = is_max ? fmaxf(fmaxf(r[0], r[1]), fmaxf(r[2], r[3])) : r[0] + r[1] + r[2] + r[3];
  }
}

__device__ __forceinline__ double wave_sum_f64(double x) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) x += __shfl_xor(x, off, 64);
  return x;
}

// one wave per tensor: rows [first, first + count) of the scratch, lane l takes rows l, l + 64, ... in ascending order
__global__ __launch_bounds__(64) void arena_stats_tensor_kernel(const float* __restrict__ scratch,
                                                                const int64_t* __restrict__ ranges, int64_t n_chunks,
                                                                double* __restrict__ out) {
  const int64_t t = blockIdx.x;
  const int64_t first = ranges[2 * t];
  int64_t count = ranges[2 * t + 1];
  if (first < 0 || count < 0 || first > n_chunks - count) count = 0;
  double s[STAT_COLS] = {0., 0., 0., 0., 0., 0.};
  float mx1 = 0.f, mx4 = 0.f;
  for (int64_t r = threadIdx.x; r < count; r += 64) {
    const float* row = scratch + (first + r) * STAT_COLS;
    s[0] += (double)row[0];
    mx1 = fmaxf(mx1, row[1]);
    s[2] += (double)row[2];
    s[3] += (double)row[3];
    mx4 = fmaxf(mx4, row[4]);
    s[5] += (double)row[5];
  }
  s[0] = wave_sum_f64(s[0]);
  s[2] = wave_sum_f64(s[2]);
  s[3] = wave_sum_f64(s[3]);
  s[5] = wave_sum_f64(s[5]);
  s[1] = (double)dv3_wave_max(mx1);
  s[4] = (double)dv3_wave_max(mx4);
  if (threadIdx.x == 0) {
#pragma unroll
    for (int k = 0; k < STAT_COLS; ++k) out[t * STAT_COLS + k] = s[k];
  }
}

}  // namespace

extern "C" int dv3_arena_stats_f32(const float* p, const float* g, const float* m, const float* v, int64_t n,
                                   const float* hyper, const float* health, const int64_t* chunks, int64_t n_chunks,
                                   const int64_t* ranges, int32_t n_tensors, float grad_prescale, float eps,
                                   float* scratch, double* out, void* stream) {
  DV3_REQUIRE(p && g && m && v && hyper && chunks && ranges && scratch && out, "arena_stats: bad args");
  DV3_REQUIRE(n > 0 && n_chunks > 0 && n_chunks < ((int64_t)1 << 31) && n_tensors > 0, "arena_stats: bad sizes");
  const uintptr_t bits = (uintptr_t)p | (uintptr_t)g | (uintptr_t)m | (uintptr_t)v;
  DV3_REQUIRE((bits & 15) == 0, "arena_stats: the arenas must be 16-byte aligned");
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(arena_stats_chunk_kernel, dim3((unsigned)n_chunks), dim3(256), 0, st, p, g, m, v, hyper, health,
                     chunks, n, grad_prescale, eps, scratch);
  hipLaunchKernelGGL(arena_stats_tensor_kernel, dim3((unsigned)n_tensors), dim3(64), 0, st, scratch, ranges, n_chunks,
                     out);
  return dv3_check_launch("arena_stats_f32");
}

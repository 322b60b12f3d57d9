// Look-ahead peak limiter: a time-varying gain that keeps every span of a flat buffer under a ceiling, so that a loudness
// target can be met where one static gain would have to give way to the loudest syllable (include/dv3hip.h:
// dv3_wave_limit_f32, where the definition is stated in full).  The reference has no counterpart.
//
// The item is cut into tiles of DV3_LIMIT_TILE samples counted from its own first sample; one workgroup of 256 per tile.
//   pass A  stages y = fmul(g, x) of the tile with 6 samples before and A + 6 behind it, takes the detector e, the
//           demanded reduction dr and its look-ahead maximum dm, then runs the release recursion from a ZERO state at the
//           tile's first sample; dq_local and the tile's end value go to scratch, with the tile's count of dr > 0;
//   pass B  one lane per item walks the end values: carry' = max(end, carry rho^T) -- every tile's true start state;
//   pass C  dq = max(dq_local, carry rho^(i + 1)) over the tile and the A samples before it, the box mean ds over
//           [n - A, n], s = 1 - ds, out = fmul(y, (float) s), and the tile's min s;
//   report  one lane per item takes min s and the sum of the counts.
// Every windowed operation is a DOUBLING over an LDS array, ping-ponged between two buffers with one barrier per step:
//   look-ahead   m_2d[n] = max(m_d[n], m_d[n + d]), closed by max(m_p[n], m_p[n + W - p]) for the window W = A + 1,
//                p the largest power of two <= W: exact, whatever the order;
//   release      v[n] = max(v[n], v[n - d] rho^d), d = 1, 2, .., T / 2, rho^(2^i) from the host: the recursion
//                dq[n] = max(dm[n], rho dq[n - 1]) written as max over k <= n of dm[k] rho^(n - k);
//   box          S_2d[n] = S_d[n] + S_d[n - d]; the window [n - A, n] is the concatenation of the power-of-two windows
//                of W's binary digits, each added once to a register: sums of non-negative terms only, so nothing
//                cancels (a difference of prefix sums over the tile would lose what the 1e-12 bound on ds asks for), and
//                A = 0 gives ds = dq exactly.  The order of the additions depends on W and n alone, not on the tile.
// A lane owns elements tid, tid + 256, ..: 32 consecutive lanes read 32 consecutive doubles, at any offset d -- every
// ds_read_b64 of a step falls on 64 distinct banks.
// dq_local is STORED (8 bytes a sample written and read) rather than recomputed in pass C: recomputing needs the detector
// (36 fp64 fmas a sample under the true-peak one) and both scans again over T + A samples with a halo of 2 A + 12.
// No atomics; nothing depends on B, on where a span lies in the flat buffer or on the launch geometry.
#include "common.h"

namespace {

constexpr int kT = DV3_LIMIT_TILE;
constexpr int kLog2T = 10;
static_assert((1 << kLog2T) == kT, "the tile is a power of two: the release scan doubles up to it");
static_assert(DV3_LIMIT_MAX_LOOKAHEAD <= kT, "pass C reads dq of one tile back at the most");
static_assert(DV3_LIMIT_RHO_POWERS == kLog2T + 1, "rho^(2^i), i = 0 .. log2 T");
constexpr int kThreads = 256;
constexpr int kBuf = kT + DV3_LIMIT_MAX_LOOKAHEAD + 8;      // doubles per ping-pong buffer (T + A + 1 used)
constexpr int kYs = kT + DV3_LIMIT_MAX_LOOKAHEAD + 16;      // staged samples (T + A + 12 used)
constexpr int64_t kMaxLen = (int64_t)1 << 30;

struct RhoPow {                         // rho^(2^i), i = 0 .. log2 T
  double p[DV3_LIMIT_RHO_POWERS];
};
struct PeakTable {
  float t[3 * DV3_TRUE_PEAK_TAPS];
};

// scratch of an item: dq_local [nt][T] | carry [nt] (pass A: the tiles' end values) | part [nt][2] (count, min s)
__device__ __forceinline__ double* item_scratch(double* scratch, int b, int nt) {
  return scratch + (int64_t)b * nt * (kT + 3);
}

// rho^m, 1 <= m <= T, as the product of the table's powers in ascending order of m's binary digits
__device__ __forceinline__ double rho_power(const RhoPow& rp, int m) {
  double v = 1.0;
#pragma unroll
  for (int i = 0; i <= kLog2T; ++i)
    if ((m >> i) & 1) v *= rp.p[i];
  return v;
}

// ---- pass A -----------------------------------------------------------------------------------------------------------
template <bool TRUE_PEAK>
__global__ __launch_bounds__(kThreads) void limit_detect_kernel(const float* __restrict__ x,
                                                                const int64_t* __restrict__ starts,
                                                                const int64_t* __restrict__ lengths, int64_t max_len,
                                                                const float* __restrict__ gain, double ceiling, int A,
                                                                RhoPow rp, PeakTable tab, int nt,
                                                                double* __restrict__ scratch) {
#pragma clang fp contract(off)
  __shared__ float s_y[kYs];
  __shared__ double s_a[kBuf], s_b[kBuf];
  __shared__ int s_cnt[kThreads / 64];
  const int b = blockIdx.y, t = blockIdx.x, tid = threadIdx.x;
  const int64_t n = min(max(lengths[b], (int64_t)0), max_len);
  const int64_t n0 = (int64_t)t * kT;                      // the tile's first sample, from the item's own start
  if (n0 >= n) return;                                     // workgroup-uniform: pass B and C read ceil(n / T) tiles
  const float* __restrict__ xs = x + starts[b];
  const float g = gain[b];
  const int NE = kT + A;                                   // dr is needed at samples n0 .. n0 + T + A - 1
  // s_y[q] = y[n0 - 6 + q], zero outside the span
  for (int q = tid; q < NE + 12; q += kThreads) {
    const int64_t i = n0 - 6 + q;
    s_y[q] = (i >= 0 && i < n) ? g * xs[i] : 0.0f;
  }
  __syncthreads();
  if (TRUE_PEAK) {
    // s_a[r] = max over p of |i_p[m]|, m = n0 - 1 + r, for -1 <= m < n (0 elsewhere): tap j reads y[m + 6 - j] = s_y[r + 11 - j]
    for (int r = tid; r < NE + 1; r += kThreads) {
      const int64_t m = n0 - 1 + r;
      double v = 0.0;
      if (m >= -1 && m < n) {
#pragma unroll
        for (int p = 0; p < 3; ++p) {
          double acc = 0.0;
#pragma unroll
          for (int j = 0; j < DV3_TRUE_PEAK_TAPS; ++j)
            acc = fma((double)tab.t[p * DV3_TRUE_PEAK_TAPS + j], (double)s_y[r + 11 - j], acc);
          v = fmax(v, fabs(acc));
        }
      }
      s_a[r] = v;
    }
    __syncthreads();
  }
  int cnt = 0;
  for (int q = tid; q < NE; q += kThreads) {               // sample n0 + q = s_y[q + 6]
    double d = 0.0;
    if (n0 + q < n) {
      double e = fabs((double)s_y[q + 6]);
      if (TRUE_PEAK) e = fmax(e, fmax(s_a[q + 1], s_a[q]));
      if (e > ceiling) d = 1.0 - ceiling / e;
      if (q < kT && d > 0.0) ++cnt;
    }
    s_b[q] = d;
  }
  __syncthreads();
  // look-ahead: the maximum over [n, n + A] by doubling (what lies past NE is past every window a tile sample has)
  double* src = s_b;
  double* dst = s_a;
  const int W = A + 1;
  int p = 1;
  for (; 2 * p <= W; p *= 2) {
    for (int q = tid; q < NE; q += kThreads) dst[q] = q + p < NE ? fmax(src[q], src[q + p]) : src[q];
    __syncthreads();
    double* sw = src; src = dst; dst = sw;
  }
  if (W > p) {
    for (int q = tid; q < NE; q += kThreads) dst[q] = q + W - p < NE ? fmax(src[q], src[q + W - p]) : src[q];
    __syncthreads();
    double* sw = src; src = dst; dst = sw;
  }
  // release from a zero state at the tile's first sample
#pragma unroll 1
  for (int i = 0; i < kLog2T; ++i) {
    const int d = 1 << i;
    const double f = rp.p[i];
    for (int q = tid; q < kT; q += kThreads) dst[q] = q >= d ? fmax(src[q], src[q - d] * f) : src[q];
    __syncthreads();
    double* sw = src; src = dst; dst = sw;
  }
  double* __restrict__ sc = item_scratch(scratch, b, nt);
  double* __restrict__ dql = sc + (int64_t)t * kT;
  for (int q = tid; q < kT; q += kThreads) dql[q] = src[q];
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) cnt += __shfl_xor(cnt, off, 64);
  if ((tid & 63) == 0) s_cnt[tid >> 6] = cnt;
  __syncthreads();
  if (tid == 0) {
    sc[(int64_t)nt * kT + t] = src[kT - 1];
    sc[(int64_t)nt * (kT + 1) + 2 * t] = (double)(((s_cnt[0] + s_cnt[1]) + s_cnt[2]) + s_cnt[3]);
  }
}

// ---- pass B: the tiles' end values become every tile's carry, dq at the sample before its first ---------------------------
__global__ __launch_bounds__(64) void limit_walk_kernel(const int64_t* __restrict__ lengths, int64_t max_len, int B, int nt,
                                                        double rhoT, double* __restrict__ scratch) {
#pragma clang fp contract(off)
  const int b = blockIdx.x * 64 + threadIdx.x;
  if (b >= B) return;
  const int64_t n = min(max(lengths[b], (int64_t)0), max_len);
  const int ntile = (int)((n + kT - 1) / kT);
  double* __restrict__ carry = item_scratch(scratch, b, nt) + (int64_t)nt * kT;
  double c = 0.0;
  for (int t = 0; t < ntile; ++t) {
    const double e = carry[t];
    carry[t] = c;
    c = fmax(e, c * rhoT);
  }
}

// ---- pass C -----------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kThreads) void limit_apply_kernel(const float* __restrict__ x, const int64_t* __restrict__ starts,
                                                               const int64_t* __restrict__ lengths, int64_t max_len,
                                                               const float* __restrict__ gain, int A, RhoPow rp, int nt,
                                                               double* __restrict__ scratch, float* __restrict__ out) {
#pragma clang fp contract(off)
  __shared__ double s_a[kBuf], s_b[kBuf];
  __shared__ double s_min[kThreads / 64];
  const int b = blockIdx.y, t = blockIdx.x, tid = threadIdx.x;
  const int64_t n = min(max(lengths[b], (int64_t)0), max_len);
  const int64_t n0 = (int64_t)t * kT;
  if (n0 >= n) return;
  double* __restrict__ sc = item_scratch(scratch, b, nt);
  const double* __restrict__ carry = sc + (int64_t)nt * kT;
  const int NE = kT + A;
  // s_a[q] = dq[max(n0 - A + q, 0)]: the tile (always written by pass A) and the A samples before it (tile t - 1)
  for (int q = tid; q < NE; q += kThreads) {
    const int64_t k = max(n0 - A + q, (int64_t)0);
    const int u = (int)(k >> kLog2T), i = (int)(k & (kT - 1));
    s_a[q] = fmax(sc[k], carry[u] * rho_power(rp, i + 1));
  }
  __syncthreads();
  // the box: S_d[q] = the sum of the d entries ending at q; sample n0 + i is entry A + i
  constexpr int kPer = kT / kThreads;
  double acc[kPer];
#pragma unroll
  for (int v = 0; v < kPer; ++v) acc[v] = 0.0;
  double* src = s_a;
  double* dst = s_b;
  const int W = A + 1;
  int off = 0;
#pragma unroll 1
  for (int d = 1; d <= W; d *= 2) {
    if (W & d) {
#pragma unroll
      for (int v = 0; v < kPer; ++v) acc[v] += src[A + v * kThreads + tid - off];
      off += d;
    }
    if (2 * d <= W) {
      for (int q = tid; q < NE; q += kThreads) dst[q] = q >= d ? src[q] + src[q - d] : src[q];
      __syncthreads();
      double* sw = src; src = dst; dst = sw;
    }
  }
  const double inv = 1.0 / (double)W;
  const float g = gain[b];
  const float* __restrict__ xs = x + starts[b];
  float* __restrict__ os = out + starts[b];
  double smin = 1.0;
#pragma unroll
  for (int v = 0; v < kPer; ++v) {
    const int64_t i = n0 + v * kThreads + tid;
    if (i < n) {
      const double s = 1.0 - inv * acc[v];
      smin = fmin(smin, s);
      const float y = g * xs[i];
      os[i] = y * (float)s;
    }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) smin = fmin(smin, __shfl_xor(smin, o, 64));
  if ((tid & 63) == 0) s_min[tid >> 6] = smin;
  __syncthreads();
  if (tid == 0) sc[(int64_t)nt * (kT + 1) + 2 * t + 1] = fmin(fmin(s_min[0], s_min[1]), fmin(s_min[2], s_min[3]));
}

__global__ __launch_bounds__(64) void limit_report_kernel(const int64_t* __restrict__ lengths, int64_t max_len, int B, int nt,
                                                          const double* __restrict__ scratch, double* __restrict__ report) {
  const int b = blockIdx.x * 64 + threadIdx.x;
  if (b >= B) return;
  const int64_t n = min(max(lengths[b], (int64_t)0), max_len);
  const int ntile = (int)((n + kT - 1) / kT);
  const double* __restrict__ part = scratch + (int64_t)b * nt * (kT + 3) + (int64_t)nt * (kT + 1);
  double smin = 1.0, over = 0.0;
  for (int t = 0; t < ntile; ++t) {
    over += part[2 * t];
    smin = fmin(smin, part[2 * t + 1]);
  }
  report[(int64_t)b * DV3_LIMIT_COLUMNS] = smin;
  report[(int64_t)b * DV3_LIMIT_COLUMNS + 1] = over;
}

}  // namespace

extern "C" int dv3_wave_limit_f32(const float* x, const int64_t* starts, const int64_t* lengths, int32_t B, int64_t max_len,
                                  const float* gain, double ceiling, int32_t lookahead, const double* rho_pow,
                                  const float* peak_table, double* scratch, float* out, double* report, void* stream) {
  DV3_REQUIRE(x, "wave_limit: x is null");
  DV3_REQUIRE(starts, "wave_limit: starts is null");
  DV3_REQUIRE(lengths, "wave_limit: lengths is null");
  DV3_REQUIRE(gain, "wave_limit: gain is null");
  DV3_REQUIRE(rho_pow, "wave_limit: rho_pow is null");
  DV3_REQUIRE(out, "wave_limit: out is null");
  DV3_REQUIRE(report, "wave_limit: report is null");
  DV3_REQUIRE(B >= 1 && B <= 65535, "wave_limit: B = %d outside [1, 65535]", (int)B);
  DV3_REQUIRE(max_len >= 0 && max_len <= kMaxLen, "wave_limit: max_len = %lld outside [0, 2^30]", (long long)max_len);
  DV3_REQUIRE(scratch || max_len == 0, "wave_limit: scratch is null with max_len = %lld", (long long)max_len);
  DV3_REQUIRE(lookahead >= 0 && lookahead <= DV3_LIMIT_MAX_LOOKAHEAD, "wave_limit: lookahead = %d outside [0, %d]",
              (int)lookahead, DV3_LIMIT_MAX_LOOKAHEAD);
  DV3_REQUIRE(ceiling > 0.0 && ceiling < (double)INFINITY, "wave_limit: ceiling = %g must be a positive finite linear value",
              ceiling);
  DV3_REQUIRE(rho_pow[0] >= 0.0 && rho_pow[0] < 1.0, "wave_limit: rho = %g outside [0, 1)", rho_pow[0]);
  for (int i = 1; i < DV3_LIMIT_RHO_POWERS; ++i)
    DV3_REQUIRE(rho_pow[i] >= 0.0 && rho_pow[i] <= rho_pow[i - 1], "wave_limit: rho_pow[%d] = %g is no power of rho = %g", i,
                rho_pow[i], rho_pow[0]);
  DV3_REQUIRE((const void*)out != (const void*)x, "wave_limit: out == x (every pass reads x: no in-place limiting)");
  DV3_REQUIRE(((uintptr_t)scratch & 7) == 0 && ((uintptr_t)report & 7) == 0 && ((uintptr_t)starts & 7) == 0 &&
                  ((uintptr_t)lengths & 7) == 0 && ((uintptr_t)x & 3) == 0 && ((uintptr_t)out & 3) == 0 &&
                  ((uintptr_t)gain & 3) == 0,
              "wave_limit: scratch, report, starts or lengths is not 8-byte aligned, or x, out or gain not 4-byte");
  PeakTable tab = {};
  if (peak_table)
    for (int i = 0; i < 3 * DV3_TRUE_PEAK_TAPS; ++i) {
      DV3_REQUIRE(peak_table[i] > -INFINITY && peak_table[i] < INFINITY, "wave_limit: peak_table[%d] is not finite", i);
      tab.t[i] = peak_table[i];
    }
  RhoPow rp;
  for (int i = 0; i < DV3_LIMIT_RHO_POWERS; ++i) rp.p[i] = rho_pow[i];
  hipStream_t s = (hipStream_t)stream;
  const int nt = (int)dv3_cdiv64(max_len, kT);
  if (nt > 0) {
    const dim3 grid(nt, B);
    if (peak_table)
      hipLaunchKernelGGL(limit_detect_kernel<true>, grid, dim3(kThreads), 0, s, x, starts, lengths, max_len, gain, ceiling,
                         (int)lookahead, rp, tab, nt, scratch);
    else
      hipLaunchKernelGGL(limit_detect_kernel<false>, grid, dim3(kThreads), 0, s, x, starts, lengths, max_len, gain, ceiling,
                         (int)lookahead, rp, tab, nt, scratch);
    int rc = dv3_check_launch("wave_limit (pass A)");
    if (rc != DV3_OK) return rc;
    hipLaunchKernelGGL(limit_walk_kernel, dim3(dv3_cdiv(B, 64)), dim3(64), 0, s, lengths, max_len, (int)B, nt,
                       rp.p[kLog2T], scratch);
    rc = dv3_check_launch("wave_limit (pass B)");
    if (rc != DV3_OK) return rc;
    hipLaunchKernelGGL(limit_apply_kernel, grid, dim3(kThreads), 0, s, x, starts, lengths, max_len, gain, (int)lookahead, rp,
                       nt, scratch, out);
    rc = dv3_check_launch("wave_limit (pass C)");
    if (rc != DV3_OK) return rc;
  }
  hipLaunchKernelGGL(limit_report_kernel, dim3(dv3_cdiv(B, 64)), dim3(64), 0, s, lengths, max_len, (int)B, nt, scratch,
                     report);
  return dv3_check_launch("wave_limit (report)");
}

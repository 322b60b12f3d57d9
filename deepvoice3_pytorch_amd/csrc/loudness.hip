// Loudness mastering: ITU-R BS.1770 integrated loudness and true peak of the utterances of a batch or a document
// (include/dv3hip.h: dv3_wave_loudness_f64, dv3_loudness_gate_f64, dv3_loudness_gains_f32, where every step is stated;
// DESIGN.md 3.6l).  The reference has no counterpart: its output stage is audio.save_wav (audio.py:16-18).
//
//   filter   The K-weighting is a 4th-order IIR filter in fp64; its high-pass pole has radius 0.989 at 22.05 kHz, so a
//            chunk cannot be warmed up by a short overlap.  Instead every item is cut into chunks of h samples counted
//            from its own first sample and the filter's linearity does the rest: the state after a chunk is
//            A^h s + (the chunk's end state from a zero state).
//              pass 1  grid (ceil(K / 64), B): a lane owns one chunk, filters it from a zero state and stores the 4-double
//                      end state;
//              pass 2  one lane per item walks its chunks with the 4x4 matrix A^h: every chunk's true start state;
//              pass 3  the grid of pass 1: a lane filters its chunk again from the true state and sums y^2 in fp64.
//            A lane reads its chunk with a stride of h samples, so a workgroup (one wave, 64 consecutive chunks) stages
//            tiles of 64 samples of each chunk through LDS: every global load is 256 contiguous bytes per wave, whatever
//            the span's alignment; the LDS rows are 65 dwords apart, so the transposed ds_read_b32 of 32 lanes falls on
//            32 banks.  The loads of tile t + 1 are in flight while tile t is filtered.
//   peak     a streaming pass of its own: a workgroup of 256 stages 1024 samples and a halo of 5 before / 6 behind in
//            LDS, a lane takes 4 samples and their 3 x 4 interpolants (12 fp32 taps each), a fixed LDS tree, one partial
//            per workgroup; a second launch takes an item's maximum.
//   gate     one wave per group, two passes over the pooled block energies.
//   gains    one lane per group: a handful of fp64 operations.
// No atomics; nothing depends on B or on where a span lies in the flat buffer.
#include "common.h"

namespace {

constexpr int kLanes = 64;              // chunks per workgroup of the filter passes, and samples of a chunk per tile
constexpr int kRow = kLanes + 1;        // LDS row stride in dwords
constexpr int kPeakThreads = 256;
constexpr int kPeakPer = DV3_TRUE_PEAK_CHUNK / kPeakThreads;      // 4 samples per lane
constexpr int kHaloLo = 5, kHaloHi = 6;
constexpr int64_t kMaxLen = (int64_t)1 << 30;

struct KCoef {                          // the two biquads, b0 b1 b2 a1 a2 each (a0 = 1), and A^h row-major
  double s[5], p[5], Ah[16];
};
struct PeakTable {
  float t[3 * DV3_TRUE_PEAK_TAPS];
};
typedef double f64x2 __attribute__((ext_vector_type(2)));

// One sample through the cascade (transposed direct form II; include/dv3hip.h states it).
__device__ __forceinline__ double kweight_step(const KCoef& c, double x, double& s1, double& s2, double& t1, double& t2) {
  const double u = c.s[0] * x + s1;
  s1 = (c.s[1] * x - c.s[3] * u) + s2;
  s2 = c.s[2] * x - c.s[4] * u;
  const double y = c.p[0] * u + t1;
  t1 = (c.p[1] * u - c.p[3] * y) + t2;
  t2 = c.p[2] * u - c.p[4] * y;
  return y;
}

// PASS 1 (ENERGY false): zero start state, the end state goes to states[b][k].  PASS 3 (ENERGY true): the start state comes
// from states[b][k], the sum of y^2 goes to energy[b][k]; chunks past the item's end get zeros in both tables.
template <bool ENERGY>
__global__ __launch_bounds__(kLanes) void kweight_chunk_kernel(const float* __restrict__ x, const int64_t* __restrict__ starts,
                                                               const int64_t* __restrict__ lengths, int64_t max_len, int h,
                                                               int K, KCoef c, double* __restrict__ states,
                                                               double* __restrict__ energy) {
  __shared__ float tile[kLanes * kRow];
  const int b = blockIdx.y, lane = threadIdx.x;
  const int k0 = blockIdx.x * kLanes, k = k0 + lane;
  const int64_t n = min(max(lengths[b], (int64_t)0), max_len);
  const int64_t base = (int64_t)k0 * h;                    // the workgroup's first sample, from the item's own start
  const int64_t mine = n - (int64_t)k * h;                 // samples left at this lane's chunk
  const int len = (int)min(max(mine, (int64_t)0), (int64_t)h);
  double* st = states + ((int64_t)b * K + k) * 4;
  if (base >= n) {                                         // workgroup-uniform: no sample of the item here
    if (ENERGY && k < K) {
      energy[(int64_t)b * K + k] = 0.0;
      *reinterpret_cast<f64x2*>(st) = f64x2{0.0, 0.0};
      *reinterpret_cast<f64x2*>(st + 2) = f64x2{0.0, 0.0};
    }
    return;
  }
  const float* __restrict__ xs = x + starts[b];
  double s1 = 0.0, s2 = 0.0, t1 = 0.0, t2 = 0.0, e = 0.0;
  if (ENERGY && len > 0) {
    const f64x2 a = *reinterpret_cast<const f64x2*>(st), d = *reinterpret_cast<const f64x2*>(st + 2);
    s1 = a[0]; s2 = a[1]; t1 = d[0]; t2 = d[1];
  }
  const int ntile = (h + kLanes - 1) / kLanes;
  float pre[kLanes];
  // Row r = chunk k0 + r: 64 consecutive samples per wave load.  Every load is unconditional, from an index clamped into
  // the item (base < n here, so n >= 1): 64 loads in flight at once, where a branch around each load would serialise
  // them.  What a clamped load brings (past the chunk's or the item's end) lands in tile columns no lane consumes: a
  // lane reads only the first len - 64 t entries of its row.
  auto fetch = [&](int t) {
    const int64_t i0 = base + t * kLanes + lane, last = n - 1;
#pragma unroll
    for (int r = 0; r < kLanes; ++r) pre[r] = xs[min(i0 + (int64_t)r * h, last)];
  };
  fetch(0);
  for (int t = 0; t < ntile; ++t) {
#pragma unroll
    for (int r = 0; r < kLanes; ++r) tile[r * kRow + lane] = pre[r];
    __syncthreads();
    if (t + 1 < ntile) fetch(t + 1);
    const int cnt = min(kLanes, len - t * kLanes);
    for (int j = 0; j < cnt; ++j) {
      const double y = kweight_step(c, (double)tile[lane * kRow + j], s1, s2, t1, t2);
      if (ENERGY) e += y * y;
    }
    __syncthreads();
  }
  if (k >= K) return;
  if (ENERGY) {
    energy[(int64_t)b * K + k] = e;
    if (len == 0) {
      *reinterpret_cast<f64x2*>(st) = f64x2{0.0, 0.0};
      *reinterpret_cast<f64x2*>(st + 2) = f64x2{0.0, 0.0};
    }
  } else if (len > 0) {
    *reinterpret_cast<f64x2*>(st) = f64x2{s1, s2};
    *reinterpret_cast<f64x2*>(st + 2) = f64x2{t1, t2};
  }
}

// PASS 2: states[b][k] holds chunk k's zero-state end state e_k; it becomes the chunk's true start state s_k:
// s_0 = 0, s_{k+1} = A^h s_k + e_k.
__global__ __launch_bounds__(64) void kweight_walk_kernel(const int64_t* __restrict__ lengths, int64_t max_len, int h, int B,
                                                          int K, KCoef c, double* __restrict__ states) {
  const int b = blockIdx.x * 64 + threadIdx.x;
  if (b >= B) return;
  const int64_t n = min(max(lengths[b], (int64_t)0), max_len);
  const int nk = (int)((n + h - 1) / h);
  double s[4] = {0.0, 0.0, 0.0, 0.0};
  for (int k = 0; k < nk; ++k) {
    double* st = states + ((int64_t)b * K + k) * 4;
    const f64x2 a = *reinterpret_cast<const f64x2*>(st), d = *reinterpret_cast<const f64x2*>(st + 2);
    const double e[4] = {a[0], a[1], d[0], d[1]};
    *reinterpret_cast<f64x2*>(st) = f64x2{s[0], s[1]};
    *reinterpret_cast<f64x2*>(st + 2) = f64x2{s[2], s[3]};
    double nx[4];
#pragma unroll
    for (int r = 0; r < 4; ++r)
      nx[r] = (((c.Ah[4 * r] * s[0] + c.Ah[4 * r + 1] * s[1]) + c.Ah[4 * r + 2] * s[2]) + c.Ah[4 * r + 3] * s[3]) + e[r];
#pragma unroll
    for (int r = 0; r < 4; ++r) s[r] = nx[r];
  }
}

// ---- true peak --------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kPeakThreads) void true_peak_chunk_kernel(const float* __restrict__ x,
                                                                       const int64_t* __restrict__ starts,
                                                                       const int64_t* __restrict__ lengths, int64_t max_len,
                                                                       int nchunk, PeakTable tab, double* __restrict__ part) {
  __shared__ float s_x[DV3_TRUE_PEAK_CHUNK + kHaloLo + kHaloHi + 5];
  __shared__ float s_m[kPeakThreads];
  const int b = blockIdx.y, cidx = blockIdx.x, tid = threadIdx.x;
  const int64_t n = min(max(lengths[b], (int64_t)0), max_len);
  const int64_t i0 = (int64_t)cidx * DV3_TRUE_PEAK_CHUNK;
  if (i0 >= n) return;                                     // workgroup-uniform: the second launch reads ceil(n / chunk)
  const float* __restrict__ xs = x + starts[b];
  for (int q = tid; q < DV3_TRUE_PEAK_CHUNK + kHaloLo + kHaloHi; q += kPeakThreads) {
    const int64_t i = i0 - kHaloLo + q;
    s_x[q] = (i >= 0 && i < n) ? xs[i] : 0.0f;             // samples outside the item's span count as zero
  }
  __syncthreads();
  float m = 0.0f;
#pragma unroll
  for (int v = 0; v < kPeakPer; ++v) {
    const int q = v * kPeakThreads + tid;                  // sample i0 + q: s_x[q + kHaloLo]
    if (i0 + q < n) {
      m = fmaxf(m, fabsf(s_x[q + kHaloLo]));
#pragma unroll
      for (int p = 0; p < 3; ++p) {
        float acc = 0.0f;
#pragma unroll
        for (int j = 0; j < DV3_TRUE_PEAK_TAPS; ++j)       // tap j multiplies x[m + 6 - j]
          acc = fmaf(tab.t[p * DV3_TRUE_PEAK_TAPS + j], s_x[q + kHaloLo + 6 - j], acc);
        m = fmaxf(m, fabsf(acc));
      }
    }
  }
  s_m[tid] = m;
  for (int st = kPeakThreads / 2; st > 0; st >>= 1) {
    __syncthreads();
    if (tid < st) s_m[tid] = fmaxf(s_m[tid], s_m[tid + st]);
  }
  if (tid == 0) part[(int64_t)b * nchunk + cidx] = (double)s_m[0];
}

__global__ __launch_bounds__(64) void true_peak_final_kernel(const int64_t* __restrict__ lengths, int64_t max_len, int B,
                                                             int nchunk, const double* __restrict__ part,
                                                             double* __restrict__ peak) {
  const int b = blockIdx.x * 64 + threadIdx.x;
  if (b >= B) return;
  const int64_t n = min(max(lengths[b], (int64_t)0), max_len);
  const int nc = (int)((n + DV3_TRUE_PEAK_CHUNK - 1) / DV3_TRUE_PEAK_CHUNK);
  double m = 0.0;
  for (int cidx = 0; cidx < nc; ++cidx) m = fmax(m, part[(int64_t)b * nchunk + cidx]);
  peak[b] = m;
}

// ---- the gate ---------------------------------------------------------------------------------------------------------
__device__ __forceinline__ double wave_sum_f64(double v) {   // a fixed butterfly: every lane ends with the same bits
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v = v + __shfl_xor(v, off, 64);
  return v;
}
__device__ __forceinline__ double wave_max_f64(double v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v = fmax(v, __shfl_xor(v, off, 64));
  return v;
}
__device__ __forceinline__ double lkfs(double z) {
#pragma clang fp contract(off)
  return -0.691 + 10.0 * log10(z);
}

__global__ __launch_bounds__(64) void loudness_gate_kernel(const double* __restrict__ energy,
                                                           const int64_t* __restrict__ lengths,
                                                           const int32_t* __restrict__ goff, const double* __restrict__ peak,
                                                           int peak_stride, int B, int K, int64_t max_len, int h,
                                                           double* __restrict__ rows) {
#pragma clang fp contract(off)
  const int g = blockIdx.x, lane = threadIdx.x;
  const int b0 = min(max(goff[g], 0), B), b1 = min(max(goff[g + 1], b0), B);
  const double inv = 1.0 / (4.0 * (double)h);
  const double ninf = -(double)INFINITY;
  double P = 0.0, nblk = 0.0, nsamp = 0.0;
  // pass A: the absolute gate, the momentary maximum, and the ungated energy for the short-group rule
  double za = 0.0, ca = 0.0, mx = ninf, eall = 0.0;
  for (int b = b0; b < b1; ++b) {
    const int64_t n = min(max(lengths[b], (int64_t)0), max_len);
    const int J = n >= 4 * (int64_t)h ? (int)((n - 4 * (int64_t)h) / h) + 1 : 0;
    const int nk = (int)((n + h - 1) / h);
    const double* __restrict__ E = energy + (int64_t)b * K;
    P = fmax(P, peak[(int64_t)b * peak_stride]);
    nblk += (double)J;
    nsamp += (double)n;
    for (int j = lane; j < J; j += 64) {
      const double z = (((E[j] + E[j + 1]) + E[j + 2]) + E[j + 3]) * inv;
      const double l = lkfs(z);
      mx = fmax(mx, l);
      if (l > -70.0) { za += z; ca += 1.0; }
    }
    for (int k = lane; k < nk; k += 64) eall += E[k];
  }
  za = wave_sum_f64(za); ca = wave_sum_f64(ca); mx = wave_max_f64(mx); eall = wave_sum_f64(eall);
  double L, cr = 0.0;
  int flags = 0;
  if (nblk == 0.0) {                                       // no complete block: measured ungated
    flags |= DV3_LOUDNESS_SHORT;
    L = (nsamp > 0.0 && eall > 0.0) ? lkfs(eall / nsamp) : ninf;
  } else if (ca == 0.0) {
    L = ninf;
  } else {
    const double gamma = lkfs(za / ca) - 10.0;
    double zr = 0.0;
    for (int b = b0; b < b1; ++b) {
      const int64_t n = min(max(lengths[b], (int64_t)0), max_len);
      const int J = n >= 4 * (int64_t)h ? (int)((n - 4 * (int64_t)h) / h) + 1 : 0;
      const double* __restrict__ E = energy + (int64_t)b * K;
      for (int j = lane; j < J; j += 64) {
        const double z = (((E[j] + E[j + 1]) + E[j + 2]) + E[j + 3]) * inv;
        const double l = lkfs(z);
        if (l > -70.0 && l > gamma) { zr += z; cr += 1.0; }
      }
    }
    zr = wave_sum_f64(zr); cr = wave_sum_f64(cr);
    L = cr > 0.0 ? lkfs(zr / cr) : ninf;
  }
  if (!(L > ninf)) flags |= DV3_LOUDNESS_SILENT;
  if (lane < DV3_LOUDNESS_COLUMNS) {
    const double row[DV3_LOUDNESS_COLUMNS] = {L, nblk, ca, cr, mx, P, (double)flags};
    double v = row[0];
#pragma unroll
    for (int q = 1; q < DV3_LOUDNESS_COLUMNS; ++q) v = lane == q ? row[q] : v;
    rows[(int64_t)g * DV3_LOUDNESS_COLUMNS + lane] = v;
  }
}

// ---- gains ------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(64) void loudness_gains_kernel(const double* __restrict__ rows, const int32_t* __restrict__ goff,
                                                            int B, int G, double target, double ceiling, double max_gain,
                                                            float* __restrict__ gain) {
#pragma clang fp contract(off)
  const int g = blockIdx.x * 64 + threadIdx.x;
  if (g >= G) return;
  const int b0 = min(max(goff[g], 0), B), b1 = min(max(goff[g + 1], b0), B);
  const double* row = rows + (int64_t)g * DV3_LOUDNESS_COLUMNS;
  const double L = row[0], P = row[5];
  double q = 1.0;
  if (!((int)row[6] & DV3_LOUDNESS_SILENT)) {
    q = pow(10.0, (target - L) / 20.0);
    if (P > 0.0) q = fmin(q, ceiling / P);
    q = fmin(q, max_gain);
  }
  const float v = (float)q;
  for (int b = b0; b < b1; ++b) gain[b] = v;
}

bool finite_all(const double* v, int n) {
  for (int i = 0; i < n; ++i)
    if (!(v[i] > -(double)INFINITY && v[i] < (double)INFINITY)) return false;
  return true;
}

}  // namespace

extern "C" int dv3_wave_loudness_f64(const float* x, const int64_t* starts, const int64_t* lengths, int32_t B,
                                     int64_t max_len, int32_t h, const double* coef, const double* Ah,
                                     const float* peak_table, double* states, double* energy, double* peak_scratch,
                                     double* true_peak, void* stream) {
  DV3_REQUIRE(x, "wave_loudness: x is null");
  DV3_REQUIRE(starts, "wave_loudness: starts is null");
  DV3_REQUIRE(lengths, "wave_loudness: lengths is null");
  DV3_REQUIRE(coef && Ah, "wave_loudness: coef or Ah is null");
  DV3_REQUIRE(B >= 1 && B <= 65535, "wave_loudness: B = %d outside [1, 65535]", (int)B);
  DV3_REQUIRE(max_len >= 0 && max_len <= kMaxLen, "wave_loudness: max_len = %lld outside [0, 2^30]", (long long)max_len);
  DV3_REQUIRE(h >= DV3_LOUDNESS_MIN_STEP && h <= DV3_LOUDNESS_MAX_STEP, "wave_loudness: h = %d outside [%d, %d]", (int)h,
              DV3_LOUDNESS_MIN_STEP, DV3_LOUDNESS_MAX_STEP);
  DV3_REQUIRE(finite_all(coef, 10) && finite_all(Ah, 16), "wave_loudness: a coefficient or an entry of Ah is not finite");
  DV3_REQUIRE((states && energy) || max_len == 0, "wave_loudness: states or energy is null with max_len = %lld",
              (long long)max_len);
  DV3_REQUIRE((peak_table == nullptr) == (true_peak == nullptr),
              "wave_loudness: peak_table and true_peak come together (both null: no true peak)");
  DV3_REQUIRE(!peak_table || peak_scratch || max_len == 0, "wave_loudness: peak_scratch is null with max_len = %lld",
              (long long)max_len);
  DV3_REQUIRE(((uintptr_t)states & 15) == 0 && ((uintptr_t)energy & 7) == 0 && ((uintptr_t)peak_scratch & 7) == 0 &&
                  ((uintptr_t)true_peak & 7) == 0 && ((uintptr_t)x & 3) == 0,
              "wave_loudness: states is not 16-byte aligned, energy, peak_scratch or true_peak not 8-byte, or x not 4-byte");
  if (peak_table)
    for (int i = 0; i < 3 * DV3_TRUE_PEAK_TAPS; ++i)
      DV3_REQUIRE(peak_table[i] > -INFINITY && peak_table[i] < INFINITY, "wave_loudness: peak_table[%d] is not finite", i);
  hipStream_t s = (hipStream_t)stream;
  const int K = (int)dv3_cdiv64(max_len, h);
  if (K > 0) {
    KCoef c;
    for (int i = 0; i < 5; ++i) { c.s[i] = coef[i]; c.p[i] = coef[5 + i]; }
    for (int i = 0; i < 16; ++i) c.Ah[i] = Ah[i];
    const dim3 grid(dv3_cdiv(K, kLanes), B);
    hipLaunchKernelGGL(kweight_chunk_kernel<false>, grid, dim3(kLanes), 0, s, x, starts, lengths, max_len, (int)h, K, c,
                       states, energy);
    int rc = dv3_check_launch("wave_loudness (pass 1)");
    if (rc != DV3_OK) return rc;
    hipLaunchKernelGGL(kweight_walk_kernel, dim3(dv3_cdiv(B, 64)), dim3(64), 0, s, lengths, max_len, (int)h, (int)B, K, c,
                       states);
    rc = dv3_check_launch("wave_loudness (pass 2)");
    if (rc != DV3_OK) return rc;
    hipLaunchKernelGGL(kweight_chunk_kernel<true>, grid, dim3(kLanes), 0, s, x, starts, lengths, max_len, (int)h, K, c,
                       states, energy);
    rc = dv3_check_launch("wave_loudness (pass 3)");
    if (rc != DV3_OK) return rc;
  }
  if (peak_table) {
    PeakTable tab;
    for (int i = 0; i < 3 * DV3_TRUE_PEAK_TAPS; ++i) tab.t[i] = peak_table[i];
    const int nchunk = (int)dv3_cdiv64(max_len, DV3_TRUE_PEAK_CHUNK);
    if (nchunk > 0) {
      hipLaunchKernelGGL(true_peak_chunk_kernel, dim3(nchunk, B), dim3(kPeakThreads), 0, s, x, starts, lengths, max_len,
                         nchunk, tab, peak_scratch);
      const int rc = dv3_check_launch("wave_loudness (true peak)");
      if (rc != DV3_OK) return rc;
    }
    hipLaunchKernelGGL(true_peak_final_kernel, dim3(dv3_cdiv(B, 64)), dim3(64), 0, s, lengths, max_len, (int)B, nchunk,
                       peak_scratch, true_peak);
    return dv3_check_launch("wave_loudness (true peak, items)");
  }
  return DV3_OK;
}

extern "C" int dv3_loudness_gate_f64(const double* energy, const int64_t* lengths, const int32_t* goff, const double* peak,
                                     int32_t peak_stride, int32_t B, int32_t G, int64_t max_len, int32_t h, double* rows,
                                     void* stream) {
  DV3_REQUIRE(lengths, "loudness_gate: lengths is null");
  DV3_REQUIRE(goff, "loudness_gate: goff is null");
  DV3_REQUIRE(peak, "loudness_gate: peak is null");
  DV3_REQUIRE(rows, "loudness_gate: rows is null");
  DV3_REQUIRE(B >= 1 && B <= 65535, "loudness_gate: B = %d outside [1, 65535]", (int)B);
  DV3_REQUIRE(G >= 1 && G <= B, "loudness_gate: G = %d outside [1, B = %d]", (int)G, (int)B);
  DV3_REQUIRE(max_len >= 0 && max_len <= kMaxLen, "loudness_gate: max_len = %lld outside [0, 2^30]", (long long)max_len);
  DV3_REQUIRE(h >= DV3_LOUDNESS_MIN_STEP && h <= DV3_LOUDNESS_MAX_STEP, "loudness_gate: h = %d outside [%d, %d]", (int)h,
              DV3_LOUDNESS_MIN_STEP, DV3_LOUDNESS_MAX_STEP);
  DV3_REQUIRE(peak_stride >= 1 && peak_stride <= 64, "loudness_gate: peak_stride = %d outside [1, 64]", (int)peak_stride);
  DV3_REQUIRE(energy || max_len == 0, "loudness_gate: energy is null with max_len = %lld", (long long)max_len);
  DV3_REQUIRE(((uintptr_t)energy & 7) == 0 && ((uintptr_t)peak & 7) == 0 && ((uintptr_t)rows & 7) == 0,
              "loudness_gate: energy, peak or rows is not 8-byte aligned");
  hipLaunchKernelGGL(loudness_gate_kernel, dim3(G), dim3(64), 0, (hipStream_t)stream, energy, lengths, goff, peak,
                     (int)peak_stride, (int)B, (int)dv3_cdiv64(max_len, h), max_len, (int)h, rows);
  return dv3_check_launch("loudness_gate");
}

extern "C" int dv3_loudness_gains_f32(const double* rows, const int32_t* goff, int32_t B, int32_t G, double target_lufs,
                                      double ceiling, double max_gain, float* gain, void* stream) {
  DV3_REQUIRE(rows, "loudness_gains: rows is null");
  DV3_REQUIRE(goff, "loudness_gains: goff is null");
  DV3_REQUIRE(gain, "loudness_gains: gain is null");
  DV3_REQUIRE(B >= 1 && B <= 65535, "loudness_gains: B = %d outside [1, 65535]", (int)B);
  DV3_REQUIRE(G >= 1 && G <= B, "loudness_gains: G = %d outside [1, B = %d]", (int)G, (int)B);
  DV3_REQUIRE(target_lufs >= -120.0 && target_lufs <= 0.0, "loudness_gains: target_lufs = %g outside [-120, 0]", target_lufs);
  const bool ok = ceiling > 0.0 && ceiling < (double)INFINITY && max_gain > 0.0 && max_gain < (double)INFINITY;
  DV3_REQUIRE(ok, "loudness_gains: ceiling = %g, max_gain = %g must be positive finite linear values", ceiling, max_gain);
  DV3_REQUIRE(((uintptr_t)rows & 7) == 0, "loudness_gains: rows is not 8-byte aligned");
  hipLaunchKernelGGL(loudness_gains_kernel, dim3(dv3_cdiv(G, 64)), dim3(64), 0, (hipStream_t)stream, rows, goff, (int)B,
                     (int)G, target_lufs, ceiling, max_gain, gain);
  return dv3_check_launch("loudness_gains");
}

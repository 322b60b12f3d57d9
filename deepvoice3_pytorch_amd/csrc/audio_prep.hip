// Waveform preparation for multi-speaker corpora (ABI 46, include/dv3hip.h: dv3_resample_items_f32,
// dv3_trim_items_f32, dv3_gather_spans_f32): what the reference's VCTK preprocessing does on the host before it makes
// features -- librosa.load(sr=...) (audio.py:12-13) and librosa.effects.trim (vctk.py:52-67) -- for B utterances of
// different lengths packed back to back, one launch each.  Every output value is a function of its own item only.
#include "common.h"

// ---- rational-ratio band-limited resampling -------------------------------------------------------------------------
// y[n] = sum_k x[k] h(n down / up - k), k = i0 - H .. i0 + H + 1, i0 = (n down) div up; the coefficient depends on
// r = n mod up and on the tap j = k - (i0 - H) only, and the table holds it as tab[j][r] (fp32), so consecutive lanes
// read consecutive coefficients.  A workgroup of 320 lanes owns RS_P * S consecutive outputs of one item, S the largest
// multiple of `up` within 320 (two periods of 147, one of 160; 320 itself when up > 320), and stages the input samples
// they read, zeros outside [0, L), in LDS once.  Lane t makes the outputs n0 + t + q S, q = 0 .. RS_P - 1: with S a
// multiple of `up` they share r, so each coefficient is loaded once for RS_P fused multiply-adds.  Each output is ONE
// fmaf chain from 0 over the taps in ascending order of k.
#define RS_P 4
#define RS_THREADS 320
template <bool SHARED>
__global__ __launch_bounds__(RS_THREADS) void resample_items_kernel(
    const float* __restrict__ x, const int64_t* __restrict__ ioff, const int64_t* __restrict__ ooff,
    const int32_t* __restrict__ toff, int B, int up, int down, int H, int S, const float* __restrict__ tab,
    float* __restrict__ y) {
  extern __shared__ float win[];
  const int tid = threadIdx.x;
  const int g = blockIdx.x;
  int lo = 0, hi = B;                                 // the item: largest b with toff[b] <= g
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if (toff[mid] <= g) lo = mid; else hi = mid;
  }
  const int b = lo;
  const float* xb = x + ioff[b];
  float* yb = y + ooff[b];
  const int64_t L = ioff[b + 1] - ioff[b], Lo = ooff[b + 1] - ooff[b];
  const int64_t n0 = (int64_t)(g - toff[b]) * (RS_P * S);
  const int64_t nl = min(n0 + (int64_t)RS_P * S, Lo) - 1;            // the tile's last output (n0 <= nl: toff counts tiles)
  const int64_t w0 = (n0 * down) / up - H;                           // first sample the tile reads
  const int W = (int)((nl * down) / up + H + 1 - w0) + 1;
  for (int i = tid; i < W; i += RS_THREADS) {
    const int64_t k = w0 + i;
    win[i] = (k >= 0 && k < L) ? xb[k] : 0.f;
  }
  __syncthreads();
  if (tid >= S) return;
  const int T = 2 * H + 2;
  int base[RS_P], r[RS_P];
  float acc[RS_P];
#pragma unroll
  for (int q = 0; q < RS_P; ++q) {
    const int64_t n = min(n0 + tid + (int64_t)q * S, nl);            // a lane past the end recomputes the last output
    const int64_t num = n * down;
    base[q] = (int)(num / up - H - w0);
    r[q] = (int)(n % up);
    acc[q] = 0.f;
  }
  if constexpr (SHARED) {
    const float* c = tab + r[0];
    for (int j = 0; j < T; ++j) {
      const float h = c[(int64_t)j * up];
#pragma unroll
      for (int q = 0; q < RS_P; ++q) acc[q] = __builtin_fmaf(h, win[base[q] + j], acc[q]);
    }
  } else {
    for (int j = 0; j < T; ++j) {
#pragma unroll
      for (int q = 0; q < RS_P; ++q) acc[q] = __builtin_fmaf(tab[(int64_t)j * up + r[q]], win[base[q] + j], acc[q]);
    }
  }
#pragma unroll
  for (int q = 0; q < RS_P; ++q) {
    const int64_t n = n0 + tid + (int64_t)q * S;
    if (n <= nl) yb[n] = acc[q];
  }
}

static int rs_half_width(int up, int down) {                         // H = ceil(Z / s), s = min(1, up / down), Z = 64
  return up >= down ? 64 : (int)dv3_cdiv64((int64_t)64 * down, up);
}
static int rs_stride(int up) { return up <= RS_THREADS ? up * (RS_THREADS / up) : RS_THREADS; }
static int64_t rs_window(int up, int down) {                         // most samples a tile stages
  return dv3_cdiv64((int64_t)RS_P * rs_stride(up) * down, up) + 2 * rs_half_width(up, down) + 3;
}

extern "C" int dv3_resample_tile(int32_t up, int32_t down) {
  if (up < 1 || down < 1 || up > 4096 || down > 4096 || rs_window(up, down) * 4 > 65536) return DV3_EINVAL;
  return RS_P * rs_stride(up);
}

extern "C" int dv3_resample_items_f32(const float* x, const int64_t* ioff, const int64_t* ooff, const int32_t* toff,
                                      int32_t B, int32_t n_tiles, int32_t up, int32_t down, const float* table, float* y,
                                      void* stream) {
  DV3_REQUIRE(x && ioff && ooff && toff && table && y && B > 0 && n_tiles > 0 && up >= 1 && down >= 1 && up <= 4096 &&
              down <= 4096 && up != down, "resample_items: bad arguments");
  const int64_t W = rs_window(up, down);
  DV3_REQUIRE(W * 4 <= 65536, "resample_items: the ratio %d / %d needs a %lld-sample window per tile (at most 16384)",
              up, down, (long long)W);
  const int H = rs_half_width(up, down), S = rs_stride(up);
  if (S % up == 0)
    hipLaunchKernelGGL(resample_items_kernel<true>, dim3(n_tiles), dim3(RS_THREADS), (size_t)W * 4, (hipStream_t)stream, x, ioff,
                       ooff, toff, B, up, down, H, S, table, y);
  else
    hipLaunchKernelGGL(resample_items_kernel<false>, dim3(n_tiles), dim3(RS_THREADS), (size_t)W * 4, (hipStream_t)stream, x, ioff,
                       ooff, toff, B, up, down, H, S, table, y);
  return dv3_check_launch("resample_items");
}

// ---- silence trimming: librosa.effects.trim(y, top_db) with frame_length 2048, hop_length 512 -----------------------
#define TRIM_FRAME 2048
#define TRIM_HOP 512
// One workgroup per frame g of the packed frame list: frame f = g - foff[b] of span b covers span samples
// [512 f - 1024, 512 f + 1024), reflected about sample 0 and sample len - 1 (numpy.pad mode "reflect"; len >= 1025, so
// one reflection suffices).  Lane t sums the squares of samples t, t + 256, ... in that order, the 256 partial sums are
// added in a fixed tree, and the total is divided by 2048: the value does not depend on B or on the grid.
__global__ __launch_bounds__(256) void trim_power_kernel(const float* __restrict__ x, const int64_t* __restrict__ start,
                                                         const int64_t* __restrict__ len, const int32_t* __restrict__ foff,
                                                         int B, float* __restrict__ mse) {
  __shared__ float red[256];
  const int tid = threadIdx.x;
  const int g = blockIdx.x;
  int lo = 0, hi = B;
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if (foff[mid] <= g) lo = mid; else hi = mid;
  }
  const int b = lo;
  const int64_t n = len[b];
  const float* xb = x + start[b];
  const int64_t i0 = (int64_t)(g - foff[b]) * TRIM_HOP - TRIM_FRAME / 2;
  float s = 0.f;
#pragma unroll
  for (int m = 0; m < TRIM_FRAME / 256; ++m) {
    int64_t i = i0 + tid + 256 * m;
    i = i < 0 ? -i : i;
    i = i >= n ? 2 * (n - 1) - i : i;
    i = min(max(i, (int64_t)0), n - 1);               // never taken for len >= 1025 and f <= len div 512: keeps a
    const float v = xb[i];                            // caller's wrong frame table inside the span
    s = __builtin_fmaf(v, v, s);
  }
  red[tid] = s;
  for (int st = 128; st > 0; st >>= 1) {
    __syncthreads();
    if (tid < st) red[tid] = red[tid] + red[tid + st];
  }
  if (tid == 0) mse[g] = red[0] * (1.0f / TRIM_FRAME);
}

// One workgroup per span: the largest frame power (fmaxf is exact), then the first and the last frame whose level
// 10 log10(max(1e-10, mse)) - 10 log10(max(1e-10, max mse)) exceeds -top_db[b].
__global__ __launch_bounds__(256) void trim_select_kernel(const float* __restrict__ mse, const int32_t* __restrict__ foff,
                                                          const int64_t* __restrict__ start, const int64_t* __restrict__ len,
                                                          const float* __restrict__ top_db, int64_t* __restrict__ ostart,
                                                          int64_t* __restrict__ olen) {
  __shared__ float red[256];
  __shared__ int rlo[256], rhi[256];
  const int tid = threadIdx.x;
  const int b = blockIdx.x;
  const int f0 = foff[b], nf = foff[b + 1] - f0;
  const int64_t s0 = start[b], n = len[b];
  if (nf <= 0) {                                      // a span too short to reflect-pad (< 1025 samples): unchanged
    if (tid == 0) {
      ostart[b] = s0;
      olen[b] = n;
    }
    return;
  }
  float m = 0.f;
  for (int f = tid; f < nf; f += 256) m = fmaxf(m, mse[f0 + f]);
  red[tid] = m;
  for (int st = 128; st > 0; st >>= 1) {
    __syncthreads();
    if (tid < st) red[tid] = fmaxf(red[tid], red[tid + st]);
  }
  __syncthreads();
  const float ref = 10.0f * log10f(fmaxf(1e-10f, red[0]));
  const float thr = -top_db[b];
  int first = nf, last = -1;
  for (int f = tid; f < nf; f += 256) {
    const float db = 10.0f * log10f(fmaxf(1e-10f, mse[f0 + f])) - ref;
    if (db > thr) {
      first = min(first, f);
      last = max(last, f);
    }
  }
  rlo[tid] = first;
  rhi[tid] = last;
  for (int st = 128; st > 0; st >>= 1) {
    __syncthreads();
    if (tid < st) {
      rlo[tid] = min(rlo[tid], rlo[tid + st]);
      rhi[tid] = max(rhi[tid], rhi[tid + st]);
    }
  }
  if (tid == 0) {
    if (rhi[0] < 0) {
      ostart[b] = s0;
      olen[b] = 0;
    } else {
      const int64_t lo_s = (int64_t)rlo[0] * TRIM_HOP;
      const int64_t hi_s = min(n, ((int64_t)rhi[0] + 1) * TRIM_HOP);
      ostart[b] = s0 + lo_s;
      olen[b] = hi_s - lo_s;
    }
  }
}

extern "C" int dv3_trim_items_f32(const float* x, const int64_t* start, const int64_t* len, const int32_t* foff, int32_t B,
                                  int32_t n_frames, const float* top_db, float* mse, int64_t* out_start, int64_t* out_len,
                                  void* stream) {
  DV3_REQUIRE(x && start && len && foff && top_db && out_start && out_len && B > 0 && n_frames >= 0 &&
              (n_frames == 0 || mse), "trim_items: bad arguments");
  if (n_frames > 0) {
    hipLaunchKernelGGL(trim_power_kernel, dim3(n_frames), dim3(256), 0, (hipStream_t)stream, x, start, len, foff, B, mse);
    const int rc = dv3_check_launch("trim_items (frame powers)");
    if (rc != DV3_OK) return rc;
  }
  hipLaunchKernelGGL(trim_select_kernel, dim3(B), dim3(256), 0, (hipStream_t)stream, mse, foff, start, len, top_db,
                     out_start, out_len);
  return dv3_check_launch("trim_items");
}

// ---- spans of a flat buffer copied back to back ----------------------------------------------------------------------
// Span b = x[start[b] .. start[b] + len[b]) goes to y[ooff[b] ..).  Per span: a head of up to 3 floats until the
// destination is 16-byte aligned, a body of 16-byte stores (fed by 16-byte loads where the source is aligned at the
// same point, by four 4-byte loads otherwise), a tail of up to 3 floats.  blockIdx.y = span, blockIdx.x = a chunk of
// GATHER_CH body quads; chunk 0 also copies head and tail.
#define GATHER_CH 1024
__global__ __launch_bounds__(256) void gather_spans_kernel(const float* __restrict__ x, const int64_t* __restrict__ start,
                                                           const int64_t* __restrict__ len,
                                                           const int64_t* __restrict__ ooff, float* __restrict__ y) {
  const int b = blockIdx.y, tid = threadIdx.x;
  const int64_t n = len[b];
  if (n <= 0) return;
  const float* src = x + start[b];
  float* dst = y + ooff[b];
  const int64_t head = min(n, (int64_t)((4 - (((uintptr_t)dst >> 2) & 3)) & 3));
  const int64_t nq = (n - head) >> 2;
  const int64_t q0 = (int64_t)blockIdx.x * GATHER_CH;
  if (q0 > 0 && q0 >= nq) return;
  if (blockIdx.x == 0) {
    if (tid < head) dst[tid] = src[tid];
    const int64_t t0 = head + 4 * nq;
    if (t0 + tid < n && tid < 3) dst[t0 + tid] = src[t0 + tid];
  }
  const float* sb = src + head;
  f32x4* db = reinterpret_cast<f32x4*>(dst + head);
  const bool aligned = (((uintptr_t)sb) & 15) == 0;
  const int64_t q1 = min(nq, q0 + GATHER_CH);
  for (int64_t q = q0 + tid; q < q1; q += 256) {
    f32x4 v;
    if (aligned) {
      v = *reinterpret_cast<const f32x4*>(sb + 4 * q);
    } else {
      v = f32x4{sb[4 * q], sb[4 * q + 1], sb[4 * q + 2], sb[4 * q + 3]};
    }
    db[q] = v;
  }
}

extern "C" int dv3_gather_spans_f32(const float* x, const int64_t* start, const int64_t* len, const int64_t* ooff,
                                    int32_t B, int64_t max_len, float* y, void* stream) {
  DV3_REQUIRE(x && start && len && ooff && y && B > 0 && B <= 65535 && max_len >= 0 && x != y,
              "gather_spans: bad arguments");
  if (max_len == 0) return DV3_OK;
  const int64_t chunks = dv3_cdiv64(dv3_cdiv64(max_len, 4), GATHER_CH);
  DV3_REQUIRE(chunks < ((int64_t)1 << 31), "gather_spans: span too long");
  hipLaunchKernelGGL(gather_spans_kernel, dim3((unsigned)chunks, B), dim3(256), 0, (hipStream_t)stream, x, start, len, ooff,
                     y);
  return dv3_check_launch("gather_spans");
}

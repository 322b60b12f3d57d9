// Batched dynamic time warping of two feature sequences (include/dv3hip.h: dv3_dtw_f32).
//
//   distance pass   64 x 64 cells per 256-thread workgroup, 4 x 4 cells per thread.  The two frame tiles are staged in LDS
//                   kDK features at a time (rows padded by one word: the 16 column readers of a wave fall on 16 banks, the
//                   4 row readers broadcast), the squared differences summed in feature order in fp32, the root taken
//                   correctly rounded.  d goes to scratch as (B, Tx, Ty) fp32, only inside each item's lengths; frames
//                   at or past a length are never loaded.  A non-finite distance is stored as NaN.
//   scan pass       one 64-lane wave per item.  Lane l owns the W = ceil(Ty / 64) columns l * W ... and works on row
//                   t - l at step t, so the cell left of its strip was finished by lane l - 1 one step earlier and comes
//                   over by a cross-lane move; the row above stays in registers (the strip width is a template
//                   parameter for that).  No barrier, no LDS.  Each cell carries its path's number of diagonal moves;
//                   the two other counts follow from the cell's position.  The next row's distances are loaded one
//                   step ahead.  With a path wanted, the chosen predecessor of every cell goes to scratch as one byte.
//   backtrack       one workgroup per item: lane 0 walks the bytes back from the end cell and stores each step at its
//                   final index (the length is known from the scan), all lanes fill the tail with -1.
// No atomics anywhere; every sum has one order: two calls agree bit for bit.
#include "common.h"

namespace {

constexpr int kTile = 64;     // cells per tile side
constexpr int kDK = 32;       // features staged per trip

__device__ __forceinline__ int clamp_len(int v, int hi) { return v < 0 ? 0 : (v > hi ? hi : v); }

__global__ __launch_bounds__(256) void dtw_dist_kernel(const float* __restrict__ x, int64_t x_bs, int64_t x_ts,
                                                       const float* __restrict__ y, int64_t y_bs, int64_t y_ts, int Tx,
                                                       int Ty, int D, int tiles_i, int tiles_j,
                                                       const int32_t* __restrict__ x_len,
                                                       const int32_t* __restrict__ y_len, float* __restrict__ d) {
  __shared__ float xs[kTile][kDK + 1];
  __shared__ float ys[kTile][kDK + 1];
  const int per_item = tiles_i * tiles_j;
  const int b = (int)blockIdx.x / per_item, rem = (int)blockIdx.x - b * per_item;
  const int i0 = (rem / tiles_j) * kTile, j0 = (rem % tiles_j) * kTile;
  const int Lx = clamp_len(x_len[b], Tx), Ly = clamp_len(y_len[b], Ty);
  if (i0 >= Lx || j0 >= Ly) return;                       // workgroup-uniform
  const int tid = threadIdx.x, tx = tid & 15, ty = tid >> 4;
  const float* __restrict__ xb = x + (int64_t)b * x_bs;
  const float* __restrict__ yb = y + (int64_t)b * y_bs;
  float acc[4][4];
#pragma unroll
  for (int r = 0; r < 4; ++r)
#pragma unroll
    for (int q = 0; q < 4; ++q) acc[r][q] = 0.f;
  for (int k0 = 0; k0 < D; k0 += kDK) {
#pragma unroll
    for (int e = 0; e < kTile * kDK / 256; ++e) {
      const int idx = tid + 256 * e, r = idx / kDK, k = idx % kDK;
      const bool kin = k0 + k < D;
      xs[r][k] = (kin && i0 + r < Lx) ? xb[(int64_t)(i0 + r) * x_ts + k0 + k] : 0.f;
      ys[r][k] = (kin && j0 + r < Ly) ? yb[(int64_t)(j0 + r) * y_ts + k0 + k] : 0.f;
    }
    __syncthreads();
#pragma unroll 8
    for (int k = 0; k < kDK; ++k) {
      float xv[4], yv[4];
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        xv[r] = xs[ty + 16 * r][k];
        yv[r] = ys[tx + 16 * r][k];
      }
#pragma unroll
      for (int r = 0; r < 4; ++r)
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          const float diff = xv[r] - yv[q];
          acc[r][q] = fmaf(diff, diff, acc[r][q]);
        }
    }
    __syncthreads();
  }
  float* __restrict__ db = d + (int64_t)b * Tx * Ty;
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int i = i0 + ty + 16 * r;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int j = j0 + tx + 16 * q;
      if (i < Lx && j < Ly) {
        float s = __fsqrt_rn(acc[r][q]);
        if (!(s < INFINITY)) s = __builtin_nanf("");
        db[(int64_t)i * Ty + j] = s;
      }
    }
  }
}

// predecessor codes of the direction bytes: 0 diagonal, 1 x advanced (from (i - 1, j)), 2 y advanced (from (i, j - 1))
template <int WT>
__global__ __launch_bounds__(64) void dtw_scan_kernel(const float* __restrict__ d, uint8_t* __restrict__ dirs, int Tx,
                                                      int Ty, int W, const int32_t* __restrict__ x_len,
                                                      const int32_t* __restrict__ y_len, float* __restrict__ out) {
  const int b = blockIdx.x, lane = threadIdx.x;
  const int Lx = clamp_len(x_len[b], Tx), Ly = clamp_len(y_len[b], Ty);
  float* __restrict__ ob = out + (int64_t)b * DV3_DTW_COLS;
  if (Lx == 0 || Ly == 0) {
    if (lane < DV3_DTW_COLS) ob[lane] = 0.f;
    return;
  }
  const float* __restrict__ db = d + (int64_t)b * Tx * Ty;
  uint8_t* __restrict__ qb = dirs ? dirs + (int64_t)b * Tx * Ty : nullptr;
  const int j0 = lane * W;
  float pC[WT], dn[WT];       // the row above (cost, diagonal moves) and the next row's distances
  int pN[WT];
#pragma unroll
  for (int c = 0; c < WT; ++c) {
    pC[c] = 0.f;
    pN[c] = 0;
    dn[c] = 0.f;
  }
  if (lane == 0) {
#pragma unroll
    for (int c = 0; c < WT; ++c) {
      if (c < W && c < Ly) dn[c] = db[c];
    }
  }
  float lastC = 0.f, dgC0 = 0.f;          // my strip's last cell of the step before; what came in as `left` then
  int lastN = 0, dgN0 = 0;
  const int steps = Lx + (Ly - 1) / W;    // the lane that owns column Ly - 1 finishes row Lx - 1 in the last one
  for (int t = 0; t < steps; ++t) {
    const int i = t - lane;
    const bool row_ok = i >= 0 && i < Lx;
    const float inC = __shfl_up(lastC, 1, 64);
    const int inN = __shfl_up(lastN, 1, 64);
    float dc[WT];
#pragma unroll
    for (int c = 0; c < WT; ++c) dc[c] = dn[c];
    const bool next_ok = i + 1 >= 0 && i + 1 < Lx;
    const float* __restrict__ nrow = db + (int64_t)(i + 1) * Ty + j0;
#pragma unroll
    for (int c = 0; c < WT; ++c) {
      if (c < W && next_ok && j0 + c < Ly) dn[c] = nrow[c];
    }
    float dgC = dgC0, lfC = inC;
    int dgN = dgN0, lfN = inN;
#pragma unroll
    for (int c = 0; c < WT; ++c) {
      if (c >= W) continue;                // wave-uniform
      const int j = j0 + c;
      const float upC = pC[c];
      const int upN = pN[c];
      float best = dgC;
      int bn = dgN + 1, dir = 0;
      if (upC < best) { best = upC; bn = upN; dir = 1; }
      if (lfC < best) { best = lfC; bn = lfN; dir = 2; }
      if (j == 0) { best = upC; bn = upN; dir = 1; }
      if (i == 0) { best = lfC; bn = lfN; dir = 2; }
      if (i == 0 && j == 0) { best = 0.f; bn = 0; dir = 0; }
      const float v = dc[c] + best;
      if (row_ok && j < Ly) {
        pC[c] = v;
        pN[c] = bn;
        if (qb) qb[(int64_t)i * Ty + j] = (uint8_t)dir;
        if (i == Lx - 1 && j == Ly - 1) {
          ob[0] = (fabsf(v) < INFINITY) ? v : __builtin_nanf("");
          ob[1] = (float)(Lx + Ly - 1 - bn);
          ob[2] = (float)bn;
          ob[3] = (float)(Lx - 1 - bn);
          ob[4] = (float)(Ly - 1 - bn);
        }
      }
      dgC = upC; dgN = upN;
      lfC = v; lfN = bn;
    }
    dgC0 = inC; dgN0 = inN;
    lastC = lfC; lastN = lfN;
  }
}

__global__ __launch_bounds__(64) void dtw_backtrack_kernel(const uint8_t* __restrict__ dirs, int Tx, int Ty,
                                                           const int32_t* __restrict__ x_len,
                                                           const int32_t* __restrict__ y_len,
                                                           const float* __restrict__ out, int32_t* __restrict__ path) {
  const int b = blockIdx.x, lane = threadIdx.x;
  const int Lx = clamp_len(x_len[b], Tx), Ly = clamp_len(y_len[b], Ty);
  const int P = Tx + Ty - 1;
  int32_t* __restrict__ pb = path + (int64_t)b * P * 2;
  int n = 0;
  if (Lx > 0 && Ly > 0) n = clamp_len((int)out[(int64_t)b * DV3_DTW_COLS + 1], P);
  for (int s = n + lane; s < P; s += 64) {
    pb[2 * s] = -1;
    pb[2 * s + 1] = -1;
  }
  if (lane != 0 || n == 0) return;
  const uint8_t* __restrict__ qb = dirs + (int64_t)b * Tx * Ty;
  int i = Lx - 1, j = Ly - 1, s = n - 1;
  for (; s >= 0 && i >= 0 && j >= 0; --s) {
    pb[2 * s] = i;
    pb[2 * s + 1] = j;
    const int dir = qb[(int64_t)i * Ty + j];
    i -= dir != 2;
    j -= dir != 1;
  }
  for (; s >= 0; --s) {         // unreachable while the bytes and the length come from one scan; leaves no row unwritten
    pb[2 * s] = -1;
    pb[2 * s + 1] = -1;
  }
}

inline int64_t dist_bytes(int64_t B, int64_t Tx, int64_t Ty) { return B * Tx * Ty * 4; }

template <int WT>
void launch_scan(int B, hipStream_t st, const float* d, uint8_t* dirs, int Tx, int Ty, int W, const int32_t* x_len,
                 const int32_t* y_len, float* out) {
  hipLaunchKernelGGL(dtw_scan_kernel<WT>, dim3(B), dim3(64), 0, st, d, dirs, Tx, Ty, W, x_len, y_len, out);
}

}  // namespace

extern "C" int dv3_dtw_scratch_bytes(int32_t B, int32_t Tx, int32_t Ty, int32_t want_path, int64_t* bytes_out) {
  DV3_REQUIRE(bytes_out, "dtw_scratch_bytes: bytes_out is null");
  *bytes_out = 0;
  DV3_REQUIRE(B >= 1, "dtw_scratch_bytes: B = %d < 1", (int)B);
  DV3_REQUIRE(Tx >= 1 && Tx <= DV3_DTW_MAX_T, "dtw_scratch_bytes: Tx = %d outside [1, %d]", (int)Tx, DV3_DTW_MAX_T);
  DV3_REQUIRE(Ty >= 1 && Ty <= DV3_DTW_MAX_T, "dtw_scratch_bytes: Ty = %d outside [1, %d]", (int)Ty, DV3_DTW_MAX_T);
  *bytes_out = dist_bytes(B, Tx, Ty) + (want_path ? (int64_t)B * Tx * Ty : 0);
  return DV3_OK;
}

extern "C" int dv3_dtw_f32(const dv3_dtw_desc* p, void* stream) {
  DV3_REQUIRE(p, "dtw: the descriptor is null");
  const int B = p->B, Tx = p->Tx, Ty = p->Ty, D = p->D;
  DV3_REQUIRE(B >= 1, "dtw: B = %d < 1", B);
  DV3_REQUIRE(Tx >= 1 && Tx <= DV3_DTW_MAX_T, "dtw: Tx = %d outside [1, %d]", Tx, DV3_DTW_MAX_T);
  DV3_REQUIRE(Ty >= 1 && Ty <= DV3_DTW_MAX_T, "dtw: Ty = %d outside [1, %d]", Ty, DV3_DTW_MAX_T);
  DV3_REQUIRE(D >= 1 && D <= DV3_DTW_MAX_D, "dtw: D = %d outside [1, %d]", D, DV3_DTW_MAX_D);
  DV3_REQUIRE(p->x, "dtw: x is null");
  DV3_REQUIRE(p->y, "dtw: y is null");
  DV3_REQUIRE(p->x_len, "dtw: x_len is null");
  DV3_REQUIRE(p->y_len, "dtw: y_len is null");
  DV3_REQUIRE(p->out, "dtw: out is null");
  DV3_REQUIRE(p->scratch, "dtw: scratch is null");
  DV3_REQUIRE(D == 1 || (p->x_feat_stride == 1 && p->y_feat_stride == 1),
              "dtw: the feature axis must be dense (strides %lld, %lld)", (long long)p->x_feat_stride,
              (long long)p->y_feat_stride);
  int64_t need = 0;
  if (dv3_dtw_scratch_bytes(B, Tx, Ty, p->path != nullptr, &need) != DV3_OK) return DV3_EINVAL;
  DV3_REQUIRE(p->scratch_bytes >= need, "dtw: scratch of %lld bytes, B = %d, Tx = %d, Ty = %d%s need %lld",
              (long long)p->scratch_bytes, B, Tx, Ty, p->path ? " with a path" : "", (long long)need);
  DV3_REQUIRE(((uintptr_t)p->scratch & 3) == 0 && ((uintptr_t)p->out & 3) == 0 && ((uintptr_t)p->path & 3) == 0,
              "dtw: out, path and scratch must be 4-byte aligned");
  const int tiles_i = dv3_cdiv(Tx, kTile), tiles_j = dv3_cdiv(Ty, kTile);
  const int64_t blocks = (int64_t)B * tiles_i * tiles_j;
  DV3_REQUIRE(blocks < (1ll << 31), "dtw: B = %d items of %d x %d tiles exceed the grid", B, tiles_i, tiles_j);
  hipStream_t st = (hipStream_t)stream;
  float* d = (float*)p->scratch;
  uint8_t* dirs = p->path ? (uint8_t*)p->scratch + dist_bytes(B, Tx, Ty) : nullptr;
  hipLaunchKernelGGL(dtw_dist_kernel, dim3((unsigned)blocks), dim3(256), 0, st, p->x, p->x_batch_stride,
                     p->x_time_stride, p->y, p->y_batch_stride, p->y_time_stride, Tx, Ty, D, tiles_i, tiles_j, p->x_len,
                     p->y_len, d);
  const int W = dv3_cdiv(Ty, 64);
  if (W <= 4) launch_scan<4>(B, st, d, dirs, Tx, Ty, W, p->x_len, p->y_len, p->out);
  else if (W <= 8) launch_scan<8>(B, st, d, dirs, Tx, Ty, W, p->x_len, p->y_len, p->out);
  else if (W <= 16) launch_scan<16>(B, st, d, dirs, Tx, Ty, W, p->x_len, p->y_len, p->out);
  else if (W <= 32) launch_scan<32>(B, st, d, dirs, Tx, Ty, W, p->x_len, p->y_len, p->out);
  else launch_scan<64>(B, st, d, dirs, Tx, Ty, W, p->x_len, p->y_len, p->out);
  if (p->path)
    hipLaunchKernelGGL(dtw_backtrack_kernel, dim3(B), dim3(64), 0, st, (const uint8_t*)dirs, Tx, Ty, p->x_len, p->y_len,
                       (const float*)p->out, p->path);
  return dv3_check_launch("dtw_f32");
}

// Monotonic alignment search: the best monotonic path through stored attention rows, and the steps it gives every key
// (include/dv3hip.h: dv3_mono_path_f32).
//
//   score pass   grid (slices, B), 4 waves per workgroup, one wave per row (the cut of alignment.hip's rows pass): the L
//                layers of a cell are summed in layer order and divided by L in fp32, floored (a NaN goes to the floor)
//                and put through the full-precision logf.  s goes to scratch as (B, T, Tk) fp32, only inside each
//                item's lengths; nothing outside t < steps[b], n < key_len[b] is read.  This keeps logf and the strided
//                layer reads off the serial axis.
//   scan pass    one 64-lane wave per item.  Key n lives in lane n % 64, register n / 64 (the register count is a
//                template parameter), so a row of s is read and a row of back-pointer bytes is written in coalesced
//                256- and 64-byte pieces.  The predecessor n - j sits j lanes down: one rotating cross-lane move per
//                register and advance, the lanes that wrap taking the register below.  An unreachable cell is -inf
//                (every score is >= T * log(floor), far from it), so feasibility is exact.  The rows of the following PF
//                steps are in flight in a register ring (the step loop is unrolled by PF to keep the ring's indices
//                static).  No barrier, no LDS.  The end cell goes to out and path[T_b - 1].
//   backtrack    one wave per item: the back-pointer rows of up to kWalkRows steps are staged in LDS by all lanes
//                (whole dwords of the item's contiguous byte block), lane 0 walks them back, counting every key's steps
//                in LDS, and all lanes store the path piece, then the durations and the two summary columns.
// No floating-point atomics, and every sum has one order: two calls agree bit for bit.
#include "common.h"

namespace {

constexpr int kRowWaves = 4;                    // rows in flight per workgroup of the score pass
constexpr int kSliceRows = 16, kMaxSlices = 64;
constexpr int kStageWords = 8192;               // the backtrack's LDS image of back-pointer rows: 32 KB
constexpr int kWalkRows = 1024;                 // rows per staged piece, at most

inline int row_slices(int T) {
  const int s = dv3_cdiv(T, kSliceRows);
  return s < 1 ? 1 : (s > kMaxSlices ? kMaxSlices : s);
}

__device__ __forceinline__ int clamp_i(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

__global__ __launch_bounds__(64 * kRowWaves) void mono_score_kernel(const float* __restrict__ attn, int64_t layer_stride,
                                                                    int64_t item_stride, int64_t step_stride, int L,
                                                                    int T, int Tk, const int32_t* __restrict__ steps,
                                                                    const int32_t* __restrict__ key_len,
                                                                    float* __restrict__ s) {
  const int b = blockIdx.y, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int Tb = clamp_i(steps[b], 0, T), Nb = clamp_i(key_len[b], 1, Tk);
  const int per = (Tb + (int)gridDim.x - 1) / (int)gridDim.x;
  const int t0 = min((int)blockIdx.x * per, Tb), t1 = min(t0 + per, Tb);
  const float* __restrict__ item = attn + (int64_t)b * item_stride;
  float* __restrict__ sb = s + (int64_t)b * T * Tk;
  const float fl = (float)L;
  for (int t = t0 + wave; t < t1; t += kRowWaves) {      // wave-uniform
    const float* __restrict__ row = item + (int64_t)t * step_stride;
    for (int n = lane; n < Nb; n += 64) {
      float sum = row[n];
      for (int l = 1; l < L; ++l) sum += row[(int64_t)l * layer_stride + n];
      const float mean = sum / fl;
      const float p = mean > DV3_MONO_FLOOR ? mean : DV3_MONO_FLOOR;     // fmaxf's value; a NaN goes to the floor
      sb[(int64_t)t * Tk + n] = logf(p);
    }
  }
}

// back-pointer byte of cell (t, n), t >= 1: the advance j of the chosen predecessor (t - 1, n - j)
template <int WT, int PF>
__global__ __launch_bounds__(64) void mono_scan_kernel(const float* __restrict__ s, uint8_t* __restrict__ bp, int T, int Tk,
                                                       int J, const int32_t* __restrict__ steps,
                                                       const int32_t* __restrict__ key_len, float* __restrict__ out,
                                                       int32_t* __restrict__ path) {
  const int b = blockIdx.x, lane = threadIdx.x;
  const int Tb = clamp_i(steps[b], 0, T), Nb = clamp_i(key_len[b], 1, Tk);
  float* __restrict__ ob = out + (int64_t)b * DV3_MONO_COLS;
  if (lane == 0) {
    ob[1] = (float)Tb;
    ob[2] = (float)Nb;
  }
  if (Tb == 0) {
    if (lane == 0) {
      ob[0] = 0.f;
      ob[3] = 0.f;
    }
    return;
  }
  const float* __restrict__ sb = s + (int64_t)b * T * Tk;
  uint8_t* __restrict__ qb = bp + (int64_t)b * T * Tk;
  // Guards are kept off the step: a key at or past N_b reads the row's last valid element instead (a valid address,
  // one broadcast line) and stays -inf, the rows past the last step are the last row again and are never used.
  int col[WT];
  bool live[WT];
#pragma unroll
  for (int c = 0; c < WT; ++c) {
    live[c] = lane + 64 * c < Nb;
    col[c] = min(lane + 64 * c, Nb - 1);
  }
  float Q[WT], ring[PF][WT];
#pragma unroll
  for (int c = 0; c < WT; ++c) Q[c] = -INFINITY;
#pragma unroll
  for (int k = 0; k < PF; ++k) {
    const float* __restrict__ row = sb + (int64_t)min(k, Tb - 1) * Tk;
#pragma unroll
    for (int c = 0; c < WT; ++c) ring[k][c] = row[col[c]];
  }
  for (int t0 = 0; t0 < Tb; t0 += PF) {
#pragma unroll
    for (int k = 0; k < PF; ++k) {
      const int t = t0 + k;
      if (t >= Tb) break;                       // wave-uniform
      float cur[WT];
#pragma unroll
      for (int c = 0; c < WT; ++c) cur[c] = ring[k][c];
      const float* __restrict__ nrow = sb + (int64_t)min(t + PF, Tb - 1) * Tk;
#pragma unroll
      for (int c = 0; c < WT; ++c) ring[k][c] = nrow[col[c]];
      if (t == 0) {
#pragma unroll
        for (int c = 0; c < WT; ++c) Q[c] = (live[c] && lane + 64 * c < J) ? cur[c] : -INFINITY;
        continue;
      }
      float best[WT];
      int bj[WT];
#pragma unroll
      for (int c = 0; c < WT; ++c) {
        best[c] = Q[c];
        bj[c] = 0;
      }
      for (int j = 1; j <= J; ++j) {
        const bool wraps = lane >= 64 - j;      // as a SOURCE lane: my value lands j lanes up, one register higher
        const int src = (lane - j) & 63;
        float v[WT];
#pragma unroll
        for (int c = 0; c < WT; ++c) {
          const float below = c > 0 ? Q[c > 0 ? c - 1 : 0] : -INFINITY;
          v[c] = __shfl(wraps ? below : Q[c], src, 64);
        }
#pragma unroll
        for (int c = 0; c < WT; ++c) {
          const bool up = v[c] > best[c];       // strictly greater: the smallest advance keeps a tie
          best[c] = up ? v[c] : best[c];
          bj[c] = up ? j : bj[c];
        }
      }
      uint8_t* __restrict__ qrow = qb + (int64_t)t * Tk;
#pragma unroll
      for (int c = 0; c < WT; ++c) {
        Q[c] = live[c] ? cur[c] + best[c] : -INFINITY;
        if (live[c]) qrow[lane + 64 * c] = (uint8_t)bj[c];
      }
    }
  }
  // the end cell: keys N_b - 1 down to N_b - J, a smaller key only when strictly greater
  float ev = -INFINITY;
  int en = -1;
#pragma unroll
  for (int c = 0; c < WT; ++c) {
    const int n = lane + 64 * c;
    if (n < Nb && n >= Nb - J && (Q[c] > ev || (Q[c] == ev && n > en))) {
      ev = Q[c];
      en = n;
    }
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    const float ov = __shfl_xor(ev, off, 64);
    const int on = __shfl_xor(en, off, 64);
    if (ov > ev || (ov == ev && on > en)) {
      ev = ov;
      en = on;
    }
  }
  if (lane == 0) {
    const bool ok = ev > -INFINITY && en >= 0;
    ob[0] = ok ? 1.f : 0.f;
    ob[3] = ok ? ev : 0.f;
    if (ok) path[(int64_t)b * T + Tb - 1] = en;
  }
}

__global__ __launch_bounds__(64) void mono_back_kernel(const uint8_t* __restrict__ bp, int T, int Tk,
                                                       const int32_t* __restrict__ steps,
                                                       const int32_t* __restrict__ key_len, float* __restrict__ out,
                                                       int32_t* __restrict__ path, int32_t* __restrict__ dur) {
  __shared__ uint32_t stage[kStageWords];
  __shared__ int32_t piece[kWalkRows];
  __shared__ int32_t count[DV3_MONO_MAX_TK];
  const int b = blockIdx.x, lane = threadIdx.x;
  const int Tb = clamp_i(steps[b], 0, T), Nb = clamp_i(key_len[b], 1, Tk);
  float* __restrict__ ob = out + (int64_t)b * DV3_MONO_COLS;
  int32_t* __restrict__ pb = path + (int64_t)b * T;
  int32_t* __restrict__ db = dur + (int64_t)b * Tk;
  const bool feasible = Tb > 0 && ob[0] != 0.f;
  for (int t = (feasible ? Tb : 0) + lane; t < T; t += 64) pb[t] = -1;
  if (!feasible) {                              // workgroup-uniform
    for (int n = lane; n < Tk; n += 64) db[n] = 0;
    if (lane == 0) {
      ob[4] = 0.f;
      ob[5] = 0.f;
    }
    return;
  }
  for (int n = lane; n < Tk; n += 64) count[n] = 0;
  int cur = clamp_i(pb[Tb - 1], 0, Nb - 1);     // the scan's end key
  const int rows = min(kWalkRows, (kStageWords * 4 - 4) / Tk);      // >= 15 at Tk = 2048
  const int64_t base = (int64_t)b * T * Tk;
  for (int hi = Tb; hi > 0; hi -= rows) {       // steps [lo, hi), from the end
    const int lo = max(hi - rows, 0);
    const int64_t g0 = base + (int64_t)lo * Tk, g1 = base + (int64_t)hi * Tk;
    const int64_t a0 = g0 & ~(int64_t)3;
    const int words = (int)((g1 - a0 + 3) >> 2);      // <= (rows * Tk + 6) / 4 <= kStageWords
    const uint32_t* __restrict__ src = (const uint32_t*)(bp + a0);
    __syncthreads();                            // the walk and the stores of the piece before are done
    for (int w = lane; w < words; w += 64) stage[w] = src[w];
    __syncthreads();
    if (lane == 0) {
      const uint8_t* bytes = (const uint8_t*)stage + (int)(g0 - a0);
      for (int t = hi - 1; t >= lo; --t) {
        piece[t - lo] = cur;
        atomicAdd(&count[cur], 1);
        if (t > 0) cur = max(cur - (int)bytes[(t - lo) * Tk + cur], 0);
      }
    }
    __syncthreads();
    for (int r = lane; r < hi - lo; r += 64) pb[lo + r] = piece[r];
  }
  __syncthreads();
  int skipped = 0, longest = 0;
  for (int n = lane; n < Tk; n += 64) {
    const int d = n < Nb ? count[n] : 0;
    db[n] = d;
    skipped += (n < Nb && d == 0);
    longest = max(longest, d);
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    skipped += __shfl_xor(skipped, off, 64);
    longest = max(longest, __shfl_xor(longest, off, 64));
  }
  if (lane == 0) {
    ob[4] = (float)skipped;
    ob[5] = (float)longest;
  }
}

template <int WT, int PF>
void launch_scan(int B, hipStream_t st, const float* s, uint8_t* bp, int T, int Tk, int J, const int32_t* steps,
                 const int32_t* key_len, float* out, int32_t* path) {
  hipLaunchKernelGGL((mono_scan_kernel<WT, PF>), dim3(B), dim3(64), 0, st, s, bp, T, Tk, J, steps, key_len, out, path);
}

}  // namespace

// scratch: s fp32 [B][T][Tk] | back-pointer bytes [B][T][Tk], rounded up to whole dwords (the backtrack stages dwords)
extern "C" int dv3_mono_path_scratch_bytes(int32_t B, int32_t T, int32_t Tk, int64_t* bytes_out) {
  DV3_REQUIRE(bytes_out, "mono_path_scratch_bytes: bytes_out is null");
  *bytes_out = 0;
  DV3_REQUIRE(B >= 1 && B <= 65535, "mono_path_scratch_bytes: B = %d outside [1, 65535]", (int)B);
  DV3_REQUIRE(T >= 1 && T <= DV3_MONO_MAX_T, "mono_path_scratch_bytes: T = %d outside [1, %d]", (int)T, DV3_MONO_MAX_T);
  DV3_REQUIRE(Tk >= 1 && Tk <= DV3_MONO_MAX_TK, "mono_path_scratch_bytes: Tk = %d outside [1, %d]", (int)Tk,
              DV3_MONO_MAX_TK);
  const int64_t cells = (int64_t)B * T * Tk;
  *bytes_out = cells * 4 + ((cells + 3) & ~(int64_t)3);
  return DV3_OK;
}

extern "C" int dv3_mono_path_f32(const dv3_mono_desc* p, void* stream) {
  DV3_REQUIRE(p, "mono_path: the descriptor is null");
  const int B = p->B, T = p->T, Tk = p->Tk, J = p->max_advance, L = p->n_layers;
  DV3_REQUIRE(p->attn, "mono_path: attn is null");
  DV3_REQUIRE(p->steps, "mono_path: steps is null");
  DV3_REQUIRE(p->key_len, "mono_path: key_len is null");
  DV3_REQUIRE(p->out, "mono_path: out is null");
  DV3_REQUIRE(p->path, "mono_path: path is null");
  DV3_REQUIRE(p->durations, "mono_path: durations is null");
  DV3_REQUIRE(p->scratch, "mono_path: scratch is null");
  DV3_REQUIRE(B >= 1 && B <= 65535, "mono_path: B = %d outside [1, 65535]", B);
  DV3_REQUIRE(T >= 1 && T <= DV3_MONO_MAX_T, "mono_path: T = %d outside [1, %d]", T, DV3_MONO_MAX_T);
  DV3_REQUIRE(Tk >= 1 && Tk <= DV3_MONO_MAX_TK, "mono_path: Tk = %d outside [1, %d]", Tk, DV3_MONO_MAX_TK);
  DV3_REQUIRE(J >= 1 && J <= DV3_MONO_MAX_ADVANCE, "mono_path: max_advance = %d outside [1, %d]", J,
              DV3_MONO_MAX_ADVANCE);
  DV3_REQUIRE(L >= 1, "mono_path: n_layers = %d < 1", L);
  int64_t need = 0;
  if (dv3_mono_path_scratch_bytes(B, T, Tk, &need) != DV3_OK) return DV3_EINVAL;
  DV3_REQUIRE(p->scratch_bytes >= need, "mono_path: scratch_bytes = %lld, B = %d, T = %d, Tk = %d need %lld",
              (long long)p->scratch_bytes, B, T, Tk, (long long)need);
  DV3_REQUIRE(((uintptr_t)p->out & 3) == 0, "mono_path: out is not 4-byte aligned");
  DV3_REQUIRE(((uintptr_t)p->path & 3) == 0, "mono_path: path is not 4-byte aligned");
  DV3_REQUIRE(((uintptr_t)p->durations & 3) == 0, "mono_path: durations is not 4-byte aligned");
  DV3_REQUIRE(((uintptr_t)p->scratch & 3) == 0, "mono_path: scratch is not 4-byte aligned");
  hipStream_t st = (hipStream_t)stream;
  float* s = (float*)p->scratch;
  uint8_t* bp = (uint8_t*)p->scratch + (int64_t)B * T * Tk * 4;
  hipLaunchKernelGGL(mono_score_kernel, dim3(row_slices(T), B), dim3(64 * kRowWaves), 0, st, p->attn,
                     L > 1 ? p->layer_stride : (int64_t)0, p->item_stride, p->step_stride, L, T, Tk, p->steps, p->key_len,
                     s);
  const int W = dv3_cdiv(Tk, 64);
#define DV3_MONO_SCAN(WT, PF) \
  launch_scan<WT, PF>(B, st, (const float*)s, bp, T, Tk, J, p->steps, p->key_len, p->out, p->path)
  if (W <= 1) DV3_MONO_SCAN(1, 8);
  else if (W <= 2) DV3_MONO_SCAN(2, 8);
  else if (W <= 4) DV3_MONO_SCAN(4, 4);
  else if (W <= 8) DV3_MONO_SCAN(8, 2);
  else if (W <= 16) DV3_MONO_SCAN(16, 2);
  else DV3_MONO_SCAN(32, 2);
#undef DV3_MONO_SCAN
  hipLaunchKernelGGL(mono_back_kernel, dim3(B), dim3(64), 0, st, (const uint8_t*)bp, T, Tk, p->steps, p->key_len, p->out,
                     p->path, p->durations);
  return dv3_check_launch("mono_path_f32");
}

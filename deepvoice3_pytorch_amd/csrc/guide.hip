// Guide table of a guided decode: per-token step counts -> the key every decoder step is centred on
// (include/dv3hip.h: dv3_guide_from_durations_i32).
//
//   one 64-lane wave per item.  The item's durations are scanned 64 keys at a time (a shuffle scan plus the carry of
//   the pieces before), the running sums go to LDS; every sum saturates at T + 1, which keeps them in int32 whatever
//   the input holds and changes nothing below T (a saturating add of non-negative ints is associative).  Then lane l
//   takes steps l, l + 64, ...: step t belongs to the first key whose running sum exceeds min(t, total - 1) -- a binary
//   search over the item's keys --, so a key of duration 0 owns no step, the rows past the item's steps repeat its last
//   spoken key, and a row is stored in coalesced 256-byte pieces.  Every index is clamped: a negative duration counts
//   as 0 and is flagged, a total above T is cut at T and flagged, a total of 0 gives a row of zeros and is flagged.
//   No atomics; integers only: two calls agree bit for bit.
#include "common.h"

namespace {

__global__ __launch_bounds__(64) void guide_from_durations_kernel(const int32_t* __restrict__ dur, int64_t dur_bs,
                                                                  const int32_t* __restrict__ key_len, int Tk, int T,
                                                                  int32_t* __restrict__ guide, int64_t guide_bs,
                                                                  int32_t* __restrict__ steps, int32_t* __restrict__ flags) {
  __shared__ int32_t cum[DV3_GUIDE_MAX_TK];
  const int b = blockIdx.x, lane = threadIdx.x;
  const int kl = key_len[b];
  const int Nb = kl < 1 ? 1 : (kl > Tk ? Tk : kl);
  const int cap = T + 1;
  const int32_t* __restrict__ db = dur + (int64_t)b * dur_bs;
  int carry = 0, negative = 0;
  for (int n0 = 0; n0 < Nb; n0 += 64) {          // wave-uniform
    const int n = n0 + lane;
    int d = n < Nb ? db[n] : 0;
    negative |= d < 0;
    d = d < 0 ? 0 : (d > cap ? cap : d);
    int run = d;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
      const int below = __shfl_up(run, off, 64);
      if (lane >= off) run = min(run + below, cap);
    }
    run = min(run + carry, cap);
    if (n < Nb) cum[n] = run;
    carry = __shfl(run, 63, 64);
  }
  __syncthreads();
  const int total = carry;                       // min(sum, T + 1)
  const int Tb = min(total, T);
  negative = __any(negative);
  if (lane == 0) {
    steps[b] = Tb;
    flags[b] = (negative ? DV3_GUIDE_NEGATIVE : 0) | (total == 0 ? DV3_GUIDE_EMPTY : 0) | (total > T ? DV3_GUIDE_OVER : 0);
  }
  int32_t* __restrict__ gb = guide + (int64_t)b * guide_bs;
  for (int t = lane; t < T; t += 64) {
    const int tt = min(t, Tb - 1);               // -1 for an empty item: every sum exceeds it, the search gives key 0
    int lo = 0, hi = Nb - 1;                     // the first n in [0, Nb) with cum[n] > tt; cum[Nb - 1] = total > tt
    while (lo < hi) {
      const int mid = (lo + hi) >> 1;
      if (cum[mid] > tt) hi = mid; else lo = mid + 1;
    }
    gb[t] = total > 0 ? lo : 0;
  }
}

}  // namespace

extern "C" int dv3_guide_from_durations_i32(const int32_t* dur, int64_t dur_bs, const int32_t* key_len, int32_t B,
                                            int32_t Tk, int32_t T, int32_t* guide, int64_t guide_bs, int32_t* steps,
                                            int32_t* flags, void* stream) {
  DV3_REQUIRE(dur, "guide_from_durations: dur is null");
  DV3_REQUIRE(key_len, "guide_from_durations: key_len is null");
  DV3_REQUIRE(guide, "guide_from_durations: guide is null");
  DV3_REQUIRE(steps, "guide_from_durations: steps is null");
  DV3_REQUIRE(flags, "guide_from_durations: flags is null");
  DV3_REQUIRE(B >= 1 && B <= 65535, "guide_from_durations: B = %d outside [1, 65535]", (int)B);
  DV3_REQUIRE(Tk >= 1 && Tk <= DV3_GUIDE_MAX_TK, "guide_from_durations: Tk = %d outside [1, %d]", (int)Tk, DV3_GUIDE_MAX_TK);
  DV3_REQUIRE(T >= 1 && T <= DV3_GUIDE_MAX_T, "guide_from_durations: T = %d outside [1, %d]", (int)T, DV3_GUIDE_MAX_T);
  DV3_REQUIRE(dur_bs >= Tk, "guide_from_durations: dur_bs = %lld below Tk = %d", (long long)dur_bs, (int)Tk);
  DV3_REQUIRE(guide_bs >= T, "guide_from_durations: guide_bs = %lld below T = %d", (long long)guide_bs, (int)T);
  hipLaunchKernelGGL(guide_from_durations_kernel, dim3(B), dim3(64), 0, (hipStream_t)stream, dur, dur_bs, key_len, (int)Tk,
                     (int)T, guide, guide_bs, steps, flags);
  return dv3_check_launch("guide_from_durations_i32");
}

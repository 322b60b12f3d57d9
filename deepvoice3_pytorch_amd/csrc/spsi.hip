// Single Pass Spectrogram Inversion: a starting phase for Griffin-Lim from the magnitudes alone (include/dv3hip.h:
// dv3_spsi_phasor_f32; DESIGN.md 3.5, "A single-pass starting phase").  Beauregard, Harish & Wyse, "Single Pass
// Spectrogram Inversion", IEEE DSP 2015.  It stands beside audio.py:37-43 of the reference, whose inv_spectrogram hands
// the spectrogram to `lws.run_lws`: that package builds an initial phase estimate before it iterates, where this port's
// Griffin-Lim started from zero phase.
//
// Per frame: the spectral peaks, each peak's instantaneous frequency from the parabola through its three bins, the peak's
// phase advanced from the previous frame by hop x that frequency, and the peak's phase given to every bin of its lobe.
// Time is a true recurrence, so ONE workgroup owns an item and loops over its frames with all bins of a frame in
// parallel; nothing is shared between workgroups, no spin-waiting, no atomics: two calls give bit-equal output and an
// item's rows do not depend on B, its neighbours or the padding.
//
//   layout     N / 4 + 64 threads (whole waves), two bins per thread (j = tid and tid + threads): F = N / 2 + 1 bins are
//              covered, a wave's 64 lanes hold 64 consecutive bins (a "segment"), and the two chains of a thread
//              interleave.
//   LDS        the frame's magnitudes with one -inf on either side (a climb stops at the edges without an index test),
//              and the accumulator in turns as fp64, both double-buffered: iteration t reads side t & 1 and writes the
//              other one, which makes ONE barrier per frame enough.
//   owner      a bin climbs to the end of the strictly rising run on its right, else of the strictly falling run on its
//              left.  The wave ballots "my right neighbour is larger" / "my left neighbour is larger" over its segment,
//              and a lane finds the end of its run as the first clear bit above (below) its own: no dependent walk
//              through LDS.  A run that leaves the segment goes on in the next one, which the whole wave reads and
//              ballots again: a wave-uniform loop over at most F / 64 + 1 segments.
//   per bin    when the bin at the end of the run is a peak, compute ITS new phase -- every bin of a lobe repeats its
//              peak's few fp64 operations, which is cheaper than a second barrier to hand the value over -- else 0.
//   fp64       the parabola's vertex d, the accumulator and the wrap.  Their cost is nothing beside the latency of the
//              loop, and they make the kernel agree with the float64 restatement (tests/spsi_ref.py) to rounding instead
//              of drifting along a peak's track over hundreds of frames.  The wrapped turn, in [0, 1), is rounded to fp32
//              only for the final sincospif (the accurate one, not the hardware approximations).
//   HBM        the magnitudes of frames t + 1 .. t + 3 are in flight in registers while frame t is processed (a frame is
//              at most 4 KB: the loop is bound by latency, not by bytes); phasors leave as 8-byte stores, a wave's 512
//              contiguous bytes at a time.
#include "common.h"

namespace {

constexpr int kBinsPerThread = 2;

template <int N>
struct SpsiShape {
  static constexpr int F = N / 2 + 1;
  static constexpr int threads = N / 4 + 64;             // 2 * threads = N / 2 + 128 >= F; a multiple of 64
};

// mp: a frame's magnitudes with mp[0] = mp[F + 1] = -inf (bin k at mp[k + 1]).  Bin index clamped into the padded row.
template <int F>
__device__ __forceinline__ float spsi_mag(const float* __restrict__ mp, int k) {
  return mp[min(max(k, -1), F) + 1];
}

// The bin a climb from `bin` ends on.  rise / fall: this lane's right / left neighbour is strictly larger (false in lanes
// past the last bin); go_right / go_left: the direction this lane climbs in (neither: it stays).  seg: the first bin of
// the wave's segment (wave-uniform).  Every lane of the wave calls this together.
template <int F>
__device__ __forceinline__ int spsi_run_end(const float* __restrict__ mp, int seg, int lane, int bin, bool rise, bool fall,
                                            bool go_right, bool go_left) {
  int e = bin;
  // rightwards: the first bin at or above mine that does not rise
  const unsigned long long still = ~__ballot(rise) >> lane;          // bit 0: mine (clear when I rise)
  bool open = go_right && still == 0ull;
  if (go_right && still != 0ull) e = bin + __builtin_ctzll(still);
  for (int s = seg + 64; s < F + 64 && __any(open); s += 64) {        // wave-uniform; the run ends at bin F - 1 at the latest
    const int k = s + lane;
    const unsigned long long stop = ~__ballot(spsi_mag<F>(mp, k + 1) > spsi_mag<F>(mp, k));
    if (open && stop != 0ull) {
      e = s + __builtin_ctzll(stop);
      open = false;
    }
  }
  // leftwards: the last bin at or below mine whose left neighbour is not larger
  const unsigned long long lstill = ~__ballot(fall) << (63 - lane);   // bit 63: mine (clear when I fall)
  open = go_left && lstill == 0ull;
  if (go_left && lstill != 0ull) e = bin - __builtin_clzll(lstill);
  for (int s = seg - 64; s >= 0 && __any(open); s -= 64) {            // wave-uniform; bin 0 has no larger left neighbour
    const int k = s + lane;
    const unsigned long long stop = ~__ballot(spsi_mag<F>(mp, k - 1) > spsi_mag<F>(mp, k));
    if (open && stop != 0ull) {
      e = s + 63 - __builtin_clzll(stop);
      open = false;
    }
  }
  return min(max(e, 0), F - 1);                                       // in range by construction; the clamp costs nothing
}

// the phase in turns a bin takes when the climb from it ended on bin e: the peak's new phase, or 0 when e is no peak.
// acc: the previous frame's turns.  Branch-free: the value of a non-peak is computed and dropped.
template <int N>
__device__ __forceinline__ double spsi_turn(const float* __restrict__ mp, const double* __restrict__ acc, int e, int hop) {
#pragma clang fp contract(off)
  constexpr int F = N / 2 + 1;
  const float lo = mp[e], me = mp[e + 1], hi = mp[e + 2];
  const bool peak = e >= 1 && e <= F - 2 && me > lo && me >= hi;
  // me > lo and me >= hi: the denominator (lo - me) + (hi - me) is strictly negative, and |lo - hi| <= -denominator, so
  // |d| <= 0.5 -- no clamp and no zero test are needed
  const double a = (double)lo, b = (double)me, c = (double)hi;
  const double d = 0.5 * (a - c) / (a - 2.0 * b + c);
  // hop * e / N without its integer turns, taken off in integer arithmetic: nothing large is ever added
  const double base = (double)((hop * e) & (N - 1)) / (double)N;
  const double x = acc[e] + base + (double)hop * d / (double)N;       // in (-0.5, 2.5)
  const double f = x - floor(x);
  return peak && f < 1.0 ? f : 0.0;                                   // x a hair below an integer rounds up to 1.0
}

template <int N>
__global__ __launch_bounds__(SpsiShape<N>::threads) void spsi_kernel(const float* __restrict__ mag,
                                                                      float* __restrict__ phasor, int T, int hop,
                                                                      const int32_t* __restrict__ tlen) {
  constexpr int F = SpsiShape<N>::F, NT = SpsiShape<N>::threads;
  static_assert(NT % 64 == 0 && kBinsPerThread * NT >= F, "whole waves that cover every bin");
  __shared__ float m_s[2][F + 2];
  __shared__ double acc_s[2][F];
  const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63;
  int Tb = T;
  if (tlen) {
    const int v = tlen[b];
    Tb = v < 0 ? 0 : (v > T ? T : v);
  }
  const float* __restrict__ mb = mag + (int64_t)b * T * F;
  dv3_f32x2* __restrict__ pb = (dv3_f32x2*)phasor + (int64_t)b * T * F;
  int bin[kBinsPerThread];
  bool live[kBinsPerThread];
#pragma unroll
  for (int i = 0; i < kBinsPerThread; ++i) {
    bin[i] = tid + i * NT;
    live[i] = bin[i] < F;
  }
  if (Tb > 0) {
    // a bin past F - 1 reads bin F - 1 again (a valid address) and is never used
    int col[kBinsPerThread];
    float sgn[kBinsPerThread], cur[kBinsPerThread], nx1[kBinsPerThread], nx2[kBinsPerThread], nx3[kBinsPerThread];
#pragma unroll
    for (int i = 0; i < kBinsPerThread; ++i) {
      col[i] = live[i] ? bin[i] : F - 1;
      sgn[i] = (bin[i] & 1) ? -1.f : 1.f;
      cur[i] = mb[col[i]];
      nx1[i] = mb[(int64_t)min(1, Tb - 1) * F + col[i]];
      nx2[i] = mb[(int64_t)min(2, Tb - 1) * F + col[i]];
      nx3[i] = mb[(int64_t)min(3, Tb - 1) * F + col[i]];
    }
    if (tid < 2) {
      m_s[tid][0] = -INFINITY;
      m_s[tid][F + 1] = -INFINITY;
    }
#pragma unroll
    for (int i = 0; i < kBinsPerThread; ++i) {
      if (live[i]) {
        m_s[0][bin[i] + 1] = cur[i];
        acc_s[0][bin[i]] = 0.0;
      }
    }
    __syncthreads();
    for (int t = 0; t < Tb; ++t) {
      const float* __restrict__ mp = m_s[t & 1];
      const double* __restrict__ acc = acc_s[t & 1];
      float nx4[kBinsPerThread];
#pragma unroll
      for (int i = 0; i < kBinsPerThread; ++i) nx4[i] = mb[(int64_t)min(t + 4, Tb - 1) * F + col[i]];
      float left[kBinsPerThread], right[kBinsPerThread];
#pragma unroll
      for (int i = 0; i < kBinsPerThread; ++i) {
        left[i] = mp[col[i]];
        right[i] = mp[col[i] + 2];
      }
      int e[kBinsPerThread];
#pragma unroll
      for (int i = 0; i < kBinsPerThread; ++i) {
        const bool rise = live[i] && right[i] > cur[i], fall = live[i] && left[i] > cur[i];
        // climb right first (a valley between two peaks goes to the right one), else left, else stay
        e[i] = spsi_run_end<F>(mp, bin[i] - lane, lane, col[i], rise, fall, rise, fall && !rise);
      }
      double turn[kBinsPerThread];
#pragma unroll
      for (int i = 0; i < kBinsPerThread; ++i) turn[i] = spsi_turn<N>(mp, acc, e[i], hop);
      double* __restrict__ acc_next = acc_s[(t + 1) & 1];
      float* __restrict__ m_next = m_s[(t + 1) & 1];
      dv3_f32x2* __restrict__ row = pb + (int64_t)t * F;
#pragma unroll
      for (int i = 0; i < kBinsPerThread; ++i) {
        float sn, cs;
        sincospif(2.0f * (float)turn[i], &sn, &cs);
        if (live[i]) {
          acc_next[bin[i]] = turn[i];
          m_next[bin[i] + 1] = nx1[i];
          // (-1)^k: a frame's transform is referenced to its first sample with the window centred at N / 2, so the bins
          // of one component alternate in sign; the accumulator stays free of the term
          const dv3_f32x2 v = {sgn[i] * cs, sgn[i] * sn};
          row[bin[i]] = v;
        }
        cur[i] = nx1[i];
        nx1[i] = nx2[i];
        nx2[i] = nx3[i];
        nx3[i] = nx4[i];
      }
      __syncthreads();
    }
  }
  // frames past the item's own: the phasor (1, 0), what a NULL phasor means to the inverse
  const int64_t rest = (int64_t)(T - Tb) * F;
  dv3_f32x2* __restrict__ tail = pb + (int64_t)Tb * F;
  const dv3_f32x2 one = {1.f, 0.f};
  for (int64_t i = tid; i < rest; i += NT) tail[i] = one;
}

template <int N>
int launch_spsi(const float* mag, float* phasor, int B, int T, int hop, const int32_t* tlen, hipStream_t st) {
  hipLaunchKernelGGL((spsi_kernel<N>), dim3(B), dim3(SpsiShape<N>::threads), 0, st, mag, phasor, T, hop, tlen);
  return dv3_check_launch("spsi_phasor");
}

}  // namespace

extern "C" int dv3_spsi_phasor_f32(const float* mag, float* phasor, int B, int T, int hop, const int32_t* tlen,
                                   int fft_size, void* stream) {
  if (fft_size != 512 && fft_size != 1024 && fft_size != 2048) {
    dv3_set_error("spsi_phasor: n_fft = %d is not supported: the FFT kernels are built for 512, 1024 and 2048", fft_size);
    return DV3_EINVAL;
  }
  DV3_REQUIRE(mag, "spsi_phasor: mag is null");
  DV3_REQUIRE(phasor, "spsi_phasor: phasor is null");
  DV3_REQUIRE(((uintptr_t)phasor & 7) == 0, "spsi_phasor: phasor is not 8-byte aligned");
  DV3_REQUIRE(((uintptr_t)mag & 3) == 0, "spsi_phasor: mag is not 4-byte aligned");
  DV3_REQUIRE(B >= 1 && B <= 65535, "spsi_phasor: B = %d outside [1, 65535]", B);
  DV3_REQUIRE(T >= 1, "spsi_phasor: T = %d < 1", T);
  DV3_REQUIRE(hop >= 1 && hop <= fft_size, "spsi_phasor: hop = %d outside [1, n_fft = %d]", hop, fft_size);
  hipStream_t st = (hipStream_t)stream;
  switch (fft_size) {
    case 512: return launch_spsi<512>(mag, phasor, B, T, hop, tlen, st);
    case 1024: return launch_spsi<1024>(mag, phasor, B, T, hop, tlen, st);
    default: return launch_spsi<2048>(mag, phasor, B, T, hop, tlen, st);
  }
}

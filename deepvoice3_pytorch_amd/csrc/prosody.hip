// Speaking rate and pitch at vocoding: a time-and-frequency warp of the Griffin-Lim magnitudes with the spectral
// envelope kept in place (include/dv3hip.h: dv3_prosody_warp_f32, where every step is stated).  The
// reference has no counterpart: its synthesis (synthesis.py:42-73) gives one rate and one pitch per text, and its
// inv_spectrogram (audio.py:37-43) takes the magnitudes as the model made them.
//
//   grid       (T_out, B): one workgroup of 256 threads per output frame; thread t owns bins t, t + 256, ... (at most
//              kBinsPerThread = 5 of the 1025), so every global access of a wave is 256 contiguous bytes.  Rows of 257 /
//              513 / 1025 floats are 4-byte aligned only: the loads and stores are dwords on purpose.
//   time       the two source rows are blended on the way in; neighbouring output frames read the same source rows, which
//              the L2 serves (one workgroup per frame keeps the kernel free of any cross-workgroup state).
//   LDS        row A holds the blended magnitudes m (plain warp) or their logarithms l (envelope mode), row X the
//              log-spectrum with its envelope taken off: the two rows other bins read.  The envelope E[k] is read back by
//              bin k alone, so it stays in that thread's registers.  8.2 KB per workgroup.
//   envelope   the triangular average as 2W + 1 direct taps from LDS: consecutive lanes read consecutive words (no bank
//              conflict), one fmaf per tap in ascending bin order -- a fixed order, so a frame is bit-equal whatever shares
//              its launch.  At W = 19 and 513 bins that is 20 k fmaf per frame beside 6 KB of HBM traffic; two running box
//              passes would save the taps and serialise the row.
//   fp64       only the two index computations (j * rate, k / ratio): they decide WHICH elements are read, and a
//              float64 restatement (tests/prosody_ref.py) must split them into the same integer and fraction.
//   math       accurate logf / expf, every product and sum written out with contraction off.
#include "common.h"

namespace {

constexpr int kThreads = 256;
constexpr int kMaxBins = 1025;
constexpr int kBinsPerThread = (kMaxBins + kThreads - 1) / kThreads;

// (1 - a) x0 + a x1 as two rounded products and one rounded sum; a == 0 returns x0 itself
__device__ __forceinline__ float lerp_f32(float a, float x0, float x1) {
#pragma clang fp contract(off)
  const float p0 = (1.0f - a) * x0, p1 = a * x1;
  return a == 0.0f ? x0 : p0 + p1;
}

__global__ __launch_bounds__(kThreads) void prosody_warp_kernel(const float* __restrict__ mag, float* __restrict__ out,
                                                                int T_in, int T_out, int bins,
                                                                const int32_t* __restrict__ tlen_in,
                                                                const int32_t* __restrict__ tlen_out,
                                                                const double* __restrict__ rate,
                                                                const double* __restrict__ ratio, int W, int preserve) {
#pragma clang fp contract(off)
  __shared__ float A[kMaxBins + 1], X[kMaxBins + 1];
  const int b = blockIdx.y, j = blockIdx.x, tid = threadIdx.x;
  int tin = T_in;
  if (tlen_in) {
    const int v = tlen_in[b];
    tin = v < 0 ? 0 : (v > T_in ? T_in : v);
  }
  int tout = tlen_out[b];
  tout = tout < 0 ? 0 : (tout > T_out ? T_out : tout);
  float* __restrict__ orow = out + ((int64_t)b * T_out + j) * bins;
  if (j >= tout || tin < 1) {                        // block-uniform: the rows past the item's own are zeros
    for (int k = tid; k < bins; k += kThreads) orow[k] = 0.0f;
    return;
  }
  // time axis: u in [0, tin - 1] whatever rate[b] holds (a NaN or a negative product reads frame 0)
  double u = (double)j * rate[b];
  if (!(u >= 0.0)) u = 0.0;
  if (u > (double)(tin - 1)) u = (double)(tin - 1);
  const int i0 = (int)floor(u);
  const float a = (float)(u - (double)i0);
  const int i1 = min(i0 + 1, tin - 1);
  const float* __restrict__ r0 = mag + ((int64_t)b * T_in + i0) * bins;
  const float* __restrict__ r1 = mag + ((int64_t)b * T_in + i1) * bins;
  float m[kBinsPerThread];
#pragma unroll
  for (int i = 0; i < kBinsPerThread; ++i) {
    const int k = tid + i * kThreads;
    m[i] = k < bins ? lerp_f32(a, r0[k], r1[k]) : 0.0f;
  }
  double q = ratio[b];
  if (!(q > 0.0)) q = 1.0;                           // a ratio that is no positive number leaves the pitch alone
  if (q == 1.0) {
#pragma unroll
    for (int i = 0; i < kBinsPerThread; ++i) {
      const int k = tid + i * kThreads;
      if (k < bins) orow[k] = m[i];
    }
    return;
  }
  // frequency axis: bin k reads position s = k / q, split like the time axis; past the last bin: the edge rule
  int s0[kBinsPerThread], s1[kBinsPerThread];
  float fa[kBinsPerThread];
  bool in[kBinsPerThread];
#pragma unroll
  for (int i = 0; i < kBinsPerThread; ++i) {
    const int k = min(tid + i * kThreads, bins - 1);
    const double s = (double)k / q;
    in[i] = s <= (double)(bins - 1);
    const double sc = in[i] ? s : (double)(bins - 1);
    s0[i] = (int)floor(sc);
    fa[i] = (float)(sc - (double)s0[i]);
    s1[i] = min(s0[i] + 1, bins - 1);
  }
  if (!preserve) {
#pragma unroll
    for (int i = 0; i < kBinsPerThread; ++i) {
      const int k = tid + i * kThreads;
      if (k < bins) A[k] = m[i];
    }
    __syncthreads();
#pragma unroll
    for (int i = 0; i < kBinsPerThread; ++i) {
      const int k = tid + i * kThreads;
      if (k < bins) orow[k] = in[i] ? lerp_f32(fa[i], A[s0[i]], A[s1[i]]) : A[bins - 1];
    }
    return;
  }
  float l[kBinsPerThread], E[kBinsPerThread];
#pragma unroll
  for (int i = 0; i < kBinsPerThread; ++i) {
    const int k = tid + i * kThreads;
    l[i] = logf(fmaxf(m[i], 1e-10f));
    if (k < bins) A[k] = l[i];
  }
  __syncthreads();
#pragma unroll
  for (int i = 0; i < kBinsPerThread; ++i) {
    const int k = tid + i * kThreads;
    if (k < bins) {
      const int lo = max(k - W, 0), hi = min(k + W, bins - 1);
      float acc = 0.0f;
      int wsum = 0;
      for (int kk = lo; kk <= hi; ++kk) {
        const int w = W + 1 - abs(kk - k);
        acc = fmaf((float)w, A[kk], acc);
        wsum += w;
      }
      E[i] = acc / (float)wsum;
      X[k] = l[i] - E[i];
    }
  }
  __syncthreads();
#pragma unroll
  for (int i = 0; i < kBinsPerThread; ++i) {
    const int k = tid + i * kThreads;
    if (k < bins) {
      const float xs = in[i] ? lerp_f32(fa[i], X[s0[i]], X[s1[i]]) : 0.0f;
      orow[k] = expf(E[i] + xs);
    }
  }
}

}  // namespace

extern "C" int dv3_prosody_warp_f32(const float* mag, float* out, int32_t B, int32_t T_in, int32_t T_out, int32_t bins,
                                    const int32_t* tlen_in, const int32_t* tlen_out, const double* rate,
                                    const double* ratio, int32_t env_half_width, int32_t preserve_envelope,
                                    void* stream) {
  DV3_REQUIRE(mag, "prosody_warp: mag is null");
  DV3_REQUIRE(out, "prosody_warp: out is null");
  DV3_REQUIRE(tlen_out, "prosody_warp: tlen_out is null");
  DV3_REQUIRE(rate, "prosody_warp: rate is null");
  DV3_REQUIRE(ratio, "prosody_warp: ratio is null");
  DV3_REQUIRE(((uintptr_t)mag & 3) == 0 && ((uintptr_t)out & 3) == 0, "prosody_warp: mag or out is not 4-byte aligned");
  DV3_REQUIRE(((uintptr_t)rate & 7) == 0 && ((uintptr_t)ratio & 7) == 0, "prosody_warp: rate or ratio is not 8-byte aligned");
  DV3_REQUIRE(mag != out, "prosody_warp: out must not be mag (a frame reads rows other frames write)");
  DV3_REQUIRE(B >= 1 && B <= 65535, "prosody_warp: B = %d outside [1, 65535]", (int)B);
  DV3_REQUIRE(T_in >= 1, "prosody_warp: T_in = %d < 1", (int)T_in);
  DV3_REQUIRE(T_out >= 1, "prosody_warp: T_out = %d < 1", (int)T_out);
  DV3_REQUIRE(bins >= 1 && bins <= kMaxBins, "prosody_warp: bins = %d outside [1, %d]", (int)bins, kMaxBins);
  DV3_REQUIRE(preserve_envelope == 0 || preserve_envelope == 1, "prosody_warp: preserve_envelope = %d is neither 0 nor 1",
              (int)preserve_envelope);
  DV3_REQUIRE(env_half_width >= 1 && env_half_width <= DV3_PROSODY_MAX_HALF_WIDTH,
              "prosody_warp: env_half_width = %d outside [1, %d]", (int)env_half_width, DV3_PROSODY_MAX_HALF_WIDTH);
  hipLaunchKernelGGL(prosody_warp_kernel, dim3(T_out, B), dim3(kThreads), 0, (hipStream_t)stream, mag, out, (int)T_in,
                     (int)T_out, (int)bins, tlen_in, tlen_out, rate, ratio, (int)env_half_width, (int)preserve_envelope);
  return dv3_check_launch("prosody_warp");
}

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
//
// Prosody marks (include/dv3hip.h: dv3_curve_warp_f32, dv3_curve_plan_f64, dv3_curve_fill_f64): the same
// frame body, warp_frame(), under a second kernel that takes the frame's position, ratio and gain from per-output-frame
// tables -- a position that is not >= 0 is a silent frame, the gain is one more fp32 product (none at exactly 1) -- and
// two latency-bound kernels that make the tables from segments (an fp64 scan per item, then one thread per table word).
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

// the last operation of every output element: one rounded product with the frame's gain, none where it is exactly 1
__device__ __forceinline__ float leveled(float v, float g) {
#pragma clang fp contract(off)
  return g == 1.0f ? v : v * g;
}

__device__ __forceinline__ int clamped_len(const int32_t* __restrict__ tlen, int b, int T, int dflt) {
  const int v = tlen ? tlen[b] : dflt;
  return v < 0 ? 0 : (v > T ? T : v);
}

// One output frame: item base `src` (tin >= 1 frames of `bins`), read at u in [0, tin - 1] along time and at k / q along
// the bins, times g.  Both kernels below are this body; they differ in where u, q and g come from.
__device__ __forceinline__ void warp_frame(const float* __restrict__ src, float* __restrict__ orow, int tin, int bins,
                                           double u, double q, float g, int W, int preserve, float* __restrict__ A,
                                           float* __restrict__ X) {
#pragma clang fp contract(off)
  const int tid = threadIdx.x;
  const int i0 = (int)floor(u);
  const float a = (float)(u - (double)i0);
  const int i1 = min(i0 + 1, tin - 1);
  const float* __restrict__ r0 = src + (int64_t)i0 * bins;
  const float* __restrict__ r1 = src + (int64_t)i1 * bins;
  float m[kBinsPerThread];
#pragma unroll
  for (int i = 0; i < kBinsPerThread; ++i) {
    const int k = tid + i * kThreads;
    m[i] = k < bins ? lerp_f32(a, r0[k], r1[k]) : 0.0f;
  }
  if (!(q > 0.0)) q = 1.0;                           // a ratio that is no positive number leaves the pitch alone
  if (q == 1.0) {
#pragma unroll
    for (int i = 0; i < kBinsPerThread; ++i) {
      const int k = tid + i * kThreads;
      if (k < bins) orow[k] = leveled(m[i], g);
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
      if (k < bins) orow[k] = leveled(in[i] ? lerp_f32(fa[i], A[s0[i]], A[s1[i]]) : A[bins - 1], g);
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
      orow[k] = leveled(expf(E[i] + xs), g);
    }
  }
}

__device__ __forceinline__ void zero_row(float* __restrict__ orow, int bins) {
  for (int k = threadIdx.x; k < bins; k += kThreads) orow[k] = 0.0f;
}

__global__ __launch_bounds__(kThreads) void prosody_warp_kernel(const float* __restrict__ mag, float* __restrict__ out,
                                                                int T_in, int T_out, int bins,
                                                                const int32_t* __restrict__ tlen_in,
                                                                const int32_t* __restrict__ tlen_out,
                                                                const double* __restrict__ rate,
                                                                const double* __restrict__ ratio, int W, int preserve) {
#pragma clang fp contract(off)
  __shared__ float A[kMaxBins + 1], X[kMaxBins + 1];
  const int b = blockIdx.y, j = blockIdx.x;
  const int tin = clamped_len(tlen_in, b, T_in, T_in), tout = clamped_len(tlen_out, b, T_out, 0);
  float* __restrict__ orow = out + ((int64_t)b * T_out + j) * bins;
  if (j >= tout || tin < 1) {                        // block-uniform: the rows past the item's own are zeros
    zero_row(orow, bins);
    return;
  }
  // time axis: u in [0, tin - 1] whatever rate[b] holds (a NaN or a negative product reads frame 0)
  double u = (double)j * rate[b];
  if (!(u >= 0.0)) u = 0.0;
  if (u > (double)(tin - 1)) u = (double)(tin - 1);
  warp_frame(mag + (int64_t)b * T_in * bins, orow, tin, bins, u, ratio[b], 1.0f, W, preserve, A, X);
}

// the same frame from per-output-frame tables: pos the source position (not >= 0: silence), ratio, gain
__global__ __launch_bounds__(kThreads) void curve_warp_kernel(const float* __restrict__ mag, float* __restrict__ out,
                                                              int T_in, int T_out, int bins,
                                                              const int32_t* __restrict__ tlen_in,
                                                              const int32_t* __restrict__ tlen_out,
                                                              const double* __restrict__ pos,
                                                              const double* __restrict__ ratio,
                                                              const float* __restrict__ gain, int W, int preserve) {
  __shared__ float A[kMaxBins + 1], X[kMaxBins + 1];
  const int b = blockIdx.y, j = blockIdx.x;
  const int64_t f = (int64_t)b * T_out + j;
  // the tables have a word for every (b, j), also past tlen_out[b]: the three are read beside the two lengths, before
  // any branch, so the frame's wave-uniform words arrive in one round trip instead of three dependent ones
  double u = pos[f];
  const double q = ratio[f];
  const float g = gain[f];
  const int tin = clamped_len(tlen_in, b, T_in, T_in), tout = clamped_len(tlen_out, b, T_out, 0);
  float* __restrict__ orow = out + f * bins;
  if (j >= tout || tin < 1 || !(u >= 0.0)) {         // block-uniform: past the item, or a silent frame (negative or NaN)
    zero_row(orow, bins);
    return;
  }
  if (u > (double)(tin - 1)) u = (double)(tin - 1);
  warp_frame(mag + (int64_t)b * T_in * bins, orow, tin, bins, u, q, g, W, preserve, A, X);
}

// ---------------------------------------------------------------------------------------------------------------------
// segments -> tables (include/dv3hip.h: dv3_curve_plan_f64, dv3_curve_fill_f64).  Latency-bound: one thread per item
// walks at most DV3_PROSODY_MAX_SEGMENTS segments; one thread per table element finds its segment by the same walk.
// ---------------------------------------------------------------------------------------------------------------------
struct Segments {
  const int32_t* __restrict__ nseg;
  const int32_t* __restrict__ bounds;   // [B][S + 1]
  const double* __restrict__ rate;      // [B][S]
  const int32_t* __restrict__ brk;      // [B][S]
  int S;
};

__device__ __forceinline__ int seg_count(const Segments& t, int b) {
  const int v = t.nseg[b];
  return v < 1 ? 1 : (v > t.S ? t.S : v);
}

// the repaired bound s + 1 from the repaired bound s (c_0 = 0): clamped into [0, n], never below its predecessor, the last n
__device__ __forceinline__ int next_bound(const Segments& t, int b, int s, int ns, int n, int c) {
  if (s + 1 == ns) return n;
  const int v = t.bounds[(int64_t)b * (t.S + 1) + s + 1];
  const int w = v < 0 ? 0 : (v > n ? n : v);
  return w > c ? w : c;
}

__device__ __forceinline__ double seg_rate(const Segments& t, int b, int s) {
  const double r = t.rate[(int64_t)b * t.S + s];
  return (r >= 1.0 / DV3_PROSODY_MAX_RATE && r <= (double)DV3_PROSODY_MAX_RATE) ? r : 1.0;
}

__device__ __forceinline__ int seg_break(const Segments& t, int b, int s) {
  const int v = t.brk[(int64_t)b * t.S + s];
  return v < 0 ? 0 : (v > DV3_PROSODY_MAX_BREAK ? DV3_PROSODY_MAX_BREAK : v);
}

// output frames of the source frames [c0, c1) at `rate`; last: the segment that ends the item keeps its last frame's place
__device__ __forceinline__ int64_t seg_frames(int c0, int c1, double rate, bool last) {
#pragma clang fp contract(off)
  if (c1 <= c0) return 0;
  if (last) return (int64_t)floor((double)(c1 - 1 - c0) / rate + 0.5) + 1;
  const double L = (double)(c1 - c0);
  int64_t len = (int64_t)ceil(L / rate);
  // the defining property, in the arithmetic the fill uses: (len - 1) rate < L <= len rate (a quotient rounded across
  // an integer would break it by one frame)
  while (len > 1 && (double)(len - 1) * rate >= L) --len;
  while ((double)len * rate < L) ++len;
  return len;
}

__global__ void curve_plan_kernel(Segments t, int B, int T_in, const int32_t* __restrict__ tlen_in, int min_frames,
                                  int32_t* __restrict__ o, int32_t* __restrict__ tlen_out) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= B) return;
  const int n = clamped_len(tlen_in, b, T_in, T_in), ns = seg_count(t, b);
  int32_t* __restrict__ orow = o + (int64_t)b * (t.S + 1);
  int64_t at = 0;
  int c = 0;
  orow[0] = 0;
  for (int s = 0; s < t.S; ++s) {
    if (s < ns) {
      const int c1 = next_bound(t, b, s, ns, n, c);
      at += seg_frames(c, c1, seg_rate(t, b, s), c1 == n) + seg_break(t, b, s);
      c = c1;
    }
    orow[s + 1] = (int32_t)(at > 0x7fffffff ? 0x7fffffff : at);      // the entries past nseg repeat the total
  }
  const int total = orow[t.S];
  tlen_out[b] = total > min_frames ? total : min_frames;
}

__global__ void curve_fill_kernel(Segments t, int B, int T_in, const int32_t* __restrict__ tlen_in,
                                  const double* __restrict__ semitones, const double* __restrict__ gain_db,
                                  const int32_t* __restrict__ o, const int32_t* __restrict__ tlen_out, int T_out, int R,
                                  double* __restrict__ pos, double* __restrict__ ratio, float* __restrict__ gain) {
#pragma clang fp contract(off)
  const int j = blockIdx.x * blockDim.x + threadIdx.x, b = blockIdx.y;
  if (j >= T_out) return;
  const int64_t f = (int64_t)b * T_out + j;
  const int n = clamped_len(tlen_in, b, T_in, T_in), ns = seg_count(t, b);
  const int tout = clamped_len(tlen_out, b, T_out, 0);
  double p = -1.0, st = 0.0, db = 0.0;
  if (j < tout && n >= 1) {
    const int32_t* __restrict__ orow = o + (int64_t)b * (t.S + 1);
    const double* __restrict__ sm = semitones + (int64_t)b * t.S;
    const double* __restrict__ gd = gain_db + (int64_t)b * t.S;
    if (j >= orow[ns]) {                             // added by the min_frames clamp: the item's last frame, held
      p = (double)(n - 1);
      st = sm[ns - 1];
      db = gd[ns - 1];
    } else {
      int c = 0;
      for (int s = 0; s < ns; ++s) {
        const int c1 = next_bound(t, b, s, ns, n, c);
        if (j < orow[s + 1]) {                       // segment s: its frames, then its break
          const int end = orow[s + 1] - seg_break(t, b, s);
          if (j < end) {
            p = (double)c + (double)(j - orow[s]) * seg_rate(t, b, s);
            st = sm[s];
            db = gd[s];
            if (R > 0) {
              // a boundary is eligible when both neighbours have frames and no break lies between them; its ramp is the R
              // frames from e - R / 2 on, cut at this segment's own ends; the right boundary wins where two overlap
              const int h = R / 2;
              int other = -1, first = 0;
              if (s + 1 < ns && seg_break(t, b, s) == 0 && orow[s + 2] - seg_break(t, b, s + 1) > orow[s + 1] &&
                  j >= orow[s + 1] - h) {
                other = s + 1, first = orow[s + 1] - h;
              } else if (s > 0 && seg_break(t, b, s - 1) == 0 && orow[s] > orow[s - 1] && j < orow[s] - h + R) {
                other = s - 1, first = orow[s] - h;
              }
              if (other >= 0) {
                const int lo = other < s ? other : s, hi = lo + 1;
                const double w = (double)(j - first + 1) / (double)(R + 1);
                st = sm[lo] + w * (sm[hi] - sm[lo]);
                db = gd[lo] + w * (gd[hi] - gd[lo]);
              }
            }
          }
          break;
        }
        c = c1;
      }
    }
  }
  pos[f] = p;
  ratio[f] = exp2(st / 12.0);
  gain[f] = (float)pow(10.0, db / 20.0);
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

extern "C" int dv3_curve_warp_f32(const float* mag, float* out, int32_t B, int32_t T_in, int32_t T_out, int32_t bins,
                                  const int32_t* tlen_in, const int32_t* tlen_out, const double* pos, const double* ratio,
                                  const float* gain, int32_t env_half_width, int32_t preserve_envelope, void* stream) {
  DV3_REQUIRE(mag, "curve_warp: mag is null");
  DV3_REQUIRE(out, "curve_warp: out is null");
  DV3_REQUIRE(tlen_out, "curve_warp: tlen_out is null");
  DV3_REQUIRE(pos, "curve_warp: pos is null");
  DV3_REQUIRE(ratio, "curve_warp: ratio is null");
  DV3_REQUIRE(gain, "curve_warp: gain is null");
  DV3_REQUIRE(((uintptr_t)mag & 3) == 0 && ((uintptr_t)out & 3) == 0 && ((uintptr_t)gain & 3) == 0,
              "curve_warp: mag, out or gain is not 4-byte aligned");
  DV3_REQUIRE(((uintptr_t)pos & 7) == 0 && ((uintptr_t)ratio & 7) == 0, "curve_warp: pos or ratio is not 8-byte aligned");
  DV3_REQUIRE(mag != out, "curve_warp: out must not be mag (a frame reads rows other frames write)");
  DV3_REQUIRE(B >= 1 && B <= 65535, "curve_warp: B = %d outside [1, 65535]", (int)B);
  DV3_REQUIRE(T_in >= 1, "curve_warp: T_in = %d < 1", (int)T_in);
  DV3_REQUIRE(T_out >= 1, "curve_warp: T_out = %d < 1", (int)T_out);
  DV3_REQUIRE(bins >= 1 && bins <= kMaxBins, "curve_warp: bins = %d outside [1, %d]", (int)bins, kMaxBins);
  DV3_REQUIRE(preserve_envelope == 0 || preserve_envelope == 1, "curve_warp: preserve_envelope = %d is neither 0 nor 1",
              (int)preserve_envelope);
  DV3_REQUIRE(env_half_width >= 1 && env_half_width <= DV3_PROSODY_MAX_HALF_WIDTH,
              "curve_warp: env_half_width = %d outside [1, %d]", (int)env_half_width, DV3_PROSODY_MAX_HALF_WIDTH);
  hipLaunchKernelGGL(curve_warp_kernel, dim3(T_out, B), dim3(kThreads), 0, (hipStream_t)stream, mag, out, (int)T_in,
                     (int)T_out, (int)bins, tlen_in, tlen_out, pos, ratio, gain, (int)env_half_width,
                     (int)preserve_envelope);
  return dv3_check_launch("curve_warp");
}

extern "C" int dv3_curve_plan_f64(const int32_t* tlen_in, int32_t B, int32_t T_in, int32_t S, const int32_t* nseg,
                                  const int32_t* bounds, const double* rate, const int32_t* break_frames,
                                  int32_t min_frames, int32_t* o, int32_t* tlen_out, void* stream) {
  DV3_REQUIRE(nseg, "curve_plan: nseg is null");
  DV3_REQUIRE(bounds, "curve_plan: bounds is null");
  DV3_REQUIRE(rate, "curve_plan: rate is null");
  DV3_REQUIRE(break_frames, "curve_plan: break_frames is null");
  DV3_REQUIRE(o, "curve_plan: o is null");
  DV3_REQUIRE(tlen_out, "curve_plan: tlen_out is null");
  DV3_REQUIRE(((uintptr_t)rate & 7) == 0, "curve_plan: rate is not 8-byte aligned");
  DV3_REQUIRE(B >= 1 && B <= 65535, "curve_plan: B = %d outside [1, 65535]", (int)B);
  DV3_REQUIRE(T_in >= 1, "curve_plan: T_in = %d < 1", (int)T_in);
  DV3_REQUIRE(S >= 1 && S <= DV3_PROSODY_MAX_SEGMENTS, "curve_plan: S = %d outside [1, %d]", (int)S,
              DV3_PROSODY_MAX_SEGMENTS);
  DV3_REQUIRE(min_frames >= 0, "curve_plan: min_frames = %d < 0", (int)min_frames);
  const Segments t = {nseg, bounds, rate, break_frames, (int)S};
  hipLaunchKernelGGL(curve_plan_kernel, dim3((B + 63) / 64), dim3(64), 0, (hipStream_t)stream, t, (int)B, (int)T_in, tlen_in,
                     (int)min_frames, o, tlen_out);
  return dv3_check_launch("curve_plan");
}

extern "C" int dv3_curve_fill_f64(const int32_t* tlen_in, int32_t B, int32_t T_in, int32_t S, const int32_t* nseg,
                                  const int32_t* bounds, const double* rate, const double* semitones,
                                  const double* gain_db, const int32_t* break_frames, const int32_t* o,
                                  const int32_t* tlen_out, int32_t T_out, int32_t ramp_frames, double* pos, double* ratio,
                                  float* gain, void* stream) {
  DV3_REQUIRE(nseg, "curve_fill: nseg is null");
  DV3_REQUIRE(bounds, "curve_fill: bounds is null");
  DV3_REQUIRE(rate, "curve_fill: rate is null");
  DV3_REQUIRE(semitones, "curve_fill: semitones is null");
  DV3_REQUIRE(gain_db, "curve_fill: gain_db is null");
  DV3_REQUIRE(break_frames, "curve_fill: break_frames is null");
  DV3_REQUIRE(o, "curve_fill: o is null");
  DV3_REQUIRE(tlen_out, "curve_fill: tlen_out is null");
  DV3_REQUIRE(pos, "curve_fill: pos is null");
  DV3_REQUIRE(ratio, "curve_fill: ratio is null");
  DV3_REQUIRE(gain, "curve_fill: gain is null");
  DV3_REQUIRE((((uintptr_t)rate | (uintptr_t)semitones | (uintptr_t)gain_db | (uintptr_t)pos | (uintptr_t)ratio) & 7) == 0,
              "curve_fill: rate, semitones, gain_db, pos or ratio is not 8-byte aligned");
  DV3_REQUIRE(B >= 1 && B <= 65535, "curve_fill: B = %d outside [1, 65535]", (int)B);
  DV3_REQUIRE(T_in >= 1, "curve_fill: T_in = %d < 1", (int)T_in);
  DV3_REQUIRE(S >= 1 && S <= DV3_PROSODY_MAX_SEGMENTS, "curve_fill: S = %d outside [1, %d]", (int)S,
              DV3_PROSODY_MAX_SEGMENTS);
  DV3_REQUIRE(T_out >= 1, "curve_fill: T_out = %d < 1", (int)T_out);
  DV3_REQUIRE(ramp_frames >= 0 && ramp_frames <= DV3_PROSODY_MAX_RAMP, "curve_fill: ramp_frames = %d outside [0, %d]",
              (int)ramp_frames, DV3_PROSODY_MAX_RAMP);
  const Segments t = {nseg, bounds, rate, break_frames, (int)S};
  hipLaunchKernelGGL(curve_fill_kernel, dim3((T_out + 255) / 256, B), dim3(256), 0, (hipStream_t)stream, t, (int)B, (int)T_in,
                     tlen_in, semitones, gain_db, o, tlen_out, (int)T_out, (int)ramp_frames, pos, ratio, gain);
  return dv3_check_launch("curve_fill");
}

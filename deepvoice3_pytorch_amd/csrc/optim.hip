// Optimiser tail of the reference train step (train.py:755-759): global-norm gradient clip
// (torch.nn.utils.clip_grad_norm_) + Adam, over ONE flat fp32 parameter arena (all trainable
// parameters are views into it; so are the gradients, which is also what the RCCL all-reduce
// buckets slice).  HBM-bound: 4 reads + 3 writes of 4 B per parameter; 5 + 4 with the moving average of the
// parameters taken in the same pass.  The guarded forms of both passes return before
// the streaming loop when the gradient norm is not finite.
#include "common.h"

namespace {

__global__ __launch_bounds__(256) void sqnorm_partial_kernel(const float* __restrict__ g, int64_t n,
                                                             float* __restrict__ partial) {
  float s = 0.f;
  const int64_t stride = (int64_t)gridDim.x * 256 * 4;
  const int64_t n4 = n & ~(int64_t)3;
  for (int64_t i = ((int64_t)blockIdx.x * 256 + threadIdx.x) * 4; i < n4; i += stride) {
    const f32x4 v = *reinterpret_cast<const f32x4*>(g + i);
    s += v[0] * v[0] + v[1] * v[1] + v[2] * v[2] + v[3] * v[3];
  }
  if (blockIdx.x == 0 && threadIdx.x < (n - n4)) {
    const float v = g[n4 + threadIdx.x];
    s += v * v;
  }
  __shared__ float red[4];
  s = dv3_wave_sum(s);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
  __syncthreads();
  if (threadIdx.x == 0) partial[blockIdx.x] = red[0] + red[1] + red[2] + red[3];
}

// out[0] = sqrt(sum partial)   (out[1] = sum, for cross-rank reduction of squared norms)
__global__ __launch_bounds__(256) void sqnorm_finish_kernel(const float* __restrict__ partial,
                                                            int n_partial, float* __restrict__ out) {
  float s = 0.f;
  for (int i = threadIdx.x; i < n_partial; i += 256) s += partial[i];
  __shared__ float red[4];
  s = dv3_wave_sum(s);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
  __syncthreads();
  if (threadIdx.x == 0) {
    const float t = red[0] + red[1] + red[2] + red[3];
    out[0] = sqrtf(t);
    out[1] = t;
  }
}

// The guard of the guarded passes: s = grad_norm[0] is the same word in every workgroup, so the whole
// grid takes one decision.  Not finite (a NaN / Inf gradient element, or a sum of squares past the fp32 range): true is
// returned and the caller leaves before its streaming loop -- nothing of p, m, v (, ema) is read or written.  Lane 0 of
// block 0 is the single writer of the two health words (plain stores): health[0] counts the skipped passes (fp32, exact
// to 2^24), health[1] is 1 after a skipped pass and 0 after an applied one.
__device__ __forceinline__ bool guard_skips(const float* __restrict__ grad_norm, float* __restrict__ health) {
  const bool skip = (__float_as_uint(grad_norm[0]) & 0x7f800000u) == 0x7f800000u;
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    if (skip) health[0] += 1.0f;
    health[1] = skip ? 1.0f : 0.0f;
  }
  return skip;
}

// hyper = {lr, 1 - beta1^t, sqrt(1 - beta2^t)} on the device (graph-replay friendly).
// GUARD: the guarded pass (dv3_clip_adam_guard_f32); after the early return the code is the unguarded kernel's, so an
// applied step writes the same bits (tests/test_gpu_health.py holds the two together).
template <bool GUARD>
__device__ __forceinline__ void clip_adam_body(float* __restrict__ p, const float* __restrict__ g,
                                               float* __restrict__ m, float* __restrict__ v, int64_t n,
                                               const float* __restrict__ grad_norm, float clip,
                                               const float* __restrict__ hyper, float beta1, float beta2, float eps,
                                               float weight_decay, float grad_prescale, float* __restrict__ health) {
  if (GUARD) {
    if (guard_skips(grad_norm, health)) return;
  }
  float coef = grad_prescale;
  if (clip > 0.f && grad_norm) {
    // clip_grad_norm_: clip_coef = max_norm / (total_norm + 1e-6), clamped to 1
    // grad_norm is the norm of the (summed) arena; the averaged gradient's norm is prescale * that
    const float c = clip / (grad_norm[0] * grad_prescale + 1e-6f);
    coef *= fminf(c, 1.0f);
  }
  const float lr = hyper[0], bc1 = hyper[1], bc2s = hyper[2];
  const float step_size = lr / bc1;
  const int64_t stride = (int64_t)gridDim.x * 256;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += stride) {
    float gi = g[i] * coef;
    const float pi = p[i];
    if (weight_decay != 0.f) gi += weight_decay * pi;
    const float mi = beta1 * m[i] + (1.f - beta1) * gi;
    const float vi = beta2 * v[i] + (1.f - beta2) * gi * gi;
    m[i] = mi;
    v[i] = vi;
    const float denom = sqrtf(vi) / bc2s + eps;
    p[i] = pi - step_size * (mi / denom);
  }
}

__global__ __launch_bounds__(256) void clip_adam_kernel(float* __restrict__ p,
                                                        const float* __restrict__ g,
                                                        float* __restrict__ m, float* __restrict__ v,
                                                        int64_t n, const float* __restrict__ grad_norm,
                                                        float clip, const float* __restrict__ hyper,
                                                        float beta1, float beta2, float eps,
                                                        float weight_decay, float grad_prescale) {
  clip_adam_body<false>(p, g, m, v, n, grad_norm, clip, hyper, beta1, beta2, eps, weight_decay, grad_prescale, nullptr);
}

__global__ __launch_bounds__(256) void clip_adam_guard_kernel(float* __restrict__ p, const float* __restrict__ g,
                                                              float* __restrict__ m, float* __restrict__ v, int64_t n,
                                                              const float* __restrict__ grad_norm, float clip,
                                                              const float* __restrict__ hyper, float beta1, float beta2,
                                                              float eps, float weight_decay, float grad_prescale,
                                                              float* __restrict__ health) {
  clip_adam_body<true>(p, g, m, v, n, grad_norm, clip, hyper, beta1, beta2, eps, weight_decay, grad_prescale, health);
}

// One element of clip_adam_kernel followed by the moving average of the updated parameter, in its increment form
// e += w (p' - e) with w = 1 - decay: at decay 0.9999 the form d e + (1 - d) p' loses the update to rounding much earlier.
// p, m, v must come out bit for bit as clip_adam_kernel writes them.  That kernel leaves the contraction of a * b + c to
// the compiler, and what the compiler fuses depends on how it pairs operations into packed instructions: of the
// expressions copied verbatim into a 16-byte-per-lane body it fused beta2 * v + ..., which it does not in the
// one-element loop.  So contraction is OFF here and the two products clip_adam_kernel is compiled with as fused
// multiply-adds (the clip denominator and the parameter update) are written as such; every other operation is a
// correctly rounded IEEE one in both kernels, whichever instruction carries it.  tests/test_gpu_ema.py holds the two
// kernels together bit for bit.
// w = 0 and w = 1 are taken exactly (e + (p' - e) is p' only while p' - e is exact).
__device__ __forceinline__ void adam_ema_elem(float& p_io, const float g_in, float& m_io, float& v_io, float& e_io,
                                              const float coef, const float step_size, const float bc2s,
                                              const float beta1, const float beta2, const float eps,
                                              const float weight_decay, const float w, const bool w_zero,
                                              const bool w_one) {
#pragma clang fp contract(off)
  float gi = g_in * coef;
  const float pi = p_io;
  if (weight_decay != 0.f) gi += weight_decay * pi;
  const float mi = beta1 * m_io + (1.f - beta1) * gi;
  const float vi = beta2 * v_io + (1.f - beta2) * gi * gi;
  m_io = mi;
  v_io = vi;
  const float denom = sqrtf(vi) / bc2s + eps;
  const float pn = __builtin_fmaf(-step_size, mi / denom, pi);      // pi - step_size * (mi / denom), fused as there
  p_io = pn;
  const float ei = e_io;
  const float en = __builtin_fmaf(w, pn - ei, ei);
  e_io = w_one ? pn : (w_zero ? ei : en);
}

// hyper = {lr, 1 - beta1^t, sqrt(1 - beta2^t), 1 - decay_t} on the device.  5 reads + 4 writes of 4 B per parameter in
// one pass.  Elements [0, n4) move 16 B per lane (n4 a multiple of 4, every pointer 16-byte aligned; the host passes
// n4 = 0 otherwise), elements [n4, n) one at a time.  The gradient, the moments and the average are touched once per
// step and nowhere else before the next one: their 16-byte accesses are non-temporal (measured on the arena of the
// 25.6 M-parameter preset: 140 us against 166 us with plain accesses); the updated parameters, which the
// next forward reads first, are stored plainly (storing them non-temporally too measured slower).
// GUARD: the guarded pass (dv3_clip_adam_ema_guard_f32), as in clip_adam_body.
template <bool GUARD>
__device__ __forceinline__ void clip_adam_ema_body(float* __restrict__ p, const float* __restrict__ g,
                                                   float* __restrict__ m, float* __restrict__ v,
                                                   float* __restrict__ e, int64_t n, int64_t n4,
                                                   const float* __restrict__ grad_norm, float clip,
                                                   const float* __restrict__ hyper, float beta1, float beta2,
                                                   float eps, float weight_decay, float grad_prescale,
                                                   float* __restrict__ health) {
#pragma clang fp contract(off)
  if (GUARD) {
    if (guard_skips(grad_norm, health)) return;
  }
  float coef = grad_prescale;
  if (clip > 0.f && grad_norm) {
    // clip_grad_norm_: clip_coef = max_norm / (total_norm + 1e-6), clamped to 1
    // grad_norm is the norm of the (summed) arena; the averaged gradient's norm is prescale * that
    const float c = clip / __builtin_fmaf(grad_norm[0], grad_prescale, 1e-6f);     // (fused as in clip_adam_kernel)
    coef *= fminf(c, 1.0f);
  }
  const float lr = hyper[0], bc1 = hyper[1], bc2s = hyper[2], w = hyper[3];
  const bool w_zero = !(w > 0.f), w_one = w >= 1.f;
  const float step_size = lr / bc1;
  const int64_t tid = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const int64_t threads = (int64_t)gridDim.x * 256;
  for (int64_t i = tid * 4; i < n4; i += threads * 4) {
    f32x4 pv = __builtin_nontemporal_load(reinterpret_cast<const f32x4*>(p + i));
    const f32x4 gv = __builtin_nontemporal_load(reinterpret_cast<const f32x4*>(g + i));
    f32x4 mv = __builtin_nontemporal_load(reinterpret_cast<const f32x4*>(m + i));
    f32x4 vv = __builtin_nontemporal_load(reinterpret_cast<const f32x4*>(v + i));
    f32x4 ev = __builtin_nontemporal_load(reinterpret_cast<const f32x4*>(e + i));
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      float pk = pv[k], mk = mv[k], vk = vv[k], ek = ev[k];
      adam_ema_elem(pk, gv[k], mk, vk, ek, coef, step_size, bc2s, beta1, beta2, eps, weight_decay, w, w_zero, w_one);
      pv[k] = pk, mv[k] = mk, vv[k] = vk, ev[k] = ek;
    }
    __builtin_nontemporal_store(mv, reinterpret_cast<f32x4*>(m + i));
    __builtin_nontemporal_store(vv, reinterpret_cast<f32x4*>(v + i));
    *reinterpret_cast<f32x4*>(p + i) = pv;
    __builtin_nontemporal_store(ev, reinterpret_cast<f32x4*>(e + i));
  }
  for (int64_t i = n4 + tid; i < n; i += threads) {
    float pk = p[i], mk = m[i], vk = v[i], ek = e[i];
    adam_ema_elem(pk, g[i], mk, vk, ek, coef, step_size, bc2s, beta1, beta2, eps, weight_decay, w, w_zero, w_one);
    p[i] = pk, m[i] = mk, v[i] = vk, e[i] = ek;
  }
}

__global__ __launch_bounds__(256) void clip_adam_ema_kernel(float* __restrict__ p, const float* __restrict__ g,
                                                            float* __restrict__ m, float* __restrict__ v,
                                                            float* __restrict__ e, int64_t n, int64_t n4,
                                                            const float* __restrict__ grad_norm, float clip,
                                                            const float* __restrict__ hyper, float beta1,
                                                            float beta2, float eps, float weight_decay,
                                                            float grad_prescale) {
  clip_adam_ema_body<false>(p, g, m, v, e, n, n4, grad_norm, clip, hyper, beta1, beta2, eps, weight_decay, grad_prescale,
                            nullptr);
}

__global__ __launch_bounds__(256) void clip_adam_ema_guard_kernel(float* __restrict__ p, const float* __restrict__ g,
                                                                  float* __restrict__ m, float* __restrict__ v,
                                                                  float* __restrict__ e, int64_t n, int64_t n4,
                                                                  const float* __restrict__ grad_norm, float clip,
                                                                  const float* __restrict__ hyper, float beta1,
                                                                  float beta2, float eps, float weight_decay,
                                                                  float grad_prescale, float* __restrict__ health) {
  clip_adam_ema_body<true>(p, g, m, v, e, n, n4, grad_norm, clip, hyper, beta1, beta2, eps, weight_decay, grad_prescale,
                           health);
}

// a <-> b in one pass, no third buffer; [0, n4) 16 B per lane, [n4, n) one element at a time (as clip_adam_ema_kernel)
__global__ __launch_bounds__(256) void swap_kernel(float* __restrict__ a, float* __restrict__ b, int64_t n,
                                                   int64_t n4) {
  const int64_t tid = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const int64_t threads = (int64_t)gridDim.x * 256;
  for (int64_t i = tid * 4; i < n4; i += threads * 4) {
    const f32x4 av = *reinterpret_cast<const f32x4*>(a + i);
    const f32x4 bv = *reinterpret_cast<const f32x4*>(b + i);
    *reinterpret_cast<f32x4*>(a + i) = bv;
    *reinterpret_cast<f32x4*>(b + i) = av;
  }
  for (int64_t i = n4 + tid; i < n; i += threads) {
    const float av = a[i], bv = b[i];
    a[i] = bv;
    b[i] = av;
  }
}

// blocks of 256 lanes x 4 elements, at most 2048 of them (8 per CU; the rest of the arena by the grid stride)
static inline unsigned stream_blocks(int64_t n) {
  int64_t nb = dv3_cdiv64(n, 256 * 4);
  return (unsigned)(nb > 2048 ? 2048 : nb);
}

}  // namespace

extern "C" int dv3_grad_sqnorm_f32(const float* g, int64_t n, float* partial, int32_t n_partial,
                                   float* out2, void* stream) {
  DV3_REQUIRE(g && partial && out2 && n > 0 && n_partial > 0, "grad_sqnorm: bad args");
  DV3_REQUIRE(((uintptr_t)g & 15) == 0, "grad_sqnorm: gradient arena must be 16-byte aligned");
  hipStream_t st = (hipStream_t)stream;
  int nb = (int)dv3_cdiv64(n, 256 * 4 * 8);
  if (nb < 1) nb = 1;
  if (nb > n_partial) nb = n_partial;
  hipLaunchKernelGGL(sqnorm_partial_kernel, dim3(nb), dim3(256), 0, st, g, n, partial);
  hipLaunchKernelGGL(sqnorm_finish_kernel, dim3(1), dim3(256), 0, st, partial, nb, out2);
  return dv3_check_launch("grad_sqnorm_f32");
}

extern "C" int dv3_clip_adam_f32(float* p, const float* g, float* m, float* v, int64_t n,
                                 const float* grad_norm, float clip, const float* hyper, float beta1,
                                 float beta2, float eps, float weight_decay, float grad_prescale,
                                 void* stream) {
  DV3_REQUIRE(p && g && m && v && hyper && n > 0, "clip_adam: bad args");
  int64_t nb = dv3_cdiv64(n, 256 * 4);
  if (nb > 4096) nb = 4096;
  hipLaunchKernelGGL(clip_adam_kernel, dim3((unsigned)nb), dim3(256), 0, (hipStream_t)stream, p, g, m,
                     v, n, grad_norm, clip, hyper, beta1, beta2, eps, weight_decay, grad_prescale);
  return dv3_check_launch("clip_adam_f32");
}

extern "C" int dv3_clip_adam_ema_f32(float* p, const float* g, float* m, float* v, float* ema, int64_t n,
                                     const float* grad_norm, float clip, const float* hyper, float beta1,
                                     float beta2, float eps, float weight_decay, float grad_prescale,
                                     void* stream) {
  DV3_REQUIRE(p && g && m && v && ema && hyper && n > 0, "clip_adam_ema: bad args");
  DV3_REQUIRE(ema + n <= p || p + n <= ema, "clip_adam_ema: the average overlaps the parameters");
  // 16 B per lane where every buffer allows it (arena slices do); a view that is not 16-byte aligned goes one element
  // at a time through the same kernel
  const uintptr_t bits = (uintptr_t)p | (uintptr_t)g | (uintptr_t)m | (uintptr_t)v | (uintptr_t)ema;
  const int64_t n4 = (bits & 15) == 0 ? (n & ~(int64_t)3) : 0;
  hipLaunchKernelGGL(clip_adam_ema_kernel, dim3(stream_blocks(n)), dim3(256), 0, (hipStream_t)stream, p, g, m, v,
                     ema, n, n4, grad_norm, clip, hyper, beta1, beta2, eps, weight_decay, grad_prescale);
  return dv3_check_launch("clip_adam_ema_f32");
}

// The guarded passes (include/dv3hip.h): the launch geometry of their unguarded forms.
extern "C" int dv3_clip_adam_guard_f32(float* p, const float* g, float* m, float* v, int64_t n,
                                       const float* grad_norm, float clip, const float* hyper, float beta1,
                                       float beta2, float eps, float weight_decay, float grad_prescale,
                                       float* health, void* stream) {
  DV3_REQUIRE(p && g && m && v && hyper && n > 0, "clip_adam_guard: bad args");
  DV3_REQUIRE(grad_norm && health, "clip_adam_guard: the gradient norm and the health words are mandatory");
  int64_t nb = dv3_cdiv64(n, 256 * 4);
  if (nb > 4096) nb = 4096;
  hipLaunchKernelGGL(clip_adam_guard_kernel, dim3((unsigned)nb), dim3(256), 0, (hipStream_t)stream, p, g, m, v, n,
                     grad_norm, clip, hyper, beta1, beta2, eps, weight_decay, grad_prescale, health);
  return dv3_check_launch("clip_adam_guard_f32");
}

extern "C" int dv3_clip_adam_ema_guard_f32(float* p, const float* g, float* m, float* v, float* ema, int64_t n,
                                           const float* grad_norm, float clip, const float* hyper, float beta1,
                                           float beta2, float eps, float weight_decay, float grad_prescale,
                                           float* health, void* stream) {
  DV3_REQUIRE(p && g && m && v && ema && hyper && n > 0, "clip_adam_ema_guard: bad args");
  DV3_REQUIRE(grad_norm && health, "clip_adam_ema_guard: the gradient norm and the health words are mandatory");
  DV3_REQUIRE(ema + n <= p || p + n <= ema, "clip_adam_ema_guard: the average overlaps the parameters");
  const uintptr_t bits = (uintptr_t)p | (uintptr_t)g | (uintptr_t)m | (uintptr_t)v | (uintptr_t)ema;
  const int64_t n4 = (bits & 15) == 0 ? (n & ~(int64_t)3) : 0;
  hipLaunchKernelGGL(clip_adam_ema_guard_kernel, dim3(stream_blocks(n)), dim3(256), 0, (hipStream_t)stream, p, g, m, v,
                     ema, n, n4, grad_norm, clip, hyper, beta1, beta2, eps, weight_decay, grad_prescale, health);
  return dv3_check_launch("clip_adam_ema_guard_f32");
}

extern "C" int dv3_swap_f32(float* a, float* b, int64_t n, void* stream) {
  DV3_REQUIRE(a && b && n > 0, "swap: bad args");
  DV3_REQUIRE(a + n <= b || b + n <= a, "swap: the two buffers are the same or overlap");
  const int64_t n4 = ((((uintptr_t)a | (uintptr_t)b) & 15) == 0) ? (n & ~(int64_t)3) : 0;
  hipLaunchKernelGGL(swap_kernel, dim3(stream_blocks(n)), dim3(256), 0, (hipStream_t)stream, a, b, n, n4);
  return dv3_check_launch("swap_f32");
}

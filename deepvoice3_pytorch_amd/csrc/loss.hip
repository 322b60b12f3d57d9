// Fused loss value + gradient kernels for the reference train step
// (train.py:261-291 sequence_mask/MaskedL1Loss, :537-582 logit/masked_mean/spec_loss,
//  :585-601 guided_attention(s), :614,:714 BCELoss, :733-740 attention loss).
// All are HBM-bound single passes: read prediction + target once, write the gradient once,
// block partial sums -> deterministic second-stage reduce (no float atomics).
#include "common.h"

namespace {

constexpr int kLossBlock = 256;

// what the spectrogram kernels take: the caller's descriptor and the loss head's two pointers (dv3_spec_loss_head_f32)
struct spec_loss_args : dv3_spec_loss_desc {
  float* dpre; float* bias_part;
};

// extra (or null) also receives the block's sum of v[1]: the done head's bias partial (bce_kernel)
__device__ __forceinline__ void block_reduce4(float v[4], float* out /* [4] per block */, float* extra = nullptr) {
  __shared__ float red[4][4];
#pragma unroll
  for (int k = 0; k < 4; ++k) v[k] = dv3_wave_sum(v[k]);
  const int w = threadIdx.x >> 6;
  if ((threadIdx.x & 63) == 0) {
#pragma unroll
    for (int k = 0; k < 4; ++k) red[w][k] = v[k];
  }
  __syncthreads();
  if (threadIdx.x < 4) {
    const float sum = red[0][threadIdx.x] + red[1][threadIdx.x] + red[2][threadIdx.x] + red[3][threadIdx.x];
    out[threadIdx.x] = sum;
    if (extra && threadIdx.x == 1) extra[0] = sum;
  }
}

// Loss head (dv3_spec_loss_head_f32): the gradient through the sigmoid that made y_hat,
// dz = (dyh * alpha) * y_hat * (1 - y_hat) with alpha = 1 -- the three products in the order of gate_bwd_kernel's
// DV3_EPI_SIGMOID branch (elementwise.hip), so the bits are those of dv3_spec_loss_f32(dyh) followed by dv3_gate_bwd_f32.
__device__ __forceinline__ float sigmoid_head_dz(float dyh, float yh) {
  const float d = dyh * 1.0f;
  return d * yh * (1.0f - yh);
}

// binary divergence of one element and its derivative (train.py:537-556):
//   L = logit(y_hat) = log(y_hat + eps) - log(1 - y_hat + eps),  z = -y L + log1p(exp(L)),  dz/dy_hat = (sigmoid(L) - y) L'
// With a = y_hat + eps, b = 1 - y_hat + eps:  exp(L) = a / b,  log1p(exp(L)) = log(a + b) - log(b),
// sigmoid(L) = a / (a + b): two logarithms and two reciprocals instead of four transcendental calls -- the loss kernels
// were VALU-bound on them (round 2: 145 us per launch whatever the access pattern).  a + b = 1 + 2 eps.
// FAST (the tiled kernel, default; DV3_SW_LOSS_FAST_LOG = 0: libm): the three logarithms by v_log_f32 (__logf: 1 ulp of
// log2 x, i.e. ~1e-7 absolute here) -- with logf the tiled kernel was still bound by its vector work (~100 instructions per
// element; 103 us for the 64 x 804 x 513 linear-spectrogram loss, round 6).  The gradient takes no logarithm.
template <bool FAST = false>
__device__ __forceinline__ void spec_bd(float yh, float y, float& z, float& dz) {
  const float eps = 1e-8f;
  const float a = yh + eps, b = 1.f - yh + eps;
  constexpr float LN2 = 0.69314718055994530942f;
  const float la = FAST ? __builtin_amdgcn_logf(a) * LN2 : logf(a), lb = FAST ? __builtin_amdgcn_logf(b) * LN2 : logf(b);
  const float ab = a + b;
  z = -y * (la - lb) + ((FAST ? __builtin_amdgcn_logf(ab) * LN2 : logf(ab)) - lb);
  const float ra = __builtin_amdgcn_rcpf(a), rb = __builtin_amdgcn_rcpf(b);
  dz = (a * __builtin_amdgcn_rcpf(ab) - y) * (ra + rb);
}

// frames that take part (ABI 42, dv3_spec_loss_desc.t_valid): the batch's own maximum when the tensors are padded further
__device__ __forceinline__ int spec_t_valid(const dv3_spec_loss_desc& p) {
  if (!p.t_valid) return p.T;
  const int tv = p.t_valid[0];
  return tv < p.T ? (tv > p.r ? tv : p.r + 1) : p.T;
}

// mask_sum as train.py:286-290 computes it: sum over the expanded (B, T-r, D) mask
__device__ __forceinline__ float spec_mask_sum(const dv3_spec_loss_desc& p) {
  float ms = 0.f;
  const int Tr = spec_t_valid(p) - p.r;
  for (int b = 0; b < p.B; ++b) {
    int l = p.lengths[b] - p.r;
    l = l < 0 ? 0 : (l > Tr ? Tr : l);
    ms += (float)l;
  }
  return ms * (float)p.D;
}

__global__ __launch_bounds__(kLossBlock) void spec_loss_kernel(const spec_loss_args p) {
  const int Tr = p.T - p.r, D = p.D;
  const int Trv = spec_t_valid(p) - p.r;       // == Tr unless the batch is padded beyond its own maximum
  const int64_t n = (int64_t)p.B * Tr * D;
  const bool use_mask = p.w_masked > 0.f && p.lengths;
  const float msum = use_mask ? spec_mask_sum(p) : 1.f;
  const float inv_n = 1.0f / (float)((int64_t)p.B * Trv * D);
  const float wm = use_mask ? p.w_masked : 0.f;
  const float c_all = (1.f - wm) * inv_n, c_msk = use_mask ? wm / msum : 0.f;
  float acc[4] = {0.f, 0.f, 0.f, 0.f};  // l1, l1 masked, z, z masked
  const int64_t stride = (int64_t)gridDim.x * kLossBlock;
  // iterate with the faster-varying axis of y_hat innermost so its accesses coalesce
  const bool t_fast = p.yh_ts < p.yh_ds;
  for (int64_t i = (int64_t)blockIdx.x * kLossBlock + threadIdx.x; i < n; i += stride) {
    int dd, t, b;
    if (t_fast) {
      t = (int)(i % Tr);
      const int64_t bd = i / Tr;
      dd = (int)(bd % D);
      b = (int)(bd / D);
    } else {
      dd = (int)(i % D);
      const int64_t bt = i / D;
      t = (int)(bt % Tr);
      b = (int)(bt / Tr);
    }
    const int64_t ih = b * p.yh_bs + t * p.yh_ts + dd * p.yh_ds;          // y_hat[:, :-r]
    const int64_t iy = b * p.y_bs + (int64_t)(t + p.r) * p.y_ts + dd * p.y_ds;  // y[:, r:]
    if (t >= Trv) {
      if (p.dyh) p.dyh[ih] = 0.f;
      if (p.dpre) p.dpre[ih] = 0.f;
      continue;
    }
    const float yh = p.y_hat[ih], y = p.y[iy];
    const float m = (use_mask && (t + p.r) < p.lengths[b]) ? 1.f : 0.f;
    const float diff = yh - y;
    const float ad = fabsf(diff);
    acc[0] += ad;
    acc[1] += m * ad;
    float dz = 0.f;
    if (p.w_bd > 0.f) {
      float z;
      spec_bd(yh, y, z, dz);
      acc[2] += z;
      acc[3] += m * z;
    }
    if (p.dyh || p.dpre) {
      const float sgn = (diff > 0.f) ? 1.f : ((diff < 0.f) ? -1.f : 0.f);
      const float coef = c_all + c_msk * m;
      const float g = p.gscale * coef * ((1.f - p.w_bd) * sgn + p.w_bd * dz);
      if (p.dyh) p.dyh[ih] = g;
      if (p.dpre) p.dpre[ih] = sigmoid_head_dz(g, yh);
    }
  }
  if (p.dpre) {   // the last r frames take no part: dz = 0 from this launch (no spec_loss_tail_zero_kernel in this form)
    const int64_t nz = (int64_t)p.B * p.r * D;
    for (int64_t i = (int64_t)blockIdx.x * kLossBlock + threadIdx.x; i < nz; i += stride) {
      const int dd = (int)(i % D);
      const int64_t bt = i / D;
      const int64_t ih = (bt / p.r) * p.yh_bs + (Tr + (bt % p.r)) * p.yh_ts + dd * p.yh_ds;
      p.dpre[ih] = 0.f;
      if (p.dyh) p.dyh[ih] = 0.f;
    }
  }
  block_reduce4(acc, p.scratch + (int64_t)blockIdx.x * 4);
}

// Row sums of dz for the layouts of spec_loss_kernel.  Its flat element walk (which the bits of out4 hang on) has no
// per-bin structure, so the sums are taken from dz by a second, small launch: one thread per (item, 64-frame tile, bin)
// adds its 64 frames in a fixed order -> bias_part[bin][item * t_tiles + tile], the layout the tiled kernel writes.
__global__ __launch_bounds__(256) void spec_head_rowsum_kernel(const spec_loss_args p, int t_tiles) {
  const int64_t n = (int64_t)p.B * t_tiles * p.D;
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const int dd = (int)(i % p.D);
  const int64_t bt = i / p.D;
  const int tt = (int)(bt % t_tiles), b = (int)(bt / t_tiles);
  const int t1 = min(tt * 64 + 64, p.T - p.r);
  float s[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};     // eight interleaved chains, joined pairwise
  for (int t = tt * 64; t < t1; ++t) s[t & 7] += p.dpre[b * p.yh_bs + t * p.yh_ts + dd * p.yh_ds];
  p.bias_part[(int64_t)dd * ((int64_t)p.B * t_tiles) + bt] = ((s[0] + s[1]) + (s[2] + s[3])) + ((s[4] + s[5]) + (s[6] + s[7]));
}

// The same loss when the prediction is time-fastest (the model's (B, T, D) outputs are transposed views of its BCT
// tensors) and the target is bin-fastest (collate_fn's (B, T, D) arrays): either thread order leaves one of the two
// tensors read with a D- or T-element stride (round 2: ~1 TB/s, 300 us for the linear-spectrogram loss).  A workgroup
// takes 64 frames x 64 bins at a time: the target tile is read bin-fastest into LDS, then every thread works
// frame-fastest -- prediction read, gradient write and the LDS reads (row stride 65) are all unit-stride.  Persistent
// grid (tiles are walked with a grid stride) so that the block partial sums fit the caller's scratch.
// A thread's frame within the tile is fixed (tid & 63) and its bins are tid >> 6, + 4, ...: the frame tests, the mask
// and the gradient's coefficient are taken once per tile, the element loop keeps the loads, the arithmetic of spec_bd
// and the stores, and it ends at the tile's last valid bin (D % 64 == 1: the last bin tile costs one bin, not 64).  The
// elements a thread adds up, and their order, are those of the flat walk q = tid, tid + 256, ... this replaces: out4
// keeps its bits.  (16 bytes per lane would hand a thread four neighbouring frames -- another assignment of elements to
// partial sums, so another out4: left out.)
// HEAD (dpre set, dv3_spec_loss_head_f32): dz = dyh * y_hat * (1 - y_hat) is written too (dyh itself only if set), the last r frames
// get dz = 0 from the threads of the item's last frame tile, and with bias_part the tile's dz goes back into the LDS
// slot its target came from: thread (bin = tid >> 2, quarter = tid & 3) adds 16 frames pairwise, two row-local
// shuffles finish -> bias_part[bin][item * t_tiles + tile].  No atomics; the sums do not depend on the grid.
template <bool FAST, bool HEAD>
__global__ __launch_bounds__(kLossBlock) void spec_loss_tiled_kernel(const spec_loss_args p, int t_tiles, int d_tiles,
                                                                     int n_tiles) {
  __shared__ float ys[64 * 65];
  const int Tr = p.T - p.r, D = p.D;
  const int Trv = spec_t_valid(p) - p.r;
  const bool use_mask = p.w_masked > 0.f && p.lengths;
  const float msum = use_mask ? spec_mask_sum(p) : 1.f;
  const float inv_n = 1.0f / (float)((int64_t)p.B * Trv * D);
  const float wm = use_mask ? p.w_masked : 0.f;
  const float c_all = (1.f - wm) * inv_n, c_msk = use_mask ? wm / msum : 0.f;
  float acc[4] = {0.f, 0.f, 0.f, 0.f};
  const int tid = threadIdx.x;
  const int tl = tid & 63, dw = tid >> 6;
  const bool sums = HEAD && p.bias_part != nullptr;
  const int64_t n_part = (int64_t)p.B * t_tiles;
  // A tile's 16 + 16 values per thread are loaded one tile AHEAD, all at once: with 4 loads in flight per thread between
  // two barriers, and the grid held at 1024 workgroups by the block partial sums (four waves per SIMD), the kernel ran
  // at the bytes it had in flight, 1.8 TB/s with its vector units a third busy.
  float tg[16], yv[16];          // target: rows dw + 4k of the tile, column tl; prediction: frame tl, bins dw + 4k
  auto fetch = [&](int tile) {
    const int dt = tile % d_tiles, tt_ = (tile / d_tiles) % t_tiles, b = tile / (d_tiles * t_tiles);
    const int t0 = tt_ * 64, d0 = dt * 64;
    const int dd = d0 + tl;
    const float* __restrict__ yp = p.y + b * p.y_bs + (int64_t)(t0 + dw + p.r) * p.y_ts + dd;
#pragma unroll
    for (int k = 0; k < 16; ++k) tg[k] = (t0 + dw + 4 * k < Tr && dd < D) ? yp[(int64_t)(4 * k) * p.y_ts] : 0.f;
    const int t = t0 + tl;
    const float* __restrict__ hp = p.y_hat + b * p.yh_bs + t + (int64_t)(d0 + dw) * p.yh_ds;
#pragma unroll
    for (int k = 0; k < 16; ++k) yv[k] = (t < Trv && d0 + dw + 4 * k < D) ? hp[(int64_t)(4 * k) * p.yh_ds] : 0.f;
  };
  if ((int)blockIdx.x < n_tiles) fetch(blockIdx.x);
  for (int tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
    const int dt = tile % d_tiles, tt_ = (tile / d_tiles) % t_tiles, b = tile / (d_tiles * t_tiles);
    const int t0 = tt_ * 64, d0 = dt * 64;
    const int nd = min(64, D - d0);
    __syncthreads();                                   // the previous tile's LDS reads are done
#pragma unroll
    for (int k = 0; k < 16; ++k) ys[(dw + 4 * k) * 65 + tl] = tg[k];   // target tile, bin-fastest: y[b][t0 + row + r][d0 + col]
    float yc[16];
#pragma unroll
    for (int k = 0; k < 16; ++k) yc[k] = yv[k];
    if (tile + (int)gridDim.x < n_tiles) fetch(tile + gridDim.x);
    __syncthreads();
    const int len_b = use_mask ? p.lengths[b] : 0;
    const int t = t0 + tl;                             // frame-fastest
    const float m = (use_mask && (t + p.r) < len_b) ? 1.f : 0.f;
    const float coef = c_all + c_msk * m;
    const int64_t ih0 = b * p.yh_bs + t + (int64_t)(d0 + dw) * p.yh_ds;
    const int64_t ihs = 4 * p.yh_ds;
    if (t < Trv) {
#pragma unroll
      for (int k = 0; k < 16; ++k) {
        const int dl = dw + 4 * k;
        if (dl >= nd) break;
        const int64_t ih = ih0 + k * ihs;
        const float yh = yc[k], y = ys[tl * 65 + dl];
        const float diff = yh - y;
        const float ad = fabsf(diff);
        acc[0] += ad;
        acc[1] += m * ad;
        float dz = 0.f;
        if (p.w_bd > 0.f) {
          float z;
          spec_bd<FAST>(yh, y, z, dz);
          acc[2] += z;
          acc[3] += m * z;
        }
        if (p.dyh || HEAD) {
          const float sgn = (diff > 0.f) ? 1.f : ((diff < 0.f) ? -1.f : 0.f);
          const float g = p.gscale * coef * ((1.f - p.w_bd) * sgn + p.w_bd * dz);
          if (p.dyh) p.dyh[ih] = g;
          if (HEAD) {
            const float gz = sigmoid_head_dz(g, yh);
            p.dpre[ih] = gz;
            if (sums) ys[tl * 65 + dl] = gz;
          }
        }
      }
    } else {
      if (t < Tr) {                                    // beyond the batch's own frames (t_valid): zero gradient
        int64_t ih = ih0;
        for (int dl = dw; dl < nd; dl += 4, ih += ihs) {
          if (p.dyh) p.dyh[ih] = 0.f;
          if (HEAD) p.dpre[ih] = 0.f;
        }
      }
      if (sums)
        for (int dl = dw; dl < nd; dl += 4) ys[tl * 65 + dl] = 0.f;
    }
    if (HEAD && tt_ == t_tiles - 1) {                  // the last r frames
      for (int tz = Tr + tl; tz < p.T; tz += 64) {
        int64_t ih = b * p.yh_bs + tz + (int64_t)(d0 + dw) * p.yh_ds;
        for (int dl = dw; dl < nd; dl += 4, ih += ihs) {
          p.dpre[ih] = 0.f;
          if (p.dyh) p.dyh[ih] = 0.f;
        }
      }
    }
    if (sums) {
      __syncthreads();
      const int bin = tid >> 2, part = tid & 3;
      float v[16];                                     // pairwise, as the row sums of gate_bwd_kernel's wave reduce are
#pragma unroll
      for (int i = 0; i < 16; ++i) v[i] = ys[(part * 16 + i) * 65 + bin];
#pragma unroll
      for (int w = 1; w < 16; w <<= 1)
#pragma unroll
        for (int i = 0; i < 16; i += 2 * w) v[i] += v[i + w];
      float s = v[0];
      s += __shfl_xor(s, 1, 4);
      s += __shfl_xor(s, 2, 4);
      if (part == 0 && bin < nd) p.bias_part[(int64_t)(d0 + bin) * n_part + (int64_t)b * t_tiles + tt_] = s;
    }
  }
  block_reduce4(acc, p.scratch + (int64_t)blockIdx.x * 4);
}

// the last r frames of y_hat take no part in the loss: their gradient is zero
__global__ __launch_bounds__(256) void spec_loss_tail_zero_kernel(const dv3_spec_loss_desc p) {
  const int64_t n = (int64_t)p.B * p.r * p.D;
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const int dd = (int)(i % p.D);
  const int64_t bt = i / p.D;
  const int t = p.T - p.r + (int)(bt % p.r);
  const int b = (int)(bt / p.r);
  p.dyh[b * p.yh_bs + t * p.yh_ts + dd * p.yh_ds] = 0.f;
}

__global__ __launch_bounds__(256) void spec_loss_finish_kernel(const dv3_spec_loss_desc p,
                                                               int n_blocks) {
  float acc[4] = {0.f, 0.f, 0.f, 0.f};
  for (int i = threadIdx.x; i < n_blocks; i += 256)
#pragma unroll
    for (int k = 0; k < 4; ++k) acc[k] += p.scratch[(int64_t)i * 4 + k];
  __shared__ float fin[4];
  block_reduce4(acc, fin);
  __syncthreads();
  if (threadIdx.x == 0) {
    const bool use_mask = p.w_masked > 0.f && p.lengths;
    const float msum = use_mask ? spec_mask_sum(p) : 1.f;
    const float n = (float)((int64_t)p.B * (spec_t_valid(p) - p.r) * p.D);
    const float wm = use_mask ? p.w_masked : 0.f;
    const float l1 = wm * (use_mask ? fin[1] / msum : 0.f) + (1.f - wm) * fin[0] / n;
    const float bd = p.w_bd > 0.f ? wm * (use_mask ? fin[3] / msum : 0.f) + (1.f - wm) * fin[2] / n : 0.f;
    p.out4[0] = l1;
    p.out4[1] = bd;
    p.out4[2] = (1.f - p.w_bd) * l1 + p.w_bd * bd;
    p.out4[3] = msum;
  }
}

// ---- guided attention ---------------------------------------------------------------------
// W[t][n] of an item with N keys and T decoder steps; train.py:585-591 evaluates this in float64 and stores float32
__device__ __forceinline__ float guided_w(int nk, int t, int N, int T, double inv2g2) {
  const double dlt = (double)nk / (double)N - (double)t / (double)T;
  return (float)(1.0 - exp(-dlt * dlt * inv2g2));
}

__global__ __launch_bounds__(256) void guided_attn_kernel(const float* __restrict__ attn,
                                                          const int32_t* __restrict__ in_len,
                                                          const int32_t* __restrict__ out_len,
                                                          float* __restrict__ dattn,
                                                          float* __restrict__ scratch, int L, int B,
                                                          int Tq, int Tk, float g, float gscale,
                                                          const int32_t* __restrict__ tq_valid,
                                                          const int32_t* __restrict__ tk_valid) {
  const int64_t per = (int64_t)B * Tq * Tk;
  // the mean's element count: the tensor's, or (ABI 42) that of the batch's own maxima
  const int64_t n = tq_valid ? (int64_t)L * B * min(tq_valid[0], Tq) * min(tk_valid[0], Tk) : per * L;
  const float inv_n = 1.0f / (float)n;
  const double inv2g2 = 1.0 / (2.0 * (double)g * (double)g);
  float acc[4] = {0.f, 0.f, 0.f, 0.f};
  const int64_t stride = (int64_t)gridDim.x * 256;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < per; i += stride) {
    const int nk = (int)(i % Tk);
    const int64_t bt = i / Tk;
    const int t = (int)(bt % Tq), b = (int)(bt / Tq);
    const int N = in_len[b], T = out_len[b];
    const float w = (nk < N && t < T) ? guided_w(nk, t, N, T, inv2g2) : 0.f;
    for (int l = 0; l < L; ++l) {
      acc[0] += attn[(int64_t)l * per + i] * w;
      if (dattn) dattn[(int64_t)l * per + i] = gscale * w * inv_n;
    }
  }
  block_reduce4(acc, scratch + (int64_t)blockIdx.x * 4);
}

// out1 = (sum of the block partial sums) * scale; with va (and vb) the scale is 1 / (count * min(va[0], cap_a) [* min(vb[0], cap_b)])
__global__ __launch_bounds__(256) void sum_finish_kernel(const float* __restrict__ scratch,
                                                         int n_blocks, float scale,
                                                         float* __restrict__ out1,
                                                         const int32_t* __restrict__ va = nullptr, int cap_a = 0,
                                                         const int32_t* __restrict__ vb = nullptr, int cap_b = 0,
                                                         int64_t count = 0) {
  float acc[4] = {0.f, 0.f, 0.f, 0.f};
  for (int i = threadIdx.x; i < n_blocks; i += 256) acc[0] += scratch[(int64_t)i * 4];
  __shared__ float fin[4];
  block_reduce4(acc, fin);
  __syncthreads();
  if (threadIdx.x == 0) {
    if (va) {
      int64_t n = count * min(va[0], cap_a);
      if (vb) n *= min(vb[0], cap_b);
      scale = 1.0f / (float)n;
    }
    out1[0] = fin[0] * scale;
  }
}

// ---- BCE (nn.BCELoss, mean; log clamped at -100 as torch does) ------------------------------
__device__ __forceinline__ float bce_elem(float x, float y) {
  const float lx = fmaxf(logf(x), -100.f), l1x = fmaxf(logf(1.f - x), -100.f);
  return -(y * lx + (1.f - y) * l1x);
}

__global__ __launch_bounds__(256) void bce_kernel(const float* __restrict__ p,
                                                  const float* __restrict__ t,
                                                  float* __restrict__ dp, float* __restrict__ scratch,
                                                  int64_t n, float gscale, int T = 0,
                                                  const int32_t* __restrict__ t_valid = nullptr,
                                                  float* __restrict__ dpre = nullptr,
                                                  float* __restrict__ bias_part = nullptr) {
  float acc[4] = {0.f, 0.f, 0.f, 0.f};   // loss terms; dz (loss head)
  // ABI 42: [rows][T] with only the first t_valid[0] columns taking part
  const int Tv = t_valid ? min(t_valid[0], T) : T;
  const float inv_n = 1.0f / (float)(t_valid ? (n / T) * Tv : n);
  const int64_t stride = (int64_t)gridDim.x * 256;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += stride) {
    if (t_valid && (int)(i % T) >= Tv) {
      if (dp) dp[i] = 0.f;
      if (dpre) dpre[i] = 0.f;
      continue;
    }
    const float x = p[i], y = t[i];
    acc[0] += bce_elem(x, y);
    if (dp || dpre) {
      const float g = gscale * inv_n * (x - y) / fmaxf((1.f - x) * x, 1e-12f);
      if (dp) dp[i] = g;
      if (dpre) {        // loss head (dv3_spec_loss_head_f32): through the sigmoid that made p, as sigmoid_head_dz
        const float gz = sigmoid_head_dz(g, x);
        dpre[i] = gz;
        acc[1] += gz;
      }
    }
  }
  block_reduce4(acc, scratch + (int64_t)blockIdx.x * 4, bias_part ? bias_part + blockIdx.x : nullptr);
}


// ---- per-item sums (held-out evaluation: train_step.Trainer.evaluate) -------------------------
// Forward only, one fp32 row per batch item: the masked sums the batch kernels above fold into one mean, kept apart per
// item, of the SAME fp32 terms (spec_bd, bce_elem, guided_w).  Grid = (slices, items): the item's OWN frames are cut
// into gridDim.x equal slices, so a long item is spread over as many workgroups as a short one and no workgroup walks
// padding.  Slice partial sums go to scratch[(b * slices + s) * 4], the finishing pass adds them in slice order.
constexpr int kItemSliceFrames = 64, kItemMaxSlices = 64;

inline int item_slices(int T) {
  const int s = dv3_cdiv(T, kItemSliceFrames);
  return s < 1 ? 1 : (s > kItemMaxSlices ? kItemMaxSlices : s);
}

__device__ __forceinline__ int clamp_len(int l, int cap) { return l < 0 ? 0 : (l > cap ? cap : l); }

// frames [t0, t1) of this workgroup's slice of an item with n frames
__device__ __forceinline__ void item_slice(int n, int& t0, int& t1) {
  const int per = (n + (int)gridDim.x - 1) / (int)gridDim.x;
  t0 = min((int)blockIdx.x * per, n);
  t1 = min(t0 + per, n);
}

// {sum |y_hat - y|, sum z} over the item's frames t < lengths[b] - r (the batch kernels' mask, (t + r) < lengths[b])
template <bool FAST>
__global__ __launch_bounds__(kLossBlock) void spec_items_kernel(const dv3_spec_items_desc p) {
  const int b = blockIdx.y, D = p.D;
  int t0, t1;
  item_slice(clamp_len(p.lengths[b] - p.r, p.T - p.r), t0, t1);
  const int nt = t1 - t0;
  const int n = nt * D;                 // (the launcher refuses shapes whose slices hold 2^31 elements)
  float acc[4] = {0.f, 0.f, 0.f, 0.f};  // l1, z
  // the faster-varying axis of y_hat innermost, as spec_loss_kernel: with a time-fastest prediction the bin-fastest
  // target is read at a D-element stride (the pattern the batch path left for its tiled kernel; cost: DESIGN.md 3.7a)
  const bool t_fast = p.yh_ts < p.yh_ds;
  for (int i = threadIdx.x; i < n; i += kLossBlock) {
    int dd, t;
    if (t_fast) {
      t = t0 + i % nt;
      dd = i / nt;
    } else {
      dd = i % D;
      t = t0 + i / D;
    }
    const float yh = p.y_hat[b * p.yh_bs + t * p.yh_ts + dd * p.yh_ds];
    const float y = p.y[b * p.y_bs + (int64_t)(t + p.r) * p.y_ts + dd * p.y_ds];
    const float diff = yh - y;
    acc[0] += fabsf(diff);
    float z, dz;
    spec_bd<FAST>(yh, y, z, dz);
    acc[1] += z;
  }
  block_reduce4(acc, p.scratch + ((int64_t)b * gridDim.x + blockIdx.x) * 4);
}

__global__ __launch_bounds__(256) void bce_items_kernel(const float* __restrict__ p, const float* __restrict__ t,
                                                        const int32_t* __restrict__ lengths,
                                                        float* __restrict__ scratch, int T) {
  const int b = blockIdx.y;
  int t0, t1;
  item_slice(clamp_len(lengths[b], T), t0, t1);
  float acc[4] = {0.f, 0.f, 0.f, 0.f};
  for (int i = t0 + threadIdx.x; i < t1; i += 256) acc[0] += bce_elem(p[(int64_t)b * T + i], t[(int64_t)b * T + i]);
  block_reduce4(acc, scratch + ((int64_t)b * gridDim.x + blockIdx.x) * 4);
}

__global__ __launch_bounds__(256) void guided_attn_items_kernel(const float* __restrict__ attn,
                                                                const int32_t* __restrict__ in_len,
                                                                const int32_t* __restrict__ out_len,
                                                                float* __restrict__ scratch, int L, int B, int Tq,
                                                                int Tk, float g) {
  const int b = blockIdx.y;
  const int N = in_len[b], T = out_len[b];
  const int Nc = clamp_len(N, Tk);            // the item's own keys and decoder steps, inside the tensor
  int t0, t1;
  item_slice(clamp_len(T, Tq), t0, t1);
  const int n = (t1 - t0) * Nc;
  const int64_t per = (int64_t)B * Tq * Tk;
  const double inv2g2 = 1.0 / (2.0 * (double)g * (double)g);
  float acc[4] = {0.f, 0.f, 0.f, 0.f};
  for (int i = threadIdx.x; i < n; i += 256) {
    const int nk = i % Nc, t = t0 + i / Nc;
    const float w = guided_w(nk, t, N, T, inv2g2);
    const int64_t at = ((int64_t)b * Tq + t) * Tk + nk;
    for (int l = 0; l < L; ++l) acc[0] += attn[(int64_t)l * per + at] * w;
  }
  block_reduce4(acc, scratch + ((int64_t)b * gridDim.x + blockIdx.x) * 4);
}

// out[b] = {the first n_sums slice sums of item b, added in slice order; its element count}, one thread per item.
// count = mult * clamp(len_a[b] - sub_a, 0, cap_a) [* clamp(len_b[b], 0, cap_b)]
__global__ __launch_bounds__(256) void items_finish_kernel(const float* __restrict__ scratch, int B, int slices,
                                                           int n_sums, float* __restrict__ out,
                                                           const int32_t* __restrict__ len_a, int sub_a, int cap_a,
                                                           const int32_t* __restrict__ len_b, int cap_b,
                                                           int64_t mult) {
  const int b = blockIdx.x * 256 + threadIdx.x;
  if (b >= B) return;
  float acc[2] = {0.f, 0.f};
  for (int s = 0; s < slices; ++s)
    for (int k = 0; k < n_sums; ++k) acc[k] += scratch[((int64_t)b * slices + s) * 4 + k];
  int64_t cnt = mult * clamp_len(len_a[b] - sub_a, cap_a);
  if (len_b) cnt *= clamp_len(len_b[b], cap_b);
  float* row = out + (int64_t)b * (n_sums + 1);
  for (int k = 0; k < n_sums; ++k) row[k] = acc[k];
  row[n_sums] = (float)cnt;         // exact up to 2^24 elements per item (include/dv3hip.h)
}

// the layouts the tiled spectrogram kernel serves (time-fastest prediction, bin-fastest target); the per-item kernel
// takes its logarithms the way the batch kernel of the same layouts does
template <class Desc>
inline bool spec_time_fast(const Desc& d) {
  return d.yh_ts == 1 && d.y_ds == 1 && d.yh_ds > 1 && d.y_ts > 1 && (int64_t)d.B * d.yh_bs < (1ll << 40);
}

inline int loss_blocks(int64_t n) {
  int64_t b = dv3_cdiv64(n, (int64_t)kLossBlock * 4);
  if (b < 1) b = 1;
  if (b > 1024) b = 1024;
  return (int)b;
}

}  // namespace

// DV3_SW_LOSS_FAST_LOG: the tiled spectrogram loss takes its logarithms by v_log_f32 (0 = logf)

extern "C" int dv3_spec_loss_scratch_floats(int32_t B, int32_t T, int32_t D) {
  // block partial sums of either form: the flat grid, or one block per 64 x 64 tile (at most 1024)
  int64_t tiles = (int64_t)B * dv3_cdiv(T, 64) * dv3_cdiv(D, 64);
  if (tiles > 1024) tiles = 1024;
  const int64_t flat = loss_blocks((int64_t)B * T * D);
  return (int)(4 * (tiles > flat ? tiles : flat) + 16);
}

static int spec_loss_launch(const dv3_spec_loss_desc* d, float* dpre, float* bias_part, void* stream) {
  DV3_REQUIRE(d && d->y_hat && d->y && d->out4 && d->scratch, "spec_loss: null pointer");
  DV3_REQUIRE(d->B > 0 && d->D > 0 && d->r >= 0 && d->T > d->r, "spec_loss: bad dims");
  DV3_REQUIRE(d->w_masked <= 0.f || d->lengths, "spec_loss: masked weight needs lengths");
  hipStream_t st = (hipStream_t)stream;
  spec_loss_args a;
  static_cast<dv3_spec_loss_desc&>(a) = *d;
  a.dpre = dpre;
  a.bias_part = bias_part;
  const int64_t n = (int64_t)d->B * (d->T - d->r) * d->D;
  int nb = loss_blocks(n);
  if (spec_time_fast(*d)) {
    // time-fastest prediction against a bin-fastest target: the tiled form
    const int t_tiles = dv3_cdiv(d->T - d->r, 64), d_tiles = dv3_cdiv(d->D, 64);
    const int64_t nt = (int64_t)d->B * t_tiles * d_tiles;
    nb = (int)(nt < 1024 ? nt : 1024);
    const bool fast_log = dv3_sw(DV3_SW_LOSS_FAST_LOG);
    auto k = dpre ? (fast_log ? spec_loss_tiled_kernel<true, true> : spec_loss_tiled_kernel<false, true>)
                     : (fast_log ? spec_loss_tiled_kernel<true, false> : spec_loss_tiled_kernel<false, false>);
    hipLaunchKernelGGL(k, dim3(nb), dim3(kLossBlock), 0, st, a, t_tiles, d_tiles, (int)nt);
  } else {
    hipLaunchKernelGGL(spec_loss_kernel, dim3(nb), dim3(kLossBlock), 0, st, a);
    if (dpre && bias_part) {
      const int t_tiles = dv3_cdiv(d->T - d->r, 64);
      const int64_t ns = (int64_t)d->B * t_tiles * d->D;
      hipLaunchKernelGGL(spec_head_rowsum_kernel, dim3((unsigned)dv3_cdiv64(ns, 256)), dim3(256), 0, st, a, t_tiles);
    }
  }
  if (d->dyh && !dpre && d->r > 0) {
    const int64_t nt = (int64_t)d->B * d->r * d->D;
    hipLaunchKernelGGL(spec_loss_tail_zero_kernel, dim3((unsigned)dv3_cdiv64(nt, 256)), dim3(256), 0,
                       st, *d);
  }
  hipLaunchKernelGGL(spec_loss_finish_kernel, dim3(1), dim3(256), 0, st, *d, nb);
  return dv3_check_launch("spec_loss_f32");
}

extern "C" int dv3_spec_loss_f32(const dv3_spec_loss_desc* d, void* stream) {
  return spec_loss_launch(d, nullptr, nullptr, stream);
}

extern "C" int dv3_spec_loss_head_f32(const dv3_spec_loss_desc* d, float* dpre, float* bias_part, void* stream) {
  DV3_REQUIRE(dpre, "spec_loss_head: dpre is required");
  return spec_loss_launch(d, dpre, bias_part, stream);
}

extern "C" int dv3_guided_attn_loss_f32(const float* attn, const int32_t* in_len,
                                        const int32_t* out_len, float* dattn, float* out1,
                                        float* scratch, int32_t L, int32_t B, int32_t Tq, int32_t Tk,
                                        float g, float gscale, void* stream) {
  DV3_REQUIRE(attn && in_len && out_len && out1 && scratch, "guided_attn: null pointer");
  DV3_REQUIRE(L > 0 && B > 0 && Tq > 0 && Tk > 0 && g > 0.f, "guided_attn: bad dims");
  hipStream_t st = (hipStream_t)stream;
  const int64_t per = (int64_t)B * Tq * Tk;
  const int nb = loss_blocks(per);
  hipLaunchKernelGGL(guided_attn_kernel, dim3(nb), dim3(256), 0, st, attn, in_len, out_len, dattn,
                     scratch, L, B, Tq, Tk, g, gscale, (const int32_t*)nullptr, (const int32_t*)nullptr);
  hipLaunchKernelGGL(sum_finish_kernel, dim3(1), dim3(256), 0, st, scratch, nb,
                     1.0f / (float)(per * L), out1, (const int32_t*)nullptr, 0, (const int32_t*)nullptr, 0, (int64_t)0);
  return dv3_check_launch("guided_attn_loss_f32");
}

extern "C" int dv3_guided_attn_loss_valid_f32(const float* attn, const int32_t* in_len, const int32_t* out_len,
                                              float* dattn, float* out1, float* scratch, int32_t L, int32_t B,
                                              int32_t Tq, int32_t Tk, float g, float gscale,
                                              const int32_t* tq_valid, const int32_t* tk_valid, void* stream) {
  DV3_REQUIRE(attn && in_len && out_len && out1 && scratch && tq_valid && tk_valid, "guided_attn_valid: null pointer");
  DV3_REQUIRE(L > 0 && B > 0 && Tq > 0 && Tk > 0 && g > 0.f, "guided_attn_valid: bad dims");
  hipStream_t st = (hipStream_t)stream;
  const int64_t per = (int64_t)B * Tq * Tk;
  const int nb = loss_blocks(per);
  hipLaunchKernelGGL(guided_attn_kernel, dim3(nb), dim3(256), 0, st, attn, in_len, out_len, dattn,
                     scratch, L, B, Tq, Tk, g, gscale, tq_valid, tk_valid);
  hipLaunchKernelGGL(sum_finish_kernel, dim3(1), dim3(256), 0, st, scratch, nb, 0.f, out1, tq_valid, (int)Tq, tk_valid,
                     (int)Tk, (int64_t)L * B);
  return dv3_check_launch("guided_attn_loss_valid_f32");
}

extern "C" int dv3_bce_loss_f32(const float* p, const float* t, float* dp, float* out1,
                                float* scratch, int64_t n, float gscale, void* stream) {
  DV3_REQUIRE(p && t && out1 && scratch && n > 0, "bce_loss: bad args");
  hipStream_t st = (hipStream_t)stream;
  const int nb = loss_blocks(n);
  hipLaunchKernelGGL(bce_kernel, dim3(nb), dim3(256), 0, st, p, t, dp, scratch, n, gscale, 0, (const int32_t*)nullptr);
  hipLaunchKernelGGL(sum_finish_kernel, dim3(1), dim3(256), 0, st, scratch, nb, 1.0f / (float)n, out1,
                     (const int32_t*)nullptr, 0, (const int32_t*)nullptr, 0, (int64_t)0);
  return dv3_check_launch("bce_loss_f32");
}

extern "C" int dv3_bce_loss_valid_f32(const float* p, const float* t, float* dp, float* out1, float* scratch,
                                      int64_t rows, int32_t T, const int32_t* t_valid, float gscale, void* stream) {
  DV3_REQUIRE(p && t && out1 && scratch && t_valid && rows > 0 && T > 0, "bce_loss_valid: bad args");
  hipStream_t st = (hipStream_t)stream;
  const int64_t n = rows * T;
  const int nb = loss_blocks(n);
  hipLaunchKernelGGL(bce_kernel, dim3(nb), dim3(256), 0, st, p, t, dp, scratch, n, gscale, (int)T, t_valid);
  hipLaunchKernelGGL(sum_finish_kernel, dim3(1), dim3(256), 0, st, scratch, nb, 0.f, out1, t_valid, (int)T,
                     (const int32_t*)nullptr, 0, rows);
  return dv3_check_launch("bce_loss_valid_f32");
}

extern "C" int dv3_bce_loss_head_parts(int64_t n) { return n > 0 ? loss_blocks(n) : 0; }

extern "C" int dv3_bce_loss_head_f32(const float* p, const float* t, float* dp, float* dpre, float* bias_part, float* out1,
                                     float* scratch, int64_t rows, int32_t T, const int32_t* t_valid, float gscale,
                                     void* stream) {
  DV3_REQUIRE(p && t && dpre && out1 && scratch && rows > 0 && T > 0, "bce_loss_head: bad args");
  hipStream_t st = (hipStream_t)stream;
  const int64_t n = rows * T;
  const int nb = loss_blocks(n);
  if (t_valid) {
    hipLaunchKernelGGL(bce_kernel, dim3(nb), dim3(256), 0, st, p, t, dp, scratch, n, gscale, (int)T, t_valid, dpre, bias_part);
    hipLaunchKernelGGL(sum_finish_kernel, dim3(1), dim3(256), 0, st, scratch, nb, 0.f, out1, t_valid, (int)T,
                       (const int32_t*)nullptr, 0, rows);
  } else {
    hipLaunchKernelGGL(bce_kernel, dim3(nb), dim3(256), 0, st, p, t, dp, scratch, n, gscale, 0, (const int32_t*)nullptr, dpre,
                       bias_part);
    hipLaunchKernelGGL(sum_finish_kernel, dim3(1), dim3(256), 0, st, scratch, nb, 1.0f / (float)n, out1,
                       (const int32_t*)nullptr, 0, (const int32_t*)nullptr, 0, (int64_t)0);
  }
  return dv3_check_launch("bce_loss_head_f32");
}

// ---- per-item sums ------------------------------------------------------------------------------
extern "C" int dv3_loss_items_scratch_floats(int32_t B, int32_t T) {
  if (B <= 0 || T <= 0) return 0;
  return (int)((int64_t)4 * B * item_slices(T));
}

extern "C" int dv3_spec_loss_items_f32(const dv3_spec_items_desc* d, void* stream) {
  DV3_REQUIRE(d && d->y_hat && d->y && d->lengths && d->out && d->scratch, "spec_loss_items: null pointer");
  DV3_REQUIRE(d->B > 0 && d->B <= 65535 && d->D > 0 && d->r >= 0 && d->T > 0, "spec_loss_items: bad dims");
  hipStream_t st = (hipStream_t)stream;
  const int Tr = d->T > d->r ? d->T - d->r : 0;      // no frame takes part in a tensor of r frames or fewer: rows of zeros
  const int S = Tr > 0 ? item_slices(Tr) : 0;
  if (S > 0) {
    DV3_REQUIRE((int64_t)dv3_cdiv(Tr, S) * d->D < (1ll << 31), "spec_loss_items: slice too large");
    if (spec_time_fast(*d) && dv3_sw(DV3_SW_LOSS_FAST_LOG))
      hipLaunchKernelGGL(spec_items_kernel<true>, dim3(S, d->B), dim3(kLossBlock), 0, st, *d);
    else
      hipLaunchKernelGGL(spec_items_kernel<false>, dim3(S, d->B), dim3(kLossBlock), 0, st, *d);
  }
  hipLaunchKernelGGL(items_finish_kernel, dim3(dv3_cdiv(d->B, 256)), dim3(256), 0, st, (const float*)d->scratch, (int)d->B,
                     S, 2, d->out, d->lengths, (int)d->r, Tr, (const int32_t*)nullptr, 0, (int64_t)d->D);
  return dv3_check_launch("spec_loss_items_f32");
}

extern "C" int dv3_bce_loss_items_f32(const float* p, const float* t, const int32_t* lengths, float* out,
                                      float* scratch, int32_t B, int32_t T, void* stream) {
  DV3_REQUIRE(p && t && lengths && out && scratch, "bce_loss_items: null pointer");
  DV3_REQUIRE(B > 0 && B <= 65535 && T > 0, "bce_loss_items: bad dims");
  hipStream_t st = (hipStream_t)stream;
  const int S = item_slices(T);
  hipLaunchKernelGGL(bce_items_kernel, dim3(S, B), dim3(256), 0, st, p, t, lengths, scratch, (int)T);
  hipLaunchKernelGGL(items_finish_kernel, dim3(dv3_cdiv(B, 256)), dim3(256), 0, st, (const float*)scratch, (int)B, S, 1,
                     out, lengths, 0, (int)T, (const int32_t*)nullptr, 0, (int64_t)1);
  return dv3_check_launch("bce_loss_items_f32");
}

extern "C" int dv3_guided_attn_loss_items_f32(const float* attn, const int32_t* in_len, const int32_t* out_len,
                                              float* out, float* scratch, int32_t L, int32_t B, int32_t Tq,
                                              int32_t Tk, float g, void* stream) {
  DV3_REQUIRE(attn && in_len && out_len && out && scratch, "guided_attn_items: null pointer");
  DV3_REQUIRE(L > 0 && B > 0 && B <= 65535 && Tq > 0 && Tk > 0 && g > 0.f, "guided_attn_items: bad dims");
  hipStream_t st = (hipStream_t)stream;
  const int S = item_slices(Tq);
  DV3_REQUIRE((int64_t)dv3_cdiv(Tq, S) * Tk < (1ll << 31), "guided_attn_items: slice too large");
  hipLaunchKernelGGL(guided_attn_items_kernel, dim3(S, B), dim3(256), 0, st, attn, in_len, out_len, scratch, (int)L,
                     (int)B, (int)Tq, (int)Tk, g);
  hipLaunchKernelGGL(items_finish_kernel, dim3(dv3_cdiv(B, 256)), dim3(256), 0, st, (const float*)scratch, (int)B, S, 1,
                     out, out_len, 0, (int)Tq, in_len, (int)Tk, (int64_t)L);
  return dv3_check_launch("guided_attn_loss_items_f32");
}

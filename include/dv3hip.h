/*
 * dv3hip.h -- C ABI of the MI355X (gfx950) DeepVoice3 hot-path library (libdv3hip.so).
 *
 * The reference (r9y9/deepvoice3_pytorch) has no FFI: its hot path is stock torch ops
 * called from Python modules.  This header is the boundary a maintainer would bind
 * (ctypes) to replace those torch calls; every entry point cites
 * the reference lines it stands in for (paths relative to the reference repo root).
 *
 * Conventions
 *  - plain C: device pointers + sizes only, no torch types.  All tensors are fp32
 *    unless a name says otherwise; "BCT" = (batch, channel, time), time contiguous --
 *    the layout the reference conv stacks use (deepvoice3_pytorch/modules.py:139-164).
 *  - every call enqueues on `stream` (a hipStream_t passed as void*), never syncs,
 *    never allocates, never frees, retains no pointer after returning.
 *  - return value: 0 on success, a negative DV3_E* code otherwise;
 *    dv3_last_error() returns a thread-local message for the last failure.
 *  - strides are in ELEMENTS.  "bs" = batch stride, "rs" = row (channel) stride.
 */
#ifndef DV3HIP_H
#define DV3HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define DV3_OK 0
#define DV3_EINVAL (-1)   /* bad argument / unsupported shape */
#define DV3_ELAUNCH (-2)  /* hipLaunch / runtime error        */

/* ABI version, bumped on any struct change; checked by the Python loader. */
#define DV3_ABI_VERSION 50
int dv3_abi_version(void);
const char* dv3_last_error(void);
/* Fills name (<=255 chars) of device `dev`, number of CUs; returns 0/err. */
int dv3_device_info(int dev, char* name, int name_len, int* n_cu);
/* sizeof(struct <name>) or -1: lets a foreign-language mirror of the descriptors self-check */
int dv3_sizeof(const char* name);
/*
 * Run-time switches of the library's dispatchers: THE list.  One row per switch --
 *   X(id, NAME, default, lowest, highest accepted value, "meaning")
 * -- from which the DV3_SW_* ids below, the library's storage and defaults, the checks of dv3_debug_set and the Python
 * side's table (_lib.SWITCHES) are all generated.  The ids are ABI: a retired id is never reused.  The defaults are
 * what the benchmark times; the other forms exist so that tests can route a small shape to the kernel form the large
 * shapes get, or keep an earlier form as a bit-identity reference.  Where each rule was measured: the comment beside
 * the dispatcher that reads the switch, and INTEGRATION.md, section 2.
 */
#define DV3_SWITCHES(X) \
  X(2, WGRAD_TILE, 0, 0, 4, "split weight gradient: 0 by rule / 1 128x128 per tap / 2 256x128 per tap / 3 all-taps / 4 two-steps-ahead all-taps") \
  X(3, X3_PINGPONG, 1, 0, 1, "8-wave split tap-GEMM tiles: 0 in-phase / 1 ping-pong main loop") \
  X(4, PLANES_TILE, 0, 0, 9, "planes tap-GEMM tile: 0 by rule, conv_c8pp first / 1 128x128 / 2 128x64 / 9 128x256; any other value: by rule, conv_c8pp kept out") \
  X(12, X3_PP2_MIN_TILES, 128, 0, 2147483647, "256x256 split tap-GEMM serves eligible grids of at least this many tiles (0 never)") \
  X(14, X3_PRIO, 0, 0, 4, "wave priority scheme of the ping-pong split main loop (kernel argument; 0 none)") \
  X(15, WGRAD_PRIO, 0, 0, 2, "wave priority scheme of the all-taps weight gradient (kernel argument; 0 none)") \
  X(17, WGRAD_TAPS2, 1, 0, 1, "all-taps weight gradient by rule: 0 one step ahead / 1 two steps ahead") \
  X(18, X3_WIDE, 1, 0, 1, "16-byte input-gradient epilogue through LDS of the split tap-GEMMs (kernel argument): 0 off / 1 on") \
  X(19, C8PP_MIN_TILES, 128, 0, 2147483647, "conv_c8pp serves eligible grids of at least this many tiles (0 never, 1 always)") \
  X(20, WGRAD_C8_PF2, 1, 0, 1, "register-transposing wgrad_c8: operands fetched 0 one / 1 two steps ahead") \
  X(22, PP2_SK, 1, 0, 3, "stream-K form of the 256x256 split tap-GEMM: 0 never / 1 by rule, forward / 2 whenever a workspace is given / 3 by rule, both directions") \
  X(29, PP2_ORD_U, 81, 0, 81, "LOAD-phase order of the unmasked 256x256 split instantiations: 0, 17 or 81 only") \
  X(30, C8PP_RF, 1, 0, 1, "conv_c8pp LOAD phase: 0 staging first / 1 fragment reads first") \
  X(31, PP2_ORD_M, 81, 0, 81, "LOAD-phase order of the masked 256x256 split instantiations: 0, 17 or 81 only") \
  X(34, C8PP_NW4, 2, 0, 2, "conv_c8pp form: 0 8 waves on 256x256 only / 1 two 4-wave workgroups per CU on 256x128 / 2 by rule") \
  X(35, C8PP_STAGGER, 0, 0, 1024, "conv_c8pp, 4-wave form: start delay (x 64 cycles) of the delayed blocks (kernel argument)") \
  X(36, C8PP_STAGGER_MASK, 1, 0, 2147483647, "conv_c8pp, 4-wave form: blocks with (blockIdx & mask) != 0 are the delayed ones (kernel argument)") \
  X(44, X3_KS, 1, 0, 2, "k-split form of the 128x64 split tile: 0 never / 1 by rule / 2 wherever eligible") \
  X(47, WGRAD_T2_WINDOW, 1, 0, 1, "two-steps-ahead weight gradient, d = 1 / 3: 0 per-tap form / 1 one window for three taps") \
  X(48, WGRAD_T2_IL, 1, 0, 1, "its window forms stage the next tile 0 after / 1 between the MFMAs") \
  X(49, WGRAD_C8_IL, 1, 0, 1, "register-transposing wgrad_c8, three taps: next tile staged 0 after / 1 between the MFMAs") \
  X(50, PP2_FAST_TAIL, 1, 0, 1, "256x256 split tap-GEMM, gated launch: 0 guarded tail everywhere / 1 straight-line tail on interior sub-tiles (kernel argument)") \
  X(51, WN_BWD_VEC4, 1, 0, 1, "weight-norm backward gather: 0 4-byte everywhere / 1 16-byte where aligned") \
  X(52, WGRAD_C8_TR, 4, 0, 4, "wgrad_c8 form: 0 register-transposing / 1 transposing LDS read / 2 + staging between the MFMAs / 3 + one barrier per two K steps / 4 both") \
  X(54, SPK_PREFETCH, 1, 0, 1, "speaker-bias backward tile loads: 0 at the top of the tile / 1 one tile ahead") \
  X(55, GATE_VEC, 1, 0, 1, "gate backward 16-byte accesses: 0 gated layers with T % 4 == 0 only / 1 rows of any length") \
  X(56, GATE_C8_FAST, 1, 0, 1, "c8 gate backward sigmoid: 0 expf and a division / 1 v_exp_f32 + v_rcp_f32") \
  X(57, LOSS_FAST_LOG, 1, 0, 1, "tiled spectrogram loss logarithms: 0 logf / 1 v_log_f32")
#define DV3_SW_ENUM_(id, name, dflt, lo, hi, doc) DV3_SW_##name = id,
enum { DV3_SWITCHES(DV3_SW_ENUM_) };
/* Sets switch `what` (a DV3_SW_* id) of this process.  DV3_EINVAL, with a dv3_last_error() message that starts
 * "debug_set(<what>, <value>): ", for an id that is not in the list -- "no such switch": the retired ids 1, 5-9, 13, 16,
 * 21, 23-28, 32, 42, 43, 45, 46 among them, so that a stale script cannot time the shipped kernel believing it timed
 * something else -- and for a value outside the row's range (29 / 31: outside {0, 17, 81}); the stored value is then
 * unchanged.  Not in the list: what = DV3_DEBUG_CENSUS, the launch census of dv3_conv_gemm_f32 (1 = clear and record /
 * 0 = stop). */
#define DV3_DEBUG_CENSUS 40
int dv3_debug_set(int what, int value);
/* Every switch of the list back to its default.  The launch census is not touched. */
int dv3_debug_reset(void);
/* *value = the switch's current value, *dflt = its default (either may be NULL).  DV3_EINVAL for an id not in the list. */
int dv3_switch_query(int what, int32_t* value, int32_t* dflt);
/* what = 3: phase stamps of the persistent decode program.  what = 40 / 41: the launch census -- the recorded dv3_conv_desc
 * structs (bytes <= count * sizeof(dv3_conv_desc)) / the kernel variant (int32 each, encoded as dv3_debug_get(10))
 * that served each; count = dv3_debug_get(40).  Any other what: DV3_EINVAL. */
int dv3_debug_read(int what, void* dst, int64_t bytes);
/* what = 10: which kernel the LAST dv3_conv_gemm_f32 call of this process launched, encoded
 * family * 1000 + tile_id * 10 + pingpong; family 1 = exact-fp32 streaming kernel, 2 = exact-fp32
 * LDS-staged kernel, 3 = split-bf16 (3 MFMAs per product), 4 = bf16 (1 MFMA per product); tile ids as
 * dv3_conv_desc.tile_hint (9 = the 8-wave 128x256 tile); + 2 on the 128x64 split tile = its k-split form.  what = 11: same for dv3_wgrad_gemm_f32
 * (family 1 = exact fp32, 3 = split-bf16, 4 = bf16; tile 1 = 128x128, 2 = 256x128).  Tests use it to
 * assert that a shape was served by the kernel the benchmark times.  Returns the value (>= 0). */
int dv3_debug_get(int what);

/* Measurement stand-in for an n-rank RCCL ring all-reduce on ONE GPU (csrc/standin.hip; dist.RingStandin): `channels`
 * persistent workgroups of `threads` (256 | 512) threads copy `bytes` (= 2 (n-1)/n x the bucket) from `src` (read only,
 * wrapped) into `scratch` (wrapped) at `bytes_per_us` for all workgroups together (the links' pace, kept by spinning on
 * the 100 MHz wall clock).  Reduces nothing.  Not on the product path.                                            */
int dv3_ring_standin(const void* src, int64_t src_bytes, void* scratch, int64_t scratch_bytes, int64_t bytes,
                     int32_t channels, int32_t threads, float bytes_per_us, void* stream);

/* ------------------------------------------------------------------------------------
 * Epilogue modes of the tap-GEMM (dv3_conv_gemm_f32).
 * ------------------------------------------------------------------------------------ */
enum {
  DV3_EPI_LINEAR = 0,  /* y = acc + bias                      1x1 Conv1d / Linear          */
  DV3_EPI_RELU = 1,    /* y = relu(acc + bias)                Conv1d + nn.ReLU             */
  DV3_EPI_SIGMOID = 2, /* y = sigmoid(acc + bias)             last 1x1 + torch.sigmoid     */
  DV3_EPI_GLU = 3,     /* Conv1dGLU:  modules.py:157-164                                   */
  DV3_EPI_HIGHWAY = 4, /* HighwayConv1d: modules.py:224-226                                */
  DV3_EPI_DGRAD = 5,   /* y = acc * dropmask(y-site) + addend   (input-gradient pass)      */
  DV3_EPI_SOFTSIGN = 6 /* y = v/(1+|v|), v = acc + bias       F.softsign(Linear(spk))      */
};
/* LINEAR/RELU/SIGMOID/SOFTSIGN: after the activation, if r  != NULL: y = (y + r ) * sqrt(.5)
 *                                               then if r2 != NULL: y = (y + r2) * sqrt(.5)
 * (AttentionLayer's `(x + residual) * sqrt(0.5)`, deepvoice3.py:175, and the decoder's outer
 *  residual, deepvoice3.py:348-349).                                                      */

enum {
  DV3_STORE_BCT = 0,       /* y[b][m][n]                                                   */
  DV3_STORE_INTERLEAVE2 = 1 /* y[b][m % Mo][2n + m / Mo], Mo = M/2: ConvTranspose1d k2 s2  */
};

/*
 * dv3_conv_gemm_f32 -- the hot kernel.  im2col-free dilated 1-D convolution as a tap-GEMM
 * on the fp32 matrix cores (v_mfma_f32_32x32x2_f32), with the whole Conv1dGLU / HighwayConv1d
 * tail fused in the epilogue.
 *
 *   acc[b][m][n] = sum_{j<J} sum_{c<Cin} A[b][j][c][m] * xd[b][c][n + j*dil - padL]
 *   xd = x * bit(xmask) * drop_scale      (bit==1 everywhere when xmask == NULL)
 *
 * Replaces, per mode (reference file:line):
 *   GLU      F.dropout -> conv -> trim -> split -> (+softsign speaker bias) -> a*sigmoid(b)
 *            -> (x+residual)*sqrt(.5)                   deepvoice3_pytorch/modules.py:145-164
 *   HIGHWAY  same conv, T=sigmoid(b); T*a+(1-T)*x       deepvoice3_pytorch/modules.py:205-226
 *   LINEAR/RELU/SIGMOID  1x1 convs and Linear layers    deepvoice3.py:51-54,65-67,227-229,
 *            262-264,360-363,517,565-567,578,604; nyanko.py:29-31,96-100,133,149-156,365-398
 *   INTERLEAVE2 store     nn.ConvTranspose1d(k=2,s=2)   deepvoice3.py:519-520,527-528
 *   per-batch A (a_bs!=0) torch.bmm(q, keys)            deepvoice3.py:143
 *   DGRAD    input gradient of all of the above (autograd of F.conv1d + F.dropout)
 *
 * A is the PACKED weight: [J][Cin][lda], m contiguous, produced by dv3_weight_norm_pack_f32.
 * For GLU/HIGHWAY the m axis holds the `a` half in [0,Cg) and the gate half at [a_half,
 * a_half+Cg); M must equal 2*Cg and the output has Cg channels.
 *
 * PLACEMENT of the tensors (tests/test_gpu_gemm_footprint.py pins every line; strides are in elements):
 *   fp32 x, r, r2, y     any 4-byte aligned base, any row stride rs >= the row length (T; 2 T for y of the interleaved
 *                        store), any batch stride bs that keeps the rows apart: views into larger buffers are fine.
 *                        The kernels WRITE the logical elements only -- never a row gap, a batch gap or a word before /
 *                        behind the tensor -- and nothing that lies outside the logical elements of an input reaches
 *                        a value (loads past a tensor's edge are clamped into it).  The 16-byte epilogues are taken
 *                        when base % 16 == 0, rs % 4 == 0, bs % 4 == 0 (and Tout % 4 == 0); they give the same bits as
 *                        the 4-byte ones, except in the summation order of pg_part.
 *   a with a_bs != 0     (an activation as the packed operand) any 4-byte aligned base and lda; staged element by
 *                        element unless base % 16 == 0 and lda, a_half, a_bs are multiples of 4
 *   ab, pg, dpg, dpg_res, pg_part    DENSE: [B][M][Tout] / [B][2M][Tout] / [2M][n_part] contiguous, no stride fields;
 *                        pg_x has strides like x
 *   xmask, ymask         rows of xmask_rs / ymask_rs >= ceil(T / 32) words, the row index dense ([B * Cin] / [B * M]);
 *                        words beyond ceil(T / 32) of a row are never used
 *   c8 tensors           16-byte aligned and contiguous; padding channels zero on entry, kept zero
 */
typedef struct dv3_conv_desc {
  const float* x;  int64_t x_bs, x_rs;      /* input  [B][Cin][Tin]                         */
  const float* a;  int64_t a_bs; int32_t lda; int32_t a_half; /* packed weights            */
  const float* bias;                         /* [M] (reference order) or NULL               */
  const float* spk; int64_t spk_bs, spk_rs, spk_ts; /* additive on the `a` half (GLU) or NULL */
  const float* r;  int64_t r_bs, r_rs;       /* residual / highway input / DGRAD addend     */
  const float* r2; int64_t r2_bs, r2_rs;     /* second residual (non-gated modes) or NULL   */
  float* y;        int64_t y_bs, y_rs;       /* output                                      */
  float* ab;                                 /* optional save of pre-gate (a,b): [B][M][Tout] */
  const uint32_t* xmask; int32_t xmask_rs;   /* dropout keep-bits over x rows [B*Cin][rs]   */
  const uint32_t* ymask; int32_t ymask_rs;   /* DGRAD: keep-bits over y rows [B*M][rs]      */
  float drop_scale;                          /* 1/(1-p)                                     */
  int32_t B, Cin, Tin, M, Cg, Tout, J, dil, padL;
  int32_t mode, residual, store_mode;
  int32_t tile_hint;                         /* 0 = auto; else forces a tile config (tests) */
  const uint16_t* a_split;                   /* split-bf16 image of `a` (dv3_split_pack_bf16) or
                                                NULL.  Non-NULL selects the bf16x3 kernel (below) */
  int32_t split_terms;                       /* 0 or 3: hi/lo bf16 split, three MFMAs per product;
                                                1: hi planes only = plain bf16 MFMA with fp32 accumulate
                                                (BASELINE.json bf16 configs); DV3_SPLIT_F16X3 (19): `a_split`
                                                is a SCALED FP16 hi/lo image (below), the activations are
                                                split the same way while staging: three fp16 MFMAs per
                                                product, 2^-22-class operands = fp32-class results      */
  const uint16_t* x_c8;                      /* the input as a c8 bf16 tensor [B][x_c8p][Tin][8] (below), written by
                                                dv3_to_c8_f32 or a c8 epilogue, or NULL.  Non-NULL requires a_split
                                                and split_terms == 1 (anything else is DV3_EINVAL) and selects the
                                                single-term bf16 kernels on c8 tensors (conv_c8pp, conv_planes):
                                                both operands are staged with plain 16-byte copies.
                                                `x` may then be NULL unless the epilogue reads it as `r`.     */
  int32_t x_c8p;                             /* 8-channel blocks per batch item in x_c8 (= round_up(Cin,32)/8) */
  float r_scale;                             /* DGRAD: y = acc * dropmask + r_scale * r (0 means 1).  The gradient
                                                that reaches a residual Conv1dGLU's input through the skip path is
                                                sqrt(.5) * dy: the epilogue reads dy itself instead of a scaled copy */
  int32_t io_bf16;                           /* bf16 STORAGE (BASELINE configs 3/4: "bf16 activations ... fp32 accum"),
                                                single-term bf16 kernels (split_terms == 1) only: DV3_IO_IN_BF16 = x, r
                                                and r2 are bf16 tensors (same element strides), DV3_IO_OUT_BF16 = y and
                                                ab are written as bf16 (round to nearest even).  0 = fp32 everywhere.  */
  const uint8_t* xmask_c8;                   /* c8 input (x_c8): dropout keep-BYTES [B][x_c8p][Tin],
                                                bit e of byte (b, g, t) = keep channel 8g+e at frame t
                                                (dv3_mask_bits_to_c8); applied while staging, 1/(1-p) = drop_scale in
                                                the epilogue.  NULL = no dropout.                                     */
  const uint8_t* ymask_c8;                   /* DGRAD with DV3_IO_OUT_C8: keep-bytes over the output rows            */
  void* sk_ws;                               /* optional stream-K workspace (dv3_conv_streamk_ws_bytes() bytes, its first
                                                4 KiB zero before the first launch that uses it; the launches leave them
                                                zero).  With it the 256 x 256 tap-GEMM kernels may run as ONE workgroup
                                                per CU over equal shares of (tile, 32-channel chunk) units instead of one
                                                tile per workgroup -- for grids that do not divide the CUs (152 tiles, 808
                                                tiles ...).  Launches that share a workspace must be ordered (same
                                                stream).  NULL = one tile per workgroup.  Results differ between the
                                                two forms by fp32 summation order only.                              */
  int64_t sk_ws_bytes;
  /* ---- round 6: the producer's gate backward inside the input-gradient tail (split kernels, DV3_EPI_DGRAD) ----------
   * The output y of an input-gradient launch is dL/d(out) of the layer that PRODUCED this layer's input.  When that
   * producer is a Conv1dGLU / HighwayConv1d whose output has no other consumer, its gate backward (autograd of
   * modules.py:157-164, 224-226; stand-alone: dv3_gate_bwd_f32) runs here, on the tile the tail already holds:
   *   pg       the producer's saved pre-gate pair [B][2M][Tout] (its `ab`), fp32; NULL = plain tail
   *   pg_x     HIGHWAY: the producer's input [B][M][Tout] (pg_x_bs / pg_x_rs element strides)
   *   dpg      out: the producer's pre-gate gradient [B][2M][Tout] (what gate_bwd writes as `dab`)
   *   dpg_res  out, HIGHWAY: the gradient of its skip path [B][M][Tout] (`dres`); GLU: the skip gradient is
   *            sqrt(.5) * y, which the producer's own DGRAD launch reads through r / r_scale as before
   *   pg_part  out: bias partial sums, TRANSPOSED [2M][n_part], n_part = ceil(B * Tout / 32): entry (row, k) = the sum
   *            of dpg[row] over the flat (b, t) columns [32 k, 32 k + 32) -- deterministic, summed by
   *            dv3_weight_norm_bwd_f32 (bias_part_t = 1)
   *   pg_mode  DV3_EPI_GLU or DV3_EPI_HIGHWAY; pg_residual as the producer's `residual`
   *   pg_pair  1: dpg is written as PAIR WORDS (below) instead of fp32
   * y itself is written as always (it is the gradient autograd is handed).
   * PAIR WORDS: a 32-bit word (bf16_rn(v) << 16) | bf16_rn(v - bf16_rn(v)) in the place of the fp32 value v -- the two
   * bf16 operands the gradient GEMMs (this entry point in DGRAD form, dv3_wgrad_gemm_f32) would otherwise build from v
   * while staging, computed once by the producer of the tensor.  Same shape, strides and bytes as the fp32 tensor.
   *   x_pair   1: x holds pair words (split_terms == 3 or 0 with a_split: the bf16-pair kernels; no xmask)        */
  const float* pg; const float* pg_x; int64_t pg_x_bs, pg_x_rs;
  float* dpg; float* dpg_res; float* pg_part;
  int32_t pg_mode, pg_residual, pg_pair, x_pair;
} dv3_conv_desc;
#define DV3_IO_IN_BF16 1
#define DV3_IO_OUT_BF16 2
#define DV3_IO_AB_BF16 4   /* only the saved pre-gate pair `ab` is bf16 (y stays fp32): halves the largest tensor a
                              training forward writes; dv3_gate_bwd_desc.ab_bf16 reads it back */
/*
 * Channel-blocked bf16 activation storage ("c8", BASELINE configs 3/4: bf16 activations in HBM, fp32 accumulate):
 * a (B, C, T) activation is held as  bf16 [B][C8][T][8],  C8 = round_up(C,32)/8 -- channel c of frame t is element
 * c%8 of the 16-byte unit (b, c/8, t); channels >= C are zero.  One unit is one MFMA B-fragment lane: a
 * tensor written by one layer's epilogue is the next layer's `x_c8` (split_terms == 1) with no conversion, the
 * tap-GEMM stages it with plain 16-byte copies, and the epilogue's accumulator tile maps to whole 8-byte halves of
 * units (csrc/conv_common.h).  Any C: the kernels write whole valid groups and keep the padding channels zero;
 * gated layers need Cg % 8 == 0 (the a and gate halves of the saved pre-gate pair start on group boundaries).
 *   DV3_IO_OUT_C8   y (and ab) are written in c8; r / r2 (and the DGRAD addend) are READ in c8
 * (the tensors on the two sides of an epilogue share one layout; x is c8 exactly when x_c8 is given).
 */
#define DV3_IO_OUT_C8 16
int dv3_conv_gemm_f32(const dv3_conv_desc* d, void* stream);
/* size in bytes of the stream-K workspace (dv3_conv_desc.sk_ws) on the current device: one accumulator image per CU
 * (128 registers x 512 threads x 4 bytes) behind a 64-byte flag slot per CU                                         */
int dv3_conv_streamk_ws_bytes(void);

/* fp32 (B,C,T) <-> c8 converters (stack entry / exit and their gradients); x strides in elements.            */
int dv3_to_c8_f32(const float* x, int64_t x_bs, int64_t x_rs, uint16_t* out, int32_t B, int32_t C, int32_t T, void* stream);
int dv3_from_c8_f32(const uint16_t* x, float* out, int64_t out_bs, int64_t out_rs, int32_t B, int32_t C, int32_t T,
                    void* stream);
/* the first C channels of a c8 tensor that holds c8p groups per batch item (the `a` half of a pre-gate gradient:
 * the per-frame speaker-bias gradient of a multi-speaker Conv1dGLU, modules.py:157-160)                     */
int dv3_from_c8_head_f32(const uint16_t* x, int32_t c8p, float* out, int64_t out_bs, int64_t out_rs, int32_t B,
                         int32_t C, int32_t T, void* stream);
/* dropout keep-bits [B*C][rs words] (dv3_dropout_bits) -> keep-bytes [B][C8][T] for c8 consumers             */
int dv3_mask_bits_to_c8(const uint32_t* bits, int32_t bits_rs, uint8_t* out, int32_t B, int32_t C, int32_t T, void* stream);

/*
 * Split-bf16 ("bf16x3") operand form.  The fp32 matrix cores run at 1/16 of the bf16 rate on
 * gfx950, so the GEMM kernels can instead write every fp32 operand as hi + lo with
 *   hi = bf16_rn(v), lo = bf16_rn(v - hi)        (|v - hi - lo| <= 2^-17 |v|: half an ulp of lo, and reached)
 * and accumulate  A_lo*B_hi + A_hi*B_lo + A_hi*B_hi  in fp32 on v_mfma_f32_32x32x16_bf16:
 * three bf16 MFMAs per product block = 16/3 x the fp32-MFMA rate.  Per product the operand error is at most
 * 2 * 2^-17 |a||b| and the dropped lo*lo term at most 2^-16 |a||b| (|lo| <= 2^-8 |v|): 2^-15 of sum|a||b| in the worst
 * case, a few 2^-18 typically -- inside the 1e-4 relative parity bar of the reference comparison
 * (tests/test_gpu_gemm_operands.py holds every element to the bound derived from these statements, against fp64).
 *
 * dv3_split_pack_bf16 converts a packed fp32 weight image [J][K][lda] (dv3_weight_norm_pack_f32's
 * fwd_pack / bwd_pack) into the layout the bf16x3 tap-GEMM stages with straight 16-byte copies:
 *   out[plane][j][k8][m][8]   plane 0 = hi, 1 = lo; k8 = k/8 over Kp = round_up(K,32) (zero rows
 *   beyond K); m < lda; 8 consecutive k per 16-byte unit (one MFMA A-fragment lane).
 * `out` holds 2*J*Kp*lda uint16 elements.
 *
 * Scaled split-fp16 ("f16x3", dtype = DV3_SPLIT_DTYPE_F16): the same images with
 *   a = v * 2^s, hi = fp16_rn(clamp(a, +-65504)), lo = fp16_rn(a - hi)      (|a - hi - lo| <= 2^-23 |a|
 *   while |a| >= 2^-2, where the residual is a normal fp16 value; below that the error is absolute, <= 2^-25 in
 *   a-units: everywhere |a - hi - lo| <= max(2^-23 |a|, 2^-25).  fp16 SUBNORMALS ARE KEPT on gfx950, by the
 *   fp32 -> fp16 conversion of dv3_split8_f16 and at the A / B inputs of the fp16 MFMA alike: measured -- operands
 *   a = m 2^-16, w' = n 2^-10 give the exact integers in every kernel form, tests/test_gpu_gemm_operands.py family E2)
 * s = DV3_F16_WEIGHT_SHIFT (8) for weights, DV3_F16_ACT_SHIFT (4) for activations (fixed powers of two:
 * exact, no amax pass; weight-normed |w| <= |g| and O(1..100) activations sit far inside the range);
 * the accumulators carry 2^12 x the result and the epilogue multiplies by 2^-12 (exact).  The forward
 * tap-GEMM uses this form: at the preset model sizes the bf16 split's 2^-17-class operands, amplified ~100x by
 * the depth of the network, exceed the 1e-4 parity bar (tests/test_gpu_preset_scale.py measures both);
 * the gradient GEMMs keep the bf16 split, whose exponent range covers gradients without a scale search.
 */
/* Range guard of the f16x3 mode.  The scale shifts are fixed, so |x| > 65504 / 2^4 = 4094 (activations) or
 * |w| > 65504 / 2^8 = 255.9 (weights) leaves the fp16 range.  Nothing is saturated silently: lo is the fp16 of the
 * UNCLAMPED residual, so the pair stays fp16-accurate up to twice the range and turns Inf / NaN beyond it (a NaN or
 * Inf input propagates as in the fp32 reference); and every kernel that builds such pairs counts the 16-byte units
 * that left the range in a sticky device counter.  dv3_f16_range_events copies the counter into dst (device int32,
 * may be NULL) and optionally clears it, both asynchronously on `stream`; the host side (ops.f16_range_events,
 * Trainer.step's scalars) uses it to move a model to the bf16x3 mode, whose operands have fp32's exponent range.
 * Replaces: nothing in the reference (its fp32 kernels have the range of fp32); deepvoice3_pytorch/modules.py:145-164
 * is the computation guarded. */
int dv3_f16_range_events(int32_t* dst, int32_t reset, void* stream);

/* Order two HIP streams: everything enqueued on `to` after this call waits for everything enqueued on `from` before
 * it (hipEventRecord on `from` + hipStreamWaitEvent on `to`, with an event from a ring the library owns; inside a
 * stream capture the pair becomes a graph dependency).  The host-side step uses it to fork the weight-gradient
 * branch of backward onto its own stream and to join it again (ops.SideStream) in one call instead of two torch
 * event calls per layer.  Replaces: nothing in the reference (single stream; train.py:755 loss.backward()). */
int dv3_stream_fork(void* from, void* to);

/* The weight-gradient branch of a CAPTURED step as its own hipGraphs.  A whole-step hipGraph (forward + backward on two
 * streams joined by dv3_stream_fork) replays with the two branches serialised: measured 4-7 % slower than eager launches
 * whenever the GPU is the bound (profiles/r03_side_stream_ab.txt, r04_three_graph_probe.txt).  The caller
 * (train_step.GraphedTrainer) therefore cuts the step into segments: while the step stream is being captured
 * (torch.cuda.CUDAGraph), the side stream is captured SEPARATELY (relaxed mode) through these entry points, and both
 * captures are closed every few layers.  Replay: step-stream segment j, an ordinary event, side segment j on the real
 * second stream -- host-issued hipEventRecord / hipStreamWaitEvent only.  (Event-record / event-wait NODES between two
 * graphs were tried first: bit-identical at small sizes, stale waits -- NaN -- at the benchmark's)
 * Replaces: nothing in the reference.
 *   dv3_graph_side_begin  begin the side stream's own capture
 *   dv3_graph_side_end    end it and instantiate; *n_nodes_out = nodes captured (0: *exec_out is NULL)
 */
int dv3_graph_side_begin(void* side_stream);
int dv3_graph_side_end(void* side_stream, void** exec_out, int32_t* n_nodes_out);
int dv3_graph_launch(void* exec, void* stream);
int dv3_graph_destroy(void* exec);

/* ABI 43: the two branches of a captured backward ordered by a DEVICE flag instead of segment boundaries.  With the
 * segments above every fork-point dependency costs two graph launches and an event pair, the step queue idles 15-40 us at
 * every boundary and side segment j cannot start before step segment j has run to its END.  Here backward is ONE graph
 * per stream: at fork point j the step stream's capture holds a one-thread kernel that publishes (epoch, j) in `flag`, the
 * side stream's capture a one-thread kernel that waits until the flag has reached (epoch, j) -- the weight gradient of a
 * layer starts when its operands exist, whatever else the step stream still has to do.
 *   flag   device uint64, zero before the first use; value = epoch * 4096 + j, monotonic over the steps
 *   epoch  device uint64 OWNED BY THE STREAM that launches the kernel (one for the step stream, one for the side stream),
 *          zero before the first use; `bump` != 0 (the first fork point of a step) increments it first -- both graphs are
 *          replayed once per step, so the two epochs agree
 *   j      fork point of the step, 1 .. 4095
 *   err    device uint32 counting waits that gave up after `timeout_ms` (a lost signal must not hang the GPU); the host
 *          reads it when it reads the step's scalars
 * Release / acquire at agent scope: what the step stream wrote before the signal is visible to the side stream's kernels
 * after the wait (kernel boundaries write back and invalidate as they always do).  The two streams must run on different
 * hardware queues (ops.concurrent_stream probes for that).  Replaces: nothing in the reference. */
int dv3_flag_signal(uint64_t* flag, uint64_t* epoch, int32_t j, int32_t bump, void* stream);
int dv3_flag_wait(const uint64_t* flag, uint64_t* epoch, int32_t j, int32_t bump, uint32_t* err, int32_t timeout_ms,
                  void* stream);

#define DV3_SPLIT_DTYPE_BF16 0
#define DV3_SPLIT_DTYPE_F16 1
#define DV3_SPLIT_F16X3 19
#define DV3_F16_WEIGHT_SHIFT 8
#define DV3_F16_ACT_SHIFT 4
int dv3_split_pack_bf16(const float* packed, uint16_t* out, int32_t J, int32_t K, int32_t lda,
                        int32_t dtype, void* stream);

/*
 * dv3_wgrad_gemm_f32 -- weight-gradient GEMM (autograd of F.conv1d w.r.t. weight; also
 * torch.bmm(p, values) of deepvoice3.py:167 when used batched with J=1).
 *
 *   out[s][j][m][c] = sum_{b in slab s} sum_t g[b][m][t] * xd[b][c][t + j*dil - padL]
 *
 * slab s covers batches {s, s+S, s+2S, ...}; S = n_slabs (S == B gives a per-batch
 * result, S == 1 a full reduction).  The slabs are summed by dv3_weight_norm_bwd_f32.
 *
 * PLACEMENT (tests/test_gpu_gemm_footprint.py; strides in elements): fp32 g and x take any 4-byte aligned base, any
 * row stride >= T / Tin and any batch stride.  The split kernels load 8 frames at a time from offsets clamped into
 * [base, base + (B-1) bs + (rows-1) rs + T): a unit that crosses a row end may READ the gap behind it (or the next row)
 * and removes those frames by a select, so what lies there never reaches a sum; nothing outside that span is read.
 * out: any 4-byte aligned base, ldo >= Cin, out_ss as the layout demands; only the first Cin floats of a row are written.
 * xmask as in dv3_conv_desc.  c8 g / x: 16-byte aligned and contiguous.
 */
typedef struct dv3_wgrad_desc {
  const float* g;  int64_t g_bs, g_rs;       /* [B][M][T]                                    */
  const float* x;  int64_t x_bs, x_rs;       /* [B][Cin][Tin]                                */
  const uint32_t* xmask; int32_t xmask_rs;   /* dropout keep-bits over x rows, or NULL       */
  float drop_scale;
  float* out;      int64_t out_ss;           /* [S][J][M][ldo]; slab stride                  */
  int32_t ldo;
  int32_t B, M, Cin, T, Tin, J, dil, padL, n_slabs;
  int32_t split_bf16;                        /* 0: exact fp32 MFMA; 1: bf16x3 split-operand MFMA;
                                                2: single-term bf16 MFMA (hi planes only)        */
  int32_t k_split;                           /* 0: slab s = batch items s, s+S, ... (S == B: a per-batch
                                                result); 1 (split-bf16 kernels): slab s = the s-th
                                                contiguous range of the (batch item, 32-step chunk)
                                                sequence -- any S, so the grid can match the chip  */
  int32_t c8;                                /* g and x are channel-blocked bf16 tensors (DV3_IO_OUT_C8 layout, over M and
                                                Cin channels; the stride fields are unused): the bf16-storage form --
                                                split_bf16 == 2, k_split, T == Tin, J in {1, 3}                     */
  const uint8_t* xmask_c8;                   /* c8: dropout keep-bytes over x [B][round_up(Cin,32)/8][Tin], or NULL   */
  int32_t g_pair;                            /* 1 (split_bf16 == 1): g holds PAIR WORDS (dv3_conv_desc: pg_pair), staged
                                                without conversion                                                     */
} dv3_wgrad_desc;
int dv3_wgrad_gemm_f32(const dv3_wgrad_desc* d, void* stream);

/* ------------------------------------------------------------------------------------
 * Weight normalisation (nn.utils.weight_norm, modules.py:85,100,109) + packing.
 *   v: [O][I][J] (Conv1d/Linear, norm over (I,J) per o)   transposed==0
 *   v: [I][O][J] (ConvTranspose1d, norm over (O,J) per i) transposed==1
 * fwd_pack  [J'][K][lda]  operand of the forward tap-GEMM
 * bwd_pack  [J'][K'][ldb] operand of the DGRAD tap-GEMM (transposed, taps reversed)
 * scale     [O or I] = 1/||v||  (saved for backward; w = g*scale*v)
 * For GLU layers (glu_cg > 0) fwd_pack puts the `a` half at [0,Cg) and the gate half at
 * [a_half, a_half+Cg).
 * ------------------------------------------------------------------------------------ */
typedef struct dv3_wn_desc {
  const float* v; const float* g;            /* g NULL => plain weight (no weight norm)     */
  float* scale;
  float* fwd_pack; int32_t lda; int32_t a_half;
  float* bwd_pack; int32_t ldb;
  int32_t O, I, J, transposed, glu_cg;
  int32_t fwd_dtype;                         /* dv3_weight_norm_split_pack_bf16: DV3_SPLIT_DTYPE_* of the
                                                FORWARD image (the input-gradient image is always bf16) */
} dv3_wn_desc;
int dv3_weight_norm_pack_f32(const dv3_wn_desc* d, void* stream);

/* Fused form for the split-bf16 GEMM modes (Conv1d / Linear layers): scale + BOTH split images
 * (dv3_split_pack_bf16 layout; fwd over K = I with lda columns, bwd over K = O with ldb columns,
 * taps reversed) straight from v, g -- no fp32 images.  d->fwd_pack / d->bwd_pack are ignored;
 * bwd_split may be NULL.  K pad rows are written as zeros; pad COLUMNS are left untouched (they
 * only feed output rows the GEMM epilogue drops).                                          */
int dv3_weight_norm_split_pack_bf16(const dv3_wn_desc* d, uint16_t* fwd_split, uint16_t* bwd_split,
                                    void* stream);

/* The same for EVERY weight-normed Conv1d / Linear layer of a model in two launches.  `table_dev` (device memory,
 * n_layers entries, each a dv3_wn_desc as above + its two image pointers), `first_row_dev[l]` = sum of O over the
 * layers before l, `first_block_dev[l]` = sum of ceil(O/32)*ceil(I/32) before l (both int32, device memory);
 * max_taps = max J.  The table holds raw pointers: build it once over fixed buffers (the trainer's flat parameter
 * arena) and reuse it every step -- the call itself reads no host memory, so it can sit inside a captured graph. */
typedef struct dv3_wn_multi_entry {
  dv3_wn_desc d;
  uint16_t* fwd_split; uint16_t* bwd_split;
} dv3_wn_multi_entry;
int dv3_weight_norm_split_pack_multi(const dv3_wn_multi_entry* table_dev, const int32_t* first_row_dev,
                                     const int32_t* first_block_dev, int32_t n_layers, int32_t total_rows,
                                     int32_t total_blocks, int32_t max_taps, void* stream);

/*
 * Per-frame speaker biases of a BLOCK of Conv1dGLU layers in one launch (forward) / three (backward).
 * Replaces, for every Conv1dGLU of a multi-speaker model in training, modules.py:158-162
 *     softsign = F.softsign(self.speaker_proj(speaker_embed)); a = a + softsign
 * (speaker_proj = weight-normed Linear(speaker_embed_dim -> C), modules.py:135) and its autograd, where speaker_embed
 * is the block's expanded and PER-FRAME dropped embedding (deepvoice3.py:78-81, 292-294): one tensor e (B, E, T) for all
 * layers of the block.  forward: layer[l].out (B, C_l, T) = softsign(bias_l + W_l e), W_l = g_l v_l / ||v_l|| by rows --
 * the tensor a layer's tap-GEMM then reads through dv3_conv_desc.spk.  backward: from layer[l].dout (the gradient of
 * that tensor, element strides dout_bs / dout_rs) and the saved out: dv_l, dg_l, dbias_l += (weight-norm backward
 * included) and de (B, E, T) = the gradient of e, overwritten.  Sums in a fixed order (bit-identical run to run).
 * `layers` is HOST memory (n_layers <= DV3_SPK_MAX_LAYERS entries, copied into the kernel arguments), E <= 16.
 * Workspace of the backward: dv3_speaker_bias_bwd_scratch_floats() floats.
 */
#define DV3_SPK_MAX_LAYERS 16
typedef struct dv3_spk_layer {
  const float* v; const float* g; const float* bias;   /* (C, E) direction, (C) magnitude or NULL, (C) bias or NULL */
  float* out;                                           /* (B, C, T) fp32, contiguous: written by fwd, read by bwd    */
  const float* dout; int64_t dout_bs; int64_t dout_rs;  /* bwd */
  float* dv; float* dg; float* dbias;                   /* bwd, += */
  int32_t C;
  int32_t dout_c8p;                                     /* bwd: != 0: `dout` is a c8 bf16 tensor [B][dout_c8p][T][8] (the
                                                           pre-gate gradient a c8 layer produced: its first C channels
                                                           are the gradient of this bias); dout_bs / dout_rs unused   */
} dv3_spk_layer;
typedef struct dv3_spk_desc {
  const float* e; int64_t e_bs; int64_t e_rs;           /* (B, E, T) fp32, element strides (frames contiguous)       */
  float* de;                                            /* bwd: (B, E, T) fp32 contiguous                             */
  float* scratch; int64_t scratch_floats;               /* bwd                                                        */
  int32_t B, E, T, n_layers;
} dv3_spk_desc;
int dv3_speaker_bias_fwd_f32(const dv3_spk_desc* d, const dv3_spk_layer* layers, void* stream);
int dv3_speaker_bias_bwd_scratch_floats(const dv3_spk_desc* d, const dv3_spk_layer* layers);
int dv3_speaker_bias_bwd_f32(const dv3_spk_desc* d, const dv3_spk_layer* layers, void* stream);

/*
 * Backward of weight norm from wgrad slabs: dW = sum_s slab[s]; dg, dv.
 *   slabs: [S][J][M][ldo] as written by dv3_wgrad_gemm_f32 (M = O rows; c = I cols;
 *   for transposed (ConvTranspose) layers M = J*O rows and the tap is folded in m).
 *   bias_part: [P][O] partial bias sums (or NULL), reduced into dbias.
 */
typedef struct dv3_wn_bwd_desc {
  const float* slabs; int64_t slab_ss; int32_t ldo; int32_t n_slabs;
  const float* v; const float* g; const float* scale;
  float* dv; float* dg;                      /* dg NULL when g NULL (plain weight: dv = dW) */
  const float* bias_part; int32_t n_part; float* dbias;
  int32_t O, I, J, transposed;
  int32_t accumulate;                        /* 1: dv, dg, dbias += (gradient buffers that are zeroed once
                                                per step and shared by every use of the parameter);
                                                0: overwrite                                          */
  int32_t bias_part_t;                       /* 0: bias_part is [n_part][O]; 1: [O][n_part] (dv3_conv_desc.pg_part) */
} dv3_wn_bwd_desc;
int dv3_weight_norm_bwd_f32(const dv3_wn_bwd_desc* d, void* stream);
/* The same for n <= DV3_WN_BWD_MULTI_MAX layers in ONE launch: one workgroup per normalised row of every layer.  A
 * layer's launch is a chain of ~24 memory round trips on 2 workgroups per CU (36 us whatever the layer size); several
 * layers together fill the chip and overlap those chains.  The descriptors (HOST memory) travel by value as kernel
 * arguments: no table upload.  Two entries must not write the same gradient buffers.  Bit-identical to n single calls.
 * Replaces: autograd of nn.utils.weight_norm for the layers of loss.backward() (train.py:755). */
#define DV3_WN_BWD_MULTI_MAX 8
int dv3_weight_norm_bwd_multi(const dv3_wn_bwd_desc* descs, int32_t n, void* stream);

/* ------------------------------------------------------------------------------------
 * Gate / activation backward (autograd of modules.py:157-164, 224-226 and of ReLU/sigmoid).
 *   mode GLU/HIGHWAY: in dy [B][Cg][T], ab [B][2Cg][T], x (highway input) ->
 *        dab [B][2Cg][T], dres [B][Cg][T] (gradient flowing to the residual / highway
 *        carry; NULL when residual==0), bias_part [B][2Cg] row sums of dab,
 *        dspk [B][Cg] (row sums of d a, = bias_part's first half; written when non-NULL)
 *   mode RELU/SIGMOID/LINEAR: in dy, y [B][M][T] -> dpre [B][M][T], bias_part [B][M]
 * ------------------------------------------------------------------------------------ */
typedef struct dv3_gate_bwd_desc {
  const float* dy; const float* ab_or_y; const float* x;
  float* dab; float* dres; float* bias_part;
  float alpha;                               /* non-gated modes: dy is scaled by alpha first */
  int32_t B, C, T, mode, residual;
  int32_t ab_bf16;                           /* gated modes: ab_or_y is a bf16 tensor (DV3_IO_AB_BF16 / _OUT_BF16)  */
  int32_t c8;                                /* every activation tensor (dy, ab_or_y, x, dab, dres) is channel-blocked
                                                bf16 (DV3_IO_OUT_C8 layout; C % 8 == 0); bias_part stays fp32        */
  int32_t dab_pair;                          /* gated modes, fp32 tensors: dab is written as PAIR WORDS (dv3_conv_desc:
                                                pg_pair) -- the layer's two gradient GEMMs stage it without conversion
                                                (dv3_conv_desc.x_pair, dv3_wgrad_desc.g_pair)                        */
} dv3_gate_bwd_desc;
int dv3_gate_bwd_f32(const dv3_gate_bwd_desc* d, void* stream);

/* ------------------------------------------------------------------------------------
 * Dropout keep-bit generator (F.dropout's bernoulli_, modules.py:147,210; deepvoice3.py:
 * 75,80,165,290,321).  Philox4x32-10, counter = (word index, site), key = seed.
 * bits[w] bit i == 1  <=>  element 32*w+i of the row is kept; p quantised to 1/65536.
 * dev_seed_offset: a device-resident step counter, so a replayed hipGraph draws new masks.
 * In full (tests/philox_ref.py states it in integers, tests/test_gpu_dropout_masks.py holds every form to it bit for
 * bit): word w is four calls q = 0..3 with the 128-bit counter (4w + q, site), each a 64-bit half, low word first, and
 * the key s = (seed + *dev_seed_offset) mod 2^64; output e of call q gives two 16-bit uniforms, the low half (h = 0)
 * first; bit 8q + 2e + h is set when the uniform is >= thr, thr = (uint32_t)(p * 65536.0f + 0.5f).  The drop rate is
 * thr / 65536 (within 2^-17 of p); from p >= 1 - 2^-17 on thr is 65536 and NOTHING is kept, though every p < 1 is
 * accepted.
 * ------------------------------------------------------------------------------------ */
int dv3_dropout_bits(uint32_t* bits, int64_t n_words, float p, uint64_t seed,
                     uint64_t site, const uint64_t* dev_seed_offset /* added to seed; NULL = 0 */,
                     void* stream);

/* The same keep decisions as dv3_dropout_bits over rows [B*C] (same seed / site / offset), written as the keep-BYTES
 * [B][round_up(C,32)/8][T] the c8 consumers read (= dv3_dropout_bits + dv3_mask_bits_to_c8 in one launch).      */
/* Both forms of one dropout site in ONE launch: keep-bits [B*C][ceil(T/32)] (what the weight-gradient and
 * input-gradient kernels read) and keep-bytes [B][round_up(C,32)/8][T] (what the 256 x 256 split tap-GEMM and the c8
 * kernels stage: one byte load per 8-channel item instead of eight keep-bit words).  Same decisions as
 * dv3_dropout_bits for the same seed / site / offset.  Replaces F.dropout's bernoulli_ (modules.py:147,210). */
int dv3_dropout_bits_keep(uint32_t* bits, uint8_t* keep, int32_t B, int32_t C, int32_t T, float p, uint64_t seed,
                          uint64_t site, const uint64_t* dev_seed_offset, void* stream);
int dv3_dropout_keep_c8(uint8_t* out, int32_t B, int32_t C, int32_t T, float p, uint64_t seed, uint64_t site,
                        const uint64_t* dev_seed_offset, void* stream);

/* Several dropout sites in ONE launch (ABI 41): site l gets exactly what dv3_dropout_bits_keep(bits, keep, B, C, T, p, seed,
 * site, ...) (bits != NULL) or dv3_dropout_keep_c8(keep, ...) (bits == NULL) writes; keep == NULL with B = 1, C = rows:
 * what dv3_dropout_bits(bits, rows * ceil(T/32), ...) writes.  A training step draws 25-35 masks
 * (one per Conv1dGLU / HighwayConv1d: modules.py:147,210), each a ~6 us launch on the forward's only queue; the host side
 * (ops.MaskPlan) issues them together at the start of the step once the step's list of sites has repeated.        */
#define DV3_DROPOUT_MULTI_MAX 48
typedef struct dv3_dropout_site {
  uint8_t* keep;  uint32_t* bits;      /* keep-bytes [B][round_up(C,32)/8][T]; keep-bits [B*C][ceil(T/32)] or NULL */
  int32_t B, C, T;  float p;
  uint64_t site;
} dv3_dropout_site;
int dv3_dropout_keep_c8_multi(const dv3_dropout_site* sites, int32_t n, uint64_t seed,
                              const uint64_t* dev_seed_offset, void* stream);

/* out[row][t] = x[row][t] * keep(bits,row,t) * scale -- a standalone F.dropout for the few
 * sites whose dropped tensor is shared by several consumers (deepvoice3.py:78-80,290,321:
 * the time-expanded speaker embedding and the decoder input).  Its own backward.          */
int dv3_dropout_apply_f32(const float* x, const uint32_t* bits, int32_t bits_rs, float scale,
                          float* out, int64_t rows, int32_t T, void* stream);

/* ------------------------------------------------------------------------------------
 * Attention (deepvoice3.py:132-176): masked softmax over the key axis + dropout.
 *   s [B][Tq][Tk] scores (in place -> probabilities p, returned PRE-dropout as the
 *   reference does, deepvoice3.py:163); pd (optional) = dropout(p) for the context GEMM.
 *   key_len [B] (int32, use_memory_mask) or NULL; last_attended (device scalar) with
 *   win_back/win_ahead: monotonic window [last-back, last+ahead) (deepvoice3.py:150-156).
 * ------------------------------------------------------------------------------------ */
typedef struct dv3_softmax_desc {
  float* s; float* pd;
  const int32_t* key_len;
  const int32_t* last_attended;              /* device int32[1] or NULL (no window)        */
  const uint32_t* mask; int32_t mask_rs; float drop_scale;
  float pd_scale;                            /* pd = dropout(p) * pd_scale (the sqrt(Tk) of deepvoice3.py:170-171) */
  int32_t B, Tq, Tk, win_back, win_ahead;
  const float* pd_scale_dev;                 /* ABI 42: device float[1] multiplied into pd_scale, or NULL (valid-length
                                              * steps: the key count of the batch is only known on the device)     */
} dv3_softmax_desc;
int dv3_attn_softmax_f32(const dv3_softmax_desc* d, void* stream);
/* backward: ds = p * (dp_total - sum_k(dp_total*p)); dp_total = dpd*bit*scale + dp_direct */
typedef struct dv3_softmax_bwd_desc {
  const float* p; const float* dpd; const float* dp_direct; float* ds;
  const uint32_t* mask; int32_t mask_rs; float drop_scale;
  int32_t B, Tq, Tk;
  const float* scale_dev;                    /* ABI 42: device float[1] multiplied into drop_scale, or NULL          */
} dv3_softmax_bwd_desc;
int dv3_attn_softmax_bwd_f32(const dv3_softmax_bwd_desc* d, void* stream);
/* Fused attention forward (deepvoice3.py:143-171, teacher-forced / training: no monotonic window): scores = q^T k
 * (exact fp32 MFMA) -> -inf beyond key_len[b] -> softmax -> P; pd = P * keep(mask) * drop_scale * pd_scale;
 * ctx[b][e][t] = sum_n v[b][e][n] * pd[b][t][n] (exact fp32 MFMA), one launch.  q (B,E,Tq), k (B,E,Tk) BCT;
 * vT (B,Tk,E) = the values in the reference's own (B,T,C) layout; P, pd (B,Tq,Tk) are both written once (P is the
 * alignment the layer returns, both are what dv3_attn_softmax_bwd_f32 and the gradient products read).  Tk <= 511. */
typedef struct dv3_attn_fwd_desc {
  const float* q; const float* k; const float* vT;
  const int32_t* key_len;
  const uint32_t* mask; int32_t mask_rs; float drop_scale;
  float pd_scale;
  float* ctx; float* P; float* pd;
  int32_t B, E, Tq, Tk;
  const float* pd_scale_dev;                 /* ABI 42: as dv3_softmax_desc.pd_scale_dev                             */
} dv3_attn_fwd_desc;
int dv3_attn_fwd_f32(const dv3_attn_fwd_desc* d, void* stream);
/* argmax over keys of one probability row -> last_attended (deepvoice3.py:445)          */
int dv3_attn_argmax_i32(const float* p_row, int32_t Tk, int32_t* out, void* stream);

/* ------------------------------------------------------------------------------------
 * Small layout / elementwise helpers.
 * ------------------------------------------------------------------------------------ */
/* y[b][c][r] = alpha * x[b][r][c] (+ beta_add[b][c][r] if non-NULL) : BTC <-> BCT      */
int dv3_transpose_f32(const float* x, float* y, const float* add, int32_t B, int32_t R,
                      int32_t C, float alpha, void* stream);
/* out[i] = alpha * (a[i] + b[i]) ; b may be NULL                                       */
int dv3_axpby_f32(const float* a, const float* b, float* out, int64_t n, float alpha,
                  void* stream);
/* out[0] = a[0] + b[0] (+ c[0]) (+ d[0]): the total of the loss terms (train.py:728-740); c, d may be NULL  */
int dv3_sum_scalars_f32(const float* a, const float* b, const float* c, const float* d, float* out, void* stream);
/* bytes of device memory to `value` -- a fill KERNEL on the caller's stream, not hipMemsetAsync (a captured memset node
 * replayed with a corrupt pattern: DESIGN.md 3.7): the gradient arena before backward (optimizer.zero_grad(),
 * train.py:683)                                                                                                 */
int dv3_memset_b8(void* p, int32_t value, int64_t bytes, void* stream);
/* `rows` runs of row_bytes each, row_stride_bytes apart (all multiples of 16, p 16-byte aligned): the padding groups of a
 * channel-blocked tensor whose channel count is not a multiple of 32 (ops._c8_empty), one launch.                    */
int dv3_memset_rows_b8(void* p, int32_t value, int64_t rows, int64_t row_bytes, int64_t row_stride_bytes, void* stream);
/* ABI 42 (valid-length steps).  x is [rows][T] elements of `words` 32-bit words each (fp32 (B, C, T): words = 1; the
 * channel-blocked bf16 [B][C8][T][8]: words = 4).  Columns t >= t_valid[0] * mult of every row are set to zero, where
 * t_valid is a device int32[1]; the host only promises T - t_valid[0] * mult <= max_tail.  What a non-causal
 * convolution of the reference sees beyond the batch's longest item is its own zero padding (modules.py:139-143:
 * nn.Conv1d(padding=...)): a batch padded further (to a lattice shape, so that captured steps can be replayed) keeps
 * that by zeroing the activations -- and, in backward, the activation gradients -- beyond the batch's own maximum.  */
int dv3_zero_tail_b32(void* x, int64_t rows, int32_t T, int32_t words, const int32_t* t_valid, int32_t mult,
                      int32_t max_tail, void* stream);
/* ABI 44 (per-utterance synthesis).  The same per batch item: x holds B items of rows_per_item rows of [T] elements of
 * `words` 32-bit words (fp32 (B, C, T): rows_per_item = C, words = 1; channel-blocked bf16 [B][C8][T][8]: rows_per_item
 * = C8, words = 4); columns t >= len[b] * mult of item b's rows are set to zero, len a device int32[B]; the host
 * promises T - len[b] * mult <= max_tail for every b.  A lone utterance's non-causal convolution sees its own zero
 * padding beyond its last frame (modules.py:139-143); in a ragged batch each item keeps that.  */
int dv3_zero_tail_items_b32(void* x, int32_t B, int64_t rows_per_item, int32_t T, int32_t words, const int32_t* len,
                            int32_t mult, int32_t max_tail, void* stream);
/* Embedding gather into BCT with optional dropout: out[b][c][t] = W[idx[b][t]][c]
 * (deepvoice3.py:74-75, nyanko.py:63).  Backward: dense scatter-add into dW.           */
int dv3_embedding_bct_f32(const int64_t* idx, const float* w, float* out,
                          const uint32_t* mask, int32_t mask_rs, float drop_scale,
                          int32_t B, int32_t T, int32_t C, int32_t n_vocab, void* stream);
int dv3_embedding_bct_bwd_f32(const int64_t* idx, const float* dout, float* dw,
                              const uint32_t* mask, int32_t mask_rs, float drop_scale,
                              int32_t B, int32_t T, int32_t C, int32_t n_vocab,
                              int32_t padding_idx, void* stream);
/* SinusoidalEncoding.forward (modules.py:30-64) at gathered positions only, BCT output:
 * out[b][c][t] = base[b][c][t] + enc, enc = (pos==0 || !apply_sincos) ? w*table[pos][c]
 *              : (c odd ? cos : sin)(w*table[pos][c]);  w = w[b] (w_per_batch) or w[0] or 1 */
int dv3_sincos_pos_bct_f32(const int64_t* pos, const float* table, const float* w,
                           int32_t w_per_batch, const float* base, float* out, int32_t B,
                           int32_t T, int32_t C, int32_t n_pos, int32_t apply_sincos,
                           void* stream);
/* gradient w.r.t. the TABLE (trainable_positional_encodings=True, deepvoice3_pytorch/__init__.py:53-57): dtable
 * [n_pos][C], row 0 (padding) zero; w NULL = rate 1; apply_sincos 0 = plain embedding rows (nyanko.py:162-169) */
int dv3_sincos_pos_table_bwd_f32(const int64_t* pos, const float* table, const float* w, int32_t w_per_batch,
                                 const float* dout, float* dtable, int32_t B, int32_t T, int32_t C,
                                 int32_t n_pos, int32_t apply_sincos, void* stream);
/* gradient of the encoding w.r.t. the rate: dw[b] = sum_{c,t} dout[b][c][t] * d enc/d w
 * (multi-speaker models learn the rate through speaker_proj1/2, deepvoice3.py:304-315).   */
int dv3_sincos_pos_bwd_f32(const int64_t* pos, const float* table, const float* w,
                           int32_t w_per_batch, const float* dout, float* dw, int32_t B, int32_t T,
                           int32_t C, int32_t n_pos, void* stream);
/* The same in two deterministic stages (round 6; ABI 40): `n_chunks` workgroups per batch item leave partial sums in
 * `partial` [B][n_chunks], a second launch adds each item's in index order -- the one-workgroup-per-item form above is
 * 64 workgroups of 200 dependent sinf / cosf iterations on a 256-CU part (160 us per call in the deepvoice3_vctk step). */
int dv3_sincos_pos_bwd2_f32(const int64_t* pos, const float* table, const float* w,
                            int32_t w_per_batch, const float* dout, float* partial, int32_t n_chunks, float* dw,
                            int32_t B, int32_t T, int32_t C, int32_t n_pos, void* stream);
/* Incremental-conv window (conv.py:34-46): buf [rows][L] shifts left one frame and takes
 * x[row * x_stride] as its newest; in place, static addresses (hipGraph-capturable decode step) */
int dv3_shift_append_f32(float* buf, const float* x, int64_t rows, int32_t L, int64_t x_stride,
                         void* stream);
/* Device-side batch padding (the `_pad` / `_pad_2d` loops of train.collate_fn, train.py:293-360, and the
 * mel time down-sampling of train.py:639-640 in the same pass): items are packed back to back as rows of
 * D 32-bit words (f32 features; int64 text ids as D = 2), item b owning rows [row_off[b], row_off[b+1]).
 *   out[b][t][0..D) = src[row_off[b] + s][0..D),  s = t * t_stride - lead,   if 0 <= s < rows of item b
 *                   = 0                                                      otherwise
 * out is [B][T_out][D].  lead = the b_pad leading zero frames, t_stride = downsample_step for the mel. */
int dv3_ragged_pad_rows_b32(const uint32_t* src, const int32_t* row_off, uint32_t* out, int32_t B,
                            int32_t T_out, int32_t D, int32_t lead, int32_t t_stride, void* stream);
/* dy [B][O][2T] -> out[b][j*O+o][t] = dy[b][o][2t+j]: operand of the ConvTranspose1d(k2,s2)
 * backward GEMMs (deepvoice3.py:519-520,527-528)                                          */
int dv3_deinterleave2_f32(const float* dy, float* out, int32_t B, int32_t O, int32_t T,
                          void* stream);

/* ------------------------------------------------------------------------------------
 * Losses (train.py:261-291,537-601,704-740), fused value + gradient.
 * ------------------------------------------------------------------------------------ */
/* spec_loss on y_hat[:, :-r] vs y[:, r:]  (BTC tensors [B][T][D]).
 *   loss = (1-wbd)*(wm*maskedL1 + (1-wm)*L1) + wbd*(wm*masked_mean(z) + (1-wm)*mean(z))
 *   z = -y*logit(yh) + log1p(exp(logit(yh))), logit eps 1e-8 (train.py:537-582).
 * out4 = {l1_loss, binary_div, total, mask_sum}; dyh gets d total / d y_hat * gscale.   */
typedef struct dv3_spec_loss_desc {
  const float* y_hat; const float* y; const int32_t* lengths; /* mask: t < lengths[b] (shifted by r) */
  float* dyh; float* out4; float* scratch;  /* scratch: >= 4*n_blocks floats                */
  int64_t yh_bs, yh_ts, yh_ds;              /* element strides of y_hat / dyh over (b,t,d):  */
  int64_t y_bs, y_ts, y_ds;                 /* BTC (T*D, D, 1) or BCT (D*T, 1, T) both fine  */
  int32_t B, T, D, r; float w_masked, w_bd, gscale;
  const int32_t* t_valid;                   /* ABI 42: device int32[1] or NULL.  The loss is the one of the tensors cut
                                             * to their first t_valid[0] frames (means over B * (t_valid - r) * D, zero
                                             * gradient beyond): a batch padded beyond its own maximum (valid-length
                                             * steps, replayed from a lattice of padded shapes)                         */
} dv3_spec_loss_desc;
int dv3_spec_loss_f32(const dv3_spec_loss_desc* d, void* stream);
/* The loss head (an addition to ABI 49: one entry point, no struct changed, so the version stays 49 -- the two pointers
 * travel beside the descriptor instead of inside it).  y_hat is the output of a sigmoid layer and the caller wants the
 * gradient of that layer's PRE-activation from the same pass as the loss.  dpre (required), laid out like dyh, gets
 *     dz = (dyh * alpha) * y_hat * (1 - y_hat),  alpha = 1,
 * the three products in the order of dv3_gate_bwd_f32 (DV3_EPI_SIGMOID): the bits are those of dv3_spec_loss_f32
 * writing dyh followed by that call.  The last r frames get dz = 0 from the same launch (no separate zeroing launch).
 * d->dyh may be NULL; if set it is written too.  out4 has the bits dv3_spec_loss_f32 gives.
 * bias_part (or NULL): fp32 [D][B * t_tiles], t_tiles = ceil((T - r) / 64) -- the sum of dz over every 64-frame tile of
 * every item, channel-major: dv3_weight_norm_bwd_f32 takes it with n_part = B * t_tiles, bias_part_t = 1.  No atomics;
 * the sums do not depend on the grid.  (Time-fastest prediction with bin-fastest target: the sums come from the loss
 * launch itself; other layouts: from a second small launch over dz.)                                                */
int dv3_spec_loss_head_f32(const dv3_spec_loss_desc* d, float* dpre, float* bias_part, void* stream);
int dv3_spec_loss_scratch_floats(int32_t B, int32_t T, int32_t D);

/* guided attention (train.py:585-601,733-740): loss = mean(attn * W),
 * W[b][t][n] = 1-exp(-(n/N_b - t/T_b)^2/(2 g^2)) inside (T_b,N_b), 0 outside.
 * attn [L][B][Tq][Tk]; dattn (optional) = W/(L*B*Tq*Tk) * gscale                        */
int dv3_guided_attn_loss_f32(const float* attn, const int32_t* in_len, const int32_t* out_len,
                             float* dattn, float* out1, float* scratch, int32_t L, int32_t B,
                             int32_t Tq, int32_t Tk, float g, float gscale, void* stream);
/* ABI 42: the same with the mean taken over L * B * tq_valid[0] * tk_valid[0] elements (device int32[1] each): the
 * alignment of a batch padded beyond its own maxima.  W is zero outside every item's (T_b, N_b), so only the divisor
 * differs from the call above on the padded tensor.                                                               */
int dv3_guided_attn_loss_valid_f32(const float* attn, const int32_t* in_len, const int32_t* out_len,
                                   float* dattn, float* out1, float* scratch, int32_t L, int32_t B,
                                   int32_t Tq, int32_t Tk, float g, float gscale, const int32_t* tq_valid,
                                   const int32_t* tk_valid, void* stream);
/* BCELoss(done_hat, done) mean (train.py:614,714) + gradient                            */
int dv3_bce_loss_f32(const float* p, const float* t, float* dp, float* out1, float* scratch,
                     int64_t n, float gscale, void* stream);
/* ABI 42: p, t are [rows][T]; only the first t_valid[0] (device int32[1]) columns of every row take part: mean over
 * rows * t_valid, zero gradient beyond.                                                                             */
int dv3_bce_loss_valid_f32(const float* p, const float* t, float* dp, float* out1, float* scratch,
                           int64_t rows, int32_t T, const int32_t* t_valid, float gscale, void* stream);

/* The loss head (addition to ABI 49) of p = sigmoid(z), a SINGLE-channel layer's output ([rows][T], the done flag): as
 * dv3_bce_loss_f32 (t_valid NULL) / dv3_bce_loss_valid_f32, and dpre (required) gets dp * p * (1 - p) as
 * dv3_gate_bwd_f32 (DV3_EPI_SIGMOID, alpha = 1) would make it from dp; dp itself only when non-NULL.  bias_part (or
 * NULL): fp32 [dv3_bce_loss_head_parts(rows * T)] workgroup sums of dpre, the one channel's partial bias gradient
 * (dv3_weight_norm_bwd_f32: n_part = that count, bias_part_t = 1).  out1 keeps the bits of the calls above.          */
int dv3_bce_loss_head_f32(const float* p, const float* t, float* dp, float* dpre, float* bias_part, float* out1,
                          float* scratch, int64_t rows, int32_t T, const int32_t* t_valid, float gscale,
                          void* stream);
int dv3_bce_loss_head_parts(int64_t n);

/* Per-item sums for held-out evaluation (train_step.Trainer.evaluate).  Additions to ABI 49: three forward-only entry
 * points, one descriptor and a scratch-size query; nothing existing changed, so the version stays 49.
 * Each writes ONE fp32 row per batch item -- the masked sums its batch counterpart above folds into one mean, of the
 * same fp32 terms -- and takes no gradient buffer.  Deterministic: the item's own frames are cut into slices (one
 * workgroup each), slice partial sums go to `scratch` (>= dv3_loss_items_scratch_floats(B, T) floats, T the frame axis
 * of the tensor: T of the spectrograms and of p, Tq of attn) and a finishing pass adds them in slice order.
 * Lengths beyond the tensor are clamped to it; an item without frames gets a row of zeros.  The count is computed in
 * 64-bit integers and stored in the fp32 row: exact up to 2^24 elements per item (n_b * 513 <= 2^24: 32 703 frames),
 * rounded to nearest beyond -- a caller that needs exact counts there rebuilds them from the lengths.
 *   spec:   out[b] = {sum |y_hat[b,t,d] - y[b,t+r,d]|, sum z (as dv3_spec_loss_f32), n_b * D},
 *           t < n_b = max(lengths[b] - r, 0): the frames the batch kernel's mask (t + r) < lengths[b] keeps.  Strides as
 *           dv3_spec_loss_desc (BTC or BCT memory)
 *   bce:    p, t [B][T]: out[b] = {sum_{t < lengths[b]} bce(p, t), lengths[b]}
 *   guided: attn [L][B][Tq][Tk]: out[b] = {sum_{l, t < T_b, n < N_b} attn * W, L * T_b * N_b},
 *           T_b = out_len[b], N_b = in_len[b]                                                                      */
typedef struct dv3_spec_items_desc {
  const float* y_hat; const float* y; const int32_t* lengths;
  float* out; float* scratch;               /* out: [B][3]                                   */
  int64_t yh_bs, yh_ts, yh_ds;
  int64_t y_bs, y_ts, y_ds;
  int32_t B, T, D, r;
} dv3_spec_items_desc;
int dv3_loss_items_scratch_floats(int32_t B, int32_t T);
int dv3_spec_loss_items_f32(const dv3_spec_items_desc* d, void* stream);
int dv3_bce_loss_items_f32(const float* p, const float* t, const int32_t* lengths, float* out, float* scratch,
                           int32_t B, int32_t T, void* stream);
int dv3_guided_attn_loss_items_f32(const float* attn, const int32_t* in_len, const int32_t* out_len, float* out,
                                   float* scratch, int32_t L, int32_t B, int32_t Tq, int32_t Tk, float g,
                                   void* stream);

/* ------------------------------------------------------------------------------------
 * Optimiser tail (train.py:755-759): clip_grad_norm_ + Adam over ONE flat fp32 arena
 * (all trainable parameters / gradients / moments are views into four flat buffers).
 *   out2 = {||g||_2, ||g||_2^2};  hyper (device) = {lr, 1-beta1^t, sqrt(1-beta2^t)};
 *   grad_prescale multiplies g first (1/world_size after a sum all-reduce).
 * ------------------------------------------------------------------------------------ */
int dv3_grad_sqnorm_f32(const float* g, int64_t n, float* partial, int32_t n_partial,
                        float* out2, void* stream);
int dv3_clip_adam_f32(float* p, const float* g, float* m, float* v, int64_t n,
                      const float* grad_norm, float clip, const float* hyper, float beta1,
                      float beta2, float eps, float weight_decay, float grad_prescale,
                      void* stream);
/* Weight averaging (additive entry points, ABI 49 as before).  dv3_clip_adam_ema_f32 is
 * dv3_clip_adam_f32 -- p, m, v come out bit for bit as there -- followed, for the same element in the same pass, by the
 * exponential moving average of the updated parameter in its increment form
 *     ema' = ema + hyper[3] * (p' - ema),      hyper (device) = {lr, 1-beta1^t, sqrt(1-beta2^t), 1 - decay_t}
 * (hyper[3] = 0 leaves ema as it is, hyper[3] = 1 copies p'; both exactly).  5 reads + 4 writes of 4 B per parameter.
 * 16 bytes per lane when p, g, m, v and ema are all 16-byte aligned (slices of the flat arenas are), one element at a
 * time otherwise.  ema must not overlap p.
 * dv3_swap_f32 exchanges the contents of two buffers of n floats in place, in one pass: a == b or overlapping ranges
 * are refused (DV3_EINVAL).  Parameter views and captured graphs hold raw addresses into the parameter arena, so
 * averaged weights are put in their place by content.                                                              */
int dv3_clip_adam_ema_f32(float* p, const float* g, float* m, float* v, float* ema, int64_t n,
                          const float* grad_norm, float clip, const float* hyper, float beta1,
                          float beta2, float eps, float weight_decay, float grad_prescale,
                          void* stream);
int dv3_swap_f32(float* a, float* b, int64_t n, void* stream);
/* Training health (additive entry points, ABI 49 as before).
 * The GUARDED passes are dv3_clip_adam_f32 / dv3_clip_adam_ema_f32 with a decision taken on the device, where a captured
 * graph can take it.  grad_norm is mandatory here and read whatever `clip` is (clip = 0 still means no clipping);
 * health points at two floats the caller owns, zeroed once.  With s = grad_norm[0]:
 *   s not finite   nothing of p, m, v (, ema) is read or written -- every workgroup returns before its loop, the step
 *                  costs no arena traffic -- and health[0] += 1, health[1] = 1;
 *   s finite       p, m, v (, ema) come out bit for bit as the unguarded entry point writes them, and health[1] = 0.
 * health[0] counts in fp32 (exact to 2^24 skipped steps).  One lane of the grid writes both words with ordinary stores.
 * s is the norm dv3_grad_sqnorm_f32 left, so s is +Inf also for a FINITE gradient whose sum of squares leaves the fp32
 * range (|g| of order 1e19): such a step is skipped too, which is the wanted behaviour.                               */
int dv3_clip_adam_guard_f32(float* p, const float* g, float* m, float* v, int64_t n,
                            const float* grad_norm, float clip, const float* hyper, float beta1,
                            float beta2, float eps, float weight_decay, float grad_prescale,
                            float* health, void* stream);
int dv3_clip_adam_ema_guard_f32(float* p, const float* g, float* m, float* v, float* ema, int64_t n,
                                const float* grad_norm, float clip, const float* hyper, float beta1,
                                float beta2, float eps, float weight_decay, float grad_prescale,
                                float* health, void* stream);
/* The per-tensor table: out[n_tensors][DV3_TENSOR_STAT_COLS] (float64) over four arenas of n floats each, in two
 * launches, no atomics (two runs on the same data give the same bits).  Columns:
 *   0 grad_sumsq      sum of (grad_prescale * g)^2 over the tensor's FINITE gradient elements
 *   1 grad_absmax     max |grad_prescale * g| over them (0 if there is none)
 *   2 grad_nonfinite  number of NaN / +-Inf gradient elements (exact)
 *   3 param_sumsq     sum of p^2                  4 param_absmax   max |p|
 *   5 update_sumsq    sum of d^2, d = (hyper[0] / hyper[1]) * m / (sqrt(v) / hyper[2] + eps): the update the last pass
 *                     applied, from the moments it left; 0 when health != NULL and health[1] != 0 (a skipped pass
 *                     moved nothing; the moments are not read then).  health may be NULL: not skipped.
 * chunks[n_chunks][3] = (element offset, length <= DV3_ARENA_CHUNK_MAX, tensor index), int64, on the device: a chunk
 * lies inside one tensor (the padding between tensors is in no chunk) and the chunks of a tensor are consecutive rows;
 * ranges[n_tensors][2] = (first chunk row, number of rows).  A row that points outside [0, n) is read as empty.
 * scratch: n_chunks * DV3_TENSOR_STAT_COLS floats.  The sums are fp32 inside a chunk and fp64 across chunks: at most 39
 * fp32 roundings deep, all terms non-negative.  The arenas must be 16-byte aligned.                 */
#define DV3_TENSOR_STAT_COLS 6
#define DV3_ARENA_CHUNK_MAX 4096
int dv3_arena_stats_f32(const float* p, const float* g, const float* m, const float* v, int64_t n,
                        const float* hyper, const float* health, const int64_t* chunks, int64_t n_chunks,
                        const int64_t* ranges, int32_t n_tensors, float grad_prescale, float eps,
                        float* scratch, double* out, void* stream);

/* ------------------------------------------------------------------------------------
 * Autoregressive decode step (Decoder.incremental_forward, deepvoice3.py:397-473): two fused kernels per
 * layer kind instead of the ~100 launches of the module-by-module path.  Both read the 0-based step counter
 * `t` from DEVICE memory, so one captured hipGraph of a step replays for every step.
 *
 * dv3_conv_step_f32 -- one incremental conv layer (conv.py:17-46) with its whole tail:
 *   window: tap J-1 = the new frame x (B, Cin); tap j = the frame (J-1-j)*dil steps back, kept in `ring`
 *   [L][B][Cin] (slot t mod L holds step t; the call stores x there; L >= (J-1)*dil + 1; zero the ring to
 *   start a sequence = conv.py clear_buffer);  acc[b][m] = sum_{j,c} a[j][c][m] * window[b][j][c]
 *   (a = the layer's weights in STEP-TILE order, written by dv3_conv_step_pack_f32 from dv3_weight_norm_pack_f32's
 *   fwd_pack: [row block of 16][window element j*Cin + c][16 rows], gated layers [..][16 `a` rows | 16 gate rows] --
 *   the 100 KB a workgroup streams per layer are one dense block; lda / a_half are ignored);  then, by mode:
 *     GLU / HIGHWAY  (+bias, +spk[b][m] on the `a` half) gate with the new frame as residual / highway carry
 *                    (modules.py:157-164, 224-226), then r2: y = (y + r2) * sqrt(.5)
 *     LINEAR / RELU / SIGMOID / SOFTSIGN  activation, then r and r2 residuals, each (y + r) * sqrt(.5)
 *   then y += post_add[t*post_add_ts + b*post_add_bs + m] (the step's position encoding, deepvoice3.py:430);
 *   y -> (B, Cout); y_act (optional) = sigmoid(y); out_seq (optional) [t][b][m] = y_act if given else y.
 * dv3_attn_step_f32 -- one attention read (deepvoice3.py:143-171 at Tq = 1): scores q.k over the window
 *   [last-win_back, last+win_ahead) (all keys when last_attended is NULL), softmax, ctx = P v * Tk*sqrt(1/Tk);
 *   attn (B, Tk) and / or attn_seq [t][b][n]; last_attended is a PAIR of device ints: slot t&1 is read, the
 *   argmax of batch item 0 (deepvoice3.py:445) is stored in slot (t+1)&1.
 *   ABI 44, per-utterance mode (key_len != NULL): item b reads only its own keys n < s = key_len[b] (clamped to
 *   [1, Tk]; Tk stays the row stride of k, v, attn and attn_seq): its window clamps to s, its softmax runs over
 *   those keys (probabilities of n >= s are written as 0) and its context scale is s * sqrt(1 / s) -- exactly what
 *   the reference computes for that utterance alone at B = 1.  last_attended is then [2][B] (slot t&1 row read,
 *   slot (t+1)&1 row written) and EVERY item stores its own first-maximum argmax.  Not taken by
 *   dv3_decode_program_run (its device-side stop rule is one flag per batch): refused there.
 *   ABI 48, slot mode (t_off != NULL, both kernels): item b runs at its OWN step t_b = t - t_off[b] -- its ring slot
 *   t_b mod L, its position-code row, its teacher-input row, its stacked rows of out_seq / attn_seq and its t_b & 1
 *   side of last_attended -- so that a batch slot whose utterance has ended can be handed to the next utterance while
 *   its neighbours keep decoding (rolling admission: t_off[b] = the global step at which slot b was admitted).  A slot
 *   whose t_b lies outside [0, t_cap) is idle: it reads only its own rows (table rows clamped into [0, t_cap)) and
 *   stores no ring frame, no stacked row and no last_attended; the attention kernel stores nothing at all for it.
 *   t_cap > 0 is then required: the rows out_seq, attn_seq, post_add and (with x_ts) x hold.  Slot mode is a separate
 *   instantiation of the kernels: with t_off == NULL the code is the shared-counter one.  dv3_decode_program_launch
 *   passes t_off through (the global t travels in t_value); dv3_decode_program_run refuses it (as it refuses key_len:
 *   its loop and stop rule are one step counter and one flag per batch).
 * ------------------------------------------------------------------------------------ */
typedef struct dv3_conv_step_desc {
  const float* x; int64_t x_bs;
  float* ring; int32_t L;
  const int32_t* t;
  const float* a; int32_t lda, a_half;
  const float* bias;
  const float* spk; int64_t spk_bs;
  const float* r;  int64_t r_bs;
  const float* r2; int64_t r2_bs;
  const float* post_add; int64_t post_add_ts, post_add_bs;
  float* y; int64_t y_bs;
  float* y_act; int64_t y_act_bs;
  float* out_seq; int64_t out_seq_ts, out_seq_bs;
  int32_t B, Cin, M, Cg, J, dil, mode, residual;
  float* y_pre; int64_t y_pre_bs;            /* optional: the layer output BEFORE post_add (nyanko.py:297-300: Q feeds the
                                                concat while Q + position code feeds the attention query)            */
  int64_t x_ts;                              /* the new frame of step t is x + t*x_ts (teacher forcing: x = test_inputs,
                                                deepvoice3.py:411-415); 0 = the same buffer every step               */
  int32_t t_value, reserved;                 /* the step index when `t` is NULL (host-driven loops: dv3_decode_program_launch) */
  const int32_t* t_off;                      /* [B] device ints: slot mode (ABI 48), item b runs at step t - t_off[b]; or NULL */
  int32_t t_cap, reserved2;                  /* slot mode: items whose step is outside [0, t_cap) are idle            */
} dv3_conv_step_desc;
int dv3_conv_step_f32(const dv3_conv_step_desc* d, void* stream);
/* fwd_pack ([J*Cin][lda] fp32; gated: `a` rows at column 0, gate rows at column a_half) -> the step-tile image
 * dv3_conv_step_f32 reads.  Cg = gated ? rows per half : 0.  out holds dv3_conv_step_pack_floats(...) floats. */
int dv3_conv_step_pack_floats(int32_t Ktot, int32_t M, int32_t Cg);
/* LDS bytes one dv3_conv_step_f32 launch of a J-tap layer with Cin input channels needs (its k-tap window of the
 * batch group + the two reduction stages); the launch is refused above DV3_CONV_STEP_LDS_MAX.  The Python decoders ask
 * this before they choose the fused step program (deepvoice3.py / nyanko.py: _fast_decode_eligible). */
#define DV3_CONV_STEP_LDS_MAX 65536
int dv3_conv_step_lds_bytes(int32_t J, int32_t Cin);
int dv3_conv_step_pack_f32(const float* fwd_pack, int32_t lda, int32_t a_half, int32_t Ktot, int32_t M, int32_t Cg,
                           float* out, void* stream);

typedef struct dv3_attn_step_desc {
  const float* q; int64_t q_bs;              /* (B, E)                                       */
  const float* k; const float* v;            /* (B, E, Tk) each, BCT (or (B, Tk, E): kv_tke)  */
  int32_t* last_attended;                    /* [2] device ints or NULL                      */
  int32_t win_back, win_ahead;
  const int32_t* t;
  float* ctx; int64_t ctx_bs;                /* (B, E)                                       */
  float* attn;                               /* (B, Tk) or NULL                              */
  float* attn_seq; int64_t attn_seq_ts;      /* [t][B][Tk] or NULL                           */
  int32_t B, E, Tk;
  int32_t t_value;                           /* the step index when `t` is NULL             */
  int32_t kv_tke, reserved;                  /* 1: k and v are (B, Tk, E) -- the reference's own layout (deepvoice3.py:
                                                132-141), a key / value row is contiguous: coalesced for a one-frame read */
  const int32_t* key_len;                    /* [B] device ints: per-utterance mode (ABI 44), or NULL           */
  const int32_t* t_off;                      /* [B] device ints: slot mode (ABI 48; needs key_len), or NULL     */
  int32_t t_cap, reserved2;                  /* slot mode: items whose step is outside [0, t_cap) store nothing  */
} dv3_attn_step_desc;
int dv3_attn_step_f32(const dv3_attn_step_desc* d, void* stream);

/* The whole decoder loop in ONE launch (Decoder.incremental_forward's `while True`, deepvoice3.py:397-473;
 * nyanko.py:277-331).  `entries` is the per-step launch program -- the same descriptors dv3_conv_step_f32 /
 * dv3_attn_step_f32 take, in execution order, in DEVICE memory; their `t` pointers are ignored (the step index is the
 * kernel's loop variable).  A persistent grid of ceil(B/4) batch groups x wg_per_group workgroups walks the program:
 * the workgroups of one batch group share an entry's output-channel blocks and meet at a group barrier after every
 * entry (the activations of 4 batch items never leave their group); all groups meet once per step, where the stop
 * rule of the reference is evaluated on the device:
 *     steps = t + 1;  stop if (done_seq != NULL and steps > min_steps and done_seq[t][b] > 0.5 for all b)
 *                     or steps > max_steps                       (deepvoice3.py:463-470; without done_seq: n_steps)
 * The number of steps executed is stored in steps_out.  `sync` is device scratch of dv3_decode_program_sync_ints(B)
 * int32 that the call zeroes first.  The grid must be co-resident (it is at most 256 workgroups of 256 threads).
 * A barrier that does not complete in ~2 s of spinning sets steps_out to -1 and the kernel exits. */
typedef struct dv3_decode_entry {
  int32_t kind;                              /* 0: conv step, 1: attention step */
  int32_t reserved;
  dv3_conv_step_desc conv;
  dv3_attn_step_desc attn;
} dv3_decode_entry;
typedef struct dv3_decode_program {
  const dv3_decode_entry* entries;           /* device */
  const dv3_decode_entry* entries_host;      /* the host copy `entries` was uploaded from: validated by the call */
  int32_t n_entries, B;
  int32_t t0, n_steps;                       /* steps t0 .. t0 + n_steps - 1 at most */
  const float* done_seq; int64_t done_ts;    /* [t][b] done flags the program writes, or NULL */
  int32_t min_steps, max_steps;
  int32_t* sync;
  int32_t* steps_out;                        /* device int: steps executed in this call */
  int32_t wg_per_group;                      /* 0 = library default */
  int32_t reserved;
} dv3_decode_program;
int dv3_decode_program_sync_ints(int32_t B);
int dv3_decode_program_run(const dv3_decode_program* prog, void* stream);
/* The same program, host driven: steps t0 .. t0 + n_steps - 1 as one kernel launch per entry per step, issued by ONE
 * call (a step of the ljspeech decoder is 17 launches: issued from Python + ctypes or as a replayed per-step hipGraph
 * they cost the host ~110 us per step, more than the GPU needs; from this loop ~3 us each).  Uses entries_host; the
 * step index travels in the descriptors (t_value), no device counter.  No stop rule here: the caller runs a chunk of
 * steps, reads the done flags of the chunk, and discards the steps after the stopping one (later steps never change
 * earlier outputs, so the kept prefix is what a step-by-step loop produces). */
int dv3_decode_program_launch(const dv3_decode_program* prog, void* stream);
/* Slot mode: start a fresh sequence in `n` batch slots of a program (the reference's start_fresh_sequence plus a zero
 * initial input, for those items only) in ONE launch.  Walks entries_host and, for every slot index s in `slots`
 * (DEVICE int32[n], each in [0, B)): zeroes item s's columns of every conv entry's ring (L, B, Cin), both rows of every
 * attention entry's last_attended ([2][B]: the entries must be per-utterance ones, key_len != NULL) and item s's row of
 * the decoder input (the x of entry 0, Cin floats).  At most 128 rings + windows per program. */
int dv3_decode_slots_reset(const dv3_decode_program* prog, const int32_t* slots, int32_t n, void* stream);

/* Guided decode (entry points added under ABI 50, no struct changes): the attention window's centre
 * comes from a table instead of from the previous step's argmax.
 * dv3_attn_step_guided_f32 -- dv3_attn_step_f32 in per-utterance mode, except that item b at step t centres its window
 *   on  la = guide[b * guide_bs + min(t, steps[b] - 1)]  (guide: DEVICE int32 rows of stride guide_bs, steps: DEVICE
 *   int32[B]; the row index is clamped into [0, guide_bs) and la into the item's own keys [0, key_len[b])): the keys
 *   [la - win_back, la + win_ahead) clamped by the same two-sided rule (deepvoice3.py:150-156), with the descriptor's
 *   win_back / win_ahead.  last_attended is neither read nor written (it may be NULL) and no argmax is taken; scores,
 *   softmax, stored rows (attn, attn_seq), context and the key_len handling are those of dv3_attn_step_f32.
 *   Requires key_len != NULL and t_off == NULL (slot mode is refused: a slot's step is t - t_off[b], the table has one
 *   step axis for the batch), win_back >= 0, win_ahead >= 1, and -- what the host can check without reading the
 *   device -- guide_bs >= t_value + 1 when the step travels in t_value (guide_bs >= 1 with a device counter).
 * dv3_decode_program_launch_guided -- dv3_decode_program_launch with the guided kernel for EVERY attention entry (all
 *   share the one table); conv entries are launched as they are.  The same requirements for every attention entry,
 *   no conv entry in slot mode, and guide_bs >= t0 + n_steps.  dv3_decode_program_run has no guided form.
 * dv3_guide_from_durations_i32 -- the table from per-key step counts.  dur: DEVICE int32 rows of stride dur_bs >= Tk,
 *   item b's first key_len[b] entries (clamped to [1, Tk]) are read.  With cum the inclusive running sum, key n owns
 *   steps [cum[n-1], cum[n]); a key of duration 0 owns none.  steps[b] = min(sum, T); guide[b * guide_bs + t] for
 *   t < T: the owner of step t, and for t >= steps[b] the last key that owns a step -- bit for bit
 *   np.repeat(np.arange(key_len), dur)[:T], continued by its last entry.  flags[b] is a bit set of DV3_GUIDE_*:
 *   NEGATIVE a duration below 0 (counted as 0), EMPTY sum 0 (steps = 0, a row of zeros), OVER sum above T (cut at T).
 *   One wave per item, integers only.  Refused: a null pointer, B outside [1, 65535], Tk outside [1, DV3_GUIDE_MAX_TK],
 *   T outside [1, DV3_GUIDE_MAX_T], dur_bs < Tk, guide_bs < T. */
#define DV3_GUIDE_NEGATIVE 1
#define DV3_GUIDE_EMPTY 2
#define DV3_GUIDE_OVER 4
#define DV3_GUIDE_MAX_TK 2048
#define DV3_GUIDE_MAX_T 1048576
int dv3_attn_step_guided_f32(const dv3_attn_step_desc* d, const int32_t* guide, int64_t guide_bs,
                             const int32_t* steps, void* stream);
int dv3_decode_program_launch_guided(const dv3_decode_program* prog, const int32_t* guide, int64_t guide_bs,
                                     const int32_t* steps, void* stream);
int dv3_guide_from_durations_i32(const int32_t* dur, int64_t dur_bs, const int32_t* key_len, int32_t B, int32_t Tk,
                                 int32_t T, int32_t* guide, int64_t guide_bs, int32_t* steps, int32_t* flags, void* stream);

/* ------------------------------------------------------------------------------------
 * Audio inverse (audio.py:37-43, synthesis.py:64-71): linear spectrogram -> waveform on the
 * device.  The reference calls the third-party `lws` package for phase reconstruction (not
 * vendored: parity unpinned); these entry points implement Griffin-Lim with
 * torch.stft / torch.istft conventions: n_fft 1024 (513 bins), periodic Hann window, hop as
 * given (preset: 256), center=True with reflect padding, istft normalised by the overlap-added
 * squared window, signal length L = hop*(T-1).
 *   mag     [B][T][513]      magnitudes ** power
 *   phasor  [B][T][513][2]   unit complex phase estimate (re, im)
 *   frames  [B][T][1024]     windowed time-domain frames
 *   y       [B][L]
 * One Griffin-Lim iteration = istft_frames -> overlap_add -> stft_phase, or fused: gl_project -> overlap_add.
 *
 * Frame size (ABI 49).  The entry points above and below that take no n_fft frame by 1024 (every reference preset).
 * Each of them has a sibling named with the suffix `_n` that takes `int32_t n_fft` in front of `stream` and frames
 * by it: n_fft = 512, 1024 or 2048 (DV3_EINVAL and a message for any other value, before anything is launched; 4096
 * would need 96 KB of LDS per workgroup and another kernel shape).  A sibling at n_fft = 1024 is its parent, bit for
 * bit.  Every "1024" of the parent's description reads n_fft and every "513" reads n_fft/2 + 1:
 *   mag [B][T][n_fft/2 + 1], phasor [B][T][n_fft/2 + 1][2], frames [B][T][n_fft], awin / swin [n_fft],
 *   hop <= n_fft, L = hop * (T - 1) > n_fft/2 on the torch framing (the reflect padding),
 *   L = (T + 1) * hop - n_fft > 0 samples on the lws framing, frame t starting at sample t * hop - (n_fft - hop).
 * The transform is an in-LDS Stockham FFT of 256 threads per frame: radix-4 passes, closed at 512 = 2 * 4^4 and
 * 2048 = 2 * 4^5 by one radix-2 pass.
 * ------------------------------------------------------------------------------------ */
/* mag = (10^((clip(x,0,1)*(-min_db) + min_db + ref_db)/20))^power   audio.py:39-41,84-93 */
int dv3_gl_prepare_f32(const float* lin, float* mag, int64_t n, float min_level_db,
                       float ref_level_db, float power, void* stream);
int dv3_istft_frames_f32(const float* mag, const float* phasor /* NULL: zero phase */,
                         float* frames, int32_t B, int32_t T, void* stream);
/* mag [B][T][n_fft/2 + 1], phasor [B][T][n_fft/2 + 1][2], frames [B][T][n_fft] */
int dv3_istft_frames_f32_n(const float* mag, const float* phasor /* NULL: zero phase */,
                           float* frames, int32_t B, int32_t T, int32_t n_fft, void* stream);
int dv3_overlap_add_f32(const float* frames, float* y, int32_t B, int32_t T, int32_t hop,
                        void* stream);
/* frames [B][T][n_fft] -> y [B][hop * (T - 1)], hop <= n_fft */
int dv3_overlap_add_f32_n(const float* frames, float* y, int32_t B, int32_t T, int32_t hop, int32_t n_fft,
                          void* stream);
/* one Griffin-Lim projection, fused: frames = istft_frames(mag, phase(stft(y))) without storing the phasors */
int dv3_gl_project_f32(const float* y, const float* mag, float* frames, int32_t B, int32_t T, int32_t hop,
                       void* stream);
/* y [B][hop * (T - 1)] (longer than n_fft/2), mag [B][T][n_fft/2 + 1] -> frames [B][T][n_fft] */
int dv3_gl_project_f32_n(const float* y, const float* mag, float* frames, int32_t B, int32_t T, int32_t hop,
                         int32_t n_fft, void* stream);
/* outputs (each may be NULL): phasor, spec = the complex STFT [B][T][513][2], mag_bct = |STFT|
 * as [B][513][T] (the channel-major operand of the mel filterbank GEMM)                     */
int dv3_stft_phase_f32(const float* y, float* phasor, float* spec, float* mag_bct, int32_t B,
                       int32_t T, int32_t hop, void* stream);
/* y [B][hop * (T - 1)] (longer than n_fft/2) -> phasor, spec [B][T][n_fft/2 + 1][2], mag_bct [B][n_fft/2 + 1][T] */
int dv3_stft_phase_f32_n(const float* y, float* phasor, float* spec, float* mag_bct, int32_t B,
                         int32_t T, int32_t hop, int32_t n_fft, void* stream);
/* Forward analysis (audio.py:21-23,31-35,46-51,79-89): preemphasis, then dv3_stft_phase_f32
 * (mag_bct), the mel filterbank as a 1x1 tap-GEMM (dv3_conv_gemm_f32, M = num_mels, Cin = 513),
 * then amplitude -> dB -> [0,1] normalisation.                                              */
int dv3_preemphasis_f32(const float* x, float* y, int32_t B, int32_t L, float coef, void* stream);
int dv3_amp_to_db_norm_f32(const float* x, float* out, int64_t n, float min_level_db,
                           float ref_level_db, void* stream);
/* y[n] = x[n] + coef*y[n-1] per row: inv_preemphasis, audio.py:26-28 (nnmnkwii's lfilter([1], [1, -coef])).  x != y
 * runs chunked in parallel over the row (exact to fp32 rounding for |coef| well below 1: each 3072-sample chunk restarts
 * 1024 samples early); x == y, or a coefficient whose memory outlasts the warm-up, runs one workgroup per row. */
int dv3_deemphasis_f32(const float* x, float* y, int32_t B, int32_t L, float coef, void* stream);

/* The same analysis / inverse on the framing of `lws.lws(fft_size, hop_size, mode="speech")` (audio.py:54-55), which the
 * reference uses for its features (`.stft`, audio.py:31-35,46-51) and for the framing of its inverse (`.istft`,
 * audio.py:42) -- the package's published conventions (python/lws.pyx; restated and cited in oracle/audio_oracle.py):
 *   awin  [1024]  analysis window: sqrt of the SYMMETRIC Hann window
 *   swin  [1024]  perfect-reconstruction synthesis window: awin / overlap-added(awin^2) -- no division in the overlap-add
 *   the signal is padded with 1024 - hop ZEROS on both sides (no reflection): T frames cover L <= (T + 1) * hop - 1024
 *   samples, frame t starts at sample t * hop - (1024 - hop).
 * Both tables are built on the host (deepvoice3_pytorch_amd/audio.py: lws_windows).  Phase reconstruction is Griffin-Lim
 * (north_star) on this framing, not lws's own run_lws iterations. */
int dv3_lws_stft_f32(const float* y, const float* awin, float* phasor, float* spec, float* mag_bct, int32_t B, int32_t T,
                     int32_t hop, int32_t L, void* stream);
int dv3_lws_istft_frames_f32(const float* mag, const float* phasor /* NULL: zero phase */, const float* swin, float* frames,
                             int32_t B, int32_t T, void* stream);
/* y [B][(T + 1) * hop - 1024] */
int dv3_lws_overlap_add_f32(const float* frames, float* y, int32_t B, int32_t T, int32_t hop, void* stream);
int dv3_lws_gl_project_f32(const float* y, const float* mag, const float* awin, const float* swin, float* frames, int32_t B,
                           int32_t T, int32_t hop, void* stream);
/* The siblings on `lws.lws(n_fft, hop)`: awin / swin [n_fft] (audio.py: lws_windows(device, hop, scale, n_fft)), n_fft - hop
 * zeros of padding on both sides, T frames cover L <= (T + 1) * hop - n_fft samples (and more than T - 1 frames do),
 * n_fft/2 + 1 bins, frames [B][T][n_fft]; overlap-add and gl_project work on y [B][(T + 1) * hop - n_fft], which must be
 * positive. */
int dv3_lws_stft_f32_n(const float* y, const float* awin, float* phasor, float* spec, float* mag_bct, int32_t B, int32_t T,
                       int32_t hop, int32_t L, int32_t n_fft, void* stream);
int dv3_lws_istft_frames_f32_n(const float* mag, const float* phasor /* NULL: zero phase */, const float* swin, float* frames,
                               int32_t B, int32_t T, int32_t n_fft, void* stream);
int dv3_lws_overlap_add_f32_n(const float* frames, float* y, int32_t B, int32_t T, int32_t hop, int32_t n_fft, void* stream);
int dv3_lws_gl_project_f32_n(const float* y, const float* mag, const float* awin, const float* swin, float* frames, int32_t B,
                             int32_t T, int32_t hop, int32_t n_fft, void* stream);

/* ABI 44 (per-utterance synthesis): the same inverse on a batch padded to T frames whose item b has only tlen[b] frames
 * (device int32[B]); lws = 1: the lws framing (swin / awin as above), 0: the torch framing.  Item b uses its own frames,
 * its own signal end (L_b = (tlen[b] + 1) * hop - 1024, or hop * (tlen[b] - 1)) for the reflection / zero padding and its
 * own overlap-add normaliser: exactly its B = 1 call on its own trimmed spectrogram.  Rows stay L(T) samples apart;
 * samples from L_b on are written as zeros; frames past tlen[b] are neither written nor read.  tlen[b] is clamped into
 * [fewest frames the framing takes at this hop, T] (T must be at least that).  */
int dv3_gl_istft_items_f32(const float* mag, const float* phasor /* NULL: zero phase */, const float* swin, float* frames,
                           int32_t B, int32_t T, int32_t hop, const int32_t* tlen, int32_t lws, void* stream);
int dv3_overlap_add_items_f32(const float* frames, float* y, int32_t B, int32_t T, int32_t hop, const int32_t* tlen,
                              int32_t lws, void* stream);
int dv3_gl_project_items_f32(const float* y, const float* mag, const float* awin, const float* swin, float* frames,
                             int32_t B, int32_t T, int32_t hop, const int32_t* tlen, int32_t lws, void* stream);
/* The siblings at n_fft: n_fft/2 + 1 bins, frames [B][T][n_fft], L_b = (tlen[b] + 1) * hop - n_fft on the lws framing or
 * hop * (tlen[b] - 1) on the torch one; the fewest frames are the fewest with L_b > 0 (lws) or L_b > n_fft/2 (torch). */
int dv3_gl_istft_items_f32_n(const float* mag, const float* phasor /* NULL: zero phase */, const float* swin, float* frames,
                             int32_t B, int32_t T, int32_t hop, const int32_t* tlen, int32_t lws, int32_t n_fft,
                             void* stream);
int dv3_overlap_add_items_f32_n(const float* frames, float* y, int32_t B, int32_t T, int32_t hop, const int32_t* tlen,
                                int32_t lws, int32_t n_fft, void* stream);
int dv3_gl_project_items_f32_n(const float* y, const float* mag, const float* awin, const float* swin, float* frames,
                               int32_t B, int32_t T, int32_t hop, const int32_t* tlen, int32_t lws, int32_t n_fft,
                               void* stream);
/* Fast Griffin-Lim (Perraudin, Balazs & Sondergaard 2013): one projection with a momentum term on the consistent
 * spectrum, for both framings (lws = 1 / 0), the whole batch (tlen NULL) or per item (tlen as above), n_fft = 512, 1024
 * or 2048.  With c = STFT(y) and c_prev what the previous call left in cprev,
 *   t = c + alpha (c - c_prev),   frames = window * irfft(mag * t / max(|t|, 1e-8)),   cprev <- c   (in place)
 * Only the phase of t is used, so alpha is the `momentum` of librosa / torchaudio (their c - alpha / (1 + alpha) c_prev is
 * t / (1 + alpha)).
 *   cprev  [B][T][n_fft/2 + 1][2] floats (re, im) in the frame order of mag, 8-byte aligned; rows of frames at or past
 *          tlen[b] are neither read nor written
 *   first  nonzero: cprev holds nothing yet -- it is not read (t = c: the call projects as dv3_gl_project_items_f32_n
 *          does) and is still written.  The first projection of a reconstruction passes 1, the others 0.
 *   alpha  in [0, 1); alpha = 0 projects as the entry points above do, and still keeps c in cprev
 * The other arguments and their checks are those of dv3_gl_project_f32_n / dv3_lws_gl_project_f32_n (tlen NULL) and
 * dv3_gl_project_items_f32_n, and hop <= n_fft on both framings; a NULL or misaligned cprev, alpha outside [0, 1) or NaN:
 * DV3_EINVAL before anything is launched.  The overlap-add that follows is dv3_overlap_add_f32_n /
 * dv3_lws_overlap_add_f32_n / dv3_overlap_add_items_f32_n.  (Added under ABI 49: nothing existing changed.) */
int dv3_gl_project_momentum_f32(const float* y, const float* mag, const float* awin, const float* swin, float* cprev,
                                float* frames, int32_t B, int32_t T, int32_t hop, const int32_t* tlen, int32_t lws,
                                int32_t n_fft, float alpha, int32_t first, void* stream);
/* de-emphasis of row b over its own first lens[b] samples (device int32[B]); the rest of the row is written as zeros */
int dv3_deemphasis_items_f32(const float* x, float* y, int32_t B, int32_t L, const int32_t* lens, float coef,
                             void* stream);

/* ABI 45 (ragged forward analysis): audio.spectrogram / audio.melspectrogram of B utterances of different lengths in one
 * launch, written as the time-major packed rows PackedBatch.lin / .mel hold (deepvoice3_pytorch_amd/data.py).  Replaces
 * the reference's per-utterance preprocessing: audio.py:31-35,46-51 (preemphasis -> lws stft -> |.| -> [mel] -> dB ->
 * normalise) as ljspeech.py:40-76 calls it, rescaling included.
 *   x         flat fp32 samples; item b is x[soff[b] .. soff[b+1])            soff: device int64[B+1], soff[0] = 0
 *   foff      device int32[B+1]: output rows of item b are foff[b] .. foff[b+1), foff[b+1] - foff[b] = T_b =
 *             lws_num_frames(L_b) = ceil((L_b + 1024 - 2 hop) / hop) + 1; n_frames = foff[B] (rows written)
 *   awin      [1024] lws analysis window (as dv3_lws_stft_f32)
 *   gain      device float[B] or NULL: item b is analysed as the fp32 products x[i] * gain[b], each rounded on its own
 *   mel_basis [n_mels][513] filterbank; mel_band device int32[n_mels][2] or NULL: filter m's nonzero bins lie in
 *             [band[2m], band[2m+1]) (NULL: all 513)
 *   lin       [n_frames][513], mel [n_frames][n_mels] (either may be NULL), both in [0, 1]
 * Frame t of item b reads item b's samples only, zeros outside [0, L_b) (the lws framing: 1024 - hop zeros in front),
 * preemphasis inline with y[0] = x[0].  Every row is a function of its own item alone -- not of B, order, neighbours or
 * padding: the linear row takes the same expressions as dv3_preemphasis_f32 -> dv3_lws_stft_f32 (mag) ->
 * dv3_amp_to_db_norm_f32, bit for bit what a B = 1 batch call gives; the mel row is one fmaf chain per filter over its
 * bins in ascending order (acc = fmaf(w[m][k], |X[k]|, acc) from acc = 0), then the same dB normalisation. */
int dv3_analysis_items_f32(const float* x, const int64_t* soff, const int32_t* foff, int32_t B, int32_t n_frames,
                           int32_t hop, float preemphasis, const float* awin, const float* gain, const float* mel_basis,
                           const int32_t* mel_band, int32_t n_mels, float min_level_db, float ref_level_db, float* lin,
                           float* mel, void* stream);
/* The sibling at n_fft: T_b = ceil((L_b + n_fft - 2 hop) / hop) + 1 frames, awin [n_fft], mel_basis [n_mels][n_fft/2 + 1],
 * mel_band clamped into [0, n_fft/2 + 1], lin [n_frames][n_fft/2 + 1]; n_fft - hop zeros in front of each item. */
int dv3_analysis_items_f32_n(const float* x, const int64_t* soff, const int32_t* foff, int32_t B, int32_t n_frames,
                             int32_t hop, float preemphasis, const float* awin, const float* gain, const float* mel_basis,
                             const int32_t* mel_band, int32_t n_mels, float min_level_db, float ref_level_db, float* lin,
                             float* mel, int32_t n_fft, void* stream);
/* hparams.rescaling (ljspeech.py:59-60): gain[b] = rescaling_max / m_b in fp32 (one correctly rounded division),
 * m_b = max |x[i]| over item b's samples; gain[b] = 1 when m_b = 0.  The reference scales as (x / m_b) * rescaling_max;
 * here x * gain[b] (dv3_analysis_items_f32), which differs from it by at most an ulp or two per sample. */
int dv3_item_gain_f32(const float* x, const int64_t* soff, int32_t B, float rescaling_max, float* gain, void* stream);

/* ABI 46 (waveform preparation for multi-speaker corpora): what the reference's VCTK preprocessing does on the host before
 * the features -- librosa.load(path, sr=hparams.sample_rate) (audio.py:12-13) and librosa.effects.trim (vctk.py:52-67) --
 * as ragged launches over B utterances packed back to back.  Every output value is a function of its own item alone: not
 * of B, the order, the neighbours or the grid.
 *
 * dv3_resample_items_f32: band-limited resampling by the rational ratio up / down (lowest terms, each <= 4096, up != down;
 * 48 kHz -> 22.05 kHz is 147 / 320).
 *   x      flat fp32 samples; item b is x[ioff[b] .. ioff[b+1]), L_b samples          ioff: device int64[B+1]
 *   y      item b's output is y[ooff[b] .. ooff[b+1]); the caller sizes it ceil(L_b up / down) as librosa.resample does
 *   toff   device int32[B+1]: item b owns workgroups toff[b] .. toff[b+1) = ceil(outputs_b / dv3_resample_tile(up, down)),
 *          n_tiles = toff[B]
 *   table  device float[2H + 2][up], H = ceil(64 / s), s = min(1, up / down): table[j][r] = fp32_rn(h(H - j + frac)) with
 *          frac = ((r down) mod up) / up, evaluated in fp64 on the host, where
 *            h(t) = s rho sinc(rho s t) w(|t| s / 64),  sinc(u) = sin(pi u) / (pi u),  rho = 0.9475937167399596,
 *            w(u) = I0(beta sqrt(1 - u^2)) / I0(beta) for u < 1, else 0,                beta = 14.769656459379492
 *          (the published design parameters of resampy's "kaiser_best" filter -- 64 zero crossings, that roll-off, that
 *          Kaiser beta --, which librosa.load used in the reference's era; in closed form, not its interpolated table).
 * Output n sits at input position n down / up: i0 = (n down) div up, r = n mod up, and
 *   y[n] = sum over j = 0 .. 2H + 1 of table[j][r] * x[i0 - H + j],   x = 0 outside [0, L_b),
 * accumulated in fp32 as ONE chain acc = fmaf(table[j][r], x[.], acc) from acc = 0 with j ascending (k ascending): the
 * roundings are the table's (one fp32 rounding per coefficient) and one per fmaf, so
 * |y - exact| <= (2H + 4) 2^-24 sum_j |h_j x_j|.  dv3_resample_tile -> outputs per workgroup for this ratio, or
 * DV3_EINVAL for a ratio the kernel does not take (a term above 4096, or a tile window above 64 KiB of LDS). */
int dv3_resample_tile(int32_t up, int32_t down);
int dv3_resample_items_f32(const float* x, const int64_t* ioff, const int64_t* ooff, const int32_t* toff, int32_t B,
                           int32_t n_tiles, int32_t up, int32_t down, const float* table, float* y, void* stream);
/* dv3_trim_items_f32: librosa.effects.trim(y, top_db) at its defaults (frame_length 2048, hop_length 512, centred frames,
 * ref = max), applied to spans: span b is x[start[b] .. start[b] + len[b]) (device int64[B] each).
 *   foff   device int32[B+1]: span b's frames are rows foff[b] .. foff[b+1) of mse, 1 + len[b] div 512 of them for
 *          len[b] >= 1025 and NONE for a shorter span; n_frames = foff[B]; mse: device float[n_frames] scratch (on return
 *          the frame powers)
 *   top_db device float[B] (vctk.py: 25 after a label cut, 15 otherwise)
 * Frame f covers span samples [512 f - 1024, 512 f + 1024), reflected at both ends as numpy.pad(mode="reflect") does
 * (librosa <= 0.9).  mse[f] = (sum of squares) / 2048 in fp32: lane t of 256 adds v^2 of samples t, t + 256, ... by fmaf,
 * the 256 partial sums are added in a fixed binary tree.  db[f] = 10 log10f(max(1e-10, mse[f])) - 10 log10f(max(1e-10,
 * max_f mse[f])); frame f is non-silent iff db[f] > -top_db[b].  With first / last the non-silent frames' extremes,
 *   out_start[b] = start[b] + 512 first,  out_len[b] = min(len[b], 512 (last + 1)) - 512 first
 * (device int64[B]); (start[b], 0) when no frame is non-silent (top_db <= 0 only: the loudest frame is at 0 dB).  A span
 * shorter than 1025 samples can not be reflect-padded (numpy raises): it is returned unchanged.  Two launches: the frame
 * powers, then one workgroup per span for the maximum and the two extremes. */
int dv3_trim_items_f32(const float* x, const int64_t* start, const int64_t* len, const int32_t* foff, int32_t B,
                       int32_t n_frames, const float* top_db, float* mse, int64_t* out_start, int64_t* out_len,
                       void* stream);
/* dv3_gather_spans_f32: y[ooff[b] + i] = x[start[b] + i], i < len[b] (device int64[B] / int64[B] / int64[B+1]; B <= 65535;
 * max_len >= every len[b] sizes the grid): the trimmed spans back to back, so that dv3_item_gain_f32 and
 * dv3_analysis_items_f32 run on them unchanged.  A copy: no rounding.  16 bytes per lane wherever the destination is
 * 16-byte aligned (per span: a head of <= 3 floats, the aligned body, a tail of <= 3). */
int dv3_gather_spans_f32(const float* x, const int64_t* start, const int64_t* len, const int64_t* ooff, int32_t B,
                         int64_t max_len, float* y, void* stream);

/* ------------------------------------------------------------------------------------
 * Alignment diagnostics for free-running synthesis (synthesis.tts_batch / RollingSynthesizer).
 * Additions to ABI 49: one entry point, a scratch-size query and a constant; nothing existing changed, so the version
 * stays 49.
 *
 * attn[b * item_stride + t * step_stride + n] (strides in elements) is the probability item b gave key n at its OWN
 * step t -- the rows the step kernels stored.  Both layouts in use are read in place: the step program's stacked buffer
 * (t_cap or n_max, B, Tk) with item_stride = Tk, step_stride = B * Tk, and a contiguous (B, T, Tk).  steps[b] is clamped
 * to [0, T] and key_len[b] to [1, Tk] (device int32[B]); only elements t < T_b = steps[b], n < N_b = key_len[b] are
 * read, and attn is never written.
 *
 * Per row t < T_b:  path[t] = argmax over n < N_b, the FIRST maximum (the rule of dv3_attn_step_f32 and
 * dv3_attn_argmax_i32, deepvoice3.py:445); a NaN never wins.  peak[t] = max / sum_n P[t, n].  A row whose sum is not
 * finite or is <= 0, or in which no element wins, is BAD: path = 0, peak = 0.
 *
 * out[b] = DV3_ALIGN_COLS fp32 columns (path[-1] = 0; names: synthesis.ALIGNMENT_COLUMNS):
 *    0 steps         T_b                          1 keys           N_b
 *    2 focus_mean    mean of peak over t < T_b    3 focus_min      their minimum              (both 0 when T_b = 0)
 *    4 last_key      path[T_b - 1]; 0 when T_b = 0
 *    5 furthest_key  max_t path[t]
 *    6 end_step      first t with path[t] >= N_b - 1; -1 if none
 *    7 tail_steps    T_b - 1 - end_step when end_step >= 0, otherwise 0
 *    8 covered_keys  distinct values in path[0 .. T_b)
 *    9 back_steps    number of t >= 1 with path[t] < path[t - 1]
 *   10 max_jump      max over t >= 0 of path[t] - path[t - 1], floored at 0
 *   11 longest_stall longest run of equal consecutive path values; 0 when T_b = 0
 *   12 bad_rows      number of bad rows
 * Every column but the two focus ones is an integer, exact in fp32.  The focus columns carry the fp32 row sum's
 * rounding (lane-strided partial sums, then a 64-lane tree: < 4e-6 relative for Tk <= 4096).
 *
 * Two launches: a 64-lane wave per row (rows of an item spread over workgroups) writes path / peak to `scratch`
 * (>= dv3_alignment_stats_scratch_bytes(B, T) bytes, 4-byte aligned; the query returns 0 for B or T < 1 or when
 * B * T * 8 does not fit an int), then one wave per item scans them.  No floating-point atomics: two calls give
 * bit-equal output.  Refused (non-zero, dv3_last_error names the argument, nothing launched): a null pointer; B, T or
 * Tk < 1; B > 65535; Tk > 4096 (the distinct-key bitmap); out or scratch not 4-byte aligned.
 * ------------------------------------------------------------------------------------ */
#define DV3_ALIGN_COLS 13
int dv3_alignment_stats_scratch_bytes(int32_t B, int32_t T);
int dv3_alignment_stats_f32(const float* attn, int64_t item_stride, int64_t step_stride,
                            int32_t B, int32_t T, int32_t Tk,
                            const int32_t* steps, const int32_t* key_len,
                            float* out /* B x DV3_ALIGN_COLS */, void* scratch, void* stream);

/* ------------------------------------------------------------------------------------
 * Batched dynamic time warping (ops.dtw, synthesis.mel_distortion / evaluate_synthesis).
 * Additions to ABI 49: a descriptor, one entry point, a scratch-size query and three constants; nothing existing
 * changed, so the version stays 49.
 *
 * For every item b, x[b] (Tx, D) and y[b] (Ty, D) fp32 are read in place through their batch and time strides (in
 * elements; the feature axis is dense), over the frames i < Lx = x_len[b] and j < Ly = y_len[b] (device int32[B],
 * clamped to [0, Tx] and [0, Ty]).  Frames at or past a length are NEVER read: they may hold anything, NaN included.
 *
 *   local cost   d(i, j) = sqrt(sum_k (x[b,i,k] - y[b,j,k])^2): from the differences themselves, summed in feature order
 *                in fp32, the square root correctly rounded
 *   recurrence   C(0, 0) = d(0, 0);  C(i, j) = d(i, j) + min(C(i-1, j-1), C(i-1, j), C(i, j-1)), in fp32
 *   tie-break    the predecessors are tried in that order -- diagonal, x advances, y advances -- and a later one replaces
 *                an earlier one only when it is STRICTLY smaller.  Part of the interface: the integer outputs depend on it.
 *
 * out[b] = DV3_DTW_COLS fp32 columns:  0 cost = C(Lx-1, Ly-1)   1 path_len   2 n_diag   3 n_x_only   4 n_y_only
 * -- the moves of the chosen path, carried with the cost through the scan (no backtracking); integers, exact in fp32;
 * path_len = 1 + n_diag + n_x_only + n_y_only, n_diag + n_x_only = Lx - 1, n_diag + n_y_only = Ly - 1.
 * path (optional, int32 (B, Tx + Ty - 1, 2)): path[b, s] = (i, j) of the s-th cell of the chosen path, s < path_len, in
 * forward order from (0, 0) to (Lx-1, Ly-1); every row s >= path_len is (-1, -1).  `out` does not depend on `path`.
 * An item with a zero length: all five columns 0, its path all -1.  An item with a non-finite feature inside its
 * lengths (or whose squared distance overflows fp32): cost = NaN, its other columns and its path unspecified (valid
 * memory, no fault); the other items are untouched.
 *
 * Three launches (two without a path): a tiled distance pass writes d to scratch, one 64-lane wave per item scans the
 * recurrence (rows pipelined across lanes, each lane a strip of ceil(Ty / 64) columns), one workgroup per item walks the
 * stored direction bytes back.  scratch: >= dv3_dtw_scratch_bytes(...) bytes = B * Tx * Ty * (4 + (want_path ? 1 : 0)),
 * 4-byte aligned; the size goes out through the pointer (it passes 2^31 at accepted sizes).  No atomics: two calls give
 * bit-equal output.  Refused (DV3_EINVAL, dv3_last_error names the numbers, nothing launched): a null pointer (path
 * excepted); B < 1; Tx or Ty outside [1, DV3_DTW_MAX_T]; D outside [1, DV3_DTW_MAX_D]; a feature stride other than 1
 * (D > 1); scratch_bytes below the query; out, path or scratch not 4-byte aligned.
 * ------------------------------------------------------------------------------------ */
#define DV3_DTW_COLS 5
#define DV3_DTW_MAX_T 4096
#define DV3_DTW_MAX_D 128
typedef struct dv3_dtw_desc {
  const float* x;                            /* (B, Tx, D) through the strides below                                  */
  const float* y;                            /* (B, Ty, D)                                                            */
  const int32_t* x_len;                      /* device int32[B]                                                       */
  const int32_t* y_len;
  int64_t x_batch_stride, x_time_stride, x_feat_stride;     /* in elements; x_feat_stride must be 1 (any when D = 1)  */
  int64_t y_batch_stride, y_time_stride, y_feat_stride;
  int32_t B, Tx, Ty, D;
  float* out;                                /* B x DV3_DTW_COLS                                                      */
  int32_t* path;                             /* null, or B x (Tx + Ty - 1) x 2                                        */
  void* scratch;
  int64_t scratch_bytes;
} dv3_dtw_desc;
int dv3_dtw_scratch_bytes(int32_t B, int32_t Tx, int32_t Ty, int32_t want_path, int64_t* bytes_out);
int dv3_dtw_f32(const dv3_dtw_desc* d, void* stream);

/* ------------------------------------------------------------------------------------
 * Monotonic alignment search: token timings from stored attention rows (ops.monotonic_path, synthesis.token_timings,
 * train_step.align_batch).  Additions to ABI 49: a descriptor, one entry point, a scratch-size query
 * and five constants; nothing existing changed, so the version stays 49.
 *
 * attn[l * layer_stride + b * item_stride + t * step_stride + n] (fp32, strides in elements, the key axis dense) is the
 * probability layer l of item b gave key n at step t.  Read in place: the step program's stacked (T, B, Tk), a
 * contiguous (B, T, Tk) and the teacher-forced (L, B, T, Tk) are all strides of it; with n_layers = L = 1 the layer
 * stride is ignored.  steps[b] is clamped to [0, T] and key_len[b] to [1, Tk] (device int32[B]) as in
 * dv3_alignment_stats_f32; only elements t < T_b = steps[b], n < N_b = key_len[b] are read -- the others may hold
 * anything, NaN included -- and attn is never written.
 *
 *   score        Pm[t, n] = (sum over l = 0 .. L-1, in that order, of attn[l, b, t, n]) / L, in fp32;
 *                s[t, n] = logf(fmaxf(Pm[t, n], DV3_MONO_FLOOR)), the full-precision logf; a NaN scores as the floor
 *   path rules   J = max_advance in [1, DV3_MONO_MAX_ADVANCE].  path[t] in [0, N_b) for t < T_b with
 *                path[0] <= J - 1;   0 <= path[t] - path[t-1] <= J;   path[T_b - 1] >= N_b - J
 *                -- at most J - 1 consecutive keys are skipped anywhere, the two ends included.  J = 1 is the classic
 *                search: start on the first key, end on the last, stay or advance by one.
 *   recurrence   Q[0, n] = s[0, n];   Q[t, n] = s[t, n] + max over 0 <= j <= J of Q[t-1, n-j], over the predecessors that
 *                exist and can be reached, in fp32.  The chosen path maximises the sum of s along it.
 *   tie-break    the advances are tried in the order j = 0, 1, .. J and a larger one replaces a smaller one only when it
 *                is STRICTLY greater; among the admissible end keys N_b - 1 is tried first and a smaller key replaces it
 *                only when STRICTLY greater.  Part of the interface: the integer outputs depend on it.
 *
 * out[b] = DV3_MONO_COLS fp32 columns (names: synthesis.TIMING_COLUMNS):
 *    0 feasible      1 when a path satisfies the rules, else 0
 *    1 steps         T_b                          2 keys           N_b
 *    3 score         Q of the chosen end cell (the fp32 recurrence's value)
 *    4 skipped_keys  keys n < N_b with duration 0
 *    5 longest       the largest duration
 * path (B, T) int32: the key of every step, -1 at t >= T_b.  durations (B, Tk) int32: the number of steps assigned to
 * each key (the histogram of path), 0 at n >= N_b; for a feasible item they sum to T_b.  All three are always fully
 * written.  An INFEASIBLE item -- no path satisfies the rules, e.g. N_b > (T_b + 1) * J - 1, or T_b = 0 -- has
 * feasible = 0, score = 0, columns 4 and 5 = 0, its path all -1 and its durations all 0; steps and keys are still
 * written, and the other items are untouched.
 *
 * What the figures are: the best monotonic reading of THIS model's attention, at decoder-step resolution (one step is
 * r mel frames; r * downsample_step frames of a recording under teacher forcing).  They are not a phonetic aligner's
 * output.
 *
 * Three launches: a score pass (one wave per row) writes s to scratch inside each item's lengths; one 64-lane wave per
 * item scans the recurrence (key n in lane n % 64, the predecessors by cross-lane moves, the rows of the next steps in
 * flight) and stores one back-pointer byte per cell; one wave per item walks the bytes back through LDS.  scratch:
 * >= dv3_mono_path_scratch_bytes(...) bytes = 4 * B * T * Tk + (B * T * Tk rounded up to a multiple of 4), 4-byte
 * aligned; the size goes out through the pointer (it passes 2^31 at accepted sizes).  No floating-point atomics: two
 * calls give bit-equal output.  Refused (DV3_EINVAL, dv3_last_error names the argument, nothing launched): a null
 * pointer; B < 1 or B > 65535; T outside [1, DV3_MONO_MAX_T]; Tk outside [1, DV3_MONO_MAX_TK]; max_advance outside
 * [1, DV3_MONO_MAX_ADVANCE]; n_layers < 1; scratch_bytes below the query; out, path, durations or scratch not 4-byte
 * aligned.
 * ------------------------------------------------------------------------------------ */
#define DV3_MONO_COLS 6
#define DV3_MONO_MAX_T 8192
#define DV3_MONO_MAX_TK 2048
#define DV3_MONO_MAX_ADVANCE 8
#define DV3_MONO_FLOOR 1e-20f
typedef struct dv3_mono_desc {
  const float* attn;                         /* (L, B, T, Tk) through the strides below                               */
  const int32_t* steps;                      /* device int32[B]                                                       */
  const int32_t* key_len;
  int64_t layer_stride, item_stride, step_stride;           /* in elements; layer_stride ignored when n_layers = 1   */
  int32_t n_layers, B, T, Tk, max_advance;
  float* out;                                /* B x DV3_MONO_COLS                                                     */
  int32_t* path;                             /* B x T                                                                 */
  int32_t* durations;                        /* B x Tk                                                                */
  void* scratch;
  int64_t scratch_bytes;
} dv3_mono_desc;
int dv3_mono_path_scratch_bytes(int32_t B, int32_t T, int32_t Tk, int64_t* bytes_out);
int dv3_mono_path_f32(const dv3_mono_desc* d, void* stream);

/* ------------------------------------------------------------------------------------
 * Mel-to-linear inversion: a normalised linear spectrogram estimated from a normalised mel spectrogram, so that a mel
 * can be put through Griffin-Lim (audio.mel_to_linear, audio.inv_melspectrogram_batch, synthesis `from_mel=`; DESIGN.md
 * 3.6g).  Additions to ABI 49: one entry point and two constants; nothing existing changed, so the version stays 49.
 *
 * mel [B][T][n_mels] fp32, normalised; tlen device int32[B] (item b has tlen[b] frames in [0, T]; NULL: all have T);
 * basis [n_mels][n_bins] fp32, the filterbank W; mel_band int32[n_mels][2], [first, last + 1) of filter m's nonzero bins
 * (the table of dv3_analysis_items_f32); bin_band int32[n_bins][2], [first, last + 1) of the filters whose band holds
 * bin k; inv_basis_sum = 1 / (the sum of all of W); lin [B][T * upsample][n_bins].  Output frame t < upsample * tlen[b]
 * of item b, with u = upsample, i0 = t / u, i1 = min(i0 + 1, tlen[b] - 1), f = (t % u) / u:
 *
 *   x_m = fmaf(f, clip(mel[b][i1][m], 0, 1), (1 - f) * clip(mel[b][i0][m], 0, 1))        frame i u is mel frame i exactly
 *   a_m = 10^((x_m * (-min_level_db) + min_level_db + ref_level_db) / 20)                 > 0
 *   b_k = sum_m W[m][k] a_m;   s_k = covered_k * (sum_m a_m) * inv_basis_sum,   covered_k = (sum_m W[m][k] > 0)
 *   iters times:   r_m = sum_k W[m][k] s_k;   d_k = sum_m W[m][k] r_m;   s_k = s_k * (b_k / max(d_k, 1e-30))
 *   lin[b][t][k] = clip((20 log10(max(10^(min_level_db / 20), s_k)) - ref_level_db - min_level_db) / -min_level_db, 0, 1)
 *
 * the last line being dv3_amp_to_db_norm_f32's expression.  Every sum over k is one fmaf chain over the filter's band in
 * ascending bin order, every sum over m one fmaf chain over the bin's filters in ascending filter order, from 0; sum_m
 * a_m is a fixed tree.  The division is IEEE.  A bin under no filter is 0 throughout and comes out as 0.0.  Rows
 * t >= upsample * tlen[b] are written as zeros: every element of lin is written.  A row depends on its own item's rows
 * alone -- not on B, the order of the items, its neighbours or the padding.  The kernel relies on each filter's support
 * lying inside its mel_band and on the filters over a bin lying inside its bin_band (entries are clamped to the
 * arrays, so a wrong table gives wrong numbers, never a wild access); it assumes no number of filters per bin.
 * One 64-lane wave per output frame, s and r in LDS, no workgroup barrier inside the iteration, no atomics: two calls
 * give bit-equal output.  Refused (DV3_EINVAL, dv3_last_error names the argument, nothing launched): a null mel, basis,
 * mel_band, bin_band or lin; B < 1; T < 1; B * T * upsample >= 2^31; n_mels outside [1, DV3_MELINV_MAX_MELS]; n_bins
 * outside [1, 1025]; upsample outside [1, 16]; iters outside [0, DV3_MELINV_MAX_ITERS]; min_level_db not < 0;
 * inv_basis_sum not a positive finite number.  tlen[b] lives on the device and is clamped to [0, T] there.
 * ------------------------------------------------------------------------------------ */
#define DV3_MELINV_MAX_MELS 256
#define DV3_MELINV_MAX_ITERS 1024
int dv3_mel_to_linear_f32(const float* mel, const int32_t* tlen, const float* basis, const int32_t* mel_band,
                          const int32_t* bin_band, float inv_basis_sum, float* lin, int32_t B, int32_t T, int32_t n_mels,
                          int32_t n_bins, int32_t upsample, int32_t iters, float min_level_db, float ref_level_db,
                          void* stream);

/* ------------------------------------------------------------------------------------
 * Single Pass Spectrogram Inversion (Beauregard, Harish & Wyse 2015): a starting phase for Griffin-Lim built from the
 * magnitudes alone, in one pass over the frames (audio.spsi_phasor, AudioConfig(griffin_lim_init="spsi")).
 * The reference's inv_spectrogram (audio.py:37-43) hands the spectrogram to lws.run_lws, which estimates an initial phase
 * before it iterates; the Griffin-Lim here started from zero phase.  An entry point added under ABI 50: no struct
 * changed, so the version stays 50.
 *
 * mag [B][T][F] fp32, F = fft_size / 2 + 1; phasor [B][T][F][2] fp32 (re, im), 8-byte aligned: the layout the inverse
 * entry points take as `phasor`; tlen device int32[B] (item b has tlen[b] frames, clamped into [0, T]) or NULL (all T).
 * Per item an accumulator acc[F] in TURNS, zero before frame 0.  For frame t < tlen[b], m = mag[b][t], all in fp64:
 *
 *   peak(k)   1 <= k <= F - 2 and m[k] > m[k-1] and m[k] >= m[k+1]
 *   d         0.5 (m[k-1] - m[k+1]) / (m[k-1] - 2 m[k] + m[k+1])             |d| <= 0.5 at a peak
 *   new[k]    frac(acc[k] + ((hop k) mod fft_size) / fft_size + hop d / fft_size)            in [0, 1)
 *   owner(j)  of a non-peak bin: owner(j+1) if m[j+1] > m[j], else owner(j-1) if m[j-1] > m[j], else none; a climb
 *             that ends on a non-peak (a plateau, bin 0, bin F - 1) has none
 *   new[j]    new[owner(j)], 0 without an owner;   acc <- new (the whole row)
 *   phasor[b][t][k] = (-1)^k (cos, sin)(2 pi new[k])
 *
 * the sums in the order written, frac(x) = x - floor(x) with 1.0 taken to 0; new[k] is rounded to fp32 once, for the
 * accurate sincospif.  The (-1)^k: every framing here references a frame's transform to its first sample with the window
 * centred at fft_size / 2, so the bins of one component alternate in sign.  Frames t >= tlen[b] are written as (1, 0):
 * every element of phasor is written, nothing outside it.  One workgroup per item (time is a recurrence), every loop
 * bounded by F, no atomics: two calls give bit-equal output, and an item's rows depend on its own frames alone.
 * Refused (DV3_EINVAL, nothing launched): fft_size other than 512, 1024, 2048; a null mag or phasor; a misaligned
 * phasor; B outside [1, 65535]; T < 1; hop outside [1, fft_size].  tests/spsi_ref.py restates it in numpy.
 * ------------------------------------------------------------------------------------ */
int dv3_spsi_phasor_f32(const float* mag, float* phasor, int B, int T, int hop, const int32_t* tlen /* or NULL */,
                        int fft_size, void* stream);

/* ------------------------------------------------------------------------------------
 * Pitch tracking: YIN (de Cheveigne & Kawahara 2002, steps 2-5) per frame of B utterances packed back to back, for F0 and
 * voicing error in evaluation.  One new entry point with plain arguments, no struct added or changed, so
 * the version stays 50.
 *
 * x, soff (device int64[B+1]) and foff (device int32[B+1]) are those of dv3_analysis_items_f32_n, and so is the framing:
 * row t of item b describes the samples of that item's linear / mel row t.  With N = n_fft, s[0 .. N) is item b's signal
 * with N - hop zeros in front and zeros past its end, from sample t hop of that padded signal on; a frame never reads
 * another item.  No pre-emphasis, no window, no gain.  With W = N - tau_max:
 *
 *   d(tau)   sum over j < W of (s[j] - s[j + tau])^2,  tau = 1 .. tau_max, fp32, from the differences themselves
 *   c(tau)   sum over k = 1 .. tau of d(k)
 *   d'(0) = 1;  d'(tau) = d(tau) tau / c(tau), evaluated (d(tau) * float(tau)) / c(tau);  d'(tau) = 1 where c(tau) = 0
 *   lag      search tau ascending over [tau_min, tau_max): at the first tau with d'(tau) < threshold, descend while
 *            d'(tau + 1) < d'(tau) (strictly) and tau + 1 < tau_max; that tau.  If there is none: the smallest tau of the
 *            range that attains the minimum of d'.  An estimate is always given; voicing is the caller's decision from ap.
 *   delta    with a, b, c = d'(lag - 1), d'(lag), d'(lag + 1) and D = (a - 2 b) + c:
 *            clamp(0.5 (a - c) / D, -1, 1) if D > 0, else 0
 *   f0 = sample_rate / (float(lag) + delta);   ap = b;   power = (1 / N) sum over j < N of s[j]^2
 *
 * An all-zero frame gives, exactly, lag = tau_min, f0 = sample_rate / tau_min, ap = 1, power = 0.
 * f0, ap, power: [n_frames] fp32 each; lag: [n_frames] int32 or NULL (the other outputs are the same without it).
 *
 * Summation orders (fixed, no atomics: two calls give bit-equal output, and a row is a function of its own item alone --
 * not of B, the order or the neighbours).  Every term is one rounded difference squared into an fmaf.
 *   d(tau)   the j range is cut into S = max(1, 256 / (tau_max / 4 + 1)) (integer divisions) slices of
 *            4 ceil(ceil(W / S) / 4) consecutive j; per slice a chain over ascending j; the slices added in ascending order
 *   c(tau)   lane l of one wave owns the CH = ceil(tau_max / 64) | 1 consecutive lags from 1 + l CH: its total (a chain
 *            from 0), an inclusive Hillis-Steele scan of the 64 totals, then from the total of the lanes before it a chain
 *            over its own lags
 *   power    thread i of 256 chains s[i], s[i + 256], ...; a wave's 64 sums meet in the xor butterfly (32, 16, .. 1);
 *            the four waves are added in order; one multiplication by 1 / N (exact)
 * Each is a summation tree of non-negative terms, so against exact arithmetic on the same fp32 samples the relative
 * error of a sum is at most (number of terms + 2) 2^-24: a tree of n fmaf / additions errs by at most n 2^-24 of the sum
 * of its terms whatever its order, with no second-order term (Jeannerod & Rump 2013), and the rounded difference
 * squared is within 2 * 2^-24 of the exact one:
 *   power    (N + 2) 2^-24
 *   d(tau)   (W + 2) 2^-24;   c(tau)  (W + tau + 2) 2^-24  (tau - 1 additions of d on top of d's own error)
 *   d'(tau)  (2 W + tau + 8) 2^-24  (d, c, the product with tau, the quotient; the second-order remainder of the
 *            quotient is below 2 * 2^-24 at every size taken)
 * These hold while no square underflows; tests/pitch_ref.py restates the definition in float64.
 *
 * Refused (DV3_EINVAL, dv3_last_error starts "yin_items:" and names the numbers, nothing launched): a null x, soff, foff,
 * f0, ap or power; B < 1; n_frames < 1; n_fft other than 512, 1024, 2048; hop outside [1, n_fft]; tau_min < 2; tau_max above
 * n_fft / 2 (at most DV3_YIN_MAX_LAG); tau_min + 1 >= tau_max; threshold outside (0, 1]; sample_rate not finite and positive.
 * ------------------------------------------------------------------------------------ */
#define DV3_YIN_MAX_LAG 1024
int dv3_yin_items_f32(const float* x, const int64_t* soff, const int32_t* foff, int32_t B, int32_t n_frames, int32_t hop,
                      int32_t n_fft, int32_t tau_min, int32_t tau_max, float threshold, float sample_rate,
                      float* f0, float* ap, float* power, int32_t* lag, void* stream);

/* ------------------------------------------------------------------------------------
 * Speaking rate and pitch at vocoding: a time-and-frequency warp of the magnitudes Griffin-Lim starts from, with the
 * spectral envelope kept in place so that formants do not move with the pitch (audio.warp_magnitudes, audio.Prosody;
 * DESIGN.md 3.6i).  The reference has no counterpart: its model gives one rate and one pitch per text.  One new entry
 * point with plain arguments, no struct added or changed, so the version stays 50.
 *
 * mag [B][T_in][bins] fp32: the magnitudes dv3_gl_prepare_f32 makes (of the model's linear output, or of
 * dv3_mel_to_linear_f32's); out [B][T_out][bins] fp32, another buffer than mag.  tlen_in device int32[B] or NULL (all
 * T_in), tlen_out device int32[B], both clamped into [0, T_in] / [0, T_out]; rate, ratio device double[B]: rate[b] source
 * frames per output frame (above 1: faster), ratio[b] the factor every frequency is multiplied by (2^(semitones / 12)).
 * With n = tlen_in[b], item b's output frame j < tlen_out[b] (n >= 1) is, in fp32 unless said otherwise, every product
 * and sum rounded once and none contracted:
 *
 *   lerp(a, x, y)  x itself if a == 0, else (1 - a) x + a y
 *   time      u = min(j rate[b], n - 1) in fp64 (a u that is not >= 0 counts as 0);  i0 = floor(u);  a = u - i0 in fp64,
 *             rounded once to fp32;  i1 = min(i0 + 1, n - 1);  m[k] = lerp(a, mag[b][i0][k], mag[b][i1][k]).
 *             Frames at or beyond n are never read.
 *   ratio[b] == 1 (or no positive number):  out[k] = m[k] -- with a == 0 a copy, bit for bit.
 *   otherwise s = k / ratio[b] in fp64.  Where s <= bins - 1:  s0 = floor(s), fa = s - s0 rounded once to fp32,
 *             s1 = min(s0 + 1, bins - 1), and read(v)[k] = lerp(fa, v[s0], v[s1]).
 *   plain (preserve_envelope == 0):   out[k] = read(m)[k] where s <= bins - 1, else m[bins - 1]
 *   envelope-preserving, W = env_half_width:
 *             l[k] = logf(max(m[k], 1e-10f))
 *             E[k] = (sum over kk = max(k - W, 0) .. min(k + W, bins - 1), ascending, of (W + 1 - |kk - k|) l[kk], each
 *                    term one fmaf into the running sum from 0) / (the sum of those integer weights, exact)
 *             X[k] = l[k] - E[k];   X'[k] = read(X)[k] where s <= bins - 1, else 0;   out[k] = expf(E[k] + X'[k])
 *             (the triangular moving average truncated at the edges and renormalised by the weights that remain; logf and
 *             expf are the accurate ones, not the hardware approximations)
 *
 * Rows j >= tlen_out[b] (and every row of an item with n < 1) are written as zeros: every element of out is written,
 * nothing outside it.  One workgroup per output frame, fixed summation order, no atomics: two calls give bit-equal
 * output, and an item's rows depend on its own frames alone -- not on B, its neighbours or the padding.  The caller
 * chooses tlen_out (audio.warp_magnitudes: floor((n - 1) / rate + 0.5) + 1, at least the inverse's shortest signal).
 * Refused (DV3_EINVAL, dv3_last_error starts "prosody_warp:", nothing launched): a null mag, out, tlen_out, rate or ratio;
 * out == mag; misaligned pointers; B outside [1, 65535]; T_in < 1; T_out < 1; bins outside [1, 1025]; preserve_envelope
 * other than 0 or 1; env_half_width outside [1, DV3_PROSODY_MAX_HALF_WIDTH] (in either mode).
 * tests/prosody_ref.py restates the definition in float64.
 * ------------------------------------------------------------------------------------ */
#define DV3_PROSODY_MAX_HALF_WIDTH 64
int dv3_prosody_warp_f32(const float* mag, float* out, int32_t B, int32_t T_in, int32_t T_out, int32_t bins,
                         const int32_t* tlen_in /* or NULL */, const int32_t* tlen_out, const double* rate,
                         const double* ratio, int32_t env_half_width, int32_t preserve_envelope, void* stream);

/* ------------------------------------------------------------------------------------
 * Prosody marks: rate, pitch, level and pauses that vary WITHIN an utterance (audio.ProsodyMarks, audio.plan_prosody,
 * audio.warp_magnitudes_curve).  The warp above with its per-item scalars replaced by per-output-frame
 * tables, and two small kernels that make the tables from segments.  Three new entry points with plain arguments, no
 * struct added or changed, so the version stays 50.  (Their names carry "curve", not the family's prefix: the suite pins
 * the list of entry points named after the family to the scalar warp alone.)
 *
 * dv3_curve_warp_f32: mag, out, tlen_in, tlen_out, bins, env_half_width, preserve_envelope as dv3_prosody_warp_f32 takes
 * them; pos, ratio device double[B][T_out], gain device float[B][T_out].  With n = tlen_in[b] (n >= 1), item b's output
 * frame j < tlen_out[b] is, in fp32 unless said otherwise, every product and sum rounded once and none contracted:
 *
 *   silence   pos[b][j] is not >= 0 (negative, or NaN):  out[k] = 0 for every k; ratio and gain are not looked at.
 *   time      u = min(pos[b][j], n - 1) in fp64;  i0 = floor(u);  a = u - i0 in fp64, rounded once to fp32;
 *             i1 = min(i0 + 1, n - 1);  m[k] = lerp(a, mag[b][i0][k], mag[b][i1][k]), lerp as above.  Frames at or beyond
 *             n are never read.
 *   frequency v[k] = what dv3_prosody_warp_f32 calls out[k], with ratio[b][j] in place of ratio[b]: m[k] itself where the
 *             ratio is 1 or no positive number; else the plain or the envelope-preserving branch, word for word.
 *   gain      out[k] = v[k] where gain[b][j] == 1, else v[k] gain[b][j]: ONE more rounded product.  The gain is NOT
 *             checked on the device: a negative, infinite or NaN gain multiplies as it stands (audio.warp_magnitudes_curve
 *             refuses one before the launch).
 *
 * Rows j >= tlen_out[b] (and every row of an item with n < 1) are zeros; every element of out is written, nothing outside
 * it; one 256-thread workgroup per output frame, fixed summation order, no atomics; an item's rows depend on that item's
 * frames and table rows alone.  With pos[b][j] = j rate[b] (the fp64 product), ratio[b][j] = ratio[b] and gain 1 the
 * output is dv3_prosody_warp_f32's bit for bit: both kernels are one body.
 * Refused (DV3_EINVAL, "curve_warp:", nothing launched): what dv3_prosody_warp_f32 refuses, with pos in the place of rate,
 * and a null gain; gain not 4-byte aligned.
 *
 * Segments -> tables.  Item b has nseg[b] segments (clamped into [1, S]; S <= DV3_PROSODY_MAX_SEGMENTS is the tables'
 * stride): bounds int32[B][S + 1] source frames, and per segment rate, semitones, gain_db double[B][S] and break_frames
 * int32[B][S], the silent frames put in AFTER the segment.  The bounds are repaired as they are read: c_0 = 0,
 * c_s = max(c_{s-1}, min(max(bounds[b][s], 0), n)) for 0 < s < nseg, c_nseg = n.  A rate outside
 * [1 / DV3_PROSODY_MAX_RATE, DV3_PROSODY_MAX_RATE] (or NaN) counts as 1, break_frames is clamped into
 * [0, DV3_PROSODY_MAX_BREAK]; semitones and gain_db are used as they stand (audio.ProsodyMarks checks all of them).
 *
 * dv3_curve_plan_f64: one thread per item, an ascending scan in fp64.  o_0 = 0 and o_{s+1} = o_s + len_s + break_s, with
 *   len_s = 0                                                  for an empty segment (c_{s+1} == c_s)
 *   len_s = floor((c_{s+1} - 1 - c_s) / rate_s + 0.5) + 1      for the segment that ends the item (c_{s+1} == n, non-empty):
 *                                                              the item's last frame keeps its place, as in the scalar warp
 *   len_s = the integer with (len_s - 1) rate_s < c_{s+1} - c_s <= len_s rate_s, both products in fp64 -- ceil((c_{s+1} -
 *           c_s) / rate_s), corrected by one where the rounded quotient crossed an integer -- for every other segment:
 *           its frames stop short of the next segment's first source frame, so the time map stays monotone.
 * o int32[B][S + 1] (entries past nseg[b] repeat o_nseg; sums saturate at 2^31 - 1), tlen_out[b] = max(min_frames, o_nseg).
 * One segment without a break gives audio.warped_frames(n, rate).
 * Refused ("curve_plan:"): a null nseg, bounds, rate, break_frames, o or tlen_out (tlen_in may be NULL: all T_in); rate not
 * 8-byte aligned; B outside [1, 65535]; T_in < 1; S outside [1, DV3_PROSODY_MAX_SEGMENTS]; min_frames < 0.
 *
 * dv3_curve_fill_f64: one thread per (b, j), j < T_out, finds its segment by a scan of o and writes all three tables:
 *   inside segment s (o_s <= j < o_s + len_s)   pos = c_s + (j - o_s) rate_s, one fp64 product and one fp64 sum
 *   in a break (o_s + len_s <= j < o_{s+1})     pos = -1
 *   o_nseg <= j < tlen_out[b]                   (frames the min_frames clamp added) pos = n - 1: the item's last frame is
 *                                               held, with the last segment's semitones and gain_db
 *   j >= tlen_out[b], or n < 1                  pos = -1, ratio = 1, gain = 1
 *   ratio = exp2(semitones / 12) in fp64;  gain = pow(10, gain_db / 20) in fp64, rounded once to fp32 (exactly 1 at 0 dB).
 * ramp_frames = R > 0: a boundary e = o_{s+1} between segments s and s + 1 is eligible when both have output frames and
 * break_s = 0.  Its ramp is the R frames e - floor(R / 2) .. e - floor(R / 2) + R - 1, cut at the far ends of the two
 * segments; frame number t of it (from 0) has semitones = x_s + w (x_{s+1} - x_s), w = (t + 1) / (R + 1) in fp64, and
 * gain_db alike.  Where the ramps of a segment's two boundaries overlap, the later boundary's holds.  The rate is not
 * ramped: pos stays piecewise linear.
 * Refused ("curve_fill:"): a null pointer other than tlen_in; a misaligned double table; B, T_in, S as above; T_out < 1;
 * ramp_frames outside [0, DV3_PROSODY_MAX_RAMP].
 * tests/prosody_curve_ref.py restates all three in float64.
 * ------------------------------------------------------------------------------------ */
#define DV3_PROSODY_MAX_SEGMENTS 64
#define DV3_PROSODY_MAX_RATE 64
#define DV3_PROSODY_MAX_BREAK 1048576
#define DV3_PROSODY_MAX_RAMP 4096
int dv3_curve_warp_f32(const float* mag, float* out, int32_t B, int32_t T_in, int32_t T_out, int32_t bins,
                       const int32_t* tlen_in /* or NULL */, const int32_t* tlen_out, const double* pos,
                       const double* ratio, const float* gain, int32_t env_half_width, int32_t preserve_envelope,
                       void* stream);
int dv3_curve_plan_f64(const int32_t* tlen_in /* or NULL */, int32_t B, int32_t T_in, int32_t S, const int32_t* nseg,
                       const int32_t* bounds, const double* rate, const int32_t* break_frames, int32_t min_frames,
                       int32_t* o, int32_t* tlen_out, void* stream);
int dv3_curve_fill_f64(const int32_t* tlen_in /* or NULL */, int32_t B, int32_t T_in, int32_t S, const int32_t* nseg,
                       const int32_t* bounds, const double* rate, const double* semitones, const double* gain_db,
                       const int32_t* break_frames, const int32_t* o, const int32_t* tlen_out, int32_t T_out,
                       int32_t ramp_frames, double* pos, double* ratio, float* gain, void* stream);

/* ------------------------------------------------------------------------------------
 * Deliverable audio: the last stage of synthesis -- measure every utterance's level, turn the levels into gains, and
 * place, scale, fade and quantise the utterances into one output in ONE launch (audio.wave_levels, audio.master_items,
 * audio.to_pcm16, synthesis.join_utterances).  The reference's counterpart is audio.save_wav
 * (audio.py:16-18): wav * 32767 / max(0.01, max|wav|) as int16, one file per line of text (synthesis.py:133-147); it joins
 * nothing.  Three new entry points with plain arguments, no struct added or changed, so the version stays 50.
 *
 * dv3_wave_levels_f32: x a flat fp32 buffer; item b is the span x[starts[b] .. starts[b] + n_b), starts / lengths device
 * int64[B] as dv3_gather_spans_f32 takes them, n_b = lengths[b] clamped into [0, max_len].  levels double[B][5]
 * (DV3_LEVEL_COLUMNS), row b:
 *   peak       max |x| over the item's finite samples (exact; 0 when there is none)
 *   sumsq      sum of x^2 over the finite samples: every square exact in fp64, the sum accumulated in fp64
 *   sum        sum of x over the finite samples, accumulated in fp64
 *   over       the number of samples with |x| >= 1 (an infinity counts, a NaN does not)
 *   nonfinite  the number of samples that are NaN or infinite
 * Summation order: the item is cut into chunks of DV3_LEVELS_CHUNK samples counted from ITS OWN first sample; in a chunk
 * lane t of 256 adds samples t, t + 256, ... in that order, the 256 partial results are added in a fixed binary tree, and
 * the chunks' results in ascending order.  No atomics.  Samples are read as single dwords, so the row is the same
 * wherever the span starts (any 4-byte alignment), whatever B is and whatever its neighbours hold: it is a function of
 * the item's samples alone.  A zero-length item gives a row of zeros.  Every row is written; nothing outside the table
 * and the scratch is.  scratch: B * ceil(max_len / DV3_LEVELS_CHUNK) * 5 doubles the call may overwrite (NULL allowed
 * when max_len is 0).  Refused (DV3_EINVAL, "wave_levels:", nothing launched): a null x, starts, lengths or levels; a null
 * scratch with max_len > 0; B outside [1, 65535]; max_len outside [0, 2^40]; levels or scratch not 8-byte aligned.
 *
 * dv3_wave_gains_f32: levels as above, lengths the same int64[B] (each clamped at 0), goff device int32[G + 1] ascending
 * from 0 to B: items goff[g] .. goff[g + 1] - 1 form group g and share one value computed from their combined levels
 * P = the largest peak, Q = the sum of sumsq (ascending item order), n = the sum of the lengths; goff = 0, 1, .., B gives
 * per-item gains.  gain float[B]; all arithmetic in fp64 (division and square root correctly rounded), rounded ONCE to
 * fp32 at the end:
 *   DV3_GAIN_PEAK       g = target / P
 *   DV3_GAIN_RMS        g = min(target / sqrt(Q / n), ceiling / P)
 *   DV3_GAIN_REFERENCE  the value written is the DIVISOR fmaxf(P, 0.01f) of audio.py:17 (P is an fp32 value), not a
 *                       multiplier; target, ceiling and max_gain are not read
 * Under PEAK and RMS g is then capped, g = min(g, max_gain), and g = 1 for a silent or empty group (P == 0 or n == 0, and
 * under RMS Q == 0).  target, ceiling and max_gain are LINEAR values (10^(dB / 20)), positive and finite.  Item indices
 * read from goff are clamped into [0, B].  Refused ("wave_gains:"): null pointers; B outside [1, 65535]; G outside [1, B];
 * a policy that is none of the three; under PEAK and RMS a target, ceiling or max_gain that is no positive finite number.
 *
 * dv3_wave_master_f32: x the flat fp32 source; S segments as device arrays -- src, len, dst int64[S], gain float[S],
 * flags int32[S] (DV3_MASTER_FADE_IN = 1, DV3_MASTER_FADE_OUT = 2): segment s is x[src[s] .. src[s] + len[s]) placed at
 * output samples dst[s] .. dst[s] + len[s]; fade float[F], 0 <= F <= DV3_MASTER_MAX_FADE (NULL allowed when F is 0), which
 * the caller makes as 0.5 - 0.5 cos(pi (i + 0.5) / F) in fp64 rounded once.  Layout rules, which the CALLER guarantees
 * (the arrays live on the device; audio.wave_master checks them on the host and refuses violations): dst ascending; the
 * ends dst[s] + len[s] ascending too; no output sample covered by more than two segments; every span inside x.  The
 * kernel reads x[src[s] + i] only for 0 <= i < len[s], whatever the table holds.  Output sample n, for every covering
 * segment s in segment order, i = n - dst[s], every product and sum in fp32 rounded once, none contracted into an
 * fma (fmul, fadd and fdiv below are the IEEE operations, what numpy's float32 operators are):
 *     w = 1
 *     if fade-in  and i < F:            w = fade[i]
 *     if fade-out and i >= len[s] - F:  w = fmul(w, fade[len[s] - 1 - i])
 *     t = fmul(fmul(gain[s], w), x[src[s] + i])
 *     y = t (one covering segment);  y = fadd(t_a, t_b) (two, a before b);  y = 0 (none)
 * so that a fade-out over the last F samples of one segment laid over the fade-in of the next sums to weight 1 within
 * one ulp: the crossfade.  Output modes (out is 16-byte aligned):
 *   DV3_MASTER_F32            out float[N]:    out[n] = y
 *   DV3_MASTER_I16            out int16_t[N]:  v = fmul(y, 32767.f); with dither v = fadd(v, d(n)); q = rintf(v) (ties to
 *                             even) clamped into [-32768, 32767]; a NaN gives 0
 *   DV3_MASTER_I16_REFERENCE  out int16_t[N]:  no fades (F == 0, flags ignored), no dither, and the caller lays no two
 *                             segments over each other; gain[s] is the DIVISOR: t = fdiv(fmul(x, 32767.f), gain[s])
 *                             (correctly rounded), q = (int16) truncf(t), saturating, NaN gives 0 -- numpy's
 *                             (wav * 32767 / max(0.01, peak)).astype(int16) of audio.py:17-18
 * Dither: d(n) is triangular (TPDF, +-1 LSB) from Philox4x32-10 as the dropout masks use it: key (lo32(seed),
 * hi32(seed)), counter (lo32(n), hi32(n), 0, 0) -- a function of the output index, not of the launch geometry --,
 * u1 = (r0 >> 8) 2^-24, u2 = (r1 >> 8) 2^-24, d = u1 - u2 (exact in fp32).
 * Every one of the N outputs is written (gaps between segments are zeros: the caller need not clear out), nothing beyond
 * N.  No atomics, no cross-lane sums: two calls give bit-equal output.  N == 0 launches nothing.  Refused
 * ("wave_master:", nothing launched): a null x, src, len, dst, gain, flags or out; a null fade with F > 0; S outside
 * [1, DV3_MASTER_MAX_SEGMENTS]; F outside [0, DV3_MASTER_MAX_FADE]; N outside [0, 2^40]; a mode that is none of the
 * three; dither other than 0 or 1; the reference mode with F > 0 or with dither; dither in the F32 mode; out not 16-byte
 * aligned; out == x.
 * tests/master_ref.py restates the three definitions in numpy float32 and in float64.
 * ------------------------------------------------------------------------------------ */
#define DV3_LEVEL_COLUMNS 5
#define DV3_LEVELS_CHUNK 16384
#define DV3_GAIN_PEAK 0
#define DV3_GAIN_RMS 1
#define DV3_GAIN_REFERENCE 2
#define DV3_MASTER_F32 0
#define DV3_MASTER_I16 1
#define DV3_MASTER_I16_REFERENCE 2
#define DV3_MASTER_FADE_IN 1
#define DV3_MASTER_FADE_OUT 2
#define DV3_MASTER_MAX_FADE 8192
#define DV3_MASTER_MAX_SEGMENTS 1048576
int dv3_wave_levels_f32(const float* x, const int64_t* starts, const int64_t* lengths, int32_t B, int64_t max_len,
                        double* scratch, double* levels, void* stream);
int dv3_wave_gains_f32(const double* levels, const int64_t* lengths, const int32_t* goff, int32_t B, int32_t G,
                       int32_t policy, double target, double ceiling, double max_gain, float* gain, void* stream);
int dv3_wave_master_f32(const float* x, const int64_t* src, const int64_t* len, const int64_t* dst, const float* gain,
                        const int32_t* flags, int32_t S, const float* fade /* or NULL when F is 0 */, int32_t F,
                        int32_t mode, int32_t dither, uint64_t seed, void* out, int64_t N, void* stream);

/* ------------------------------------------------------------------------------------
 * Loudness mastering: ITU-R BS.1770 integrated loudness and true peak, mono, channel weight 1 (audio.wave_loudness,
 * audio.loudness_gains, Mastering(level="lufs"); csrc/loudness.hip).  The reference has no counterpart.
 * Three new entry points with plain arguments, no struct added or changed, so the version stays 50.
 *
 * The measure.  fs the sample rate, 8000 <= fs <= 192000.  Step h = floor(0.1 fs + 0.5) samples (DV3_LOUDNESS_MIN_STEP
 * <= h <= DV3_LOUDNESS_MAX_STEP); a block is 4 h samples.
 *   K-weighting: two biquads in cascade, fp64, from a zero state at the item's own first sample.  The caller computes
 *   the coefficients in fp64 by the bilinear transform of the analogue prototypes (audio.k_weighting):
 *     shelf      f0 = 1681.974450955533, G = 3.999843853973347 dB, Q = 0.7071752369554196; K = tan(pi f0 / fs),
 *                Vh = 10^(G / 20), Vb = Vh^0.4996667741545416, a0 = 1 + K / Q + K^2;
 *                b = [Vh + Vb K / Q + K^2, 2 (K^2 - Vh), Vh - Vb K / Q + K^2] / a0
 *                a = [1, 2 (K^2 - 1) / a0, (1 - K / Q + K^2) / a0]
 *     high-pass  f0 = 38.13547087602444, Q = 0.5003270373238773; b = [1, -2, 1] (NOT divided by a0), a as above
 *   At 48 kHz these are the standard's table.  coef (a HOST array of 10 doubles) = shelf b0 b1 b2 a1 a2, high-pass
 *   b0 b1 b2 a1 a2.  Each biquad runs in transposed direct form II, state (s1, s2) for the shelf and (t1, t2) for the
 *   high-pass, per input sample x (an fp32 value widened exactly):
 *     u  = b0 x + s1;   s1 = (b1 x - a1 u) + s2;   s2 = b2 x - a2 u         (the shelf's b, a)
 *     y  = b0 u + t1;   t1 = (b1 u - a1 y) + t2;   t2 = b2 u - a2 y         (the high-pass's b, a)
 *   in fp64; the compiler may contract a product and a sum into one fma.  The zero-input transition of the state vector
 *   s = (s1, s2, t1, t2) is the matrix
 *     A = [ -a1           1   0    0 ]      (row 0, 1: the shelf's a; c = the high-pass's b, d = the high-pass's a)
 *         [ -a2           0   0    0 ]
 *         [ c1 - d1 c0    0  -d1   1 ]
 *         [ c2 - d2 c0    0  -d2   0 ]
 *   and Ah (a HOST array of 16 doubles, row-major) is A^h, built by the caller in fp64 (numpy.linalg.matrix_power).
 *   Sub-block energies: E[b][k] = sum of y^2 over samples [k h, (k + 1) h) of item b, accumulated in fp64 in ascending
 *   sample order; the last, partial sub-block is kept.  Block j of item b covers [j h, j h + 4 h): an item of n samples
 *   has J = (n - 4 h) / h + 1 (integer division) blocks when n >= 4 h, else none; blocks never straddle items.
 *     z_j = (((E[j] + E[j+1]) + E[j+2]) + E[j+3]) * (1 / (4 h));   l_j = -0.691 + 10 log10 z_j
 *   Gating over a group (items goff[g] .. goff[g + 1] - 1, the offsets dv3_wave_gains_f32 takes), its blocks pooled:
 *     1. the absolute gate keeps l_j > -70;
 *     2. Gr = -0.691 + 10 log10(mean z over the absolute-gated blocks) - 10;
 *     3. L  = -0.691 + 10 log10(mean z over the blocks with l_j > -70 and l_j > Gr).
 *   Two edge rules that are NOT in the standard: a group with no complete block is measured ungated,
 *   L = -0.691 + 10 log10(sum of E / sum of n) over its items' sub-blocks, and flagged DV3_LOUDNESS_SHORT; a group with
 *   blocks none of which passes the absolute gate has L = -inf and is flagged DV3_LOUDNESS_SILENT (so is a short group
 *   whose energy or length is 0: the flag says "L is -inf", and such a group takes gain 1).
 *   True peak: the largest |v| over the item's samples x[m] and the interpolants y[4 m + p], p = 1, 2, 3, m = 0 .. n - 1,
 *   of the 4x oversampled signal, samples outside the item's span counting as zero.  Interpolator
 *   g[i] = sinc(i / 4) kaiser(49, beta = 8)[i + 24], i = -24 .. 24 (phase 0 is the identity), each phase
 *   DV3_TRUE_PEAK_TAPS = 12 taps: y[4 m + p] = sum over j = 0 .. 11 of table[p - 1][j] x[m + 6 - j], table[p - 1][j] =
 *   g[p + 4 (j - 6)], built in fp64 and rounded once to fp32 (audio.true_peak_table); the sum runs in fp32 from 0 in
 *   ascending j, each step one fmaf.  4x oversampling under-reads content near Nyquist.
 *
 * dv3_wave_loudness_f64: x, starts, lengths, B, max_len as dv3_wave_levels_f32 takes them (n_b = lengths[b] clamped into
 * [0, max_len]; max_len <= 2^30); K = ceil(max_len / h).  Three launches (csrc/loudness.hip says why no warm-up overlap
 * can replace them: the high-pass pole has radius 0.989 at 22.05 kHz):
 *   pass 1  every chunk [k h, (k + 1) h) of every item is filtered from a zero state; its end state e_k is stored;
 *   pass 2  per item, s_0 = 0, s_{k+1}[r] = ((((Ah[r][0] s_k[0] + Ah[r][1] s_k[1]) + Ah[r][2] s_k[2]) + Ah[r][3] s_k[3])
 *           + e_k[r]) for k ascending: every chunk's true start state;
 *   pass 3  every chunk is filtered again from s_k, and E[b][k] is summed.
 * Outputs: states double[B][K][4], 16-byte aligned: states[b][k] = s_k = (s1, s2, t1, t2) before sample k h of item b
 * (for k > 0 that is the filter's state after sample k h - 1), zeros for chunks at or past the item's end; energy
 * double[B][K]: E[b][k], zeros past the item's end.  With peak_table (a HOST array of 3 x 12 floats) and true_peak
 * double[B] non-NULL (both or neither), a fourth and fifth launch write true_peak[b] (0 for an empty item); peak_scratch:
 * B * ceil(max_len / DV3_TRUE_PEAK_CHUNK) doubles the call may overwrite.  A row is a function of the item's samples
 * alone: it does not depend on B, on the neighbours or on where the span lies (any 4-byte alignment).  No atomics.
 * Nothing outside the named tables is written; max_len == 0 launches no filter pass.  Refused (DV3_EINVAL,
 * "wave_loudness:", nothing launched): a null x, starts, lengths, coef or Ah; null states or energy with max_len > 0;
 * peak_table without true_peak or the reverse; a null peak_scratch with a peak_table and max_len > 0; B outside
 * [1, 65535]; max_len outside [0, 2^30]; h outside [DV3_LOUDNESS_MIN_STEP, DV3_LOUDNESS_MAX_STEP]; a coefficient, an
 * entry of Ah or of peak_table that is not finite; states not 16-byte aligned, energy, peak_scratch or true_peak not
 * 8-byte aligned.
 *
 * dv3_loudness_gate_f64: energy, lengths, max_len and h as above, goff device int32[G + 1] ascending from 0 to B (indices
 * clamped into [0, B]), peak: item b's peak is peak[b * peak_stride] (true_peak with stride 1, or the level table of
 * dv3_wave_levels_f32 with stride DV3_LEVEL_COLUMNS: its sample peak).  rows double[G][DV3_LOUDNESS_COLUMNS], row g:
 *   lufs           L of the group (-inf when silent)
 *   blocks         the number of blocks of its items
 *   gated_abs      blocks that pass the absolute gate
 *   gated_rel      blocks that pass both gates (0 for a short group)
 *   momentary_max  the largest l_j over all its blocks (-inf when there is none)
 *   peak           the largest of its items' peaks
 *   flags          DV3_LOUDNESS_SHORT | DV3_LOUDNESS_SILENT
 * One wave per group.  Summation order of every mean: the items in ascending order, lane t of 64 adding blocks t,
 * t + 64, ... of each item to its own fp64 partial; the 64 partials are added in a fixed butterfly (xor 32, 16, .., 1).
 * The gates compare l_j as computed on the device (fp64 log10).  goff = 0, 1, .., B gives a per-item table.  Refused
 * ("loudness_gate:"): a null lengths, goff, peak or rows; a null energy with max_len > 0; B outside [1, 65535]; G outside
 * [1, B]; max_len or h outside their ranges; peak_stride outside [1, 64]; a table not 8-byte aligned.
 *
 * dv3_loudness_gains_f32: rows as above, gain float[B]; per group, in fp64 (pow and division as the device's library
 * rounds them), rounded ONCE to fp32:
 *     g = 10^((target_lufs - L) / 20);  if peak > 0: g = min(g, ceiling / peak);  g = min(g, max_gain)
 * and g = 1 for a group flagged DV3_LOUDNESS_SILENT; every item of the group gets g.  target_lufs in LUFS (dB),
 * ceiling and max_gain LINEAR (10^(dB / 20)).  Refused ("loudness_gains:"): null pointers; B outside [1, 65535]; G
 * outside [1, B]; target_lufs outside [-120, 0]; a ceiling or max_gain that is no positive finite number; rows not
 * 8-byte aligned.
 * tests/loudness_ref.py restates all of it in numpy float64.
 * ------------------------------------------------------------------------------------ */
#define DV3_LOUDNESS_COLUMNS 7
#define DV3_LOUDNESS_SHORT 1
#define DV3_LOUDNESS_SILENT 2
#define DV3_LOUDNESS_MIN_STEP 800
#define DV3_LOUDNESS_MAX_STEP 19200
#define DV3_TRUE_PEAK_TAPS 12
#define DV3_TRUE_PEAK_CHUNK 1024
int dv3_wave_loudness_f64(const float* x, const int64_t* starts, const int64_t* lengths, int32_t B, int64_t max_len,
                          int32_t h, const double* coef, const double* Ah, const float* peak_table /* or NULL */,
                          double* states, double* energy, double* peak_scratch /* or NULL */,
                          double* true_peak /* or NULL */, void* stream);
int dv3_loudness_gate_f64(const double* energy, const int64_t* lengths, const int32_t* goff, const double* peak,
                          int32_t peak_stride, int32_t B, int32_t G, int64_t max_len, int32_t h, double* rows,
                          void* stream);
int dv3_loudness_gains_f32(const double* rows, const int32_t* goff, int32_t B, int32_t G, double target_lufs,
                           double ceiling, double max_gain, float* gain, void* stream);

/* ------------------------------------------------------------------------------------
 * Look-ahead peak limiter: a time-varying gain that holds every span under a ceiling, so that a loudness target is met
 * where one static gain would give way to the loudest syllable (audio.limit_spans, audio.Limiter,
 * Mastering(limiter=); csrc/limiter.hip).  The reference has no counterpart.  One new entry point with
 * plain arguments, no struct added or changed, so the version stays 50.
 *
 * dv3_wave_limit_f32: x, starts, lengths, B, max_len as dv3_wave_loudness_f64 takes them (span b is x[starts[b] ..
 * starts[b] + L), L = lengths[b] clamped into [0, max_len]; max_len <= 2^30).  Per span: the pre-gain g = gain[b] (device
 * float[B]), the ceiling c > 0 (LINEAR), the look-ahead A samples, 0 <= A <= DV3_LIMIT_MAX_LOOKAHEAD, the release factor
 * rho in [0, 1), and the detector: the sample peak (peak_table NULL) or the true peak (peak_table: a HOST array of 3 x 12
 * floats, audio.true_peak_table(), as dv3_wave_loudness_f64 takes it).  Everything between the first and the last line is
 * fp64:
 *     y[n]  = fmul(g, x[n])                                 fp32 product, rounded once, then widened; y is 0 outside [0, L)
 *     e[n]  = |y[n]|                                        sample-peak detector
 *             true-peak detector: i_p[m] = sum over j = 0 .. 11 of table[p - 1][j] y[m + 6 - j], p = 1 .. 3, m = -1 .. L - 1
 *             (the interpolant at m + p / 4; summed from 0 in ascending j, each step one fma),
 *             e[n] = max(|y[n]|, max_p |i_p[n]|, max_p |i_p[n - 1]|)     an interpolant counts for both of its neighbours
 *     dr[n] = e[n] > c ? 1 - c / e[n] : 0                   the gain reduction this sample demands
 *     dm[n] = max over j in [n, min(n + A, L - 1)] of dr[j] look-ahead
 *     dq[n] = max(dm[n], rho dq[n - 1]),  dq[-1] = 0        instant hold, exponential release
 *     ds[n] = (1 / (A + 1)) * sum over k in [n - A, n] of dq[max(k, 0)]       attack: a box of the look-ahead's length
 *     s[n]  = 1 - ds[n]
 *     out[n] = fmul(y[n], (float) s[n])                     fp32, rounded once
 * Consequences.  ds[n] >= dr[n]: every dq[k] of the box has n inside its look-ahead window (k <= n <= k + A), and the
 * clamp max(k, 0) keeps that true for the first A samples; so under the sample-peak detector |out[n]| <= c (1 + 2^-22),
 * one rounding of s and one of the product.  Under the true-peak detector the gain varies across an interpolant's 12
 * taps, so the true peak of out may pass c by a little: measure it (dv3_wave_loudness_f64) and trim.  Where nothing
 * exceeds c every table is 0, s is exactly 1 and out[n] = fmul(g, x[n]), the bits dv3_wave_master_f32 makes from x and g.
 * Nothing depends on B, on where the span lies in the flat buffer (any 4-byte alignment) or on the launch geometry.
 *
 * How the device evaluates it.  The span is cut into tiles of DV3_LIMIT_TILE samples from its own first sample.  The
 * release is evaluated as dq[n] = max over k <= n of dm[k] rho^(n - k): the same recursion, associative, different only
 * in rounding.  rho_pow (a HOST array of DV3_LIMIT_RHO_POWERS doubles) holds rho^(2^i), i = 0 .. log2(DV3_LIMIT_TILE), made
 * by the caller in fp64, each one pow rounded once; rho_pow[0] is rho.  Pass A runs the recursion inside a tile from a zero
 * state (steps v[n] = max(v[n], v[n - d] rho^d), d = 1, 2, 4, ..), pass B carries the tiles' end values along the span,
 * carry' = max(end, carry rho^T), and pass C takes dq[n] = max(dq_local[n], carry rho^(i + 1)), i = n mod T, rho^(i + 1)
 * the product of the powers of i + 1's binary digits in ascending order.  The box sum adds the sums of the power-of-two
 * windows that W = A + 1 decomposes into (lowest digit first, the window ending at n; each window's sum built by
 * doubling, S_2d[n] = S_d[n] + S_d[n - d]): non-negative terms only, nothing cancels, and A = 0 gives ds = dq exactly.
 * The fp64 tables hold to 1e-12 absolute against the sequential form; tests/limiter_ref.py restates both.
 *
 * report double[B][DV3_LIMIT_COLUMNS]: (gain_min, over_samples) = (the smallest s[n] of the span, the number of samples
 * with dr[n] > 0); (1, 0) for an empty span.  out float[] of x's layout: only span samples are written.  scratch:
 * B * ceil(max_len / DV3_LIMIT_TILE) * (DV3_LIMIT_TILE + 3) doubles the call may overwrite (NULL allowed when max_len is
 * 0).  Four launches; no atomics; every read of x is guarded by the span, whatever the tables hold; two calls give
 * bit-equal output.  Refused (DV3_EINVAL, "wave_limit:", nothing launched): a null x, starts, lengths, gain, rho_pow, out
 * or report; a null scratch with max_len > 0; B outside [1, 65535]; max_len outside [0, 2^30]; lookahead outside
 * [0, DV3_LIMIT_MAX_LOOKAHEAD]; a ceiling that is no positive finite number; rho_pow[0] outside [0, 1), or a later entry
 * that is negative, not a number or above its predecessor; out == x; scratch, report, starts or lengths not 8-byte
 * aligned, x, out or gain not 4-byte aligned; an entry of peak_table that is not finite.
 * ------------------------------------------------------------------------------------ */
#define DV3_LIMIT_TILE 1024
#define DV3_LIMIT_MAX_LOOKAHEAD 512
#define DV3_LIMIT_RHO_POWERS 11
#define DV3_LIMIT_COLUMNS 2
int dv3_wave_limit_f32(const float* x, const int64_t* starts, const int64_t* lengths, int32_t B, int64_t max_len,
                       const float* gain, double ceiling, int32_t lookahead, const double* rho_pow,
                       const float* peak_table /* or NULL */, double* scratch, float* out, double* report, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* DV3HIP_H */

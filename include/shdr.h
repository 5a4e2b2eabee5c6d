/*
 * libshdr -- MI355X (gfx950) native kernels for the SingleHDR hot path.
 *
 * C ABI drop-in boundary.  The reference
 * (ShinYwings/SingleHDR-tf2) has no native code and no FFI: every entry point
 * below replaces a *TensorFlow op call site* of the reference, cited per
 * function as file:line under /root/reference.
 *
 * Conventions
 *  - all tensors are dense NHWC float32 in device memory, owned by the caller;
 *    the library allocates nothing and keeps no mutable global state;
 *  - every call is asynchronous on `stream` (a hipStream_t passed as void*);
 *    no implicit device synchronisation;
 *  - return value: SHDR_OK (0) or a negative SHDR_E_* code; the message of the
 *    last error on the calling thread is available from shdr_last_error();
 *    shapes, alignment and strides are validated on the host before launch;
 *  - filters are HWIO ([KH][KW][Cin][Cout] row-major), as in Keras.
 */
#ifndef SHDR_H_
#define SHDR_H_

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* The library reads its SHDR_* environment switches once per process; call this after changing one in a running process. */
void shdr_config_reload(void);

#define SHDR_OK          0
#define SHDR_E_SHAPE    (-1)  /* inconsistent / unsupported dimensions          */
#define SHDR_E_ALIGN    (-2)  /* pointer or channel count not suitably aligned  */
#define SHDR_E_ARCH     (-3)  /* no gfx950 device / wrong code object           */
#define SHDR_E_LAUNCH   (-4)  /* hipLaunchKernel reported an error              */
#define SHDR_E_NULL     (-5)  /* required pointer is NULL                       */

/* activation codes for the conv epilogue */
#define SHDR_ACT_NONE   0
#define SHDR_ACT_RELU   1
#define SHDR_ACT_LRELU  2   /* leaky relu, slope 0.1 (dequantization_net.py:13) */
#define SHDR_ACT_TANH   3

/* kernel selection for shdr_conv2d_fwd_f32 */
#define SHDR_ALGO_AUTO    0
#define SHDR_ALGO_MFMA    1  /* fp32-MFMA implicit GEMM (needs (C1+C2)%4==0, Cout%16==0) */
#define SHDR_ALGO_DIRECT  2  /* VALU direct convolution (any shape)                     */
#define SHDR_ALGO_MFMA_REG 3 /* MFMA kernel with register-staged LDS fill (the LDS-DMA  */
                             /* variant is preferred whenever x2_scale == 1)           */
/* Reduced-precision MFMA operands for BASELINE configs[4] ("finetune_real_dataset.py ... fp16 MFMA conv path"):
 * tensors stay fp32 in HBM; activations and filters are rounded to nearest-even to fp16 (bf16) when they are
 * packed into the operands of v_mfma_f32_16x16x32_{f16,bf16}; products accumulate in fp32.  Needs x2_scale == 1.
 * Accepted by shdr_conv2d_fwd_f32 and, through the same descriptor, by shdr_conv2d_wgrad_f32. */
#define SHDR_ALGO_MFMA_F16  4  /* force the MFMA path with fp16 operands                 */
#define SHDR_ALGO_MFMA_BF16 5  /* force the MFMA path with bf16 operands                 */
#define SHDR_ALGO_AUTO_F16  6  /* AUTO; fp16 operands wherever the MFMA path is taken    */
#define SHDR_ALGO_AUTO_BF16 7  /* AUTO; bf16 operands wherever the MFMA path is taken    */
#define SHDR_ALGO_AUTO_EXACT 8 /* AUTO without the split-operand fp16 kernels (SHDR_PLAN_X3): every product an fp32 FMA / fp32 MFMA */

const char* shdr_last_error(void);
/* library / code-object version string, e.g. "libshdr 0.1 gfx950" */
const char* shdr_version(void);

/* CRC-32C (Castagnoli) of `n` bytes, continuing from `crc` (0 to start).  Host-side helper of the TensorFlow
 * tensor-bundle checkpoint reader / writer (the format tf_utils.py:149-169 saves). */
uint32_t shdr_crc32c(const void* data, uint64_t n, uint32_t crc);

/* TF 'SAME' rule: out = ceil(in/stride); total = max((out-1)*stride+k-in,0);
 * *pad_before = total/2 (extra cell goes to the bottom/right). */
int shdr_same_pad(int in_size, int k, int stride, int* out_size, int* pad_before);

/*
 * Convolution forward with fused prologue/epilogue.
 * Replaces tf.keras.layers.Conv2D / tf.nn.conv2d (+bias_add, activation,
 * inference BatchNormalization, residual add, channel concat) at
 *   dequantization_net.py:8-9,21-22,27,35-36,46,62-63
 *   refinement_net.py:8-9,21-22,27,35-36,47,63-66
 *   linearization_net.py:12-25,55-64,91-92,28-48,67-83
 *   hallucination_net.py:47-48,63-65,81,87-89,97,101-105,121-123,140-142
 *   vgg16.py:33-35
 *
 * Input  = channel-concat [x1 (C1 ch), x2_scale * x2 (C2 ch)]   (x2 may be NULL, C2 = 0)
 * y[n,oh,ow,co] = act2( affine( act1( conv + bias ) ) + residual ),  co < cout_valid
 *   affine(v) = v*scale[co] + shift[co]      (folded inference BN; scale==NULL -> identity)
 *   residual  = res[n,oh,ow,co] read with channel stride res_cstride (NULL -> 0)
 */
typedef struct shdr_conv2d_desc {
  int32_t N, H, W;          /* input batch / height / width                     */
  int32_t C1, C2;           /* channels of x1 and x2                            */
  int32_t Cout, KH, KW;
  int32_t stride;           /* same in both directions                          */
  int32_t pad_t, pad_l;     /* zero padding before (top / left)                 */
  int32_t Ho, Wo;           /* output height / width                            */
  float   x2_scale;         /* multiplier applied to x2 (hallucination_net.py:101) */
  int32_t act1, act2;       /* SHDR_ACT_*                                        */
  int32_t res_cstride;      /* channels per pixel of the residual tensor         */
  int32_t y_cstride;        /* channels per pixel of y (0 -> cout_valid)          */
  int32_t algo;             /* SHDR_ALGO_*                                       */
  int32_t cout_valid;       /* channels stored to y (0 -> Cout).  Cout may be a  */
                            /* zero-padded filter width (multiple of 16) so that */
                            /* e.g. a 3-channel head runs on the MFMA tile       */
  int64_t w_batch_stride;   /* filter elements between consecutive images; 0 =   */
                            /* one filter for the whole batch.  Used by the      */
                            /* Winograd path: 16 GEMMs with 16 filters, 1 launch */
  /* Strided placement of the output (0 / 1 = dense [N,Ho,Wo,...]): pixel (oh, ow) is written at (oh * y_pix_stride + y_off_h,
   * ow * y_pix_stride + y_off_w) of a [N, y_H, y_W, ...] tensor; the residual is read at the same place.  Used by the input
   * gradient of the stride-2 convolutions (linearization_net.py:12,16,91): their phases are written in place, interleaved. */
  int32_t y_pix_stride, y_off_h, y_off_w, y_H, y_W;
  /* Operator fused IN FRONT of the convolution (SHDR_PROLOGUE_*, forward calls that take a prepared filter only).
   * SHDR_PROLOGUE_BILINEAR2X: x1 is the LOW-RES tensor [N, H/2, W/2, C1] and the convolution runs on
   * tf.image.resize(x1, 2x, BILINEAR) (hallucination_net.py:86-88, dequantization_net.py:25-27); H, W stay the dimensions of the
   * convolution's input, i.e. of the up-sampled image.  On the fused Winograd plan the up-sampled tensor never exists in HBM;
   * every other plan materialises it in the workspace (shdr_conv2d_workspace_bytes_f32 accounts for it). */
  int32_t prologue;
  /* Kind of the optional 2x2 / stride-2 pooled second output y_pool of the forward calls that take a prepared filter:
   * SHDR_POOL_MAX (MaxPool2D(2): hallucination_net.py:47-49, vgg16.py:72-83) or SHDR_POOL_AVG (AveragePooling2D(2):
   * dequantization_net.py:9-10, the encoder of both U-Nets pools each level's output for the next one).  Written by the conv
   * kernel's own epilogue on the fused Winograd (max), split-operand and narrow split-operand plans, by a pooling launch otherwise. */
  int32_t pool;
} shdr_conv2d_desc;
enum { SHDR_POOL_MAX = 0, SHDR_POOL_AVG = 1 };
enum { SHDR_PROLOGUE_NONE = 0, SHDR_PROLOGUE_BILINEAR2X = 1,
       /* split-operand kernel only (shdr_conv2d_fwd_x3_f32): x1 is scaled in the kernel by the power of two that brings max |x1| -- written
        * into the prepared filter's header by shdr_conv2d_x3_input_absmax_f32 -- into the fp16 range; for inputs far below it (gradients) */
       SHDR_PROLOGUE_RANGE_SCALE = 2 };

int shdr_conv2d_fwd_f32(const shdr_conv2d_desc* d,
                        const float* x1, const float* x2, const float* w,
                        const float* bias, const float* scale, const float* shift,
                        const float* residual, float* y, void* stream);

/* the same; y_range (or NULL) = range slot that receives max |y| from the kernel's epilogue (see shdr_conv2d_fwd_prepared_ranged_f32) */
int shdr_conv2d_fwd_yrange_f32(const shdr_conv2d_desc* d,
                               const float* x1, const float* x2, const float* w,
                               const float* bias, const float* scale, const float* shift,
                               const float* residual, float* y, float* y_range, void* stream);

/* ---- dispatch below the ABI: plan / prepare / run.  algo = SHDR_ALGO_AUTO resolves to one of these kernel families from the
 *      descriptor alone (and from whether a residual is fused), the same way in all the calls below. */
enum {
  SHDR_PLAN_DIRECT = 0,           /* VALU direct convolution (shapes the MFMA tile cannot take)                       */
  SHDR_PLAN_MFMA = 1,             /* implicit GEMM: LDS-DMA / register-staged / register-A kernel, chosen by shape    */
  SHDR_PLAN_WINOGRAD_FUSED = 2,   /* one-kernel Winograd F(2x2,3x3) (3x3 stride 1 SAME, Cin % 8 == 0, Cout % 64 == 0) */
  SHDR_PLAN_WINOGRAD_PLANES = 3,  /* three-kernel Winograd for wide layers whose Cout is not a multiple of 64         */
  SHDR_PLAN_X3 = 4,               /* 3x3 stride 1, C % 32 == 0 per source, Cout % 64 == 0, enough tiles to fill the chip: fp32 operands split
                                     into two fp16 terms, three v_mfma_f32_16x16x32_f16 per product, fp32 accumulation (conv_x3.hip) */
  SHDR_PLAN_X3N = 5               /* the same arithmetic for the narrow layers (Cout 16 / 32, <= 32 channels per tap; conv_x3n.hip) */
};
int shdr_conv2d_plan_f32(const shdr_conv2d_desc* d, int has_residual);
/* The prepared form of the HWIO filter `w` for that plan: the packed Winograd transform U = G g G^T, or the plain filter with
 * x2_scale (hallucination_net.py:101) folded into the rows of the second source.  Prepare once per filter version. */
int64_t shdr_conv2d_prepared_filter_elems_f32(const shdr_conv2d_desc* d, int has_residual);
int shdr_conv2d_filter_is_plain_f32(const shdr_conv2d_desc* d, int has_residual);   /* 1: `w` itself is the prepared filter */
int shdr_conv2d_prepare_filter_f32(const shdr_conv2d_desc* d, int has_residual, const float* w, float* prepared, void* stream);
/* caller-provided scratch of shdr_conv2d_fwd_prepared_f32 (0 for every plan but WINOGRAD_PLANES) */
int64_t shdr_conv2d_workspace_bytes_f32(const shdr_conv2d_desc* d, int has_residual);
/* y = act2(affine(act1(conv + bias)) + residual) with the planned kernel; y_pool (optional) = MaxPool2D(2)(y) or, with
 * desc.pool = SHDR_POOL_AVG, AveragePooling2D(2)(y) -- written by the same launch on the fused Winograd (max only) and
 * split-operand plans (where y itself may then be NULL on the wide ones), by a pooling launch otherwise
 * (hallucination_net.py:47-49,63-66: the conv + max-pool pairs of the encoder). */
int shdr_conv2d_fwd_prepared_f32(const shdr_conv2d_desc* d, const float* x1, const float* x2, const float* prepared,
                                 const float* bias, const float* scale, const float* shift, const float* residual, float* y,
                                 float* y_pool, void* workspace, void* stream);
/* The same with RANGE SLOTS (see shdr_conv2d_fwd_x3_f32): x1_range / x2_range = device words holding an upper bound of max |x| of the
 * sources, or NULL = unknown.  The split-operand plans (SHDR_PLAN_X3 / X3N) scale their input by it; an unknown range is MEASURED here
 * (one absmax pass over that source into the tail of the workspace: shdr_conv2d_workspace_bytes_f32 accounts for it), so these plans
 * are as range-safe as the fp32 kernels whatever the caller passes -- shdr_conv2d_fwd_prepared_f32 is this call with three NULLs.
 * y_range (or NULL): the slot that receives max |y| (atomicMax, the caller zeroes it) -- from the kernel's own epilogue on the
 * split-operand plans, from one pass over y otherwise -- to be handed to the consumer of y (a pooled / resized / clipped copy of y
 * has the same bound).  Replaces the fp32 Conv2D call sites of hallucination_net.py:43-75,146-190 and vgg16.py:33-35 at full range. */
int shdr_conv2d_fwd_prepared_ranged_f32(const shdr_conv2d_desc* d, const float* x1, const float* x2, const float* prepared,
                                        const float* bias, const float* scale, const float* shift, const float* residual, float* y,
                                        float* y_pool, void* workspace, const float* x1_range, const float* x2_range, float* y_range,
                                        void* stream);
/* The planned forward call with a PROJECTED output: y_proj[n,h,w,j] = sum_c proj[j][c] * y[n,h,w,c] (proj: [3][Cout] floats, y_proj:
 * [N,Ho,Wo,3]), formed in the epilogue that holds y in registers; y and y_pool are written only when given (either may be NULL).
 * Replaces the pair "3x3 conv, then a 1x1 conv to 3 channels" where the 1x1 map is linear in the conv's output: the tail of the
 * Hallucination-Net (hallucination_net.py:179-185: skip layer s1 on concat[u1, d1 / 255], then conv2 -- two linear maps in a row)
 * needs only such a projection of u1 and of d1, whose full-resolution 64-channel tensors are then never written nor read back.
 * shdr_conv2d_projected_ok_f32: 1 if the layer's planned kernel can do it (the split-operand plan, 64 output channels, stride 1);
 * the call refuses other layers with SHDR_E_SHAPE (run the two convolutions then). */
int shdr_conv2d_projected_ok_f32(const shdr_conv2d_desc* d);
int shdr_conv2d_fwd_prepared_projected_f32(const shdr_conv2d_desc* d, const float* x1, const float* x2, const float* prepared,
                                           const float* bias, const float* scale, const float* shift, const float* proj, float* y_proj,
                                           float* y, float* y_pool, void* workspace, const float* x1_range, const float* x2_range,
                                           float* y_range, void* stream);

/* The up-sampling 3x3 layers with the channel mix at LOW resolution (csrc/up2_lowres.hip; hallucination_net.py:77-91, inference):
 * tf.image.resize(2x, BILINEAR) acts per channel, so conv3x3(resize2x(x)) = a 1x1 convolution Cin -> 9 Cout on the low-res image (one
 * Cin x Cout matrix per tap: four times fewer MFMAs than the convolution on the up-sampled image) followed by a stencil pass that sums
 * the nine tap planes with the bilinear weights (clamped indices; taps outside the up-sampled image left out) and applies the conv
 * epilogue.  Same accuracy class as SHDR_PLAN_X3, other roundings: an OPT-IN form next to desc.prologue = SHDR_PROLOGUE_BILINEAR2X of
 * shdr_conv2d_fwd_prepared_f32, whose descriptor `d` it takes (H, W: the up-sampled size).
 * _ok: 1 if the layer is taken -- 3x3 / stride 1 / SAME, one source, even H and W, Cin % 32 == 0 and >= 64, Cout % 64 == 0, algo AUTO,
 *      the low-res GEMM on the split-operand plan (SHDR_X3_MIN_BLOCKS applies to it); 0 under SHDR_NO_UP2_LOWRES=1.
 * _filter_elems / _prepare_filter: floats of the prepared filter (16-byte aligned) and its preparation from the HWIO filter w
 *      [3,3,Cin,Cout], once per filter version.
 * _workspace_bytes: bytes the caller provides per forward call (the tap planes z [N,H/2,W/2,9 Cout (+ pad)], 256-byte aligned).
 * _fwd: x the low-res tensor [N,H/2,W/2,Cin] -> y [N,H,W,Cout] = act2(affine(act1(conv + bias))); two launches on `stream`.
 *      x_range / y_range: range slots as in shdr_conv2d_fwd_prepared_ranged_f32 (x_range NULL: measured). */
int shdr_conv2d_up2_lowres_ok_f32(const shdr_conv2d_desc* d);
int64_t shdr_conv2d_up2_lowres_filter_elems_f32(const shdr_conv2d_desc* d);
int shdr_conv2d_up2_lowres_prepare_filter_f32(const shdr_conv2d_desc* d, const float* w, float* prepared, void* stream);
int64_t shdr_conv2d_up2_lowres_workspace_bytes_f32(const shdr_conv2d_desc* d);
int shdr_conv2d_fwd_up2_lowres_f32(const shdr_conv2d_desc* d, const float* x, const float* prepared, const float* bias,
                                   const float* scale, const float* shift, float* y, void* workspace, const float* x_range,
                                   float* y_range, void* stream);

/* The same layer in ONE launch for 64 output channels (csrc/up2_fused.hip; the Hallucination-Net's u1, whose tap planes would be 2.7 GB at
 * batch 16): a block computes the nine tap planes on a low-res tile with its one-pixel halo and folds them in registers, so neither the
 * planes nor -- with a projected output -- the 64-channel result reach memory.  Descriptor, prepared filter (the _lowres_ one: same
 * packed taps, same scale) and arithmetic are those of shdr_conv2d_fwd_up2_lowres_f32: y is bit-identical to it, range slot included.
 * The narrow forms (the `up` blocks of the Dequantization-Net: 32 and 16 output channels) are the same kernel with Cout / 16 waves per
 * low-res patch, so a block of four waves finishes two or four patches; their prepared filter is the same pack of the [Cin, 9 Cout]
 * matrix padded to whole 64-column slices.  They write y only.
 * _ok: 1 if the layer is taken -- as _lowres_ok without the fill threshold, and Cout == 64 with 64 <= Cin <= 128, Cout == 32 with
 *      32 <= Cin <= 128, or Cout == 16 with Cin 32 or 64 (Cout < 64: not under SHDR_NO_UP2_NARROW=1); 0 under SHDR_NO_UP2_FUSED=1.
 * _narrow_enabled: 0 under SHDR_NO_UP2_NARROW=1, the A/B arm of the narrow forms and of the Dequantization-Net's use of the low-res forms.
 * _fwd: writes y [N,H,W,Cout], at 64 couts the projected output y_proj [N,H,W,3] = sum_c proj[j][c] y[c] (proj [3][64], as in
 *      shdr_conv2d_fwd_prepared_projected_f32), or both (y_proj with proj; at least one output).  x_range: the input's range slot
 *      (required); y_range (or NULL): receives max |y| when y is written. */
int shdr_conv2d_up2_fused_ok_f32(const shdr_conv2d_desc* d);
int shdr_conv2d_up2_narrow_enabled(void);
int64_t shdr_conv2d_up2_fused_filter_elems_f32(const shdr_conv2d_desc* d);
int shdr_conv2d_up2_fused_prepare_filter_f32(const shdr_conv2d_desc* d, const float* w, float* prepared, void* stream);
int shdr_conv2d_fwd_up2_fused_f32(const shdr_conv2d_desc* d, const float* x, const float* prepared, const float* bias,
                                  const float* scale, const float* shift, const float* proj, float* y_proj, float* y,
                                  const float* x_range, float* y_range, void* stream);

/*
 * Convolution backward (GradientTape.gradient through Conv2D: joint_training.py:185,
 * train.py:175,195,242, finetune_real_dataset.py:177).
 *
 * Weight gradient w.r.t. the rows of source `which` (0: x1, 1: x2) of the forward conv `d`:
 *   dw[kh][kw][ci_off + ci][co] += scale * sum_{n,oh,ow} x[n, oh*s+kh-pad_t, ow*s+kw-pad_l, ci] * dz[n,oh,ow,co]
 * (ci_off = 0 / C1, scale = 1 / x2_scale).  dz = gradient w.r.t. the pre-activation conv output,
 * [N,Ho,Wo,cout_valid]; dw = the full [KH,KW,C1+C2,cout_valid] gradient, ACCUMULATED into (the
 * caller zeroes it).  fp32 atomics: the summation order over pixel slices is not fixed.
 */
int shdr_conv2d_wgrad_f32(const shdr_conv2d_desc* d, const float* x, int which, const float* dz,
                          float* dw, void* stream);
/* dgrad filter: wt[kh][kw][co][ci - c_begin] = scale * w[KH-1-kh][KW-1-kw][ci][co], ci in
 * [c_begin, c_begin + c_count): the input gradient of a stride-1 SAME conv is
 * shdr_conv2d_fwd_f32(dz, wt) with the same padding. */
int shdr_filter_transform_f32(const float* w, float* wt, int KH, int KW, int Cin, int Cout,
                              int c_begin, int c_count, float scale, void* stream);
/* Input gradient of the forward conv `d` w.r.t. source `which` (0: x1, 1: x2): dx [N,H,W,C_which] from dz [N,Ho,Wo,cout_valid] and
 * the forward HWIO filter w [KH,KW,C1+C2,Cout] (GradientTape.gradient through Conv2D, joint_training.py:185).  Stride 1 (odd
 * filters; the fused Winograd kernel where the transposed layer qualifies), 1x1 stride 2 (linearization_net.py:12,16: coarse-grid
 * conv written to every second pixel) and general stride 2 (linearization_net.py:91: polyphase form, four stride-1 convs written in
 * place).  Narrow tensors are zero-padded onto the MFMA tile inside.  workspace: shdr_conv2d_dgrad_workspace_bytes_f32 bytes. */
int64_t shdr_conv2d_dgrad_workspace_bytes_f32(const shdr_conv2d_desc* d, int which);
int shdr_conv2d_dgrad_f32(const shdr_conv2d_desc* d, int which, const float* dz, const float* w, float* dx, void* workspace,
                          void* stream);
/* The same with range slots (see shdr_conv2d_fwd_prepared_ranged_f32): dz_range = upper bound of max |dz| or NULL (then measured where the
 * split-operand kernels need it: one pass over dz); dx_range = slot that receives max |dx| from the kernel's epilogue, allowed where
 * shdr_conv2d_dgrad_tracks_range_f32 answers 1 (stride-1 layers on the split-operand / exact MFMA kernels).  A chain conv <- activation <- conv
 * of a backward pass hands the slot on (|act'(.) dz| <= |dz|) and never measures. */
int shdr_conv2d_dgrad_tracks_range_f32(const shdr_conv2d_desc* d, int which);
int shdr_conv2d_dgrad_ranged_f32(const shdr_conv2d_desc* d, int which, const float* dz, const float* w, float* dx, void* workspace,
                                 const float* dz_range, float* dx_range, void* stream);
/* workspace a caller must provide for one call of an op: arg = has_residual (CONV2D_FWD), source (CONV2D_DGRAD,
 * CONV2D_WGRAD_WINOGRAD: the dU scratch), channel count (BATCHNORM: the double-precision partial sums) */
enum { SHDR_OP_CONV2D_FWD = 0, SHDR_OP_CONV2D_DGRAD = 1, SHDR_OP_CONV2D_WGRAD_WINOGRAD = 2, SHDR_OP_BATCHNORM = 3,
       SHDR_OP_ACT_BWD_BIAS = 4 /* arg = channels: one row of C floats per reduction block; optional (ws = NULL: atomics) */ };
/* BATCHNORM workspace = 2 C (1 + SHDR_BN_MAX_BLOCKS) doubles: the sums and one partial row per reduction block (the fp16 kernels
 * reduce without atomics and without a memset; the fp32 kernels use the first 2 C doubles) */
#define SHDR_BN_MAX_BLOCKS 1024
int64_t shdr_workspace_bytes(int op, const shdr_conv2d_desc* d, int arg);
/* db[c] += sum_p dz[p][c] (bias gradient; the caller zeroes db). */
int shdr_bias_grad_f32(const float* dz, float* db, int64_t npix, int C, void* stream);

/* Spatial-aware soft histogram, parametric bin count
 * (linearization_net.py:336-350).  x [npix, C] -> y [npix, B*C], channel
 * order [bin1.c0..c(C-1), bin2...].  Bit-exact w.r.t. the IEEE fp32
 * evaluation of the reference formula. */
int shdr_soft_hist_fwd_f32(const float* x, float* y, int64_t npix, int C, int B, void* stream);
/* its gradient: dx[p][c] = sum_i dy[p][(i-1)*C + c] * (-+B inside the support of bin i)  (tape through linearization_net.py:336-350) */
int shdr_soft_hist_bwd_f32(const float* x, const float* dy, float* dx, int64_t npix, int C, int B, void* stream);

/* Linearization-Net front end (linearization_net.py:310-322):
 * y = concat[img(3), sobel(6), hist4(12), hist8(24), hist16(48)] zero-padded
 * to y_channels (93 <= y_channels, y_channels % 4 == 0 recommended: 96). */
int shdr_lin_frontend_fwd_f32(const float* img, float* y, int N, int H, int W,
                              int y_channels, void* stream);

/* AveragePooling2D(2,2) VALID (dequantization_net.py:10); H, W even. */
int shdr_avgpool2_fwd_f32(const float* x, float* y, int N, int H, int W, int C, void* stream);
/* MaxPool2D(2,2,SAME) on even dims (hallucination_net.py:49,66; vgg16.py:54). */
int shdr_maxpool2_fwd_f32(const float* x, float* y, int N, int H, int W, int C, void* stream);
/* MaxPool2D(3,3,stride 2,SAME) (linearization_net.py:94). */
int shdr_maxpool3s2_fwd_f32(const float* x, float* y, int N, int H, int W, int C, void* stream);
/* tf.image.resize(x, 2x, BILINEAR), half-pixel centres
 * (dequantization_net.py:25, hallucination_net.py:86). */
int shdr_resize2x_fwd_f32(const float* x, float* y, int N, int H, int W, int C, void* stream);
/* tf.reduce_mean(x,[1,2]) (linearization_net.py:118): x [N,HW,C] -> y [N,C]. */
int shdr_gap_fwd_f32(const float* x, float* y, int N, int HW, int C, void* stream);

/* Dense(11) + EMoR PCA decode (linearization_net.py:185-192, 231-253):
 * out[b,k] = g0[k] + sum_j hinv[k,j] * (feat[b,:] @ wfc[:,j] + bfc[j]).
 * table = [K,12] (col 0 = g0, cols 1..11 = hinv). */
int shdr_invcrf_decode_fwd_f32(const float* feat, const float* wfc, const float* bfc,
                               const float* table, float* out, int B, int F, int K,
                               void* stream);
/* linearization_net.py:368-392 (_increase): rf [B,K] -> monotone CDF [B,K]. */
int shdr_increase_fwd_f32(const float* rf, float* out, int B, int K, void* stream);
/* tf_utils.apply_rf (tf_utils.py:54-105): x [B, n_per_batch], rf [B,K]. */
int shdr_apply_rf_fwd_f32(const float* x, const float* rf, float* y, int B,
                          int64_t n_per_batch, int K, void* stream);

/* Elementwise glue of the step closures ---------------------------------- */
/* tf.clip_by_value (test_real_refinement.py:91). */
int shdr_clip_fwd_f32(const float* x, float* y, int64_t n, float lo, float hi, void* stream);
/* x*255, RGB->BGR, subtract VGG mean (hallucination_net.py:149-153, vgg16.py:101-109).
 * x [npix,3] -> y [npix,out_channels], out_channels 3 or 4 (4: zero 4th channel). */
int shdr_vgg_preprocess_fwd_f32(const float* x, float* y, int64_t npix, int out_channels,
                                void* stream);
/* channel reversal of 3-channel pixels (tf_utils.py:5-13). */
int shdr_reverse3_fwd_f32(const float* x, float* y, int64_t npix, void* stream);
/* alpha = clamp((max_c b - 1 + thr)/thr, 0, 1); a = b + alpha * reverse3(hal)
 * (test_real_refinement.py:98-105, joint_training.py:141-145,165).
 * alpha_out (npix floats) may be NULL. */
int shdr_alpha_blend_fwd_f32(const float* b, const float* hal, float* a, float* alpha_out,
                             int64_t npix, float thr, void* stream);
/* concat of up to four 3-channel images into out_channels (>= 3*nsrc, zero
 * padded) -- the Refinement-Net input tf.concat([A,B,C],-1)
 * (test_real_refinement.py:108). */
int shdr_pack3_fwd_f32(const float* s0, const float* s1, const float* s2, const float* s3,
                       int nsrc, float* y, int out_channels, int64_t npix, void* stream);
/* y[p][c] = c < Cin ? x[p][c] : 0 for c < Cout (zero channel padding for the MFMA / DMA tiles). */
int shdr_pad_channels_f32(const float* x, float* y, int64_t npix, int Cin, int Cout, void* stream);
/* log(1+10x)/log(11) (joint_training.py:166,173). */
int shdr_logc_fwd_f32(const float* x, float* y, int64_t n, void* stream);
/* y = act(x * scale[c] + shift[c] + residual) on [npix, C] (scale / shift / residual may be null): the inference
 * BatchNormalization + residual join + relu of linearization_net.py:13-47,55-82 and hallucination_net.py:88-89,164-165 as a
 * stand-alone op, for a `net(x, training=False)` call recorded on a gradient tape (frozen BatchNorm statistics). */
int shdr_affine_act_f32(const float* x, const float* scale, const float* shift, const float* residual, float* y,
                        int64_t npix, int C, int act, void* stream);

/* ---- backward / training (GradientTape.gradient + Adam.apply_gradients:
 *      joint_training.py:185-186, train.py:175-176,195-196,242-243,
 *      finetune_real_dataset.py:177-178).  Parameter gradients (dw, db, dgamma,
 *      dbeta, dwfc, dbfc, drf) are ACCUMULATED into buffers the caller zeroes. ---- */
/* dx = dy * act'(.) evaluated from the activation OUTPUT y (relu / lrelu 0.1 / tanh). */
int shdr_act_bwd_f32(const float* dy, const float* y, float* dx, int64_t n, int act, void* stream);
/* tf.clip_by_value gradient: passes where lo <= x <= hi. */
int shdr_clip_bwd_f32(const float* dy, const float* x, float* dx, int64_t n, float lo, float hi, void* stream);
int shdr_add_f32(const float* a, const float* b, float* y, int64_t n, void* stream);
/* the same; y_range (or NULL) = range slot that receives max |y|: the sums of a backward pass (a forked tensor's gradients, a residual
 * join) feed split-operand input / weight gradients, which then need not measure them */
int shdr_add_ranged_f32(const float* a, const float* b, float* y, int64_t n, float* y_range, void* stream);
/* input gradients of the pooling / resize ops; N,H,W,C describe the op's INPUT x. */
int shdr_avgpool2_bwd_f32(const float* dy, float* dx, int N, int H, int W, int C, void* stream);
int shdr_maxpool2_bwd_f32(const float* x, const float* dy, float* dx, int N, int H, int W, int C, void* stream);
/* y = the forward's pooled output (an element takes a window's gradient only where it equals y and no
 * earlier element of the window does). */
int shdr_maxpool3s2_bwd_f32(const float* x, const float* y, const float* dy, float* dx, int N, int H, int W, int C, void* stream);
int shdr_resize2x_bwd_f32(const float* dy, float* dx, int N, int H, int W, int C, void* stream);
/* the same; dx_range (or NULL) = range slot that receives max |dx| (shdr_add_ranged_f32) */
int shdr_resize2x_bwd_ranged_f32(const float* dy, float* dx, int N, int H, int W, int C, float* dx_range, void* stream);
int shdr_gap_bwd_f32(const float* dy, float* dx, int N, int HW, int C, void* stream);
/* dx[n,2i,2j,:] = dy[n,i,j,:], zero elsewhere (input gradient of a 1x1 stride-2 conv). */
int shdr_upsample_zero2_f32(const float* dy, float* dx, int N, int H, int W, int C, void* stream);
/* BatchNormalization, training mode (linearization_net.py:13-25, hallucination_net.py:82,122,141):
 * batch mean / biased variance over (N,H,W) accumulated in double (ws = caller workspace of
 * shdr_workspace_bytes(SHDR_OP_BATCHNORM, NULL, C) bytes: the 2*C sums + one partial row per reduction
 * block, no atomics); optional Keras moving-average update (momentum 0.99, unbiased variance). */
int shdr_bn_stats_f32(const float* x, double* ws, float* mean, float* var, float* moving_mean,
                      float* moving_var, int64_t npix, int C, float momentum, void* stream);
int shdr_bn_train_apply_f32(const float* x, const float* mean, const float* var, const float* gamma,
                            const float* beta, float* y, int64_t npix, int C, float eps, int relu,
                            void* stream);
/* the same; y_range (or NULL) = range slot that receives max |y| (see shdr_conv2d_fwd_prepared_ranged_f32): the consumer of a
 * training-mode BatchNorm output is usually a split-operand convolution, which then need not measure its input */
int shdr_bn_train_apply_ranged_f32(const float* x, const float* mean, const float* var, const float* gamma, const float* beta, float* y,
                                   int64_t npix, int C, float eps, int relu, float* y_range, void* stream);
/* y_relu != NULL: the forward applied relu after BN; dy is masked by y_relu > 0 first. */
int shdr_bn_bwd_f32(const float* dy, const float* x, const float* y_relu, const float* mean,
                    const float* var, const float* gamma, double* ws, float* dgamma, float* dbeta,
                    float* dx, int64_t npix, int C, float eps, void* stream);
/* the same; dx_range (or NULL) = range slot that receives max |dx| */
int shdr_bn_bwd_ranged_f32(const float* dy, const float* x, const float* y_relu, const float* mean,
                           const float* var, const float* gamma, double* ws, float* dgamma, float* dbeta,
                           float* dx, int64_t npix, int C, float eps, float* dx_range, void* stream);
int shdr_invcrf_decode_bwd_f32(const float* dinv, const float* feat, const float* wfc,
                               const float* table, float* dfeat, float* dwfc, float* dbfc, int B,
                               int F, int K, void* stream);
int shdr_increase_bwd_f32(const float* rf, const float* dout, float* drf, int B, int K, void* stream);
/* drf accumulated; dx may be NULL (joint training feeds data, not a prediction). */
int shdr_apply_rf_bwd_f32(const float* x, const float* rf, const float* dy, float* drf, float* dx,
                          int B, int64_t n_per_batch, int K, void* stream);
/* per-sample mean loss out[b] = mean((a-b)^2) (mode 0, tf_utils.py:110-111) or mean|a-b| (mode 1,
 * joint_training.py:169-173) and its gradient da = g[b] * d out[b] / d a. */
int shdr_diff_loss_f32(const float* a, const float* b, float* out, int B, int64_t n_per_sample,
                       int mode, void* stream);
int shdr_diff_loss_bwd_f32(const float* a, const float* b, const float* g, float* da, int B,
                           int64_t n_per_sample, int mode, int accumulate, void* stream);
/* batch-global TV loss with SYMMETRIC pad (joint_training.py:175-179): out[0]. */
int shdr_tv_loss_f32(const float* y, float* out, int N, int H, int W, int C, void* stream);
int shdr_tv_loss_bwd_f32(const float* y, const float* g, float* dy, int N, int H, int W, int C,
                         int accumulate, void* stream);
int shdr_logc_bwd_f32(const float* dy, const float* x, float* dx, int64_t n, void* stream);
/* alpha[p] = clamp((max_c x - 1 + thr)/thr, 0, 1) (joint_training.py:141-145). */
int shdr_alpha_mask_f32(const float* x, float* alpha, int64_t npix, float thr, void* stream);
/* d hal = reverse3(alpha * dA) for A = B + alpha * reverse3(hal), alpha constant. */
int shdr_alpha_blend_bwd_f32(const float* dA, const float* alpha, float* dhal, int64_t npix, void* stream);
int shdr_vgg_preprocess_bwd_f32(const float* dy, float* dx, int64_t npix, int in_channels, void* stream);
/* Keras Adam on a flat buffer: g' = grad_scale*g; m = b1 m + (1-b1) g'; v = b2 v + (1-b2) g'^2;
 * p -= lr_t * m / (sqrt(v) + eps), lr_t = lr*sqrt(1-b2^t)/(1-b1^t) computed by the caller. */
int shdr_adam_f32(float* p, const float* g, float* m, float* v, int64_t n, float lr_t, float beta1,
                  float beta2, float eps, float grad_scale, void* stream);

/* ---- Winograd F(2x2,3x3) for wide 3x3 stride-1 SAME convs (hallucination_net.py:47-48,63-65,81,121;
 *      vgg16.py:33): y = output_transform( V[xi] @ U[xi] ),  xi = 0..15.  The 16 GEMMs are ONE call of
 *      shdr_conv2d_fwd_f32 with N=16, H=rows/16, W=16, 1x1, w_batch_stride = Cin*Cout. ---- */
/* u[16][Cin][Cout] = G g G^T of the HWIO 3x3 filter w. */
int shdr_winograd_filter_f32(const float* w, float* u, int Cin, int Cout, void* stream);
/* rows of each V / M plane: N*ceil(H/2)*ceil(W/2) rounded up to 128. */
int64_t shdr_winograd_tiles(int N, int H, int W);
/* v[16][rows][C] = B^T d B of the 4x4 patches of x [N,H,W,C] (zero padded). */
int shdr_winograd_input_f32(const float* x, float* v, int N, int H, int W, int C, void* stream);
/* y [N,H,W,C] = act2(affine(act1(A^T m A + bias))), m [16][rows][C]. */
int shdr_winograd_output_f32(const float* m, float* y, const float* bias, const float* scale,
                             const float* shift, int N, int H, int W, int C, int act1, int act2,
                             void* stream);

/* ---- chained fine-tuning step (finetune_real_dataset.py:144-183) ---- */
/* dimg[N,H,W,3] = J^T dF of the front end (identity + REFLECT sobel + soft-histogram slopes). */
int shdr_lin_frontend_bwd_f32(const float* img, const float* dF, float* dimg, int N, int H, int W,
                              int y_channels, void* stream);
/* A = B + alpha(B)*reverse3(hal): gradients w.r.t. B (through the alpha mask too) and hal. */
int shdr_alpha_blend_full_bwd_f32(const float* b, const float* hal, const float* dA, float* dB,
                                  float* dhal, int64_t npix, float thr, void* stream);
/* o_s[p][0..2] = y[p][3s..3s+2], s < nout (backward of pack3; slice of the Refinement-Net input). */
int shdr_unpack3_f32(const float* y, float* o0, float* o1, float* o2, float* o3, int nout,
                     int channels, int64_t npix, void* stream);
/* out[b] = sum_i a[b][i] * (b ? b[b][i] : 1). */
int shdr_sample_dot_f32(const float* a, const float* b, float* out, int B, int64_t n_per_sample, void* stream);
/* out = r / (eps + sum[b]/n) * target and its gradient (finetune_real_dataset.py:170). */
int shdr_mean_norm_fwd_f32(const float* r, const float* sum, float* out, int B, int64_t n_per_sample,
                           float eps, float target, void* stream);
int shdr_mean_norm_bwd_f32(const float* g, const float* sum, const float* gdot, float* dr, int B,
                           int64_t n_per_sample, float eps, float target, void* stream);

/* Backward of  y = act(conv + bias):  dz = dy * act'(y) (from the activation OUTPUT) and db[c] += sum_p dz[p][c] in one
 * pass (the caller zeroes db).  act == SHDR_ACT_NONE: dz is not written (dz = dy) and only db is accumulated.
 * C / 4 must be a power of two <= 256.  Replaces the act_bwd + bias_grad pair of GradientTape.gradient through
 * tf.nn.leaky_relu / relu(conv(x) + b) (dequantization_net.py:13-14, hallucination_net.py:48-52). */
int shdr_act_bwd_bias_f32(const float* dy, const float* y, float* dz, float* db, float* ws, int64_t npix, int C, int act, void* stream);

/* U = G g G^T of a 3x3 HWIO filter in the operand order of the fused kernel (one coalesced float4 per lane, chunk and
 * operand group; layout documented at winograd_filter_packed_kernel).  up: 16*Cin*Cout floats. */
int shdr_winograd_filter_packed_f32(const float* w, float* up, int Cin, int Cout, void* stream);
/* Fused Winograd F(2x2,3x3): 3x3 / stride 1 / SAME convolution with the input transform, the 16 GEMMs and the output
 * transform in one kernel (no V / M planes in HBM).  u = shdr_winograd_filter_packed_f32(w);
 * y = act2(affine(act1(conv + bias))).  Needs Cin % 8 == 0, Cout % 64 == 0.  Same call sites as shdr_conv2d_fwd_f32. */
int shdr_conv2d_winograd_fused_f32(const float* x, const float* u, const float* bias, const float* scale,
                                   const float* shift, float* y, int N, int H, int W, int Cin, int Cout,
                                   int act1, int act2, void* stream);

/* The same kernel on a channel concatenation [x, x2] (the skip connections of the U-Net decoders:
 * dequantization_net.py:50-58, hallucination_net.py:115-144 -- tf.concat + Conv2D): both sources [N,H,W,C1], C2 == C1 (or
 * x2 == NULL, C2 == 0); u packs the filter over all C1 + C2 input channels, x's channels first.
 * y_pool (or NULL): [N,H/2,W/2,Cout] = MaxPool2D(2)(y) written by the same epilogue (H, W even) -- the conv + max_pool
 * pairs of the VGG-shaped encoders (hallucination_net.py:43-75 needs both tensors; vgg16.py:72-83 only the pooled one:
 * y may then be NULL and is not stored). */
int shdr_conv2d_winograd_fused2_f32(const float* x, const float* x2, const float* u, const float* bias,
                                    const float* scale, const float* shift, float* y, float* y_pool, int N, int H, int W,
                                    int C1, int C2, int Cout, int act1, int act2, void* stream);

/* The same kernel with tf.image.resize(x, 2x, BILINEAR) fused in front (hallucination_net.py:86-88, dequantization_net.py:25-27:
 * resize + Conv2D 3x3): x is the LOW-RES tensor [N,H/2,W/2,Cin], H x W (even) the size of the up-sampled image and of
 * y [N,H,W,Cout].  The block stages the low-res patch and expands it in LDS with the arithmetic of shdr_resize2x_fwd_f32; the
 * up-sampled tensor is never written.  Reached through shdr_conv2d_fwd_prepared_f32 with desc.prologue = SHDR_PROLOGUE_BILINEAR2X. */
int shdr_conv2d_winograd_fused_up2_f32(const float* x, const float* u, const float* bias, const float* scale,
                                       const float* shift, float* y, int N, int H, int W, int Cin, int Cout,
                                       int act1, int act2, void* stream);

/* fp32 3x3 / stride-1 / SAME convolution on the fp16 matrix pipe (SHDR_PLAN_X3; csrc/conv_x3.hip): x = xh + xl 2^-11, w 2^S = wh + wl in
 * fp16, x w = xh wh + xl (wh 2^-11) + xh wl accumulated in fp32 -- 3 * 2^-22 relative per product, the level of fp32 rounding itself.
 * Also the 7x7 / stride-2 stem (linearization_net.py:91) as four stride-1 phase launches over the parity-subsampled input, accumulating in y.
 * Needs C1 % 32 == 0, C2 % 32 == 0, Cout % 64 == 0.  RANGE: fp16 overflows at 65504 and loses mantissa below 2^-14, an fp32 convolution
 * (hallucination_net.py:47-48, vgg16.py:33-35) does not -- the _ranged entry points take a RANGE SLOT per source (device word: upper
 * bound of max |x|, from the producer's y_range or shdr_absmax_f32) and scale the input by the power of two that brings it to
 * [2^10, 2^11) while splitting (exact; undone in the epilogue), and can write the range of their own output (y_range, atomicMax; the
 * caller zeroes the slot).  Elements down to 2^-25 of the tensor maximum keep 22 mantissa bits; non-finite inputs give non-finite
 * outputs on their receptive field.  The entry points WITHOUT range slots split the input as it stands (|x| < 65504 required) unless
 * desc.prologue = SHDR_PROLOGUE_RANGE_SCALE names the slot in the prepared filter's header (shdr_conv2d_x3_input_absmax_f32).
 * prepared: shdr_conv2d_x3_filter_elems_f32 floats, written by
 * shdr_conv2d_x3_prepare_filter_f32 (the skip scale of the second source folded in).  y = act2(affine(act1(conv + bias)));
 * y_pool (or NULL) = MaxPool2D(2)(y) from the same epilogue (y may then be NULL); desc.prologue = SHDR_PROLOGUE_BILINEAR2X: x1 is the
 * low-res tensor and the 2x bilinear up-sampling runs inside the kernel's patch loader.
 * Same call sites as shdr_conv2d_winograd_fused2_f32; reached through shdr_conv2d_fwd_prepared_f32 / shdr_conv2d_dgrad_f32. */
int shdr_conv2d_x3_ok_f32(const shdr_conv2d_desc* d);
int64_t shdr_conv2d_x3_filter_elems_f32(const shdr_conv2d_desc* d);
int shdr_conv2d_x3_prepare_filter_f32(const shdr_conv2d_desc* d, const float* w, float* prepared, void* stream);
/* max |x| over n floats -> header of `prepared` (after shdr_conv2d_x3_prepare_filter_f32, before the SHDR_PROLOGUE_RANGE_SCALE launch) */
int shdr_conv2d_x3_input_absmax_f32(const float* x, int64_t n, float* prepared, void* stream);
int shdr_conv2d_fwd_x3_f32(const shdr_conv2d_desc* d, const float* x1, const float* x2, const float* prepared, const float* bias,
                           const float* scale, const float* shift, float* y, float* y_pool, void* stream);
int shdr_conv2d_fwd_x3_ranged_f32(const shdr_conv2d_desc* d, const float* x1, const float* x2, const float* prepared, const float* bias,
                                  const float* scale, const float* shift, float* y, float* y_pool, const float* x1_range,
                                  const float* x2_range, float* y_range, void* stream);
/* the same with a residual [N,Ho,Wo,res_cstride] added between the affine and act2 (stride-1 layers: the ResNet joins of
 * linearization_net.py:6-48 on the 1x1 layers); reached through shdr_conv2d_fwd_prepared_f32 */
int shdr_conv2d_fwd_x3_residual_f32(const shdr_conv2d_desc* d, const float* x1, const float* x2, const float* prepared, const float* bias,
                                    const float* scale, const float* shift, const float* residual, float* y, const float* x1_range,
                                    const float* x2_range, float* y_range, void* stream);
/* the same launch with a projected output (see shdr_conv2d_fwd_prepared_projected_f32); proj [3][64], Cout = 64 */
int shdr_conv2d_fwd_x3_projected_f32(const shdr_conv2d_desc* d, const float* x1, const float* x2, const float* prepared, const float* bias,
                                     const float* scale, const float* shift, const float* proj, float* y_proj, float* y, float* y_pool,
                                     const float* x1_range, const float* x2_range, float* y_range, void* stream);
/* range slot of a tensor: *range = max(*range, max |x|) (bit pattern of a non-negative float, atomicMax; the caller zeroes the slot) */
int shdr_absmax_f32(const float* x, int64_t n, float* range, void* stream);

/* The split-operand arithmetic for the NARROW layers (SHDR_PLAN_X3N; csrc/conv_x3n.hip): stride 1, 3x3 / 5x5 / 7x7 SAME, Cout 16 or 32
 * (cout_valid <= Cout stored), one source of 4 ... 32 channels (C1 % 4 == 0) or two of 16 -- the full-resolution layers of the
 * Dequantization- / Refinement-Net U-Nets (dequantization_net.py:8-63).  Whole filter + raw patch in LDS, persistent blocks.
 * y = act2(affine(act1(conv + bias)) + residual).  prepared: shdr_conv2d_x3n_filter_elems_f32 floats from
 * shdr_conv2d_x3n_prepare_filter_f32 (w: HWIO with the descriptor's Cout columns).  Reached through shdr_conv2d_fwd_prepared_f32. */
int shdr_conv2d_x3n_ok_f32(const shdr_conv2d_desc* d);
int64_t shdr_conv2d_x3n_filter_elems_f32(const shdr_conv2d_desc* d);
int shdr_conv2d_x3n_prepare_filter_f32(const shdr_conv2d_desc* d, const float* w, float* prepared, void* stream);
int shdr_conv2d_fwd_x3n_f32(const shdr_conv2d_desc* d, const float* x1, const float* x2, const float* prepared, const float* bias,
                            const float* scale, const float* shift, const float* residual, float* y, float* y_pool, void* stream);
int shdr_conv2d_fwd_x3n_ranged_f32(const shdr_conv2d_desc* d, const float* x1, const float* x2, const float* prepared, const float* bias,
                                   const float* scale, const float* shift, const float* residual, float* y, float* y_pool,
                                   const float* x1_range, const float* x2_range, float* y_range, void* stream);

/* Split-operand weight gradient (csrc/wgrad_x3.hip): dW of the fp32 convolution on the fp16 matrix pipe, both operands split --
 * X 2^Tx = Xh + Xl 2^-11, dZ 2^Tz = Zh + Zl 2^-11, three v_mfma_f32_16x16x32_f16 per operand pair into two fp32 accumulator sets, per-product
 * error <= 3 * 2^-22 (GradientTape.gradient w.r.t. the Conv2D kernels, joint_training.py:185-186).  shdr_x3_split_planes_f32 writes the two
 * fp16 planes of a tensor (n % 8 == 0) scaled by the power of two its range slot asks for; shdr_conv2d_wgrad_x3_f32 accumulates
 * dw [KH*KW][C1+C2][Cout] += x_scale * sum_p X[p + tap] dZ[p] for source `which` from the planes and the SAME two slots (any stride / padding of
 * the descriptor; channels of the source and Cout multiples of 64: shdr_conv2d_wgrad_x3_ok_f32). */
int shdr_x3_split_planes_f32(const float* x, int64_t n, const float* range, void* hi, void* lo, void* stream);
int shdr_conv2d_wgrad_x3_ok_f32(const shdr_conv2d_desc* d, int which);
int shdr_conv2d_wgrad_x3_f32(const shdr_conv2d_desc* d, const void* xh, const void* xl, int which, const void* zh, const void* zl,
                             const float* x_range, const float* z_range, float* dw, void* stream);

/* Winograd-domain weight gradient of a 3x3 / stride-1 / SAME convolution (the backward counterpart of the fused Winograd
 * forward): dU[xi] += V[xi]^T Q[xi] over all 2x2 tiles (du: 16*Cx*Cout floats, zeroed by the caller), then
 * dw[3][3][Ct][Cout] (rows ci_off .. ci_off+Cx) += x_scale * G^T dU G.  x [N,H,W,Cx], dz [N,H,W,Cout];
 * Cx % 32 == 0, Cout % 64 == 0.  Same call sites as shdr_conv2d_wgrad_f32. */
int shdr_conv2d_wgrad_winograd_f32(const float* x, const float* dz, float* du, float* dw, int N, int H, int W, int Cx,
                                   int Cout, int Ct, int ci_off, float x_scale, void* stream);

/* ---- inference-tool image plumbing (test_real_refinement.py:119-155) -------------- */
/* y[p][c] = x[p][reverse ? 2-c : c] / 255: the decoded 8-bit image as float in [0,1] (:125). */
int shdr_u8_to_unit_f32(const uint8_t* x, float* y, int64_t npix, int reverse_channels, void* stream);
/* cv2.resize(..., interpolation=cv2.INTER_CUBIC) on NHWC float (:133, :146): A = -0.75 bicubic, half-pixel
 * centres, replicated border, no antialiasing. */
int shdr_resize_cubic_f32(const float* x, float* y, int N, int H, int W, int C, int Ho, int Wo, void* stream);
/* np.pad(x, pad, 'symmetric') over H and W (:136): y [N, H+2*pad, W+2*pad, C]. */
int shdr_pad_symmetric_f32(const float* x, float* y, int N, int H, int W, int C, int pad, void* stream);
/* float RGB -> Radiance RGBE bytes [npix,4], the pixel conversion of cv2.imwrite("*.hdr") (:150);
 * reverse_channels != 0 reads the pixel as BGR. */
int shdr_rgbe_encode_f32(const float* x, uint8_t* y, int64_t npix, int reverse_channels, void* stream);

/* Host-side Radiance scanline RLE of an RGBE image [height][width][4] (the adaptive run-length form of "*.hdr"
 * files, :150).  Returns the number of bytes written to `out`, or -1 (see shdr_last_error) if `capacity` is less than
 * height * (4 + 4 * (width + width / 127 + 2)). */
int64_t shdr_rgbe_rle_encode(const uint8_t* rgbe, int width, int height, uint8_t* out, int64_t capacity);
/* The inverse, host side: `size` bytes of scanline data (after the resolution line) -> RGBE [height][width][4]; flat and
 * adaptive-RLE scanlines, the pixel source of cv2.imread("*.hdr") (dataset.py:182).  Returns the number of bytes consumed,
 * or -1 (see shdr_last_error) on truncated or corrupt data; never reads past `size` or writes past the image. */
int64_t shdr_rgbe_rle_decode(const uint8_t* data, int64_t size, int width, int height, uint8_t* rgbe);

/* The same encoder on the device (csrc/hdr_rle.hip), for a BATCH of RGBE images of different sizes in one call: the bytes of
 * image i are exactly what shdr_rgbe_rle_encode writes for it (adaptive RLE for 8 <= W <= 32767, flat lines outside).
 *      rgbe        device bytes, 4-byte aligned: the images' [H][W][4] pixels back to back (a same-size batch [N][H][W][4] out of
 *                  shdr_rgbe_encode_f32 is already in this layout)
 *      shapes      int32 [n_images][2] = (H, W), as a host array, which is validated, and as the device copy of that very array
 *                  (shapes_dev), which the kernels read
 *      out         device bytes: the images' coded scanlines back to back; out_capacity must be at least the out_bytes of
 *                  shdr_rgbe_rle_encode_batch_sizes (the host routine's bound, 4 + 4 * (W + W / 127 + 2) per coded line)
 *      offsets     device int64 [n_images + 1]: image i is out[offsets[i] .. offsets[i + 1])
 *      workspace   workspace_bytes of shdr_rgbe_rle_encode_batch_sizes, 16-byte aligned, owned by the caller
 * Four stream-ordered launches (first rows, coded sizes per row and component, an exclusive scan over all rows, the write pass), no
 * atomics -- the same input gives the same bytes -- no host wait and no allocation.  Arguments are checked before anything is
 * launched.  The _timed form also fills stage_ms [SHDR_RLE_STAGES] with the device-event times of the four launches and then waits
 * for the last one (measurement only).  For every stage_ms of this library: an event call that fails never fails the call that is
 * measured; each time that could not be read is reported as -1. */
#define SHDR_RLE_STAGES 4
int shdr_rgbe_rle_encode_batch_sizes(const int32_t* shapes, int n_images, int64_t* out_bytes, int64_t* workspace_bytes);
int shdr_rgbe_rle_encode_batch(const uint8_t* rgbe, const int32_t* shapes, const int32_t* shapes_dev, int n_images, uint8_t* out,
                               int64_t out_capacity, int64_t* offsets, void* workspace, void* stream);
int shdr_rgbe_rle_encode_batch_timed(const uint8_t* rgbe, const int32_t* shapes, const int32_t* shapes_dev, int n_images, uint8_t* out,
                                     int64_t out_capacity, int64_t* offsets, void* workspace, void* stream, float* stage_ms);

/* ---- Radiance scanlines read on the device (hdr_io.rle_decode_device; csrc/hdr_rle_dec.h, csrc/hdr_rle_dec.hip) -------------- */
/* Per-file status of the reader, host twin and device alike (csrc/hdr_rle_dec.h holds the rules both run).  With the failing
 * scanline y, Python composes the text shdr_rgbe_rle_decode leaves in shdr_last_error (_ops.RGBE_DEC_REASONS). */
#define SHDR_RGBE_DEC_OK               0
#define SHDR_RGBE_DEC_TRUNCATED        1   /* "truncated data in scanline y": the data ends in front of a count byte or inside a packet */
#define SHDR_RGBE_DEC_CORRUPT_RUN      2   /* "corrupt run in scanline y": a run past the line's end */
#define SHDR_RGBE_DEC_CORRUPT_LITERAL  3   /* "corrupt literal in scanline y": a literal past the line's end */
#define SHDR_RGBE_DEC_TRUNCATED_FLAT   4   /* "truncated data in flat scanline y": fewer than 4 W bytes left for a flat line */
#define SHDR_RGBE_DEC_FALLBACK         5   /* (batch) more than 2 H + 64 line markers in the file: left to the host routine */
/* The host twin of shdr_rgbe_rle_decode, written from csrc/hdr_rle_dec.h: accepts exactly what that routine accepts, the same pixels
 * and the same return value (the bytes consumed; bytes behind line height - 1 are ignored).  On a refused file it returns -1 and
 * stores the status, the failing scanline and the offset at which the reader stood: the count byte of the failing packet (size, when
 * the data ended in front of a count byte) or the start of the flat line cut short.  Accepted: *status 0, *line -1, *stop the return
 * value.  -1 with *status untouched (see shdr_last_error) for bad arguments only.  Never reads past `size` or writes past the image. */
int64_t shdr_rgbe_rle_decode_status(const uint8_t* data, int64_t size, int width, int height, uint8_t* rgbe, int* status, int* line,
                                    int64_t* stop);
/* The same reader on the device for a BATCH of files of different shapes in one call.
 *      src                 device bytes, any alignment: the scanline data of all files back to back (the bytes after the resolution line)
 *      src_off             int64 [n_files + 1], non-decreasing, inside src, at most 2^31 - 1 bytes per file: a host array, which is
 *                          validated, and the device copy of that very array (_dev), which the kernels read and clamp again
 *      shapes              int32 [n_files][2] = (H, W), host array and device copy, as for shdr_rgbe_rle_encode_batch
 *      out                 device bytes, 4-byte aligned: the [H][W][4] pixels of all files back to back; out_bytes must be at least the
 *                          out_bytes of shdr_rgbe_rle_decode_batch_sizes (4 H W per file)
 *      out_off_dev         device int64 [n_files + 1], WRITTEN: file i is out[out_off[i] .. out_off[i + 1])
 *      workspace           device, 16-byte aligned, at least the workspace_bytes of shdr_rgbe_rle_decode_batch_sizes for the same tables
 *      status, line        device int32 [n_files]: SHDR_RGBE_DEC_* and the failing scanline (-1 for an accepted or FALLBACK file)
 *      consumed            device int64 [n_files]: the bytes consumed (accepted), the twin's stop offset (refused), -1 (FALLBACK)
 *      stage_ms            NULL, or float [SHDR_RGBE_DEC_STAGES] for the device-event times of the four stages (mark and compact the line
 *                          markers; parse every marked line; rank: rows by pointer doubling; expand) -- measurement only: the call
 *                          then waits for them
 * An accepted file's slot holds the host routine's pixels.  A FALLBACK file's slot is not written at all; a refused file's slot is
 * unspecified inside its bounds.  Nothing outside a file's own slot is written on its behalf, nothing outside src is read, and a
 * refused file does not affect the others.  Six stream-ordered launches, no global atomics -- the same input gives the same bytes --
 * no host wait and no allocation.  Arguments are checked before anything is launched. */
#define SHDR_RGBE_DEC_STAGES 4
int shdr_rgbe_rle_decode_batch_sizes(const int32_t* shapes, const int64_t* src_off, int n_files, int64_t* out_bytes,
                                     int64_t* workspace_bytes);
int shdr_rgbe_rle_decode_batch(const uint8_t* src, int64_t src_bytes, const int64_t* src_off, const int64_t* src_off_dev,
                               const int32_t* shapes, const int32_t* shapes_dev, int n_files, uint8_t* out, int64_t out_bytes,
                               int64_t* out_off_dev, void* workspace, int64_t workspace_bytes, int32_t* status, int32_t* line,
                               int64_t* consumed, void* stream, float* stage_ms);

/* ---- training-set patch sampler (dataset.py:141-252; cv2.resize with the default INTER_LINEAR, see csrc/dataset.hip) ---- */
/* HDRDataset._hdr_read_resize (dataset.py:181-202): RGBE [H0][W0][4] -> float BGR [H][W][3] (Ward's decode without +0.5,
 * channels reversed, clip(0, None)), resized by cv2's bilinear rule (half-pixel centres, replicated border). */
int shdr_hdr_load_resize_f32(const uint8_t* rgbe, float* y, int H0, int W0, int H, int W, void* stream);
/* np.mean of the 512 x 512 x 3 crop of PatchHDRDataset.__getitem__ (dataset.py:214-221, :268) for every (file, parity):
 * means[2 f + p].  Images at arena + offsets[f], dims[f] = {H, W}, min(H, W) == 512.  partials: 2 * n_files * 64 floats.
 * Deterministic (fixed-order fp32 tree). */
int shdr_hdr_window_means_f32(const float* arena, const int64_t* offsets, const int32_t* dims, int n_files, float* partials,
                              float* means, void* stream);
/* PatchHDRDataset.__getitem__ (dataset.py:212-252) for N samples in one launch: y [N][P][P][3].  params [N][param_stride]
 * int32 on the device: {idx, S, y0, x0, k, flip0, flip1}: crop of file idx / 2 and parity idx % 2, 0.5 x / (mean + 1e-6),
 * linear resize 512 -> S x S, crop P x P at (y0, x0), np.rot90(k), flip(axis 0), flip(axis 1).  P % 16 == 0; the
 * caller checks 0 <= idx < 2 n_files, P <= S, y0 + P <= S and x0 + P <= S (taps are clamped into the crop regardless). */
int shdr_hdr_patch_sample_f32(const float* arena, const int64_t* offsets, const int32_t* dims, const float* means,
                              const int32_t* params, int param_stride, int N, int n_files, int P, float* y, void* stream);

/* ---- OpenEXR training files (exr.py; single-part scanline, NONE / RLE / ZIPS / ZIP, see csrc/exr.hip) -------------- */
#define SHDR_EXR_HALF   1   /* OpenEXR pixel types (UINT = 0 is not a colour type here) */
#define SHDR_EXR_FLOAT  2
/* Host side: OpenEXR's signed-count RLE (a count byte c < 0 as int8: -c literal bytes follow; otherwise the next byte
 * repeated c + 1 times) of `size` bytes -> `out`.  Returns the number of bytes written, or -1 (see shdr_last_error) when a
 * run or literal overruns the input or `capacity`; never reads past `size` or writes past `capacity`.  The output is still
 * interleaved and delta-coded (shdr_exr_unpredict_u8 undoes both). */
int64_t shdr_exr_rle_decode(const uint8_t* data, int64_t size, uint8_t* out, int64_t capacity);
/* Chunks [chunk_off[c], chunk_off[c + 1]) of `payload` (size bytes, c < n_chunks; chunk_off int64 [n_chunks + 1] and coded
 * uint8 [n_chunks] on the device): coded chunks get the RLE / ZIP predictor and the byte interleave undone, the others are
 * copied; `out` has the payload's layout.  One workgroup per chunk, deterministic.  Offsets are clamped into [0, size]. */
int shdr_exr_unpredict_u8(const uint8_t* payload, uint8_t* out, int64_t size, const int64_t* chunk_off, const uint8_t* coded,
                          int n_chunks, void* stream);
/* Planar scanline bytes (size bytes; row r at chunk_off[r / lines] + (r % lines) * row_bytes, n_chunks = ceil(H0 / lines))
 * -> float [H][W][3]: output channel i is the run at byte chan_off[i] of each scanline, of type chan_type[i]
 * (SHDR_EXR_HALF / SHDR_EXR_FLOAT; chan_off and chan_type are 3-entry HOST arrays).  clip != 0 applies np.clip(x, 0, None)
 * to the source samples (NaN and +inf pass).  Resized by the rule of shdr_hdr_load_resize_f32 with the same arithmetic;
 * H == H0 and W == W0 is an exact copy.  Sample reads are clamped into the buffer. */
int shdr_exr_load_resize_f32(const uint8_t* planes, int64_t size, const int64_t* chunk_off, int n_chunks, int lines,
                             int64_t row_bytes, const int64_t* chan_off, const int32_t* chan_type, int H0, int W0, float* y,
                             int H, int W, int clip, void* stream);

/* ---- zlib streams inflated (exr.py read_stored / upload_batch; csrc/inflate.h, csrc/inflate.hip) ------------------------- */
/* Per-chunk status of the decoder, host and device alike (csrc/inflate.h holds the code both run). */
#define SHDR_INFLATE_OK               0
#define SHDR_INFLATE_TRUNCATED        1   /* the stream ends inside the header, a block or the Adler-32 */
#define SHDR_INFLATE_HEADER           2   /* CM != 8, CINFO > 7 or the header check */
#define SHDR_INFLATE_DICTIONARY       3   /* FDICT */
#define SHDR_INFLATE_BLOCK_TYPE       4   /* BTYPE 3 */
#define SHDR_INFLATE_STORED_LENGTH    5   /* LEN != ~NLEN */
#define SHDR_INFLATE_COUNTS           6   /* HLIT > 286 or HDIST > 30 */
#define SHDR_INFLATE_CODE_LENGTH_SET  7   /* the code-length code is over-subscribed or incomplete */
#define SHDR_INFLATE_REPEAT           8   /* repeat-16 with no previous length */
#define SHDR_INFLATE_RUN              9   /* a run overflows HLIT + HDIST */
#define SHDR_INFLATE_NO_END_OF_BLOCK 10   /* symbol 256 has no code */
#define SHDR_INFLATE_LITERAL_SET     11   /* literal/length code set over-subscribed or incomplete */
#define SHDR_INFLATE_DISTANCE_SET    12   /* distance code set over-subscribed or incomplete */
#define SHDR_INFLATE_LITERAL_CODE    13   /* a code no literal/length symbol owns, or symbol 286 / 287 */
#define SHDR_INFLATE_DISTANCE_CODE   14   /* a code no distance symbol owns, or symbol 30 / 31 */
#define SHDR_INFLATE_DISTANCE_FAR    15   /* a distance beyond the bytes produced so far */
#define SHDR_INFLATE_OVERFLOW        16   /* the output is longer than the slot */
#define SHDR_INFLATE_SHORT           17   /* the stream is complete, its output shorter than the slot */
#define SHDR_INFLATE_CHECKSUM        18   /* Adler-32 */
#define SHDR_INFLATE_RAW_SIZE        19   /* (batch) a stored-raw chunk whose size is not the slot's */
#define SHDR_INFLATE_MODE            20   /* (batch) a mode byte other than 0 / 1 */
/* The zlib stream src[0 .. n) (RFC 1950 / 1951: stored, fixed and dynamic blocks; zlib's acceptance rules, no preset dictionary;
 * bytes after the Adler-32 are ignored) into dst[0 .. capacity), capacity <= 2^30 being the size the output must have (host).
 * Returns the number of bytes written, never more than `capacity`, and stores the status in *status; nothing outside
 * [src, src + n) is read, whatever the bytes are.  -1 (see shdr_last_error) for bad arguments only. */
int64_t shdr_inflate_host(const uint8_t* src, int64_t n, uint8_t* dst, int64_t capacity, int* status);
/* The same decoder on the device for a BATCH of chunks in one launch, one 64-lane workgroup per chunk: chunk c is read from
 * src[src_off[c] .. src_off[c + 1]) and written into the slot dst[dst_off[c] .. dst_off[c + 1]); any byte alignment of both.
 *      src_off, dst_off   int64 [n_chunks + 1], non-decreasing, inside the buffers, chunks and slots of 0 .. 2^30 bytes: host arrays,
 *                         which are validated before anything is launched, and the device copies of those very arrays (_dev),
 *                         which the kernel reads and clamps into the buffers again
 *      mode               device uint8 [n_chunks], or NULL for all 1: 1 a zlib stream, 0 stored raw (copied if its size is the slot's)
 *      status, written    device int32 [n_chunks] and int64 [n_chunks]: SHDR_INFLATE_* and the bytes written into the slot
 *                         (never more than the slot; bytes of the slot beyond them are left untouched)
 *      stage_ms           NULL, or float [SHDR_INFLATE_STAGES] for the device-event time of the launch (measurement only: the call
 *                         then waits for it)
 * Stream-ordered, deterministic, no global atomics, no host wait, no allocation.  shdr_inflate_batch_sizes validates the two tables
 * and returns the bytes that src and dst must hold at least. */
#define SHDR_INFLATE_STAGES 1
int shdr_inflate_batch_sizes(const int64_t* src_off, const int64_t* dst_off, int n_chunks, int64_t* src_bytes, int64_t* dst_bytes);
int shdr_inflate_batch(const uint8_t* src, int64_t src_bytes, const int64_t* src_off, const int64_t* src_off_dev, uint8_t* dst,
                       int64_t dst_bytes, const int64_t* dst_off, const int64_t* dst_off_dev, const uint8_t* mode, int n_chunks,
                       int32_t* status, int64_t* written, void* stream, float* stage_ms);

/* ---- OpenEXR PIZ chunks decoded (exr.py piz="host" / "device"; csrc/piz.h, csrc/piz.hip) -------------------------------- */
/* Per-chunk status of the decoder, host and device alike (csrc/piz.h holds the rules both run).  The reader is UNPINNED: the format is
 * restated from memory of OpenEXR 2.x, and no OpenEXR-written file has been read. */
#define SHDR_PIZ_OK               0
#define SHDR_PIZ_TRUNCATED        1   /* the chunk ends inside minNonZero / maxNonZero or the length field */
#define SHDR_PIZ_BITMAP           2   /* maxNonZero >= 8192, or the bitmap runs past the chunk */
#define SHDR_PIZ_LENGTH           3   /* the Huffman block's length is negative or runs past the chunk */
#define SHDR_PIZ_NO_DATA          4   /* length == 0 or nBits == 0 */
#define SHDR_PIZ_HUFF_HEADER      5   /* a block of fewer than 20 bytes, im or iM >= 65537, im > iM */
#define SHDR_PIZ_TABLE_TRUNCATED  6   /* the code-length table runs past the block */
#define SHDR_PIZ_TABLE_RUN        7   /* a zero run past iM + 1 */
#define SHDR_PIZ_OVER_SUBSCRIBED  8   /* the code lengths' Kraft sum exceeds 1 */
#define SHDR_PIZ_NBITS            9   /* nBits beyond the bytes that follow the table */
#define SHDR_PIZ_BAD_CODE        10   /* bits that no code owns */
#define SHDR_PIZ_DATA_TRUNCATED  11   /* a code word or a run count runs past nBits */
#define SHDR_PIZ_RUN_NO_PREV     12   /* a run with no previous value */
#define SHDR_PIZ_TOO_MANY        13   /* more values than the chunk holds */
#define SHDR_PIZ_TOO_FEW         14   /* nBits consumed and fewer values than the chunk holds */
#define SHDR_PIZ_RAW_SIZE        15   /* (batch) a stored-raw chunk, or a slot, whose size is not the shape's */
#define SHDR_PIZ_MODE            16   /* (batch) a mode byte other than 0 / 1 */
/* The PIZ chunk src[0 .. n) of `rows` (1 .. 32) scanlines of `width` pixels and n_chan (1 .. 64) channels in name order, chan_words[c]
 * being 1 for a HALF channel and 2 for FLOAT / UINT, into dst[0 .. capacity): the planar scanlines (row by row, channel by channel
 * within a row, little-endian) that shdr_exr_load_resize_f32 reads; capacity must be 2 * width * rows * sum(chan_words) <= 2^28 (host).
 * Returns the bytes written -- capacity, or 0 for a refused chunk, whose dst is left untouched -- and stores the status in *status;
 * nothing outside [src, src + n) is read, whatever the bytes are.  -1 (see shdr_last_error) for bad arguments only. */
int64_t shdr_piz_decode_host(const uint8_t* src, int64_t n, int width, int rows, const int32_t* chan_words, int n_chan, uint8_t* dst,
                             int64_t capacity, int* status);
/* The same decoder on the device for a BATCH of chunks of any files and shapes, two launches (Huffman decode, one workgroup per chunk:
 * header pass, self-synchronising subsequences of sub_bits bits, scan, write; then the inverse wavelet, one workgroup per strip of a
 * word plane).  Chunk c is read from src[src_off[c] .. src_off[c + 1]) and written into the slot dst[dst_off[c] .. dst_off[c + 1]).
 *      src_off, dst_off   int64 [n_chunks + 1] as for shdr_inflate_batch (host arrays, validated, and their device copies); chunks of
 *                         at most 2^28 bytes; a slot starts at an even byte and has exactly the size of the chunk's shape
 *      geom               int32 [n_chunks][4]: width, rows, first entry and number of entries in chan_words (host and device copy)
 *      chan_words         int32 [n_words]: 1 or 2 per channel (host and device copy)
 *      mode               device uint8 [n_chunks], or NULL for all 1: 1 a PIZ chunk, 0 stored raw (copied if its size is the slot's)
 *      sub_bits           bits per subsequence, 128 .. 2^20; 0: the default (256)
 *      workspace          device, 16-byte aligned, at least the bytes shdr_piz_batch_sizes returns for the same tables and sub_bits
 *      status, written    device int32 [n_chunks] and int64 [n_chunks]: SHDR_PIZ_* and the bytes written into the slot (all or 0: the
 *                         slot of a refused chunk is left untouched)
 *      rounds             NULL, or device int32 [n_chunks][SHDR_PIZ_ROUND_STATS] (measurement): the synchronisation rounds each chunk
 *                         took, then the subsequences that round 0, 1, ... decoded (round 0: all of them; zero past the last round)
 *      stage_ms           NULL, or float [SHDR_PIZ_STAGES] for the device-event times of the two launches (measurement only: the call
 *                         then waits for them)
 * Stream-ordered, deterministic, no atomics, no host wait, no allocation. */
#define SHDR_PIZ_STAGES 2
#define SHDR_PIZ_ROUND_STATS 9
int shdr_piz_batch_sizes(const int64_t* src_off, const int64_t* dst_off, const int32_t* geom, const int32_t* chan_words, int n_words,
                         int n_chunks, int sub_bits, int64_t* src_bytes, int64_t* dst_bytes, int64_t* workspace_bytes);
int shdr_piz_batch(const uint8_t* src, int64_t src_bytes, const int64_t* src_off, const int64_t* src_off_dev, uint8_t* dst,
                   int64_t dst_bytes, const int64_t* dst_off, const int64_t* dst_off_dev, const uint8_t* mode, const int32_t* geom,
                   const int32_t* geom_dev, const int32_t* chan_words, const int32_t* chan_words_dev, int n_words, int n_chunks,
                   int sub_bits, void* workspace, int64_t workspace_bytes, int32_t* status, int64_t* written, int32_t* rounds,
                   void* stream, float* stage_ms);

/* ---- OpenEXR PIZ chunks encoded (exr.py compression="piz", piz="host" / "device"; csrc/piz.h, csrc/piz_enc.hip) -------------- */
/* UNPINNED AGAINST THE OPENEXR LIBRARY, LIKE THE READER: the format is restated from memory of OpenEXR 2.x and NO OpenEXR-built
 * reader has opened a file written here.  What is pinned: tests/piz_ref.py writes the same bytes, and this library's decoders and
 * piz_ref's read them back.
 * The planar scanlines raw[0 .. n) of one chunk (rows 1 .. 32, n_chan 1 .. 64 channels in name order, chan_words[c] 1 for HALF and 2
 * for FLOAT / UINT, n = 2 * width * rows * sum(chan_words) <= 2^28; host) -> its PIZ bytes in dst, WHATEVER THEIR SIZE: *written
 * receives their number.  A caller that stores a chunk raw when coding does not shrink it (OpenEXR's rule) compares *written with n:
 * the chunk counts as coded only if the PIZ bytes are STRICTLY fewer.  The rules (csrc/piz.h): bitmap of the values present, value 0
 * implied; the forward LUT is the rank among them; forward wavelet per word plane (the 14-bit pair while fewer than 16385 values
 * are present); a stretch of equal values is the value once and, from 3 repeats on, run codes of at most 255 repeats each; the
 * optimal code of the tokens' frequencies by the two-queue method (leaves in (count, symbol) order, a leaf before an internal node
 * of the same weight); canonical codes; the 6-bit length table with both zero-run forms, cut greedily.
 * Returns SHDR_OK, or a negative SHDR_E_* code (see shdr_last_error) for a NULL pointer, rows outside 1 .. 32, n_chan outside
 * 1 .. 64, words other than 1 / 2, an n that is not the shape's, or a capacity below the bytes to write (nothing is written then);
 * shdr_piz_encode_bound returns a capacity that always suffices (-1 for a shape out of range). */
int64_t shdr_piz_encode_bound(int width, int rows, const int32_t* chan_words, int n_chan);
/* One wavelet pair of csrc/piz.h (host; for tests of the rules): which = 0 enc14, 1 enc16 -- (a, b) -> out = (l, h) --, 2 dec14, 3 dec16
 * -- (l, h) -> out = (a, b); the arguments are taken mod 2^16. */
int shdr_piz_wavelet_pair(int which, unsigned a, unsigned b, uint16_t* out);
int shdr_piz_encode_host(const uint8_t* raw, int64_t n, int width, int rows, const int32_t* chan_words, int n_chan, uint8_t* dst,
                         int64_t capacity, int64_t* written);
/* The same encoder on the device for a BATCH of chunks of any widths, row counts and channel sets: chunk c is
 * planar[chunk_off[c] .. chunk_off[c + 1]), its shape geom[c].
 *      planar       device bytes, 2-byte aligned: the chunks' planar scanlines (what shdr_exr_pack_f32 writes with lines = 32)
 *      chunk_off    int64 [n_chunks + 1], chunk_off[0] = 0, host array (validated: every chunk has its shape's size) and its device copy
 *      geom, chan_words   as for shdr_piz_batch (host arrays and device copies)
 *      pad, out, out_offsets, coded   as for shdr_deflate_huffman_batch: chunk c is stored at out[out_offsets[c] + pad ..
 *                   out_offsets[c + 1]) -- the bytes of shdr_piz_encode_host where those are STRICTLY fewer than the chunk's
 *                   (coded[c] = 1), else the chunk's scanline bytes -- so that shdr_exr_finish_chunks finishes the files;
 *                   out_capacity at least the out_bytes of the _sizes call (the chunks' bytes + pad * n_chunks)
 *      workspace    workspace_bytes of the _sizes call (about 2.5 MB per chunk + 3 bytes per input byte), 16-byte aligned
 *      stats        NULL, or device int32 [n_chunks][SHDR_PIZ_ENC_STATS] (measurement): the symbols the chunk's code has, and the ticks
 *                   of the device's constant-rate counter (wall_clock64) that the one-lane merge of the code lengths took
 *      stage_ms     NULL, or float [SHDR_PIZ_ENC_STAGES]: device-event times of clear, front (bitmap, LUT, wavelet), hist, code (sort,
 *                   merge, canonical codes, table), bits, scan, final (measurement only: the call then waits)
 * Byte for byte the host routine's output and run to run identical: integer atomics only (LDS atomicOr for the bitmap, global atomicAdd
 * for the per-chunk histogram, global atomicOr for the bit streams), all of them commutative.  Stream-ordered, no host wait, no
 * allocation.  Arguments are checked before anything is launched. */
#define SHDR_PIZ_ENC_STAGES 7
#define SHDR_PIZ_ENC_STATS 2
int shdr_piz_encode_batch_sizes(const int64_t* chunk_off, const int32_t* geom, const int32_t* chan_words, int n_words, int n_chunks, int pad,
                                int64_t* out_bytes, int64_t* workspace_bytes);
int shdr_piz_encode_batch(const uint8_t* planar, const int64_t* chunk_off, const int64_t* chunk_off_dev, const int32_t* geom,
                          const int32_t* geom_dev, const int32_t* chan_words, const int32_t* chan_words_dev, int n_words, int n_chunks, int pad,
                          uint8_t* out, int64_t out_capacity, int64_t* out_offsets, uint8_t* coded, void* workspace, int64_t workspace_bytes,
                          int32_t* stats, void* stream, float* stage_ms);

/* ---- OpenEXR output (exr.py encode_exr / write_exr; csrc/exr_write.hip, csrc/deflate.hip) ------------------------------ */
/* Huffman-only zlib stream of src[0 .. n), 1 <= n <= 2^30 (host): 78 01, one final dynamic-Huffman block of literals with a
 * fixed-length header (csrc/deflate_huffman.h), the big-endian Adler-32.  zlib's inflate reads it.  Returns the stream's length,
 * or -1 (see shdr_last_error) for bad arguments or when `capacity` is less than that length (nothing is written then).  The
 * stream is written whatever its size; a caller that stores a chunk raw when coding does not shrink it (OpenEXR's rule)
 * compares the returned length with n: the chunk counts as coded only if the stream is STRICTLY smaller. */
int64_t shdr_deflate_huffman_host(const uint8_t* src, int64_t n, uint8_t* dst, int64_t capacity);
/* The code lengths of that stream (host): lengths[257], literals 0..255 and end-of-block; 0 for unused symbols, 1..15 for the
 * others, Kraft sum exactly 1. */
int shdr_deflate_huffman_lengths_host(const uint8_t* src, int64_t n, uint8_t* lengths);
/* The same encoder on the device for a BATCH of chunks: chunk c is data[offsets[c] .. offsets[c + 1]).
 *      data         device bytes
 *      raw          device bytes with the same offsets, or NULL for `data`: what is stored for a chunk that is not coded
 *      offsets      int64 [n_chunks + 1], offsets[0] = 0, as a host array, which is validated, and as the device copy of that
 *                   very array (offsets_dev), which the kernels read (clamped into the data)
 *      pad          bytes left untouched in front of every stored chunk (room for a caller's chunk header), 0 .. 4096
 *      out          device bytes: per chunk `pad` bytes, then the stream of shdr_deflate_huffman_host if it is strictly smaller
 *                   than the chunk, else the chunk's `raw` bytes; out_capacity at least the out_bytes of the _sizes call
 *                   (the chunks' bytes + pad * n_chunks)
 *      out_offsets  device int64 [n_chunks + 1]: chunk c is stored at out[out_offsets[c] + pad .. out_offsets[c + 1])
 *      coded        device uint8 [n_chunks]: 1 where the stream was stored
 *      workspace    workspace_bytes of the _sizes call, 16-byte aligned, owned by the caller
 *      stage_ms     NULL, or float [SHDR_DEFLATE_STAGES] for the device-event times of the three launches (measurement only: the
 *                   call then waits for the last one)
 * Three stream-ordered launches (histogram + code lengths + Adler-32 per chunk, an exclusive scan of the stored sizes, the write
 * pass in tiles of SHDR_DEFLATE_TILE symbols), no global atomics -- the same input gives the same bytes -- no host wait and no
 * allocation.  Arguments are checked before anything is launched. */
#define SHDR_DEFLATE_STAGES 3
#define SHDR_DEFLATE_TILE 1024
int shdr_deflate_huffman_batch_sizes(const int64_t* offsets, int n_chunks, int pad, int64_t* out_bytes, int64_t* workspace_bytes);
int shdr_deflate_huffman_batch(const uint8_t* data, const uint8_t* raw, const int64_t* offsets, const int64_t* offsets_dev,
                               int n_chunks, int pad, uint8_t* out, int64_t out_capacity, int64_t* out_offsets, uint8_t* coded,
                               void* workspace, void* stream, float* stage_ms);
/* zlib stream WITH LZ77 matches of src[0 .. n), 1 <= n <= 2^30 (host): 78 01, one final dynamic-Huffman block of literals,
 * lengths and distances with a fixed-length header, the big-endian Adler-32 (csrc/deflate_lz.h states the parse: a chainless
 * hash table read in groups of 64 positions, the run candidate p - 1, greedy).  zlib's inflate reads it.  Returns and the
 * caller's coded-only-if-strictly-smaller rule as shdr_deflate_huffman_host; the call allocates 4 n bytes of scratch. */
int64_t shdr_deflate_lz_host(const uint8_t* src, int64_t n, uint8_t* dst, int64_t capacity);
/* The parse of that stream (host): tokens[n], one per position -- 0 where an earlier match covers the position,
 * SHDR_DEFLATE_LZ_LITERAL | byte for a literal, length << 16 | distance for a match (3..258, 1..32768). */
#define SHDR_DEFLATE_LZ_LITERAL 0x80000000u
int shdr_deflate_lz_parse_host(const uint8_t* src, int64_t n, uint32_t* tokens);
/* The same encoder on the device for a BATCH of chunks: the arguments, the stored form, the status codes and the refusals of
 * shdr_deflate_huffman_batch, with the streams of shdr_deflate_lz_host.  The workspace also holds one 4-byte token per input
 * byte (workspace_bytes of this _sizes call).  Three stream-ordered launches (parse + counts + code lengths + Adler-32, one
 * 64-lane wave per chunk; the scan; the write pass in tiles of SHDR_DEFLATE_LZ_TILE positions), no global atomics, no host
 * wait, no allocation; stage_ms receives SHDR_DEFLATE_STAGES times. */
#define SHDR_DEFLATE_LZ_TILE 1024
int shdr_deflate_lz_batch_sizes(const int64_t* offsets, int n_chunks, int pad, int64_t* out_bytes, int64_t* workspace_bytes);
int shdr_deflate_lz_batch(const uint8_t* data, const uint8_t* raw, const int64_t* offsets, const int64_t* offsets_dev,
                          int n_chunks, int pad, uint8_t* out, int64_t out_capacity, int64_t* out_offsets, uint8_t* coded,
                          void* workspace, void* stream, float* stage_ms);

/* float32 images [H][W][3] -> OpenEXR scanline bytes, for a BATCH of images of different sizes in one launch.  A chunk is `lines`
 * scanlines (1: NONE / ZIPS, 16: ZIP, 32: PIZ; the last chunk of an image may hold fewer); a scanline is W samples of B, then G, then R
 * (the name-sorted order), HALF or FLOAT.  reverse_channels = 0: the pixel is R, G, B; != 0: it is B, G, R (the networks' order).
 * HALF is round to nearest even with subnormals, overflow to +-inf and NaN kept (numpy's astype(float16)); saturate != 0 first
 * turns finite values beyond +-65504 into +-65504.
 *      pixels     device floats: the images back to back
 *      shapes     int32 [n_images][2] = (H, W), host: validated
 *      table_dev  device int64 [3][n_images + 1], the device copy of the `table` of shdr_exr_pack_sizes: row 0 the first chunk of
 *                 image i, row 1 its first pixel, row 2 H_i * 2^32 + W_i (column n_images: the totals, and 0)
 *      chunk_off  device int64 [n_chunks + 1]: chunk c is bytes [chunk_off[c], chunk_off[c + 1]) of planar / predicted
 *      planar     device bytes [bytes]: the scanline bytes
 *      predicted  NULL, or device bytes [bytes]: per chunk, the even bytes then the odd bytes, delta-coded
 *                 (d[0] = t[0], d[i] = t[i] - t[i-1] + 128): what ZIP / ZIPS deflate
 * shdr_exr_pack_sizes validates the shapes and returns the number of chunks and of bytes and, if the pointers are given, fills
 * the HOST arrays table [3 * (n_images + 1)] and chunk_off [n_chunks + 1] that the caller uploads. */
int shdr_exr_pack_sizes(const int32_t* shapes, int n_images, int pixel_type, int lines, int64_t* n_chunks, int64_t* bytes,
                        int64_t* table, int64_t* chunk_off);
int shdr_exr_pack_f32(const float* pixels, const int32_t* shapes, int n_images, int pixel_type, int lines, int reverse_channels,
                      int saturate, const int64_t* table_dev, const int64_t* chunk_off, uint8_t* planar, uint8_t* predicted,
                      void* stream);
/* Chunk headers and offset tables of a batch of files whose chunks shdr_deflate_huffman_batch (or shdr_piz_encode_batch, lines = 32)
 * stored with pad = 8: writes
 * int32 y, int32 size in front of every chunk at records[out_offsets[c]] and the uint64 file offset of chunk c to
 * tables[8 c]: header_len[i] + 8 * (chunks of image i) + the chunk's distance from the image's first chunk.  table_dev as
 * above; header_len: device int64 [n_images], the bytes of file i in front of its offset table. */
int shdr_exr_finish_chunks(uint8_t* records, uint8_t* tables, const int64_t* out_offsets, const int64_t* table_dev,
                           const int64_t* header_len, int n_images, int64_t n_chunks, int lines, void* stream);

/* ---- camera-pipeline simulator (joint_training.py:26-69 `_preprocessing`) ------------- */
/* Philox4x32-10 block function (host): the counter-based generator the noise kernel uses; exported so that tests can
 * check the published known-answer vectors. */
int shdr_philox4x32_10(const uint32_t counter[4], const uint32_t key[2], uint32_t out[4]);
/* hdr_t = relu(hdr*t + N(0,1)*(sigma_s*hdr*t) + sigma_c*N(0,1)), sigma_s = 0.08/6*U, sigma_c = 0.005*U per (sample,
 * channel) (:30-40); clipped = min(hdr_t, 1) (:43).  hdr [N,H,W,3], t [N].  Stateless: the same seed gives the same
 * noise field for any launch geometry. */
int shdr_camera_expose_f32(const float* hdr, const float* t, float* hdr_t, float* clipped, int N, int H, int W,
                           uint64_t seed, void* stream);
/* jpeg = tf.cast(tf.image.adjust_jpeg_quality(uint8(round(ldr*255)), quality[n]), float32) / 255 (:46-52) -- a
 * baseline-JPEG round trip (4:2:0, islow DCT, fancy upsampling) in libjpeg's integer arithmetic, bit for bit -- and
 * loss_mask [N] (:54-63; may be NULL).  H % 16 == W % 16 == 0.  ws_planes: N*H*W*3/2 bytes, ws_counts: 2*N int32. */
int shdr_jpeg_round_trip_f32(const float* ldr, const int32_t* quality, float* jpeg, float* loss_mask,
                             uint8_t* ws_planes, int32_t* ws_counts, int N, int H, int W, void* stream);

/* HDR-Real record augmentation (finetune_real_dataset.py:49-61): per sample,
 * y = rot90(flip_left_right(x) if flip[n] else x, k = rot[n]) / divisor on square NHWC images [N,S,S,C]
 * (tf.image.rot90 = counter-clockwise). */
int shdr_flip_rot90_f32(const float* x, float* y, const int32_t* flip, const int32_t* rot, int N, int S, int C,
                        float divisor, void* stream);

/* ---- HDR-Real image folders resident on the device (convert_to_tf_record.py:50-86, finetune_real_dataset.py:43-61; SURVEY.md
 *      section 8f rank 4).  Every HDR_gt / LDR_in pair lies once in two flat arenas, LDR as uint8 RGB and HDR as float32 RGB, both
 *      [arena_pixels, 3], addressed by ONE table:
 *        images  int64 [n_images, 3]   (first pixel of the image in both arenas, H, W)
 *        patches int32 [n_patches, 3]  (image, h1, w1): top-left corner of a size x size patch
 *        samples int32 [b, 3]          (patch, flip 0 / 1, rot 0 .. 4; 4 is 0: int(u * 4 + 0.5) of finetune_real_dataset.py:58)
 *      The kernels trust their tables, so the library checks them first: every table is passed twice, `*_host` in host memory, which
 *      the call validates before anything is launched, and the caller's device copy of the same bytes, which the kernel reads.  A patch
 *      that leaves its image, an image that leaves the arenas, an index out of a table, a flip or rot out of range, size <= 0 and
 *      b <= 0 are refused with SHDR_E_SHAPE, a NULL pointer with SHDR_E_NULL.  The stats call checks every patch, the gather call the
 *      patches its samples name.  Nothing is allocated and nothing is copied by the library. ---- */
/* count[p] = pixels of LDR patch p whose grey value r*0.299f + g*0.587f + b*0.114f (fp32, left to right, every product and sum
 * rounded) is >= 249 or <= 6 (convert_to_tf_record.py:54-55); mean[p] = (float)(sum of HDR patch p in float64 / (size*size*3)).
 * One workgroup per patch, a fixed reduction tree, no atomics: the same data give the same bits. */
int shdr_pair_patch_stats(const uint8_t* ldr, const float* hdr, int64_t arena_pixels, const int64_t* images_host,
                          const int64_t* images, int n_images, const int32_t* patches_host, const int32_t* patches, int n_patches,
                          int size, int32_t* count, float* mean, void* stream);
/* out_ldr[n] = rot90(flip_left_right(LDR patch) if flip else LDR patch, rot) / 255.0f and
 * out_hdr[n] = rot90(flip(HDR patch), rot) / (1e-6f + mean[patch]) * 0.5f, both float32 [b, size, size, 3], in one launch. */
int shdr_pair_patch_gather_f32(const uint8_t* ldr, const float* hdr, int64_t arena_pixels, const int64_t* images_host,
                               const int64_t* images, int n_images, const int32_t* patches_host, const int32_t* patches,
                               int n_patches, const float* mean, const int32_t* samples_host, const int32_t* samples, int b, int size,
                               float* out_ldr, float* out_hdr, void* stream);


/* ---- native-fp16 activation path: BASELINE configs[4] ("finetune_real_dataset.py with Refinement-Net, 1024x1024 tiles,
 *      fp16 MFMA conv path").  Feature maps are NHWC fp16 (`void*` = _Float16 / IEEE binary16) with C % 8 == 0, image-like
 *      3-channel tensors and every parameter / parameter gradient stay fp32, accumulation is fp32.  These are the `_f16` twins of
 *      the entry points above and replace the same TF call sites (finetune_real_dataset.py:144-178). ---- */
/* number of fp16 elements of the packed filter of a [KH,KW,C1+C2,Cout] conv */
int64_t shdr_conv2d_packed_filter_elems_f16(int KH, int KW, int C1, int C2, int Cout);
/* fp32 HWIO filter -> packed fp16 [k-chunk][Cout][32] in the k order of shdr_conv2d_fwd_f16; x2_scale is folded into the rows of
 * the second source (hallucination_net.py:101) */
int shdr_conv2d_pack_filter_f16(const float* w, void* wp, int KH, int KW, int C1, int C2, int Cout, float x2_scale, void* stream);
/* y = act1(conv(concat[x1, x2], wp) + bias): tf.keras.layers.Conv2D forward, and -- run on dZ with the flipped / transposed
 * filter -- GradientTape.gradient w.r.t. its input.  d->C1 % 8 == d->C2 % 8 == 0, d->Cout % 16 == 0; y fp16 [N,Ho,Wo,Cout], or
 * fp32 [N,Ho,Wo,cout_valid] when y_is_f32 (the 3-channel heads); scale / shift / residual / act2 of the desc are not used. */
int shdr_conv2d_fwd_f16(const shdr_conv2d_desc* d, const void* x1, const void* x2, const void* wp, const float* bias, void* y,
                        int y_is_f32, void* stream);
/* Inference form: y = act2(affine(act1(conv(concat[x1, x2], wp) + bias)) + residual), affine(v) = v * scale[co] + shift[co] -- the
 * epilogue of shdr_conv2d_fwd_f32 on fp16 feature maps, accumulation and epilogue in fp32, one rounding to fp16.  Replaces, with
 * training=False and the folded inference BatchNormalization: the conv -> BN -> relu of hallucination_net.py:163-165, the `up` blocks'
 * conv -> relu -> BN -> relu (:86-89), the composed s1 -> conv2 -> norm2 -> relu tail (:179-185), the heads tanh(out(x)) + input
 * (dequantization_net.py:62-63) and relu(input[..., 0:3] + out(x)) (refinement_net.py:63-66).
 * scale / shift: fp32 per output channel or NULL (identity); residual: NULL, or fp32 (residual_is_f32) / fp16 [N,Ho,Wo,d->res_cstride]
 * read at channel co; act2 = d->act2.  y as shdr_conv2d_fwd_f16 (fp16 [N,Ho,Wo,Cout], or fp32 [N,Ho,Wo,cout_valid]).  tanh (act1 or
 * act2) on an fp16 output is refused (SHDR_E_SHAPE).  Without scale, shift, residual and act2 this IS shdr_conv2d_fwd_f16. */
int shdr_conv2d_fwd_fused_f16(const shdr_conv2d_desc* d, const void* x1, const void* x2, const void* wp, const float* bias,
                              const float* scale, const float* shift, const void* residual, int residual_is_f32, void* y, int y_is_f32,
                              void* stream);
/* dw[kh][kw][ci_off + ci][co] += scale * sum_p x[p + tap][ci] * dz[p][co]  (fp32, accumulated with atomics; the caller zeroes dw).
 * x = source `which` of the forward conv `d` (d->C1 / d->C2 = channels per pixel of the fp16 tensors, possibly zero-padded),
 * dz fp16 with dz_channels per pixel; dw = [KH,KW,c1_rows + c2_rows, d->Cout], of which the first cout_valid columns are written. */
int shdr_conv2d_wgrad_f16(const shdr_conv2d_desc* d, const void* x, int which, const void* dz, int dz_channels, int c1_rows,
                          int c2_rows, float* dw, void* stream);
/* specialised forms the two entry points above dispatch to (exported so that a host can test / force them): the narrow-layer
 * forward with the raw patch and the whole filter resident in LDS, and the all-taps weight gradient of stride-1 layers */
int shdr_conv2d_patch_ok_f16(const shdr_conv2d_desc* d);
int shdr_conv2d_fwd_patch_f16(const shdr_conv2d_desc* d, const void* x1, const void* x2, const void* wp, const float* bias, void* y,
                              int y_is_f32, void* stream);
int shdr_conv2d_w3_ok_f16(const shdr_conv2d_desc* d);       /* wide 3x3 / stride-1 layers: raw patch per 32-channel chunk in LDS */
int shdr_conv2d_fwd_w3_f16(const shdr_conv2d_desc* d, const void* x1, const void* x2, const void* wp, const float* bias, void* y,
                           void* stream);
int shdr_conv2d_wgrad_alltaps_ok_f16(const shdr_conv2d_desc* d, int which, int dz_channels);
int shdr_conv2d_wgrad_alltaps_f16(const shdr_conv2d_desc* d, const void* x, int which, const void* dz, int dz_channels, int c1_rows,
                                  int c2_rows, float* dw, void* stream);
int shdr_cast_f32_to_f16(const float* x, void* y, int64_t n, void* stream);
int shdr_cast_f16_to_f32(const void* x, float* y, int64_t n, void* stream);
/* fp32 [npix, Cin] -> fp16 [npix, Cout] zero-padded (narrow gradients of the 3-channel heads onto 8-channel groups) */
int shdr_pad_channels_f32_to_f16(const float* x, void* y, int64_t npix, int Cin, int Cout, void* stream);
/* tf.concat of up to four 3-channel fp32 images -> fp16 [npix, out_channels] (zero-padded; test_real_refinement.py:108);
 * vgg_preprocess: x*255, RGB->BGR, minus mean of hallucination_net.py:149-153 on the single source */
int shdr_pack3_f16(const float* s0, const float* s1, const float* s2, const float* s3, int nsrc, void* y, int out_channels,
                   int64_t npix, int vgg_preprocess, void* stream);
/* its backward: the first nout 3-channel slices of fp16 y [npix, channels] -> fp32 images */
int shdr_unpack3_f16(const void* y, float* o0, float* o1, float* o2, float* o3, int nout, int channels, int64_t npix,
                     int vgg_preprocess_bwd, void* stream);
/* dz = dy * act'(y) (skipped for act NONE), db[c] += sum_p dz[p][c] (skipped when db is NULL) */
int shdr_act_bwd_bias_f16(const void* dy, const void* y, void* dz, float* db, float* ws, int64_t npix, int C, int act, void* stream);
/* y = a + b, optionally relu (residual joins of linearization_net.py:45-47,80-82; gradient accumulation at fan-out points) */
int shdr_add_f16(const void* a, const void* b, void* y, int64_t n, int relu, void* stream);
int shdr_avgpool2_fwd_f16(const void* x, void* y, int N, int H, int W, int C, void* stream);
int shdr_avgpool2_bwd_f16(const void* dy, void* dx, int N, int H, int W, int C, void* stream);
int shdr_maxpool2_fwd_f16(const void* x, void* y, int N, int H, int W, int C, void* stream);
int shdr_maxpool2_bwd_f16(const void* x, const void* dy, void* dx, int N, int H, int W, int C, void* stream);
int shdr_maxpool3s2_fwd_f16(const void* x, void* y, int N, int H, int W, int C, void* stream);
int shdr_maxpool3s2_bwd_f16(const void* x, const void* y, const void* dy, void* dx, int N, int H, int W, int C, void* stream);
int shdr_resize2x_fwd_f16(const void* x, void* y, int N, int H, int W, int C, void* stream);
int shdr_resize2x_bwd_f16(const void* dy, void* dx, int N, int H, int W, int C, void* stream);
int shdr_upsample_zero2_f16(const void* dy, void* dx, int N, int H, int W, int C, void* stream);
/* tf.reduce_mean(x,[1,2]): fp16 [N,HW,C] -> fp32 [N,C], and its backward (fp32 dy -> fp16 dx) */
int shdr_gap_fwd_f16(const void* x, float* y, int N, int HW, int C, void* stream);
int shdr_gap_bwd_f16(const float* dy, void* dx, int N, int HW, int C, void* stream);
/* training-mode BatchNormalization on fp16 tensors; statistics, parameters and their gradients fp32 (sums in double);
 * ws: shdr_workspace_bytes(SHDR_OP_BATCHNORM, NULL, C) bytes */
int shdr_bn_stats_f16(const void* x, double* ws, float* mean, float* var, float* moving_mean, float* moving_var, int64_t npix, int C,
                      float momentum, void* stream);
int shdr_bn_train_apply_f16(const void* x, const float* mean, const float* var, const float* gamma, const float* beta, void* y,
                            int64_t npix, int C, float eps, int relu, void* stream);
int shdr_bn_bwd_f16(const void* dy, const void* x, const void* y_relu, const float* mean, const float* var, const float* gamma,
                    double* ws, float* dgamma, float* dbeta, void* dx, int64_t npix, int C, float eps, void* stream);
/* Linearization-Net front end (linearization_net.py:310-322) fp32 image -> fp16 [N,H,W,y_channels >= 93], and its backward */
int shdr_lin_frontend_fwd_f16(const float* img, void* y, int N, int H, int W, int y_channels, void* stream);
int shdr_lin_frontend_bwd_f16(const float* img, const void* dF, float* dimg, int N, int H, int W, int y_channels, void* stream);

/* ---- validation metrics (csrc/metrics.hip): PSNR-L, PSNR-mu, SSIM-mu and the fine-tuning loss of an HDR estimate against its
 *      ground truth, per image, on the device.  pred, gt: fp32 [N,H,W,3], H >= 11 and W >= 11 (one 11x11 SSIM window).  With
 *        s_p, s_g = float32(0.5 / (1e-6 + mean(image)))  (normalise != 0: the mean normalisation of finetune_real_dataset.py:47,173)
 *                   or 1 (normalise == 0),
 *        p = max(s_p * pred, 0),  g = max(s_g * gt, 0),  peak = max(g),
 *        T(x) = log(1 + mu * min(x / peak, 1)) / log(1 + mu),  logc(x) = log(1 + 10 x) / log(11)
 *      the outputs are, per image and in float64,
 *        mse_l = mean((p - g)^2) / peak^2,  mse_mu = mean((T(p) - T(g))^2),  l1_logc = mean|logc(p) - logc(g)|,
 *        ssim_mu = SSIM (Wang et al. 2004) of T(p) against T(g) per channel: 11x11 Gaussian window of sigma 1.5 with weights summing
 *                  to 1, the (H-10)(W-10) valid windows only, weighted population variances, C1 = 1e-4, C2 = 9e-4, mean over
 *                  windows and channels.
 *      peak == 0 (an all-black gt) is not special-cased: the results are the IEEE ones -- mse_l = inf (NaN for a black pred),
 *      mse_mu = ssim_mu = NaN (T(0 / 0) is NaN: the min passes it on), l1_logc finite.
 *      Every reduction has two stages: a grid that depends on the shape alone writes float64 partial sums into `workspace`
 *      (shdr_metrics_workspace_bytes(N, H, W) bytes, owned by the caller, 8-byte aligned), one block per image adds them in a fixed
 *      order.  No floating-point atomics: the same inputs give the same bits.  NULL pointer -> SHDR_E_NULL; H < 11, W < 11 or
 *      N <= 0 -> SHDR_E_SHAPE.  Asynchronous on `stream`, nothing is allocated. ---- */
int64_t shdr_metrics_workspace_bytes(int N, int H, int W);
/* scale_pred[n], scale_gt[n] (the float32 values s_p, s_g, stored as float64) and peak[n] = max(g) (exact: the product of two
 * float32 numbers in float64) */
int shdr_pair_moments_f32(const float* pred, const float* gt, int N, int H, int W, int normalise, double* scale_pred,
                          double* scale_gt, double* peak, void* workspace, void* stream);
/* the four metrics, from the scales and peaks of shdr_pair_moments_f32 (device arrays [N]).  One block per tile of
 * SHDR_METRICS_TILE_H x SHDR_METRICS_TILE_W windows. */
#define SHDR_METRICS_TILE_H 16
#define SHDR_METRICS_TILE_W 32
int shdr_hdr_metrics_f32(const float* pred, const float* gt, int N, int H, int W, float mu, const double* scale_pred,
                         const double* scale_gt, const double* peak, double* mse_l, double* mse_mu, double* l1_logc,
                         double* ssim_mu, void* workspace, void* stream);
/* 8-bit preview: y = round(255 * T(max(scale[n] * x, 0))^(1/2.2)) with peak[n] in T; scale == NULL -> 1.  uint8 [N,H,W,3];
 * reverse_channels != 0 reads the pixel as BGR (as shdr_rgbe_encode_f32). */
int shdr_tonemap_u8_f32(const float* x, const double* scale, const double* peak, uint8_t* y, int N, int H, int W, float mu,
                        int reverse_channels, void* stream);

/* ---- baseline-JPEG file decoder (csrc/jpeg.hip): a BATCH of files of different sizes, layouts and tables -> quantised
 *      coefficients and uint8 RGB, bit for bit libjpeg's default decode (islow IDCT, fancy upsampling).  The host parses the
 *      markers, removes the FF 00 stuffing and cuts the scan at its RSTn markers (jpeg.py); the device decodes the Huffman stream
 *      with the self-synchronising scheme of Weissenberger & Schmidt (2018): every restart segment is cut into subsequences of
 *      `subseq_bits` bits, one thread each, 256 per workgroup; a workgroup lies inside ONE image.
 *
 *      data       device bytes: the unstuffed segments, each starting on a 4-byte boundary (padding content is irrelevant)
 *      tables     device bytes: per image SHDR_JPEG_TABLE_BYTES at image.table_off (a multiple of 4): four quantisation tables
 *                 (64 uint16 each, natural order), then four Huffman tables of SHDR_JPEG_HUFF_BYTES: uint16 look[512] (the next
 *                 9 bits -> code length << 8 | symbol, 0 when the code is longer), int32 maxcode[17] (largest code of length l,
 *                 -1: none), int32 valoff[17] (index of the first symbol of length l minus its first code), uint8 symbols[256]
 *      images     one shdr_jpeg_image per file; segs: SHDR_JPEG_SEG_FIELDS int32 per restart segment; sub_seg: per subsequence
 *                 slot its segment, or -1 for the unused slots at the end of an image's last workgroup.  Each table is passed as
 *                 a host array, which is validated, and as the device copy of that very array, which the kernels read.
 *      coef       device int16 [n_blocks][64], natural order, DC prediction undone; an image's blocks start at image.blk_off,
 *                 component c at comp[c].blk_off, raster order over its bw x bh blocks
 *      out        device uint8: image i is [height, width, 3] RGB at image.out_off (grey: R = G = B)
 *      errors     device int32 [n_images]: 0 or the SHDR_JPEG_E_* of the first subsequence of the image that failed; such an image's
 *                 coefficients and pixels are unspecified, other images are not affected
 *      workspace  shdr_jpeg_workspace_bytes(n_sub, n_blocks, plane_bytes) bytes, 16-byte aligned, owned by the caller
 *      Whatever the bytes of `data`, no read leaves a segment and no write leaves an image's blocks.  No atomics: the same input
 *      gives the same bits.  The calls wait on `stream` once per synchronisation pass after the first two (a pass flag comes back
 *      to the host); they allocate nothing.  The number of launches is 9 (11 with pixels) plus one per pass. ---- */
#define SHDR_JPEG_HUFF_BYTES 1416
#define SHDR_JPEG_TABLE_BYTES (512 + 4 * SHDR_JPEG_HUFF_BYTES)
#define SHDR_JPEG_E_CODE 1      /* a bit pattern that is no code word of the table, or a decoder state that cannot occur */
#define SHDR_JPEG_E_BITS 2      /* the segment ends before its blocks are complete */
#define SHDR_JPEG_E_OVERRUN 3   /* a run of zeros leaves the block */
typedef struct shdr_jpeg_component {
  int32_t h, v;                 /* sampling factors: luma 1x1, 2x1 or 2x2, chroma 1x1 (a grey image: 1x1); anything else is refused */
  int32_t tq, dc_slot, ac_slot; /* its quantisation table and Huffman tables (0..3) in the image's table block */
  int32_t bw, bh;               /* blocks per row / column of the padded plane: mcus_x * h, mcus_y * v */
  int32_t blk_off;              /* first block, relative to image.blk_off: the blocks of the components before it */
  int32_t plane_off;            /* its plane in the workspace, relative to image.plane_off: 64 bytes per block before it */
  int32_t cw, ch;               /* libjpeg's downsampled size: ceil(width * h / hmax), ceil(height * v / vmax) */
} shdr_jpeg_component;
typedef struct shdr_jpeg_image {
  int64_t blk_off;              /* first block of the image in `coef` (strictly increasing over the images) */
  int64_t plane_off;            /* first byte of its component planes (in total 64 bytes per block) */
  int64_t out_off;              /* first byte of its pixels in `out` */
  int64_t table_off;            /* first byte of its tables in `tables` */
  int32_t width, height, ncomp; /* ncomp: 1 or 3 */
  int32_t mcus_x, mcus_y, blocks_per_mcu, restart_interval;       /* restart_interval in MCUs, 0: none */
  int32_t first_wg, n_wg;       /* its workgroups: subsequence slots first_wg * 256 .. (first_wg + n_wg) * 256 */
  int32_t reserved, reserved2;
  shdr_jpeg_component comp[3];
} shdr_jpeg_image;
#define SHDR_JPEG_SEG_FIELDS 6
#define SHDR_JPEG_SEG_DWORD 0        /* offset of the segment in `data`, in 4-byte units */
#define SHDR_JPEG_SEG_BITS 1         /* its length in bits (the unstuffed bytes * 8) */
#define SHDR_JPEG_SEG_FIRST_SUB 2    /* its first subsequence slot; it has max(1, ceil(bits / subseq_bits)) consecutive ones */
#define SHDR_JPEG_SEG_FIRST_BLOCK 3  /* its first block in the image's scan order (MCU by MCU, component by component) */
#define SHDR_JPEG_SEG_BLOCKS 4       /* the blocks it must hold */
#define SHDR_JPEG_SEG_IMAGE 5
#define SHDR_JPEG_STAGES 6
typedef struct shdr_jpeg_batch {
  const uint8_t* data;
  const uint8_t* tables;
  const shdr_jpeg_image* images;     /* host */
  const shdr_jpeg_image* images_dev;
  const int32_t* segs;               /* host */
  const int32_t* segs_dev;
  const int32_t* sub_seg;            /* host */
  const int32_t* sub_seg_dev;
  int32_t* passes;                   /* host, may be NULL: receives the number of synchronisation passes launched */
  float* stage_ms;                   /* host, may be NULL: receives SHDR_JPEG_STAGES device-event times in ms (the call then
                                      * waits for its last kernel): clearing the workspace, the synchronisation passes (with the
                                      * host's waits between them), block scan + write pass, DC scan + DC, IDCT, upsample + colour;
                                      * the last two are 0 from shdr_jpeg_entropy_decode */
  int64_t data_bytes, table_bytes, n_sub, n_blocks, plane_bytes, out_bytes;
  int32_t n_images, n_segs, subseq_bits, reserved;       /* subseq_bits: 256, 512, 1024 or 2048 */
} shdr_jpeg_batch;
int64_t shdr_jpeg_workspace_bytes(int64_t n_sub, int64_t n_blocks, int64_t plane_bytes);      /* -1 on bad sizes */
int shdr_jpeg_entropy_decode(const shdr_jpeg_batch* batch, int16_t* coef, int32_t* errors, void* workspace, void* stream);
int shdr_jpeg_decode_u8(const shdr_jpeg_batch* batch, int16_t* coef, uint8_t* out, int32_t* errors, void* workspace, void* stream);
/* measurement: per subsequence slot the round (pass * 258 + iteration inside the workgroup; 0: never) in which its end state last
 * changed during the decode that last used `workspace`, copied to the host array rounds [n_sub]; waits on `stream` */
int shdr_jpeg_sync_rounds(const void* workspace, int64_t n_sub, int64_t n_blocks, int64_t plane_bytes, int32_t* rounds, void* stream);

/* ---- the `data` arena of shdr_jpeg_batch built on the device (csrc/jpeg_scan.hip; the rules are csrc/jpeg_scan.h, shared with the
 *      host twin): a BATCH of scan regions, each the bytes of a file from the first byte after its SOS header to the end of the file.
 *      In a region b[0 .. n) a marker is FF followed by a byte that is not 00, not FF and not D0 .. D7; `end` is the first marker.
 *      Before `end`, FF D0 .. D7 is a restart marker (neither byte is kept, a new segment starts after it), a 00 after FF is dropped,
 *      FF FF sets the fill flag, every other byte is kept; nothing at or after `end` counts.
 *
 *      src        device bytes, 16-byte aligned: the regions, each at image.offset (a multiple of 16); fewer than 2^33 bytes
 *      images     one shdr_jpeg_scan_image per region, as a host array, which is validated, and as the device copy of that very
 *                 array, which the kernels read
 *      report     device, one shdr_jpeg_scan_report per region
 *      bounds     device int64 [n_bounds]: slot image.first_bound + k receives the number of kept bytes before restart marker k,
 *                 for k < seg_cap - 1; slots that no marker fills hold -1, markers beyond the slots are counted in n_rst only
 *      workspace  shdr_jpeg_scan_workspace_bytes(n_images, n_tiles) bytes, 16-byte aligned, owned by the caller; n_tiles: the sum
 *                 of ceil(length / SHDR_JPEG_SCAN_TILE).  shdr_jpeg_compact reads what shdr_jpeg_scan left in it for the same batch.
 *      seg_dword  device int32: entry s * seg_stride is the SHDR_JPEG_SEG_DWORD of segment s (the `segs` table itself with
 *                 seg_stride = SHDR_JPEG_SEG_FIELDS will do); segment image.first_seg + s holds the kept bytes between boundaries
 *                 s - 1 and s of the image (everything after the last slot is in the last segment)
 *      arena      device bytes: filled with FF, then kept byte j of a segment goes to arena[seg_dword * 4 + (j - its boundary)];
 *                 a byte whose place is outside [0, arena_bytes) is not written
 *      Whatever the bytes of `src`, no read leaves a region and no write leaves report, the image's slots or the arena.  Both
 *      calls are asynchronous on `stream`, run no host work between their launches (7 and 1, plus a fill each) and allocate
 *      nothing; stage_ms, if not NULL, receives the device-event time of the call in ms (the call then waits for its last kernel).
 *      shdr_jpeg_scan_host is the same on host memory, byte by byte: report and bounds, and with seg_dword != NULL the arena. ---- */
#define SHDR_JPEG_SCAN_TILE 4096
typedef struct shdr_jpeg_scan_image {
  int64_t offset;               /* first byte of the region in `src`, a multiple of 16 */
  int64_t length;
  int64_t first_tile;           /* the tiles of the images before it */
  int32_t seg_cap;              /* the segments its header implies: ceil(MCUs / restart interval), or 1 */
  int32_t first_bound;          /* its first slot in `bounds`: the sum of seg_cap - 1 over the images before it */
  int32_t first_seg;            /* its first segment: the sum of seg_cap over the images before it */
  int32_t reserved;
} shdr_jpeg_scan_image;
typedef struct shdr_jpeg_scan_report {
  int64_t end;                  /* position of the end marker's FF in the region, -1: the region has none */
  int64_t kept;                 /* kept bytes */
  int32_t n_rst;                /* restart markers before `end` */
  int32_t fill;                 /* 1: FF FF before `end` */
  int32_t end_marker;           /* the byte after that FF (D9: EOI), -1 without an end */
  int32_t reserved;
} shdr_jpeg_scan_report;
int64_t shdr_jpeg_scan_workspace_bytes(int n_images, int64_t n_tiles);                       /* -1 on bad sizes */
int shdr_jpeg_scan(const uint8_t* src, int64_t src_bytes, const shdr_jpeg_scan_image* images, const shdr_jpeg_scan_image* images_dev,
                   int n_images, shdr_jpeg_scan_report* report, int64_t* bounds, int64_t n_bounds, void* workspace, void* stream,
                   float* stage_ms);
int shdr_jpeg_compact(const uint8_t* src, int64_t src_bytes, const shdr_jpeg_scan_image* images, const shdr_jpeg_scan_image* images_dev,
                      int n_images, const int64_t* bounds, int64_t n_bounds, const int32_t* seg_dword, int seg_stride, int64_t n_segs,
                      uint8_t* arena, int64_t arena_bytes, const void* workspace, void* stream, float* stage_ms);
int shdr_jpeg_scan_host(const uint8_t* src, int64_t src_bytes, const shdr_jpeg_scan_image* images, int n_images,
                        shdr_jpeg_scan_report* report, int64_t* bounds, int64_t n_bounds, const int32_t* seg_dword, int seg_stride,
                        int64_t n_segs, uint8_t* arena, int64_t arena_bytes);

/* ---- baseline-JPEG writer (csrc/jpeg_enc.hip; the rules are csrc/jpeg_enc.h, shared with the host twin in csrc/api.cpp) ----
 * Files as libjpeg writes them for 8-bit RGB pixels: JFIF YCbCr, 4:4:4 / 4:2:2 / 4:2:0, the Annex-K quantisation tables scaled by
 * the IJG quality rule (clamped to 1 .. 255), the islow integer DCT, the four Annex-K Huffman tables, an optional restart interval --
 * byte for byte what PIL's Image.save(f, "JPEG", quality=, subsampling=, restart_marker_blocks=) writes.  No grey or CMYK images,
 * no optimised tables, no progressive or arithmetic coding, no EXIF / ICC / comment segments, no 4:4:0.
 *
 * An image is described by a shdr_jpeg_enc_image.  Its coefficient arena is int16 [blocks][64]: MCU after MCU in scan order, in an MCU
 * the h*v Y blocks row-major, then Cb, then Cr, every block in zig-zag order with the DC as a value (not a difference), the dummy
 * blocks of partial MCUs included.
 *
 * Host twin, two stages that can be called on their own (host memory; the negative SHDR_E_* code on failure, see shdr_last_error):
 *      shdr_jpeg_encode_blocks          the blocks of an image; *out_bytes (may be NULL): an upper bound of its file
 *      shdr_jpeg_encode_header_host     the bytes from SOI to the end of the SOS header into out [SHDR_JPEG_ENC_HEADER_MAX]; their count
 *      shdr_jpeg_encode_transform_host  rgb uint8 [H][W][3] -> the arena (coef_blocks: its room, in blocks); the blocks written
 *      shdr_jpeg_encode_entropy_host    the arena (coef_blocks: exactly the image's) -> the entropy-coded scan: the stuffed restart
 *                                       segments with the RSTn markers between them, neither header nor EOI; the bytes written.  A
 *                                       coefficient outside the baseline range (an AC of category > 10, a DC difference of category
 *                                       > 11) fails with a message that names the block.  Nothing is written at or past out + capacity:
 *                                       a scan that does not fit fails
 *      shdr_jpeg_encode_host            both stages and the header: the complete file
 *
 * Device, a BATCH of images of different sizes, layouts, qualities and restart intervals in one call:
 *      pixels      device: the images' [H][W][3] pixels back to back, uint8 (SHDR_JPEG_ENC_U8) or float32 in [0, 1]
 *                  (SHDR_JPEG_ENC_F32, quantised as shdr_jpeg_round_trip_f32 does: rintf(x * 255), clamped)
 *      images      one descriptor per image, as a host array, which is validated, and as the device copy of that very array
 *                  (images_dev), which the kernels read
 *      headers     [n_images][SHDR_JPEG_ENC_HEADER_MAX]: what shdr_jpeg_encode_header_host composes for every image, as a host array,
 *                  which is validated, and as its device copy (headers_dev)
 *      out         device bytes, 4-byte aligned: the files back to back; out_capacity must be at least the out_bytes of
 *                  shdr_jpeg_encode_batch_sizes
 *      offsets     device int64 [n_images + 1]: file i is out[offsets[i] .. offsets[i + 1])
 *      status      device int32 [n_images]: 0, or SHDR_JPEG_ENC_OUT_OF_RANGE for an image with a coefficient outside the baseline range;
 *                  the bytes of such an image are unspecified and its offset range is empty
 *      workspace   workspace_bytes of shdr_jpeg_encode_batch_sizes, 16-byte aligned, owned by the caller
 *      stage_ms    NULL, or [SHDR_JPEG_ENC_STAGES] device-event times: transform, bits per block, scan + segments, bit stream,
 *                  FF count + scan, sizes + scan, final copy (measurement only: the call then waits)
 * shdr_jpeg_encode_entropy_batch takes the images' coefficient arenas back to back (16-byte aligned, coef_blocks: the sum of their
 * blocks) instead of pixels and writes what shdr_jpeg_encode_entropy_host writes: scans without header and EOI (quality is not used).
 * Stream-ordered launches, no global atomics -- the same input gives the same bytes -- no host wait and no allocation.  Arguments are
 * checked before anything is launched. */
#define SHDR_JPEG_ENC_HEADER_MAX 640
#define SHDR_JPEG_ENC_STAGES 7
#define SHDR_JPEG_ENC_OUT_OF_RANGE 1
#define SHDR_JPEG_ENC_U8 0
#define SHDR_JPEG_ENC_F32 1
typedef struct shdr_jpeg_enc_image {
  int32_t height, width;
  int32_t layout;                             /* 0: 4:4:4, 1: 4:2:2, 2: 4:2:0 */
  int32_t quality;                            /* 1 .. 100 */
  int32_t restart;                            /* MCUs per restart segment, 0 .. 65535; 0: none */
  int32_t reserved;
} shdr_jpeg_enc_image;
int64_t shdr_jpeg_encode_blocks(const shdr_jpeg_enc_image* image, int64_t* out_bytes);
int shdr_jpeg_encode_header_host(const shdr_jpeg_enc_image* image, uint8_t* out);
int64_t shdr_jpeg_encode_transform_host(const uint8_t* rgb, const shdr_jpeg_enc_image* image, int16_t* coef, int64_t coef_blocks);
int64_t shdr_jpeg_encode_entropy_host(const int16_t* coef, int64_t coef_blocks, const shdr_jpeg_enc_image* image, uint8_t* out,
                                      int64_t capacity);
int64_t shdr_jpeg_encode_host(const uint8_t* rgb, const shdr_jpeg_enc_image* image, uint8_t* out, int64_t capacity);
int shdr_jpeg_encode_batch_sizes(const shdr_jpeg_enc_image* images, int n_images, int64_t* out_bytes, int64_t* n_blocks,
                                 int64_t* workspace_bytes);
int shdr_jpeg_encode_batch(const void* pixels, int pixel_type, const shdr_jpeg_enc_image* images, const shdr_jpeg_enc_image* images_dev,
                           const uint8_t* headers, const uint8_t* headers_dev, int n_images, uint8_t* out, int64_t out_capacity,
                           int64_t* offsets, int32_t* status, void* workspace, void* stream, float* stage_ms);
int shdr_jpeg_encode_entropy_batch(const int16_t* coef, int64_t coef_blocks, const shdr_jpeg_enc_image* images,
                                   const shdr_jpeg_enc_image* images_dev, int n_images, uint8_t* out, int64_t out_capacity,
                                   int64_t* offsets, int32_t* status, void* workspace, void* stream, float* stage_ms);

/* ---- PNG writer (csrc/png_enc.hip; the rules are csrc/png.h, shared with the host twin) -----------------------------------------
 * Lossless 8-bit files: bit depth 8, no interlace, C = 1 grey (colour type 0), C = 3 RGB (2), C = 4 RGBA (6); H >= 1, W >= 1 and
 * H (W C + 1) < 2^31.  No 16-bit samples, no palettes, no ancillary chunks.  A scanline is filtered with one of PNG's five predictors,
 * the same for every row (SHDR_PNG_FILTER_NONE .. _PAETH) or per row the one whose filtered bytes, read as signed, have the smallest
 * sum of absolute values, the lowest number on a tie (_ADAPTIVE).  The filtered stream is cut every SHDR_PNG_SEGMENT bytes into
 * segments that are deflated on their own -- by the Huffman-only encoder or the one with LZ77 matches (shdr_deflate_*) -- and joined
 * into ONE zlib stream as Z_SYNC_FLUSH joins them: an empty stored block behind every segment but the last, BFINAL in the last, a
 * stored block wherever the coded segment would not be strictly fewer than n + 5 bytes, the Adler-32 of the whole stream at the end.
 * One IDAT per segment.  Any PNG reader opens the files; they are larger than zlib level 6 makes them.
 *
 * Host (host memory; a negative SHDR_E_* code on failure, see shdr_last_error):
 *      shdr_crc32            CRC-32 (IEEE, reflected 0xEDB88320: zlib's crc32) of n bytes, continuing from `crc` (0 to start)
 *      shdr_png_filter_host  pixels uint8 [H][W][C] -> the filtered stream, H (W C + 1) bytes; returns that count
 *      shdr_png_encode_host  the twin: pixels -> the complete file; returns its length.  A capacity of exactly that length suffices;
 *                            with less, nothing is written.  shdr_png_encode_batch_sizes of the one image gives an upper bound
 *
 * Device, a BATCH of images of different sizes and channel counts in one call:
 *      pixels      device uint8: the images' [H][W][C] pixels back to back (pixel_bytes of shdr_png_encode_batch_sizes)
 *      images      int32 [n_images][4]: H, W, C, 0 -- as a host array, which is validated, and as the device copy of that very
 *                  array (images_dev), which the kernels read
 *      out         device bytes: the files back to back; out_capacity must be at least the out_bytes of
 *                  shdr_png_encode_batch_sizes (every segment stored)
 *      offsets     device int64 [n_images + 1]: file i is out[offsets[i] .. offsets[i + 1])
 *      workspace   workspace_bytes of shdr_png_encode_batch_sizes (for the same `deflate`), 16-byte aligned, owned by the caller: the
 *                  filtered streams, the segment tables and the encoder's workspace (with _LZ 4 bytes per filtered byte)
 *      stage_ms    NULL, or [SHDR_PNG_STAGES] device-event times: tables + filter, the encoder's three launches (sizes and
 *                  checksums, scan, blocks), framing + CRC (measurement only: the call then waits)
 * Stream-ordered launches, no global atomics -- the same input gives the same bytes -- no host wait and no allocation.  Arguments are
 * checked before anything is launched. */
#define SHDR_PNG_SEGMENT 65520
#define SHDR_PNG_STAGES 5
#define SHDR_PNG_FILTER_NONE 0
#define SHDR_PNG_FILTER_SUB 1
#define SHDR_PNG_FILTER_UP 2
#define SHDR_PNG_FILTER_AVERAGE 3
#define SHDR_PNG_FILTER_PAETH 4
#define SHDR_PNG_FILTER_ADAPTIVE 5
#define SHDR_PNG_DEFLATE_HUFFMAN 0
#define SHDR_PNG_DEFLATE_LZ 1
uint32_t shdr_crc32(const void* data, uint64_t n, uint32_t crc);
int64_t shdr_png_filter_host(const uint8_t* pixels, int h, int w, int c, int filter, uint8_t* out, int64_t capacity);
int64_t shdr_png_encode_host(const uint8_t* pixels, int h, int w, int c, int filter, int deflate, uint8_t* out, int64_t capacity);
int shdr_png_encode_batch_sizes(const int32_t* images, int n_images, int deflate, int64_t* pixel_bytes, int64_t* out_bytes,
                                int64_t* n_segments, int64_t* workspace_bytes);
int shdr_png_encode_batch(const uint8_t* pixels, const int32_t* images, const int32_t* images_dev, int n_images, int filter, int deflate,
                          uint8_t* out, int64_t out_capacity, int64_t* offsets, void* workspace, void* stream, float* stage_ms);

/* ---- gain maps (csrc/gainmap.hip; the rules are csrc/gainmap.h, shared with the host twins) ----------------------------------------
 * The arithmetic of Ultra HDR v1 / Adobe hdrgm gain-map files, in both directions (the container is ultrahdr.py).  ENCODE: an SDR image
 * uint8 [H][W][3] RGB and an HDR image float32 [H][W][3] (reverse_channels: its channel 2 is red) -> a map uint8 [h][w][3] with
 * h = ceil(H / f), w = ceil(W / f), f in {1, 2, 4, 8}, and one shdr_gainmap_meta.  Per channel a cell holds
 * g = log2((mean of s hdr + 1/64) / (mean of sRGB-linear sdr + 1/64)) clamped to [lo, hi], coded as rint(255 (g - min) / (max - min)),
 * min and max those of the image (max at least min + 2^-10).  HDR values are sanitised first (NaN, negatives -> 0, +inf -> FLT_MAX).
 * s is scales[i], or with scales NULL the exposure alignment exp2(mean log2 Y_sdr - mean log2 max(Y_hdr, 2^-20)) over the pixels whose
 * SDR bytes all lie in [16, 239] (count of them in the meta record; none: s = 1), summed in float64 in a fixed tree.  log2 and exp2
 * are polynomials of the header, so the device bits are the host twin's bits.  APPLY: out = max((lin(sdr) + offset_sdr) exp2(L weight)
 * - offset_hdr, 0), L = min (1 - r) + max r, r the map (1 or 3 channels) sampled bilinearly at (x + 0.5) / f - 0.5, through
 * exp2(log2(r) / gamma) when gamma != 1.
 *
 * Both directions take a BATCH of images of different sizes out of flat arenas (sdr uint8 [arena_pixels][3], hdr / out float32
 * [arena_pixels][3], image i starting at pixel pix_off) through one descriptor table: a host array, which is validated before anything
 * is launched (an image that leaves its arena, a factor outside the set, an empty image and derived fields that are not what the
 * *_sizes call writes are refused), and the device copy of that very array, which the kernels read.
 *      shdr_gainmap_encode_sizes  fills the derived fields of the descriptors; the bytes of all maps back to back (image i's map
 *                                 starts at byte 3 cell_off) and of the workspace
 *      shdr_gainmap_encode        three stream-ordered launches: alignment statistics (with scales given: only the clearing of the
 *                                 min / max slots), cells (g as fp32 into the workspace, min / max by integer atomics on ordered bits),
 *                                 quantise (maps and meta records).  maps: map_capacity bytes, meta: meta_capacity records, both on the
 *                                 device; workspace 16-byte aligned, owned by the caller; stage_ms NULL or [SHDR_GAINMAP_STAGES]
 *      shdr_gainmap_encode_host   the twin, host memory: the same bits
 *      shdr_gainmap_apply_sizes   fills block0 of the descriptors; the launch's blocks
 *      shdr_gainmap_apply         one launch; out: out_capacity PIXELS, image i at pixel pix_off as in the sdr arena
 *      shdr_gainmap_apply_host    the twin
 *      shdr_gainmap_math_host     y[i] = log2 (op 0) or exp2 (op 1) of x[i] by the header's polynomials; op 2: y[0 .. n) = the sRGB table (n <= 256)
 * A destination smaller than needed is refused and nothing is written.  No host wait, no allocation on the device routes. */
#define SHDR_GAINMAP_CELLS_PER_BLOCK 1024
#define SHDR_GAINMAP_PIXELS_PER_BLOCK 1024
#define SHDR_GAINMAP_STAGES 3
typedef struct shdr_gainmap_image {
  int64_t pix_off;                            /* first pixel of the image in both arenas */
  int64_t cell_off;                           /* derived: map cells of the images before this one */
  int32_t height, width;                      /* 1 .. 65535 */
  int32_t factor;                             /* 1, 2, 4 or 8 */
  int32_t stat_block0, cell_block0;           /* derived: the image's first block of the statistics and of the cell launch */
  int32_t reserved;
} shdr_gainmap_image;
typedef struct shdr_gainmap_meta {
  float gain_min, gain_max;                   /* GainMapMin, GainMapMax (log2) */
  float scale;                                /* s */
  int32_t reserved;
  int64_t count;                              /* pixels that took part in the alignment; 0 with scales given */
} shdr_gainmap_meta;
typedef struct shdr_gainmap_apply_image {
  int64_t pix_off;                            /* first pixel in the sdr arena and in out */
  int64_t map_off;                            /* first byte of the map */
  int32_t height, width, map_height, map_width;
  int32_t factor;                             /* 1 .. 64; map_height = ceil(height / factor), map_width likewise */
  int32_t map_channels;                       /* 1 or 3 */
  float gain_min, gain_max, gamma, offset_sdr, offset_hdr, weight;
  int32_t block0;                             /* derived: the image's first block */
  int32_t reserved;
} shdr_gainmap_apply_image;
int shdr_gainmap_math_host(int op, const float* x, int64_t n, float* y);
int shdr_gainmap_encode_sizes(shdr_gainmap_image* images, int n_images, int64_t* map_bytes, int64_t* workspace_bytes);
int shdr_gainmap_encode_host(const uint8_t* sdr, const float* hdr, int64_t arena_pixels, const shdr_gainmap_image* images, int n_images,
                             const float* scales, float lo, float hi, int reverse_channels, uint8_t* maps, int64_t map_capacity,
                             shdr_gainmap_meta* meta, int64_t meta_capacity);
int shdr_gainmap_encode(const uint8_t* sdr, const float* hdr, int64_t arena_pixels, const shdr_gainmap_image* images,
                        const shdr_gainmap_image* images_dev, int n_images, const float* scales, const float* scales_dev, float lo, float hi,
                        int reverse_channels, uint8_t* maps, int64_t map_capacity, shdr_gainmap_meta* meta, int64_t meta_capacity,
                        void* workspace, void* stream, float* stage_ms);
int shdr_gainmap_apply_sizes(shdr_gainmap_apply_image* images, int n_images, int64_t* n_blocks);
int shdr_gainmap_apply_host(const uint8_t* sdr, int64_t arena_pixels, const uint8_t* maps, int64_t map_bytes,
                            const shdr_gainmap_apply_image* images, int n_images, float* out, int64_t out_capacity);
int shdr_gainmap_apply(const uint8_t* sdr, int64_t arena_pixels, const uint8_t* maps, int64_t map_bytes,
                       const shdr_gainmap_apply_image* images, const shdr_gainmap_apply_image* images_dev, int n_images, float* out,
                       int64_t out_capacity, void* stream);

/* ---- Deterministic mode: bit-reproducible forms of the fp32 training reductions -----------------------------------------------------------
 * The default weight-gradient, bias-gradient, CRF-head and loss kernels end in floating-point atomics: several blocks add partial sums to
 * the same address, in the order in which they happen to arrive, and two runs of one call differ in the last bits.  Each entry point
 * below computes the same quantity as its namesake without the _det, with the same arguments plus a workspace, and returns the same bits
 * for the same inputs on every run:
 *   - every block STORES its partial result to a slab / row of its own in the caller's workspace (the kernel's address arithmetic plus
 *     block * stride), and a second launch adds the slabs in block order, in double, and rounds once;
 *   - where the namesake accumulates (dw, db, dwfc, dbfc, drf, dgamma, dbeta) the fold computes the sum S without reading the output and
 *     then writes out = out + S, one thread per address and NO atomic: accumulating into g0 gives exactly g0 + (the result into zeros), and
 *     the caller must order the call against every other writer of that output (two streams may not accumulate into one range unordered);
 *   - the fold touches only what the call owns: shdr_conv2d_wgrad_det_f32 the rows [ci_off, ci_off + Cx) of every tap.
 * The library allocates nothing and waits for nothing; everything is ordered on `stream`.  A workspace belongs to ONE call until that call
 * has finished on its stream: concurrent calls on two streams need two workspaces.  Its size comes from shdr_det_workspace_bytes(op, d, n, c,
 * k); it needs no initialisation; pointers must be 16-byte aligned.  The pixel slices of the deterministic weight gradients depend on the
 * layer, not on the device (a constant 512 block slots, not the occupancy; SHDR_WGRAD_ROUNDS is ignored), so the query needs no GPU and the
 * bits are the same on every device.  The kernel-family switches SHDR_NO_ALLTAPS and SHDR_NO_WGRAD96 still pick the kernel and its tile, and
 * with them the slices: results are bit-identical from run to run under ONE setting of these two switches.
 *   op                              n                     c          k      call
 *   SHDR_DET_CONV2D_WGRAD           -                     which      -      shdr_conv2d_wgrad_det_f32 (d = the layer): slices x KH KW (C1+C2) Cout floats
 *   SHDR_DET_CONV2D_WGRAD_WINOGRAD  -                     which      -      shdr_conv2d_wgrad_winograd_det_f32 (d: N, H, W, C1 / C2, Cout): slices x 16 Cx Cout floats
 *   SHDR_DET_CONV2D_WGRAD_X3        -                     which      -      shdr_conv2d_wgrad_x3_det_f32 (d = the layer): slices x KH KW (C1+C2) Cout floats
 *   SHDR_DET_BIAS_GRAD              npix                  C          -      shdr_bias_grad_det_f32: one row of C floats per block
 *   SHDR_DET_ACT_BWD_BIAS           npix                  C          -      shdr_act_bwd_bias_det_f32 (never more than SHDR_OP_ACT_BWD_BIAS)
 *   SHDR_DET_BATCHNORM              npix                  C          -      shdr_bn_stats_det_f32, shdr_bn_bwd_ranged_det_f32 (never more than SHDR_OP_BATCHNORM)
 *   SHDR_DET_DIFF_LOSS              n_per_sample          B          -      shdr_diff_loss_det_f32
 *   SHDR_DET_TV_LOSS                N H W C               -          -      shdr_tv_loss_det_f32
 *   SHDR_DET_SAMPLE_DOT             n_per_sample          B          -      shdr_sample_dot_det_f32
 *   SHDR_DET_INVCRF_DECODE_BWD      -                     B          F      shdr_invcrf_decode_bwd_det_f32: B rows of (F + 1) x 11 floats
 *   SHDR_DET_APPLY_RF_BWD           n_per_batch           B          K      shdr_apply_rf_bwd_det_f32: one [B][K] slab per block column
 * shdr_conv2d_wgrad_det_f32 runs the exact-fp32 kernels of shdr_conv2d_wgrad_f32 (algo AUTO, AUTO_EXACT, MFMA or DIRECT; the reduced-precision
 * algos are refused).  shdr_conv2d_wgrad_winograd_det_f32 gives every unit slice its own slab of the dU scratch (16 x Cx x Cout), folds the
 * slabs into `du` (every element written: no memset) and runs the dU -> dW transform as before (one thread per address, no atomic).
 * shdr_conv2d_wgrad_x3_det_f32 is the slab form of the split-operand kernel.  A query answers -1 for a layer its family does not take.
 * shdr_apply_rf_bwd_det_f32 fills the block's LDS table without atomics (every bin has one owning thread,
 * which walks the staged pixels in order) and takes K <= 4096.  shdr_lin_frontend_bwd_det_f32 is the GATHER form of the front end's backward:
 * one thread per pixel sums the transposed REFLECT Sobel stencil in a fixed order and writes dimg once (no memset, no workspace).  The BatchNorm
 * _det entries differ from their namesakes only where C % 4 != 0 (the float4 reduction is deterministic already). */
enum { SHDR_DET_CONV2D_WGRAD = 0, SHDR_DET_BIAS_GRAD = 1, SHDR_DET_ACT_BWD_BIAS = 2, SHDR_DET_BATCHNORM = 3, SHDR_DET_DIFF_LOSS = 4,
       SHDR_DET_TV_LOSS = 5, SHDR_DET_SAMPLE_DOT = 6, SHDR_DET_INVCRF_DECODE_BWD = 7, SHDR_DET_APPLY_RF_BWD = 8,
       SHDR_DET_CONV2D_WGRAD_WINOGRAD = 9, SHDR_DET_CONV2D_WGRAD_X3 = 10 };
int64_t shdr_det_workspace_bytes(int op, const shdr_conv2d_desc* d, int64_t n, int c, int k);
int shdr_conv2d_wgrad_winograd_det_f32(const float* x, const float* dz, float* du, float* dw, void* ws, int64_t ws_bytes, int N, int H, int W,
                                       int Cx, int Cout, int Ct, int ci_off, float x_scale, void* stream);
int shdr_conv2d_wgrad_x3_det_f32(const shdr_conv2d_desc* d, const void* xh, const void* xl, int which, const void* zh, const void* zl,
                                 const float* x_range, const float* z_range, float* dw, void* ws, int64_t ws_bytes, void* stream);
int shdr_conv2d_wgrad_det_f32(const shdr_conv2d_desc* d, const float* x, int which, const float* dz, float* dw, void* ws, int64_t ws_bytes,
                              void* stream);
int shdr_bias_grad_det_f32(const float* dz, float* db, void* ws, int64_t ws_bytes, int64_t npix, int C, void* stream);
int shdr_act_bwd_bias_det_f32(const float* dy, const float* y, float* dz, float* db, float* ws, int64_t npix, int C, int act, void* stream);
int shdr_bn_stats_det_f32(const float* x, double* ws, float* mean, float* var, float* moving_mean, float* moving_var, int64_t npix, int C,
                          float momentum, void* stream);
int shdr_bn_bwd_ranged_det_f32(const float* dy, const float* x, const float* y_relu, const float* mean, const float* var, const float* gamma,
                               double* ws, float* dgamma, float* dbeta, float* dx, int64_t npix, int C, float eps, float* dx_range,
                               void* stream);
int shdr_invcrf_decode_bwd_det_f32(const float* dinv, const float* feat, const float* wfc, const float* table, float* dfeat, float* dwfc,
                                   float* dbfc, void* ws, int64_t ws_bytes, int B, int F, int K, void* stream);
int shdr_apply_rf_bwd_det_f32(const float* x, const float* rf, const float* dy, float* drf, float* dx, void* ws, int64_t ws_bytes, int B,
                              int64_t n_per_batch, int K, void* stream);
int shdr_diff_loss_det_f32(const float* a, const float* b, float* out, void* ws, int64_t ws_bytes, int B, int64_t n_per_sample, int mode,
                           void* stream);
int shdr_tv_loss_det_f32(const float* y, float* out, void* ws, int64_t ws_bytes, int N, int H, int W, int C, void* stream);
int shdr_sample_dot_det_f32(const float* a, const float* b, float* out, void* ws, int64_t ws_bytes, int B, int64_t n_per_sample, void* stream);
int shdr_lin_frontend_bwd_det_f32(const float* img, const float* dF, float* dimg, int N, int H, int W, int y_channels, void* stream);
/* Diagnostic: a process-wide count, kept on the host, of the launches whose RESULT depends on the order in which floating-point atomics
 * reach memory -- the default forms of the entry points above (fp32 and fp16) whenever more than one block, or one block's LDS atomics, add
 * to one address.  It does not move while a training step runs on the deterministic forms alone. */
int64_t shdr_order_dependent_launches(void);

#ifdef __cplusplus
}
#endif
#endif  /* SHDR_H_ */

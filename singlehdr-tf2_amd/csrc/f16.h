// What the native-fp16 MFMA kernels share (conv_f16.hip, conv_f16_patch.hip, conv_f16_w3.hip, wgrad_f16.hip, wgrad_f16_alltaps.hip; the
// transposed-read pieces also serve wgrad_x3.hip): the LDS swizzles, the argument and block-id conventions, the
// epilogues and the host-side checks.  The vector types, the zero page and the launch set-up are in shdr_internal.h.
// Every device function here is force-inlined into its callers and none asks which kernel called it.
#pragma once
#include <stddef.h>

#include <type_traits>

#include "shdr_internal.h"

// The fused inference forms of the two specialised forward kernels: shdr_conv2d_fwd_fused_f16 dispatches to them when their predicate
// takes every fused option of the call, the general kernel runs the layer otherwise.  Internal: include/shdr.h does not declare them.
extern "C" int shdr_conv2d_patch_fused_ok_f16(const shdr_conv2d_desc* d, int y_is_f32);
extern "C" int shdr_conv2d_fwd_patch_fused_f16(const shdr_conv2d_desc* d, const void* x1, const void* x2, const void* wp, const float* bias,
                                               const shdr::FusedEpiF16* f, void* y, void* stream);
extern "C" int shdr_conv2d_w3_fused_ok_f16(const shdr_conv2d_desc* d, int has_residual);
extern "C" int shdr_conv2d_fwd_w3_fused_f16(const shdr_conv2d_desc* d, const void* x1, const void* x2, const void* wp, const float* bias,
                                            const shdr::FusedEpiF16* f, void* y, void* stream);

namespace shdr {

// ---- LDS swizzles --------------------------------------------------------------------------------------------------------------------
// (row_swz, the slot swizzle of the images with 64-byte rows, is in shdr_internal.h: the split-operand kernels use it too)
// Pixel-major images read with ds_read_b64_tr_b16 (the weight gradients): the 32-byte channel windows of pixel row p, T channels wide,
// are XOR-ed with win_swz<T>(p) so that the 8 rows one half-wave reads hit 8 different bank groups (T = 16 stays 2-way).
template <int T>
__host__ __device__ constexpr int win_swz(int p) {
  return T >= 128 ? ((p & 3) | (((p >> 3) & 1) << 2)) : T == 64 ? (((p >> 1) & 1) | (((p >> 3) & 1) << 1)) : T == 32 ? ((p >> 3) & 1) : 0;
}
// two transposed reads are one MFMA operand
union Frag {
  sv4 h[2];
  f16x8 v;
};

// ---- kernel arguments ----------------------------------------------------------------------------------------------------------------
// The inference instantiations of a forward kernel take the fused epilogue behind the training arguments; the training ones keep Base.
template <class Base>
struct WithFusedEpi : Base {
  FusedEpiF16 f;
};
template <class Base, bool FUSED>
using FusedArgsT = std::conditional_t<FUSED, WithFusedEpi<Base>, Base>;
// The kernels' parameter layout is that of the hand-written Base / `struct ...FusedArgs : Base { FusedEpiF16 f; }` pairs this replaced:
// the sizes measured on those, f directly behind Base.
#define SHDR_F16_ARGS_LAYOUT(Base, base_bytes, fused_bytes)                                                             \
  _Pragma("clang diagnostic push") _Pragma("clang diagnostic ignored \"-Winvalid-offsetof\"")                           \
  static_assert(sizeof(Base) == base_bytes && sizeof(shdr::WithFusedEpi<Base>) == fused_bytes &&                        \
                    offsetof(shdr::WithFusedEpi<Base>, f) == base_bytes, "kernel argument layout changed");             \
  _Pragma("clang diagnostic pop")

// ---- block id -> tile ----------------------------------------------------------------------------------------------------------------
// hardware block id -> (cout block pn, pixel tile (tx, ty) of image img) of an nblk_m x nblk_n grid, tile columns fastest: XCD-aware, and
// the cout blocks of one pixel tile are neighbours
struct BlockTile {
  int pn, tx, ty, img;
};
__device__ __forceinline__ BlockTile block_tile_of(int bid, int nblk_m, int nblk_n, int tiles_x, int tiles_y) {
  const int L = xcd_remap(bid, nblk_m * nblk_n);
  const int pn = L % nblk_n;
  int pm = L / nblk_n;
  const int tx = pm % tiles_x;
  pm /= tiles_x;
  const int ty = pm % tiles_y;
  const int img = pm / tiles_y;
  return BlockTile{pn, tx, ty, img};
}

// ---- the fp16 output epilogue: fp32 -> fp16 through an LDS staging tile -> 16-byte row-contiguous stores -----------------------------------
// Staging tile: [rows][BN + 8] halves.  The +8 (16 bytes) keeps every row 16-byte aligned for the drain's b128 reads and moves consecutive
// rows 4 banks apart, so the 8-byte writes of the 16 pixels of a lane group do not all land on the same banks.
constexpr int f16_stage_stride(int BN) { return BN + 8; }
// One step: four consecutive couts n0 + cl .. + 3 of one pixel (n0 = the block's first cout) -- bias, act1, the fused epilogue of the
// FUSED instantiations, conversion, the write to the pixel's `row` of the staging tile.  `pix` / `res_ok`: the output pixel for the
// residual and whether it exists (a caller whose layers never carry a residual passes 0 / false and the read is compiled out).
// No tanh: the entries decline it on an fp16 output (the general kernel's training instantiations take it, with a step of their own).
template <bool FUSED, class Args>
__device__ __forceinline__ void f16_stage4(const Args& a, f32x4 v, int n0, int cl, size_t pix, bool res_ok, _Float16* row) {
  if (a.bias) {
    const float4 b4 = *reinterpret_cast<const float4*>(a.bias + n0 + cl);
    v[0] += b4.x; v[1] += b4.y; v[2] += b4.z; v[3] += b4.w;
  }
  act_apply4<0>(v, a.act1);
  if constexpr (FUSED) fused_epi4_f16<0>(v, n0 + cl, pix, 4, res_ok, a.f);
  f16x4 h;
#pragma unroll
  for (int e = 0; e < 4; ++e) h[e] = (_Float16)v[e];
  *reinterpret_cast<f16x4*>(row + cl) = h;
}
// The drain: the whole block, after the __syncthreads() that follows the last f16_stage4 of any of its waves (and the staging tile may
// overlay the pipeline buffers only after the barrier that ends their last read).  ROWS tile pixels (16 per tile row) x BN couts from
// cout n0, the tile's first pixel at (oh0, ow0) of image img; pixels outside Ho x Wo are skipped.
template <int ROWS, int BN>
__device__ __forceinline__ void f16_drain(const _Float16* stage, _Float16* y, int img, int oh0, int ow0, int Ho, int Wo, int Cout, int n0) {
  constexpr int RS = f16_stage_stride(BN), QR = BN / 8;        // 16-byte pieces per tile row
#pragma unroll 2
  for (int e = threadIdx.x; e < ROWS * QR; e += 256) {
    const int r = e / QR, q = e - r * QR;
    const int oh = oh0 + (r >> 4), ow = ow0 + (r & 15);
    if (oh >= Ho || ow >= Wo) continue;
    const size_t pix = ((size_t)img * Ho + oh) * Wo + ow;
    *reinterpret_cast<f16x8*>(y + pix * Cout + n0 + 8 * q) = *reinterpret_cast<const f16x8*>(stage + r * RS + 8 * q);
  }
}

// ---- host side -----------------------------------------------------------------------------------------------------------------------
// The pointer checks every forward entry makes, each at its own place among the entry's shape checks (a call with several faults reports
// the one it always reported): `who` is the entry's name in the messages.
struct F16FwdPointers {
  const char* who;
  const shdr_conv2d_desc* d;
  const void *x1, *x2, *wp;
  const float* bias;
  const void* y;
  int given() const {
    SHDR_REQUIRE(d && x1 && wp && y, SHDR_E_NULL, "%s: null desc/x1/wp/y", who);
    return SHDR_OK;
  }
  int x2_iff_c2() const {
    SHDR_REQUIRE((d->C2 == 0) == (x2 == nullptr), SHDR_E_NULL, "%s: x2 must be given iff C2 > 0", who);
    return SHDR_OK;
  }
  int aligned() const {
    SHDR_REQUIRE(aligned16(x1) && (!x2 || aligned16(x2)) && aligned16(wp) && aligned16(y) && (!bias || aligned16(bias)), SHDR_E_ALIGN,
                 "%s: tensors must be 16-byte aligned", who);
    return SHDR_OK;
  }
};
// ... and every weight-gradient entry (dw is the target of 4-byte atomics: no alignment asked)
struct F16WgradPointers {
  const char* who;
  const shdr_conv2d_desc* d;
  const void *x, *dz;
  const float* dw;
  int given() const {
    SHDR_REQUIRE(d && x && dz && dw, SHDR_E_NULL, "%s: null pointer", who);
    return SHDR_OK;
  }
  int aligned() const {
    SHDR_REQUIRE(aligned16(x) && aligned16(dz), SHDR_E_ALIGN, "%s: tensors must be 16-byte aligned", who);
    return SHDR_OK;
  }
};
// the fields both weight-gradient kernels take from the call: source `which` of the layer, the rows / columns of dW that exist
template <class Args>
inline void f16_wgrad_fill(Args& a, const shdr_conv2d_desc* d, const void* x, int which, const void* dz, int dz_channels, int c1_rows,
                           int c2_rows, float* dw) {
  a.x = reinterpret_cast<const _Float16*>(x);
  a.dz = reinterpret_cast<const _Float16*>(dz);
  a.dw = dw;
  a.N = d->N; a.H = d->H; a.W = d->W;
  a.Cx = which ? d->C2 : d->C1;                                // channels per pixel of x (possibly zero-padded)
  a.Cz = dz_channels;
  a.Ct = c1_rows + c2_rows;
  a.ci_off = which ? c1_rows : 0;
  a.ci_valid = which ? c2_rows : c1_rows;
  a.Cout = d->Cout;                                            // the row length of dw; co_valid = its columns that are written
  a.co_valid = d->cout_valid > 0 ? d->cout_valid : d->Cout;
  a.x_scale = which ? d->x2_scale : 1.0f;
}

}  // namespace shdr

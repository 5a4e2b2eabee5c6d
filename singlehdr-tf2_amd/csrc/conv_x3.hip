// fp32 3x3 / stride-1 convolution on the fp16 matrix pipe: every fp32 operand is split into two fp16 terms and a product is the sum of
// three v_mfma_f32_16x16x32_f16 (fp32 accumulation) -- "x3".  Replaces the same tf.keras.layers.Conv2D call sites as the fused
// Winograd kernel (hallucination_net.py:43-75,115-144, dequantization_net.py:35-46, refinement_net.py, vgg16.py:72-83: the 3x3
// layers with a multiple of 32 input channels per source and a multiple of 64 output channels), forward and input gradient.
//
// Arithmetic.  x = xh + xl * 2^-11 with xh = fp16(x), xl = fp16((x - xh) * 2^11): 22 mantissa bits, no underflow of the low term
// (it is stored scaled).  w' = w * 2^S (S per layer: max |w'| in [2^13, 2^14), so the low term of a weight is a normal fp16 number
// down to |w| = max |w| * 2^-17) = wh + wl.  Then
//     x * w' = xh * wh + xl * (wh * 2^-11) + xh * wl + (dropped: xl * wl * 2^-11, < 2^-22 |x w'|)
// i.e. three MFMAs with the filter operands wh, wh * 2^-11 (exact: a power-of-two scaling, formed in registers from the wh fragment with
// four v_pk_mul_f16 -- one LDS image and a third of the filter bytes less than a stored copy) and wl, all into ONE fp32 accumulator; the
// epilogue multiplies by 2^-S (exact).  Per-product error <= 3 * 2^-22 = 7e-7 relative, of random sign -- the level of the fp32
// rounding of a K >= 288 dot product itself; measured against the float64 oracle in tests/test_gpu_ops.py (same 1e-5 bar as the
// exact-fp32 kernels, errors reported next to the Winograd kernel's).
// Range.  fp16(x) overflows at |x| >= 65504 and loses the high term's mantissa below 2^-14, which an fp32 convolution does not.  Every
// launch therefore takes a RANGE SLOT per source -- a device word holding (the bit pattern of) an upper bound of max |x| of the tensor,
// written by the producing kernel's epilogue (y_range of the conv kernels), by shdr_absmax_f32, or known to the host -- and multiplies
// the input by the power of two 2^T that brings that bound into [2^10, 2^11) while it splits (one v_fma_mix per term: the scaling costs
// no instruction), the epilogue multiplies by 2^-T: both exact.  Elements down to 2^-25 of the tensor's maximum keep all 22 bits, smaller
// ones an absolute precision of 2^-46 of the maximum; non-finite inputs give non-finite outputs on their receptive field, as the fp32
// kernels do.  A launch without a slot (the low-level entry point only) runs unscaled.
//
// Kernel (the layout of conv_f16_w3.hip with fp32 tensors in HBM): block = 16 x 16 pixels x 64 couts, 4 waves; per 32-channel chunk
// the raw 18 x 18 fp32 patch is loaded ONCE into registers (coalesced 128-byte lines), split, and written as two fp16 images of
// 64-byte rows (16-byte slot XOR-swizzled: conflict-free ds_read_b128); the two filter images stream through LDS per tap (8 KB,
// stored one tap ahead, double-buffered).  Per tap and wave: 16 operand reads feed 48 MFMAs.  58 KB of LDS, two blocks per CU.
// The patch of chunk c + 1 is issued at the top of chunk c, BEHIND the filter unit that tap LOOK of the chunk needs; the filter units
// are loaded LOOK taps ahead through a scalar base and waited for with counted vmcnt, so the patch flies under LOOK + 1 taps of MFMAs
// before a wait can sit it out (template parameter LOOK below; the order it replaced, and why its prefetch never landed under the
// MFMAs: DESIGN.md section 6).
// Fused around it: MaxPool2D(2) in the epilogue (the conv + max-pool pairs of hallucination_net.py:43-75 / vgg16.py:72-83: the 2 x 2
// window is two accumulator rows of a lane and its neighbour lane) and tf.image.resize(x, 2x, BILINEAR) in the prologue (UP = true;
// hallucination_net.py:86-88, dequantization_net.py:25-27): the block loads the 10 x 10 LOW-RES patch of a chunk (a quarter of the
// bytes), parks it in 12.5 KB of LDS and builds the 18 x 18 up-sampled patch from it with resize2x_kernel's arithmetic and order
// (bit-identical to the two-kernel path) on the way into the fp16 images.
#include <hip/hip_fp16.h>
#include <stdlib.h>

#include <type_traits>

#include "split.h"

namespace {

using u32x4 = __attribute__((ext_vector_type(4))) unsigned;

constexpr int BN = 64, NT = 4, MT = 4;
constexpr int IMG_HALVES = BN * 32;                            // one filter image of a tap: [64 couts][32 channels]
constexpr int UNIT_HALVES = 2 * IMG_HALVES;                    // wh, wl
constexpr int LRW = 10, LRPIX = LRW * LRW;                     // low-res patch of the up-sampling prologue
constexpr int LRJ = (LRPIX * 8 + 255) / 256;                   // float4 pieces per thread (4)
// KH x KW taps over a 16 x 16 output tile: raw patch (16 + KH - 1) x (16 + KW - 1).  3 x 3 and 1 x 1 = the stride-1 layers; 4 x 4 = the
// patch of the 7 x 7 / stride-2 layer, whose four phases run 4 x 4, 4 x 3, 3 x 4 and 3 x 3 taps on it (MP, see x3_forward)
template <int KH, int KW>
struct X3G {
  static constexpr int PH = 16 + KH - 1, PWID = 16 + KW - 1, PPIX = PH * PWID;
  static constexpr int PJ = (PPIX * 8 + 255) / 256;           // float4 pieces per thread and chunk
  static constexpr int PATCH_HALVES = PPIX * 32;              // one fp16 image of the patch
  static constexpr int LDS_BYTES = (2 * PATCH_HALVES + 2 * UNIT_HALVES) * 2;
  static constexpr int LDS_BYTES_UP = LDS_BYTES + LRPIX * 32 * 4;
  static constexpr int RANGE_BYTES = 16;                       // + the waves' output maxima (shdr::range_out), behind everything else
};

struct X3Args {
  const float* x1;
  const float* x2;
  const _Float16* wp;      // packed [Cout / 64][units = Ct / 32 * taps][2 images: wh, wl][64][32]
  const float* hdr;        // packed header (split.h): hdr[kHdrInvScale] = 2^-S
  const float* bias;
  const float* scale;
  const float* shift;
  float* y;                // [N,H,W,Cout] (or null when only the pooled tensor is wanted)
  float* yp;               // [N,H/2,W/2,Cout] = MaxPool2D(2)(y), or null
  const float* res;        // residual added between the affine and act2 (the ResNet joins of linearization_net.py:6-48), or null
  int res_cs;              // its channels per pixel
  int N, H, W, C1, C2, Cout, tiles_x, tiles_y, nblk_m, nblk_n, act1, act2;
  int Hl, Wl;              // UP: x1 is the low-res tensor [N,Hl,Wl,C1], H = 2 Hl, W = 2 Wl
  int Hin, Win;            // input tensor [N,Hin,Win,C]; tap (kh, kw) of output (oh, ow) reads input (in_s (oh + kh) + bh, in_s (ow + kw) + bw)
  int in_s, bh, bw;        // stride-1 3x3 SAME: in_s = 1, bh = bw = -1
  int pool_avg;            // yp = AveragePooling2D(2)(y) instead of MaxPool2D(2)(y)
  const unsigned* xr1;     // range slots of the two sources (bits of an upper bound of max |x|; null: no scaling)
  const unsigned* xr2;
  unsigned* yr;            // range slot of the output: atomicMax of max |y| (null: not wanted)
  int nphase;              // MP kernel (the 7x7 / stride-2 stem in ONE launch): phase p runs pth[p] x ptw[p] taps at input offset (pbh[p], pbw[p]) with
  int pth[4], ptw[4], pbh[4], pbw[4];      // the packed sub-filter pwp[p]; all phases accumulate in the block's registers
  const _Float16* pwp[4];
  const float* proj;       // [3][64] or null: a linear map applied to the 64 output channels of every pixel in the epilogue ...
  float* yproj;            // ... yproj[N,H,W,3][j] = sum_c proj[j][c] y[c] (shdr_conv2d_fwd_x3_projected_f32; Cout = 64)
};

// ---- the tile epilogue of conv_x3_kernel (NW = 4 waves, PROJ) and conv_x3_wide_kernel (NW = 8; no projected output, which needs Cout = 64).
// The wave holds acc[MT][NT] = the MT pixel rows from oh_row0 on x the 64 couts from n0 on; the lane's tile column is ow (pc in the tile: the
// pcol permutation), its couts the quads 4 fg of each 16; ixs = 2^-T of the input scaling; range_lds = NW words of LDS for shdr::range_out.
template <int NW, bool PROJ>
__device__ __forceinline__ void x3_tile_epilogue(const X3Args& a, f32x4 (&acc)[MT][NT], int img, int oh_row0, int ow, int pc, int fg, int n0, float ixs,
                                                 int lane, int wave, unsigned* range_lds) {
  // y = act2(affine(act1(acc * 2^-S + bias))), 16-byte stores (lane = pixel x 4 consecutive couts); the 2 x 2 pooling window of the
  // optional second output is two rows of this lane and of its neighbour lane
  const float inv_s = a.hdr[shdr::kHdrInvScale] * ixs;
  // bias / scale / shift of the lane's four cout quads are loaded ONCE, in front of the store loop: a load inside it is followed by
  // "s_waitcnt vmcnt(0)", which also sits out the round trip of the output store issued just before it -- the stores of a block went
  // out one at a time
  // (the offsets pass through an opaque asm so that the loads are not hoisted above the tap loop, where their registers would be live
  //  for the whole kernel)
  const unsigned yr_seen = a.yr ? __hip_atomic_load(a.yr, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : 0u;
  int ep0 = n0;
  asm volatile("" : "+s"(ep0));
  f32x4 bias_r[NT], scale_r[NT], shift_r[NT];
#pragma unroll
  for (int ni = 0; ni < NT; ++ni) {
    const int cl = ni * 16 + 4 * fg;
    const bool cv = ep0 + cl < a.Cout;                           // (false only in the zero half of a 32-cout layer's slice: nothing loaded, nothing stored)
    bias_r[ni] = (a.bias && cv) ? *reinterpret_cast<const f32x4*>(a.bias + ep0 + cl) : (f32x4){0.f, 0.f, 0.f, 0.f};
    scale_r[ni] = (a.scale && cv) ? *reinterpret_cast<const f32x4*>(a.scale + ep0 + cl) : (f32x4){1.f, 1.f, 1.f, 1.f};
    shift_r[ni] = (a.scale && cv) ? *reinterpret_cast<const f32x4*>(a.shift + ep0 + cl) : (f32x4){0.f, 0.f, 0.f, 0.f};
  }
  // the residual, batched in front of the stores for the same reason
  f32x4 res_r[MT / 2][NT][2];
  if (a.res) {
#pragma unroll
    for (int mp = 0; mp < MT / 2; ++mp)
#pragma unroll
      for (int ni = 0; ni < NT; ++ni)
#pragma unroll
        for (int r = 0; r < 2; ++r) {
          const int oh = oh_row0 + 2 * mp + r;
          res_r[mp][ni][r] = (oh < a.H && ow < a.W && ep0 + ni * 16 + 4 * fg < a.Cout)
                                 ? *reinterpret_cast<const f32x4*>(a.res + ((size_t)(img * a.H + oh) * a.W + ow) * a.res_cs + ep0 + ni * 16 + 4 * fg)
                                 : (f32x4){0.f, 0.f, 0.f, 0.f};
        }
  }
  float ym = 0.0f;                                             // max |y| over this lane's stored values (a.yr)
#pragma unroll
  for (int mp = 0; mp < MT / 2; ++mp) {
    const int oh = oh_row0 + 2 * mp;                           // even row of the pair (H even whenever yp is given)
    if (oh >= a.H) continue;                                   // wave-uniform
    float pj[2][3] = {{0.f, 0.f, 0.f}, {0.f, 0.f, 0.f}};      // a.proj: this lane's share (16 of the 64 couts) of the projected pixel, rows oh, oh + 1
#pragma unroll
    for (int ni = 0; ni < NT; ++ni) {
      const int cl = ni * 16 + 4 * fg;
      f32x4 v[2];
#pragma unroll
      for (int r = 0; r < 2; ++r) {
        v[r] = acc[2 * mp + r][ni] * inv_s;
        asm("" : "+v"(v[r]));                                  // the product is rounded on its own: without the fence the compiler contracts it
                                                               // with the bias into one FMA (other output bits; conv_x3_1x1_kernel has the same)
        v[r] += bias_r[ni];
        shdr::act_apply4<0>(v[r], a.act1);
        if (a.scale) v[r] = v[r] * scale_r[ni] + shift_r[ni];
        if (a.res) v[r] += res_r[mp][ni][r];
        shdr::act_apply4<0>(v[r], a.act2);
        if (a.y && oh + r < a.H && ow < a.W && n0 + cl < a.Cout)
          *reinterpret_cast<f32x4*>(a.y + ((size_t)(img * a.H + oh + r) * a.W + ow) * a.Cout + n0 + cl) = v[r];
        if (PROJ && a.proj) {
#pragma unroll
          for (int j = 0; j < 3; ++j) {
            const f32x4 q = *reinterpret_cast<const f32x4*>(a.proj + j * 64 + cl);
            pj[r][j] += v[r][0] * q[0] + v[r][1] * q[1] + v[r][2] * q[2] + v[r][3] * q[3];
          }
        }
#ifndef SHDR_ABL_NO_YM
        if (a.yr && oh + r < a.H) ym = fmaxf(fmaxf(fmaxf(fmaxf(ym, fabsf(v[r][0])), fabsf(v[r][1])), fabsf(v[r][2])), fabsf(v[r][3]));      // two v_max3_f32
#endif
      }
      if (a.yp) {
        f32x4 m;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          if (a.pool_avg) {                                    // (top-left + top-right) + (bottom-left + bottom-right), as pool.hip adds them
            const float t = v[0][e] + __shfl_xor(v[0][e], 1, 64), b = v[1][e] + __shfl_xor(v[1][e], 1, 64);
            m[e] = 0.25f * (t + b);
          } else {
            m[e] = fmaxf(v[0][e], v[1][e]);
            m[e] = fmaxf(m[e], __shfl_xor(m[e], 1, 64));
          }
        }
        if (!(pc & 1) && ow < a.W && n0 + cl < a.Cout)           // lanes fi and fi ^ 1 hold columns pc and pc ^ 1
          *reinterpret_cast<f32x4*>(a.yp + ((size_t)(img * (a.H >> 1) + (oh >> 1)) * (a.W >> 1) + (ow >> 1)) * a.Cout + n0 + cl) = m;
      }
    }
    if (PROJ && a.proj) {                                      // the four lane groups fg hold 16 couts each of the same pixel
#pragma unroll
      for (int r = 0; r < 2; ++r) {
#pragma unroll
        for (int j = 0; j < 3; ++j) {
          float t = pj[r][j];
          t += __shfl_xor(t, 16, 64);
          t += __shfl_xor(t, 32, 64);
          pj[r][j] = t;
        }
        if (fg == 0 && oh + r < a.H && ow < a.W) {
          float* o = a.yproj + ((size_t)(img * a.H + oh + r) * a.W + ow) * 3;
          o[0] = pj[r][0]; o[1] = pj[r][1]; o[2] = pj[r][2];
        }
      }
    }
  }
#ifndef SHDR_ABL_NO_TAIL
  // (a pooled output is bounded by the same maximum).  The waves' words have LDS of their own: without a barrier after the last chunk (the
  // 1 x 1 form) wave 0 may still be reading patch pixel (0, 0) when another wave writes its maximum
  if (a.yr)
    shdr::range_out<NW>(a.yr, ow < a.W ? ym : 0.0f, lane, wave, yr_seen, range_lds);
#endif
}

// (filter images: rows = couts, 16-row aligned fragments, slots swizzled by row_swz)
// Patch images: the 16-byte slot of channel group kg of patch column c is kg ^ sx(c).  A ds_read_b128 is served in lane groups of
// {8 lanes of one kg, 8 lanes of kg ^ 1}; with the lane -> tile-column permutation pcol() below each set of 8 reads 8 CONSECUTIVE
// columns, so (column mod 8, kg) -- and with it (64-byte quarter, slot) -- is distinct for every tap shift: conflict-free at any
// alignment (the row-keyed swizzle of the filter images 2-way-conflicted on 23 % of the LDS cycles here), and the address splits
// into a per-lane column term (one register per kw) + a scalar row term: one VALU add per tap instead of six per operand read.
__host__ __device__ inline int sx(int col) { return ((col >> 2) & 1) * 2; }
__device__ __forceinline__ int pcol(int fi) { return fi < 4 ? fi : (fi >= 12 ? fi - 8 : fi + 4); }

// The input is multiplied by the power of two that brings its range bound (a.xr1 / a.xr2) to [2^10, 2^11) before the split and the result
// divided by it -- both exact.  This matters at both ends: activations beyond the fp16 range, and the output gradients dz of the
// training steps far below it (max |dz| 3e-8 ... 2e-2 in the joint step: unscaled, their high terms are fp16 subnormals and the
// parameter gradient differed from the exact-fp32 kernels' by 3e-5; scaled, by the run-to-run noise).
// MP (with KH = KW = 4, the largest phase): the four parity phases of a 7x7 / stride-2 layer in ONE launch -- a phase loop around the chunk loop
// with the tap counts, the input offset and the sub-filter of each phase taken from the argument arrays; the partial sums stay in the
// accumulators (the four-launch form of the first rounds, DESIGN.md section 4, wrote and re-read them three times).  The patch geometry is that of the
// 4 x 4 phase for every phase: a 3-tap dimension loads one row / column it does not use.
// LOOK = 1, 2: how many taps ahead a filter unit is loaded (the arithmetic, and with it every output bit, is the same for both; the
// history of the order, and of the one it replaced, is DESIGN.md section 6).  A unit is a block-uniform 64-bit base in SGPRs plus ONE
// loop-invariant VGPR byte offset (no address arithmetic, no wait between a tap's barrier and its MFMAs), loaded LOOK taps ahead into
// fr[LOOK][FJ] by inline asm (outside the compiler's scoreboard), and the unit that tap u + LOOK needs is issued IN FRONT of the chunk's
// patch loads.  The wait in front of the store to LDS is counted: "vmcnt(loads issued after the unit)" leaves the later units and, in the
// first LOOK taps of a chunk, the patch loads in flight -- the patch flies for LOOK + 1 taps before a wait can sit it out.  Out-of-image
// pieces are zeros without a load, so the number of patch loads a WAVE issues is not static: pcnt counts the pieces with at least one
// lane inside the image (a lower bound of the loads issued, which is the safe side), the wait is coded for pcnt = PJ, PJ - 1 and PJ - 2
// (interior tiles and plain edges) and falls back to sitting the patch out.
//   1  every form: the stem (out of registers at 2), the one-tap 1 x 1 form, and the nine-tap forms under SHDR_X3_LOOK=1
//   2  the nine-tap forms by default: units alternate between two register slots, the taps of a chunk are unrolled (see NFR below)
template <bool UP, int KH, int KW, bool MP = false, int LOOK = 1>
__global__ __launch_bounds__(256, 2) void conv_x3_kernel(const X3Args a) {
  using G = X3G<KH, KW>;
  constexpr int PWID = G::PWID, PPIX = G::PPIX, PJ = G::PJ, PATCH_HALVES = G::PATCH_HALVES, NTAPS = KH * KW;
  static_assert(!UP || (KH == 3 && KW == 3), "the up-sampling prologue belongs to the 3 x 3 stride-1 form");
  static_assert(!MP || (!UP && KH == 4 && KW == 4), "the phase loop is built on the 4 x 4 patch geometry");
  static_assert(LOOK >= 1 && LOOK <= 2 && LOOK <= KW, "filter look-ahead: 1 or 2 taps");
  extern __shared__ __attribute__((aligned(16))) _Float16 xsm[];
  // LDS regions as expressions of the __shared__ symbol (pointer VARIABLES captured by the lambdas below lost their address space: the
  // compiler kept them as 64-bit generic pointers in scratch and reloaded them inside the tap loop)
#define patch_h (xsm)                                          /* [PATCH_HALVES] */
#define patch_l (xsm + PATCH_HALVES)
#define filt (xsm + 2 * PATCH_HALVES)                          /* [2][UNIT_HALVES] */
#define lrs (reinterpret_cast<float*>(xsm + 2 * PATCH_HALVES + 2 * UNIT_HALVES))       /* UP: [LRPIX][32] fp32 */

  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int L = shdr::xcd_remap(blockIdx.x, a.nblk_m * a.nblk_n);
  const int pn = L % a.nblk_n;
  int pm = L / a.nblk_n;
  const int tx = pm % a.tiles_x;
  pm /= a.tiles_x;
  const int ty = pm % a.tiles_y;
  const int img = pm / a.tiles_y;
  const int n0 = pn * BN, oh0 = ty * 16, ow0 = tx * 16;

  // ---- patch geometry (fixed per block): piece p = tid + 256 j -> (patch pixel, float4 of the 32-channel chunk) ----------------
  int ppix[PJ];                                                // pixel index in the image tensor, -1: padding / beyond the patch
  int pdst[PJ];                                                // half offset of the 8-byte destination inside an image
  int pcnt = 0;                                                // patch loads per chunk this wave is sure to issue (wave-uniform)
  auto patch_geometry = [&](int bh, int bw) __attribute__((always_inline)) {                  // (MP: once per phase)
    pcnt = 0;
#pragma unroll
    for (int j = 0; j < (UP ? 0 : PJ); ++j) {
      const int p = tid + 256 * j;
      const int pix = p >> 3, q = p & 7;
      const int py = pix / PWID, px = pix - py * PWID;
      const int ih = a.in_s * (oh0 + py) + bh, iw = a.in_s * (ow0 + px) + bw;
      const bool ok = pix < PPIX && (unsigned)ih < (unsigned)a.Hin && (unsigned)iw < (unsigned)a.Win;
      ppix[j] = ok ? (img * a.Hin + ih) * a.Win + iw : -1;
      pdst[j] = pix < PPIX ? pix * 32 + 8 * ((q >> 1) ^ sx(px)) + 4 * (q & 1) : -1;
      pcnt += __ballot(ppix[j] >= 0) != 0ull;
    }
  };
  if (!MP) patch_geometry(a.bh, a.bw);
  if (!MP && !UP) pcnt = __builtin_amdgcn_readfirstlane(pcnt);
  // UP: low-res pieces of this thread: piece p = tid + 256 j -> (low-res patch pixel, float4)
  int lpix[LRJ];
  if (UP) {
#pragma unroll
    for (int j = 0; j < LRJ; ++j) {
      const int p = tid + 256 * j;
      const int pix = p >> 3;
      const int ly = pix / LRW, lx = pix - ly * LRW;
      const int r = (oh0 >> 1) - 1 + ly, c = (ow0 >> 1) - 1 + lx;
      lpix[j] = (pix < LRPIX && (unsigned)r < (unsigned)a.Hl && (unsigned)c < (unsigned)a.Wl) ? (img * a.Hl + r) * a.Wl + c : -1;
      pcnt += __ballot(lpix[j] >= 0) != 0ull;
    }
    pcnt = __builtin_amdgcn_readfirstlane(pcnt);
  }
  const int nch1 = a.C1 >> 5, nch = (a.C1 + a.C2) >> 5;
  int nunits = nch * NTAPS;                                    // (MP: per phase)
  // 1 x 1 layers run ONE tap (48 MFMAs, ~0.4 us) per chunk: a patch load issued one chunk ahead still has most of its HBM latency in
  // front of it when the chunk is needed -- they prefetch TWO chunks ahead into two register sets (the chunk loop below alternates them)
  constexpr int DEPTH = (NTAPS == 1 && !UP && !MP) ? 2 : 1;
  using Set0 = std::integral_constant<int, 0>;
  using Set1 = std::integral_constant<int, DEPTH - 1>;
  f32x4 pr_sets[DEPTH][PJ];
#define pr (pr_sets[0])                                        /* the UP paths and the single-set kernels */
  // The registers of a prefetch are zeroed IN FRONT of the filter unit issued before it (zero_patch): the compiler cannot tell
  // that the set's previous loads were waited for (store_patch sits under another condition) and guards the first write with a full wait,
  // which must not find that unit in flight
  auto zero_patch = [&](auto setc) __attribute__((always_inline)) {
    constexpr int S = decltype(setc)::value;
#pragma unroll
    for (int j = 0; j < (UP ? LRJ : PJ); ++j) pr_sets[S][j] = (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int j = 0; j < (UP ? LRJ : PJ); ++j) asm volatile("" : "+v"(pr_sets[S][j]));
  };
  auto load_lr = [&](int c, bool zeroed) __attribute__((always_inline)) {                     // UP: low-res chunk c -> the first LRJ registers
#pragma unroll
    for (int j = 0; j < LRJ; ++j) {
      const int q = (tid + 256 * j) & 7;
      if (!zeroed) pr[j] = (f32x4){0.f, 0.f, 0.f, 0.f};
      if (lpix[j] >= 0) pr[j] = *reinterpret_cast<const f32x4*>(a.x1 + (size_t)(unsigned)lpix[j] * (unsigned)a.C1 + (c << 5) + 4 * q);
    }
  };
  auto park_lr = [&]() __attribute__((always_inline)) {                                       // UP: registers -> LDS scratch [pixel][32]
#pragma unroll
    for (int j = 0; j < LRJ; ++j)
      if (tid + 256 * j < LRPIX * 8) *reinterpret_cast<f32x4*>(lrs + 4 * (tid + 256 * j)) = pr[j];
  };
  float xs = 1.0f, ixs = 1.0f;                                 // input scale 2^T and its inverse: set BEHIND the first patch / filter loads below (the
                                                               // slot is a dependent scalar load: in front of them it delayed every block's first fetch)
  auto split_store = [&](int dst, const f32x4 v4) __attribute__((always_inline)) {            // one float4 -> 8 bytes in each fp16 image
    unsigned h[2], l[2];
    shdr::split4(v4, xs, h, l);
    *reinterpret_cast<uint2*>(patch_h + dst) = make_uint2(h[0], h[1]);
    *reinterpret_cast<uint2*>(patch_l + dst) = make_uint2(l[0], l[1]);
  };
  auto expand_store = [&]() __attribute__((always_inline)) {   // UP: scratch -> up-sampled 18 x 18 patch (the arithmetic of resize2x_kernel) -> images
    // the geometry of a piece is recomputed per chunk (a few integer operations) instead of being held in 22 registers: the
    // expansion needs them for its four taps
    const int r0 = (oh0 >> 1) - 1, c0 = (ow0 >> 1) - 1;
    int t0 = tid;
    asm volatile("" : "+v"(t0));                               // computed HERE: hoisted out of the chunk loop the 11 geometries are 90 live registers (spills)
#pragma unroll
    for (int j = 0; j < PJ; ++j) {
      const int p = t0 + 256 * j;
      const int pix = p >> 3, q = p & 7;
      if (pix >= PPIX) continue;
      const int py = pix / PWID, px = pix - py * PWID;
      const int ih = oh0 - 1 + py, iw = ow0 - 1 + px;
      f32x4 v = (f32x4){0.f, 0.f, 0.f, 0.f};
      if ((unsigned)ih < (unsigned)a.Hin && (unsigned)iw < (unsigned)a.Win) {
        const int mr = ih >> 1, mc = iw >> 1;
        const int ra = (ih & 1) ? mr : max(mr - 1, 0), rb = (ih & 1) ? min(mr + 1, a.Hl - 1) : mr;
        const int ca = (iw & 1) ? mc : max(mc - 1, 0), cb = (iw & 1) ? min(mc + 1, a.Wl - 1) : mc;
        const float* s00 = lrs + ((ra - r0) * LRW + (ca - c0)) * 32 + 4 * q;
        const int dx = (cb - ca) * 32, dy = (rb - ra) * LRW * 32;
        const float wx = (iw & 1) ? 0.25f : 0.75f, wy = (ih & 1) ? 0.25f : 0.75f;
        const f32x4 q00 = *reinterpret_cast<const f32x4*>(s00), q01 = *reinterpret_cast<const f32x4*>(s00 + dx);
        const f32x4 q10 = *reinterpret_cast<const f32x4*>(s00 + dy), q11 = *reinterpret_cast<const f32x4*>(s00 + dy + dx);
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const float t = q00[e] + (q01[e] - q00[e]) * wx;      // horizontal first, then vertical
          const float u = q10[e] + (q11[e] - q10[e]) * wx;
          v[e] = t + (u - t) * wy;
        }
      }
      split_store(pix * 32 + 8 * ((q >> 1) ^ sx(px)) + 4 * (q & 1), v);
      if (j & 1) __builtin_amdgcn_sched_barrier(0);            // two pieces (32 registers of taps) in flight, not eleven: no spills
    }
  };
  auto load_patch = [&](int c, auto setc, bool zeroed = false) __attribute__((always_inline)) {      // chunk c -> register set setc
    constexpr int S = decltype(setc)::value;
    if (UP) { load_lr(c, zeroed); return; }
    const bool second = c >= nch1;
    const float* src = second ? a.x2 : a.x1;
    const int Cs = second ? a.C2 : a.C1;
    const int c0 = (second ? c - nch1 : c) << 5;
#pragma unroll
    for (int j = 0; j < PJ; ++j) {
      const int q = (tid + 256 * j) & 7;
      if (!zeroed) pr_sets[S][j] = (f32x4){0.f, 0.f, 0.f, 0.f};
      if (ppix[j] >= 0) pr_sets[S][j] = *reinterpret_cast<const f32x4*>(src + (size_t)(unsigned)ppix[j] * (unsigned)Cs + c0 + 4 * q);
    }
  };
  auto store_patch = [&](auto setc) __attribute__((always_inline)) {                          // register set setc -> the two fp16 images
    constexpr int S = decltype(setc)::value;
    if (UP) { expand_store(); return; }
#pragma unroll
    for (int j = 0; j < PJ; ++j)
      if (pdst[j] >= 0) split_store(pdst[j], pr_sets[S][j]);
  };
  // ---- filter units: 8 KB per tap = 512 pieces of 16 bytes, two per thread --------------------------------------------------------
  constexpr int FJ = 2;
  const _Float16* wbase = a.wp + (size_t)pn * nunits * UNIT_HALVES;      // (MP: per phase)
  int fdst[FJ];
#pragma unroll
  for (int j = 0; j < FJ; ++j) {
    const int p = tid + 256 * j;
    const int im = p >> 8, co = (p & 255) >> 2, slot = p & 3;
    fdst[j] = im * IMG_HALVES + co * 32 + 8 * (slot ^ row_swz(co));
  }
  // LOOK = 2: units alternate between two register slots.  The slot of a unit has to be a compile-time constant (a slot chosen by a branch
  // on the unit's parity left the compiler free to keep it in other registers on either side and to copy a load in flight), so the nine
  // taps of a chunk are unrolled: the unit of tap k sits in slot k & 1.  Nine is odd: behind the last tap, where the chunk's loads are
  // waited for anyway, the unit of the next chunk's tap 1 moves from slot 0 to slot 1.  (Three slots indexed by kw need no move and spill.)
  constexpr int NFR = LOOK < 2 ? 1 : 2;
  static_assert(LOOK < 2 || (!MP && KH == 3 && KW == 3), "LOOK = 2 is built for the nine-tap kernels");
  u32x4 fr[NFR][FJ];
#pragma unroll
  for (int s = 0; s < NFR; ++s)
#pragma unroll
    for (int j = 0; j < FJ; ++j) fr[s][j] = (u32x4){0u, 0u, 0u, 0u};
  // The thread's two pieces lie 4096 bytes apart -- past the 13-bit signed offset field, hence the offset register points between them.
  // Always issued, past the last unit of the layer (MP: of the phase) the last unit again: the number of loads in flight stays static.
  // (s: a constant once the kw loop is unrolled)
  const unsigned foff = 16u * (unsigned)tid + 2048u;
  auto issue_filt = [&](int u, int s) __attribute__((always_inline)) {
    const _Float16* ub = wbase + (size_t)(u < nunits ? u : nunits - 1) * UNIT_HALVES;
    asm volatile("global_load_dwordx4 %0, %1, %2 offset:-2048" : "+v"(fr[s][0]) : "v"(foff), "s"(ub) : "memory");
    asm volatile("global_load_dwordx4 %0, %1, %2 offset:2048" : "+v"(fr[s][1]) : "v"(foff), "s"(ub) : "memory");
  };
  constexpr int PJL = UP ? LRJ : PJ;                           // patch loads of a thread and chunk at most
  constexpr int WB = (LOOK - 1) * FJ;                          // loads of the later units, always behind the one waited for
#define X3_WAIT_VM(N) asm volatile("s_waitcnt vmcnt(%0)" : : "n"(N) : "memory")
  // Unit v (slot s) has landed = everything but the (LOOK - 1) FJ loads of the later units and the np patch loads issued after
  // it (np < 0: the prologue, nothing was issued after it); then registers -> LDS buffer v & 1.  The counted wait names no register
  // (under a branch, an asm that ties fr is given registers of its own, and the copy into them reads the load in flight); ONE fence
  // behind the branches ties the slot, so that every use of it is ordered after the wait.
  auto wait_store_filt = [&](int v, int s, int np, bool st) __attribute__((always_inline)) {
    if (np < 0) X3_WAIT_VM(0);
    else if (np >= PJL) X3_WAIT_VM(WB + PJL);
    else if (np >= PJL - 1) X3_WAIT_VM(WB + PJL - 1);
    else if (np >= PJL - 2) X3_WAIT_VM(WB + PJL - 2);
    else X3_WAIT_VM(WB);
    asm volatile("" : "+v"(fr[s][0]), "+v"(fr[s][1]) : : "memory");
    if (st) {                                                  // (only the store is conditional: no asm that names fr under a branch)
#pragma unroll
      for (int j = 0; j < FJ; ++j) *reinterpret_cast<u32x4*>(filt + (v & 1) * UNIT_HALVES + fdst[j]) = fr[s][j];
    }
  };

  f32x4 acc[MT][NT];
#pragma unroll
  for (int mi = 0; mi < MT; ++mi)
#pragma unroll
    for (int ni = 0; ni < NT; ++ni) acc[mi][ni] = (f32x4){0.f, 0.f, 0.f, 0.f};

  const int fi = lane & 15, fg = lane >> 4;
  int acol[KW], b_rd[NT];                                      // A operand: half offset of (column pcol + kw, channel group fg) inside a patch row
  const int pc = pcol(fi);
#pragma unroll
  for (int kw = 0; kw < KW; ++kw) acol[kw] = (pc + kw) * 32 + 8 * (fg ^ sx(pc + kw));
#pragma unroll
  for (int ni = 0; ni < NT; ++ni) {
    const int row = ni * 16 + fi;
    b_rd[ni] = row * 32 + 8 * (fg ^ row_swz(row));
  }

  int kh_n = KH, kw_n = KW;                                    // taps of the phase (MP)
#pragma unroll 1
  for (int phase = 0; phase < (MP ? a.nphase : 1); ++phase) {
  if (MP) {
    kh_n = a.pth[phase];
    kw_n = a.ptw[phase];
    nunits = nch * kh_n * kw_n;
    wbase = a.pwp[phase] + (size_t)pn * nunits * UNIT_HALVES;
    patch_geometry(a.pbh[phase], a.pbw[phase]);
    pcnt = __builtin_amdgcn_readfirstlane(pcnt);
    if (phase > 0) __syncthreads();                            // every wave has read the last tap of the previous phase (patch and filter buffers)
  }
  load_patch(0, Set0{});
  if (DEPTH == 2 && nch > 1) load_patch(1, Set1{});
  issue_filt(0, 0);
  if (!MP || phase == 0) shdr::range_scale(a.xr1, a.xr2, xs, ixs);
  if (UP) {
    park_lr();
    __syncthreads();
  }
  store_patch(Set0{});
  wait_store_filt(0, 0, -1, true);
  if (LOOK == 2) issue_filt(1, 1);
  // one chunk: `cur` = the register set chunk c was loaded into (already split into LDS: free for chunk c + DEPTH), `nxt` = the set of chunk c + 1
  auto chunk = [&](int c, auto cur, auto nxt) __attribute__((always_inline)) {
    const bool pf = c + DEPTH < nch;
    // the unit of tap LOOK in FRONT of the patch loads: the waits of taps 0 .. LOOK - 1 are for units older than the patch
    zero_patch(cur);                                           // (unconditionally: under "if (pf)" every patch load got the compiler's full wait instead)
    __builtin_amdgcn_sched_barrier(0);
    issue_filt((MP ? c * kh_n * kw_n : c * NTAPS) + LOOK, LOOK % NFR);        // (slot of tap 0 + LOOK)
    __builtin_amdgcn_sched_barrier(0);
    if (pf) load_patch(c + DEPTH, cur, true);                  // lands under the taps of this chunk (and, for the 1 x 1 layers, of the next)
    __builtin_amdgcn_sched_barrier(0);
    const int np = pf ? pcnt : 0;
    // One tap, as a macro: the first row of a chunk is peeled off the kh loop (FIRST): its first tap's look-ahead unit is already issued
    // and its first LOOK waits leave the patch in flight -- as straight-line code, since a filter load or a wait that names fr under a
    // branch on kh lets the compiler hold the slot in other registers on the two sides and copy a load in flight.
    //   barrier: unit u (and, at the first tap, the patch) is in LDS; buffer (u + 1) & 1 is free
    //   rowh: scalar, the first patch row of this wave and tap; the A-operand reads run one pixel row ahead of the MFMAs that use them
    //   ws = wh 2^-11: exact (power of two; gradual underflow below |wh| = 2^-3 as in fp16 itself)
    //   the unit stored at the end is read after the next barrier
#define X3_SLOT(D) (NFR == 1 ? 0 : (kh * KW + kw + (D)) % NFR)  /* slot of the unit D taps on */
#define X3_TAP(FIRST)                                                                                                          \
  {                                                                                                                             \
    if (MP && kw >= kw_n) continue;                                                                                            \
    const int u = MP ? (c * kh_n + kh) * kw_n + kw : c * NTAPS + kh * KW + kw;                                                 \
    __syncthreads();                                                                                                           \
    if (!(FIRST) || kw > 0) issue_filt(u + LOOK, X3_SLOT(LOOK));                                                               \
    const _Float16* F = filt + (u & 1) * UNIT_HALVES;                                                                          \
    const int rowh = (wave * MT + kh) * PWID * 32;                                                                             \
                                                                                                                               \
    f16x8 wh[NT], ws[NT], wl[NT], ph[2], pl[2];                                                                                \
    auto read_a = [&](int mi, int slot) __attribute__((always_inline)) {                                                       \
      const int o = rowh + mi * PWID * 32 + acol[kw];                                                                          \
      ph[slot] = *reinterpret_cast<const f16x8*>(patch_h + o);                                                                 \
      pl[slot] = *reinterpret_cast<const f16x8*>(patch_l + o);                                                                 \
    };                                                                                                                         \
_Pragma("unroll")                                                                                                              \
    for (int ni = 0; ni < NT; ++ni) {                                                                                          \
      wh[ni] = *reinterpret_cast<const f16x8*>(F + b_rd[ni]);                                                                  \
      wl[ni] = *reinterpret_cast<const f16x8*>(F + IMG_HALVES + b_rd[ni]);                                                     \
    }                                                                                                                          \
    read_a(0, 0);                                                                                                              \
_Pragma("unroll")                                                                                                              \
    for (int ni = 0; ni < NT; ++ni) ws[ni] = wh[ni] * (_Float16)(1.0f / 2048.0f);                                              \
_Pragma("unroll")                                                                                                              \
    for (int mi = 0; mi < MT; ++mi) {                                                                                          \
      if (mi + 1 < MT) read_a(mi + 1, (mi + 1) & 1);                                                                           \
      __builtin_amdgcn_sched_barrier(0);                                                                                       \
_Pragma("unroll")                                                                                                              \
      for (int ni = 0; ni < NT; ++ni) acc[mi][ni] = __builtin_amdgcn_mfma_f32_16x16x32_f16(wh[ni], ph[mi & 1], acc[mi][ni], 0, 0, 0); \
_Pragma("unroll")                                                                                                              \
      for (int ni = 0; ni < NT; ++ni) acc[mi][ni] = __builtin_amdgcn_mfma_f32_16x16x32_f16(ws[ni], pl[mi & 1], acc[mi][ni], 0, 0, 0); \
_Pragma("unroll")                                                                                                              \
      for (int ni = 0; ni < NT; ++ni) acc[mi][ni] = __builtin_amdgcn_mfma_f32_16x16x32_f16(wl[ni], ph[mi & 1], acc[mi][ni], 0, 0, 0); \
      __builtin_amdgcn_sched_barrier(0);                                                                                       \
    }                                                                                                                          \
    wait_store_filt(u + 1, X3_SLOT(1), ((FIRST) && kw < LOOK) ? np : 0, u + 1 < nunits);                                       \
  }
    if (LOOK == 1) {
      {
        const int kh = 0;
#pragma unroll
        for (int kw = 0; kw < KW; ++kw) X3_TAP(true)           // unrolled: acol[kw] stays a register
      }
#pragma unroll 1
      for (int kh = 1; kh < (MP ? kh_n : KH); ++kh) {
#pragma unroll
        for (int kw = 0; kw < KW; ++kw) X3_TAP(false)
      }
    } else {
#pragma unroll
      for (int kh = 0; kh < KH; ++kh) {
#pragma unroll
        for (int kw = 0; kw < KW; ++kw) X3_TAP(kh == 0)
      }
      // every load of the chunk has landed (the patch is needed below): the unit of the next chunk's tap 1, issued into slot 0 at tap 8
      asm volatile("s_waitcnt vmcnt(0)" : "+v"(fr[0][0]), "+v"(fr[0][1]) : : "memory");
#pragma unroll
      for (int j = 0; j < FJ; ++j) fr[NFR - 1][j] = fr[0][j];
    }
#undef X3_TAP
#undef X3_SLOT
    if (c + 1 < nch) {
      if (UP) {
        park_lr();                                             // the scratch was last read before the tap loop of this chunk
        __syncthreads();                                       // ... and every wave has read the last tap of this chunk's patch
      } else {
        __syncthreads();                                       // every wave has read the last tap of this chunk's patch
      }
      store_patch(nxt);                                        // visible after the barrier at the top of the next tap loop
    }
  };
#pragma unroll 1
  for (int c = 0; c < nch; c += DEPTH) {
    chunk(c, Set0{}, Set1{});
    if (DEPTH == 2 && c + 1 < nch) chunk(c + 1, Set1{}, Set0{});
  }
  }                                                            // phase loop
#undef pr
#undef X3_WAIT_VM

  x3_tile_epilogue<4, true>(a, acc, img, oh0 + wave * MT, ow0 + pc, pc, fg, n0, ixs, lane, wave,
                            reinterpret_cast<unsigned*>(reinterpret_cast<char*>(xsm) + (UP ? G::LDS_BYTES_UP : G::LDS_BYTES)));
}

#undef patch_h
#undef patch_l
#undef filt
#undef lrs

// ---- 1 x 1 layers: one split per chunk for up to 256 couts ---------------------------------------------------------------------------
// A 1 x 1 layer runs ONE tap (48 MFMAs per wave) on every chunk it splits: conv_x3_kernel<false, 1, 1> with 64 couts per block fetched,
// split and staged each 32-channel chunk once per 64-cout slice -- four times for Cout = 256 -- and was vector-issue bound (6.3 VALU
// instructions per MFMA, 2.1 TB/s).  Here a block is BP = 128 CONSECUTIVE output pixels (no halo: any run of pixels is a patch) x NS
// slices of 64 couts (NS = 4: 256 couts, NS = 2: 128); wave w takes slice w % NS and the 128 / (4 / NS) pixels of group w / NS
// (MT1 = 2 NS 16-pixel rows: 128 accumulator registers at NS = 4).  Per chunk the block loads 16 KB of fp32 input, splits it ONCE into the
// two fp16 images (four float4 per thread) and every wave consumes it: split VALU per MFMA 2 / NS of the 64-cout form.
// The wave's filter fragments (wh, wl of its slice: 8 KB per chunk, the packed layout [Cout / 64][chunks][wh, wl][64][32] read as it is)
// come straight from global memory (L2: every block of the layer reads the same filter) into registers one chunk ahead -- no LDS image,
// no staging; the patch images are double-buffered (32 KB) and the raw input prefetched two chunks ahead in two register sets, so a
// chunk takes ONE barrier.  Operands, chunk order, MFMA order per product (wh xh, ws xl, wl xh) and the epilogue are those of
// conv_x3_kernel<false, 1, 1>: the results are bit-identical to it.
constexpr int X1_BP = 128;
template <int NS>
__global__ __launch_bounds__(256, 2) void conv_x3_1x1_kernel(const X3Args a) {
  constexpr int MT1 = 2 * NS, BP = X1_BP;
  constexpr int PJ1 = BP * 8 / 256;                            // float4 pieces per thread and chunk (4)
  constexpr int IMG = BP * 32;                                 // halves of one fp16 image of a chunk (8 KB)
  static_assert(NS * (BP / (MT1 * 16)) == 4, "four waves: NS cout slices x pixel groups");
  __shared__ __attribute__((aligned(16))) _Float16 x1sm[2 * 2 * IMG];       // [buffer][h, l][BP pixels][32], 16-byte slots swizzled by sx()
  __shared__ unsigned x1rw[4];                                 // the waves' output maxima (shdr::range_out)

  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int slice = wave % NS, grp = wave / NS;
  const int L = shdr::xcd_remap(blockIdx.x, a.nblk_m * a.nblk_n);
  const int pn = L % a.nblk_n, pm = L / a.nblk_n;
  const int P0 = pm * BP, Ptot = a.N * a.H * a.W;

  // ---- patch geometry (fixed per block): piece p = tid + 256 j -> (block pixel p >> 3, float4 p & 7 of the chunk) -------------------
  int ppix[PJ1];                                               // input pixel of the piece's output pixel, -1: beyond the layer
  const int pdst = (tid >> 3) * 32 + 8 * (((tid & 7) >> 1) ^ sx((tid >> 3) & 15)) + 4 * (tid & 1);      // + 32 * 32 j (same column)
#pragma unroll
  for (int j = 0; j < PJ1; ++j) {
    const int P = P0 + (tid >> 3) + 32 * j;
    ppix[j] = -1;
    if (P < Ptot) {
      const int ow = P % a.W, t = P / a.W;
      const int oh = t % a.H, img = t / a.H;
      const int ih = a.in_s * oh + a.bh, iw = a.in_s * ow + a.bw;
      if ((unsigned)ih < (unsigned)a.Hin && (unsigned)iw < (unsigned)a.Win) ppix[j] = (img * a.Hin + ih) * a.Win + iw;
    }
  }
  const int nch1 = a.C1 >> 5, nch = (a.C1 + a.C2) >> 5;
  using Set0 = std::integral_constant<int, 0>;
  using Set1 = std::integral_constant<int, 1>;
  f32x4 pr_sets[2][PJ1];
  auto load_patch = [&](int c, auto setc) __attribute__((always_inline)) {                    // chunk c -> register set setc
    constexpr int S = decltype(setc)::value;
    const bool second = c >= nch1;
    const float* src = second ? a.x2 : a.x1;
    const int Cs = second ? a.C2 : a.C1;
    const int c0 = (second ? c - nch1 : c) << 5;
#pragma unroll
    for (int j = 0; j < PJ1; ++j) {
      pr_sets[S][j] = (f32x4){0.f, 0.f, 0.f, 0.f};
      if (ppix[j] >= 0) pr_sets[S][j] = *reinterpret_cast<const f32x4*>(src + (size_t)(unsigned)ppix[j] * (unsigned)Cs + c0 + 4 * (tid & 7));
    }
  };
  float xs = 1.0f, ixs = 1.0f;
  auto store_patch = [&](int buf, auto setc) __attribute__((always_inline)) {                 // register set setc -> the two images of buffer buf
    constexpr int S = decltype(setc)::value;
#pragma unroll
    for (int j = 0; j < PJ1; ++j) {
      unsigned h[2], l[2];
      shdr::split4(pr_sets[S][j], xs, h, l);
      *reinterpret_cast<uint2*>(x1sm + buf * 2 * IMG + pdst + 1024 * j) = make_uint2(h[0], h[1]);
      *reinterpret_cast<uint2*>(x1sm + buf * 2 * IMG + IMG + pdst + 1024 * j) = make_uint2(l[0], l[1]);
    }
  };
  // ---- filter fragments of the wave's slice, straight from the packed filter (lane: cout row ni * 16 + fi, channels 8 fg .. 8 fg + 7).
  //      A chunk runs in two halves, couts ni = 0, 1 (fragments f0) and ni = 2, 3 (f1), over all MT1 pixel rows; each half's fragments
  //      are loaded while the other half runs (32 registers instead of 64 for a whole chunk held one chunk ahead: 256 couts fit two waves
  //      per SIMD without spilling), at the price of reading the patch images twice
  const int fi = lane & 15, fg = lane >> 4;
  const _Float16* wsl = a.wp + (size_t)(pn * NS + slice) * nch * UNIT_HALVES + fi * 32 + 8 * fg;
  f16x8 f0h[2], f0l[2], f1h[2], f1l[2];
  auto load_w = [&](int c, int half, f16x8 (&h)[2], f16x8 (&l)[2]) __attribute__((always_inline)) {
    const _Float16* g = wsl + (size_t)c * UNIT_HALVES + half * 2 * 16 * 32;
#pragma unroll
    for (int k = 0; k < 2; ++k) {
      h[k] = *reinterpret_cast<const f16x8*>(g + k * 16 * 32);
      l[k] = *reinterpret_cast<const f16x8*>(g + IMG_HALVES + k * 16 * 32);
    }
  };

  f32x4 acc[MT1][NT];
#pragma unroll
  for (int mi = 0; mi < MT1; ++mi)
#pragma unroll
    for (int ni = 0; ni < NT; ++ni) acc[mi][ni] = (f32x4){0.f, 0.f, 0.f, 0.f};
  const int pc = pcol(fi);
  const int a_rd = (grp * MT1 * 16 + pc) * 32 + 8 * (fg ^ sx(pc));      // B operand: (pixel grp * MT1 * 16 + pc, channel group fg) + 16 mi pixels

  // couts ni = 2 half, 2 half + 1 of chunk c (patch buffer buf) over all pixel rows of the wave
  auto half_pass = [&](int buf, auto halfc, const f16x8 (&wh)[2], const f16x8 (&wl)[2]) __attribute__((always_inline)) {
    constexpr int H = decltype(halfc)::value;
    const int bo = buf * 2 * IMG + a_rd;
    f16x8 ws[2], ph[2], pl[2];
    auto read_a = [&](int mi, int slot) __attribute__((always_inline)) {
      ph[slot] = *reinterpret_cast<const f16x8*>(x1sm + bo + mi * 16 * 32);
      pl[slot] = *reinterpret_cast<const f16x8*>(x1sm + IMG + bo + mi * 16 * 32);
    };
    read_a(0, 0);
#pragma unroll
    for (int k = 0; k < 2; ++k) ws[k] = wh[k] * (_Float16)(1.0f / 2048.0f);                // exact (as in conv_x3_kernel)
#pragma unroll
    for (int mi = 0; mi < MT1; ++mi) {
      if (mi + 1 < MT1) read_a(mi + 1, (mi + 1) & 1);
      __builtin_amdgcn_sched_barrier(0);
#pragma unroll
      for (int k = 0; k < 2; ++k) acc[mi][2 * H + k] = __builtin_amdgcn_mfma_f32_16x16x32_f16(wh[k], ph[mi & 1], acc[mi][2 * H + k], 0, 0, 0);
#pragma unroll
      for (int k = 0; k < 2; ++k) acc[mi][2 * H + k] = __builtin_amdgcn_mfma_f32_16x16x32_f16(ws[k], pl[mi & 1], acc[mi][2 * H + k], 0, 0, 0);
#pragma unroll
      for (int k = 0; k < 2; ++k) acc[mi][2 * H + k] = __builtin_amdgcn_mfma_f32_16x16x32_f16(wl[k], ph[mi & 1], acc[mi][2 * H + k], 0, 0, 0);
      __builtin_amdgcn_sched_barrier(0);
    }
  };
  using Half0 = std::integral_constant<int, 0>;
  using Half1 = std::integral_constant<int, 1>;

  load_patch(0, Set0{});
  if (nch > 1) load_patch(1, Set1{});
  load_w(0, 0, f0h, f0l);
  shdr::range_scale(a.xr1, a.xr2, xs, ixs);                    // (behind the first loads: the slot is a dependent scalar load)
  store_patch(0, Set0{});
  if (nch > 2) load_patch(2, Set0{});
  // chunk c: buffer c & 1 holds it; `nxt` = the register set of chunk c + 1 (split into the other buffer here, then refilled with c + 3)
  auto chunk = [&](int c, auto nxt) __attribute__((always_inline)) {
    __syncthreads();                                           // chunk c is in buffer c & 1; every wave is done with the other buffer (chunk c - 1)
    load_w(c, 1, f1h, f1l);
    if (c + 1 < nch) {
      store_patch((c + 1) & 1, nxt);
      if (c + 3 < nch) load_patch(c + 3, nxt);
    }
    half_pass(c & 1, Half0{}, f0h, f0l);
    if (c + 1 < nch) load_w(c + 1, 0, f0h, f0l);
    half_pass(c & 1, Half1{}, f1h, f1l);
  };
#pragma unroll 1
  for (int c = 0; c < nch; c += 2) {
    chunk(c, Set1{});
    if (c + 1 < nch) chunk(c + 1, Set0{});
  }

  // ---- epilogue: conv_x3_kernel's, per 16-pixel row mi: lane = pixel P0 + grp * MT1 * 16 + 16 mi + pc x 4 consecutive couts ------------
  const float inv_s = a.hdr[shdr::kHdrInvScale] * ixs;
  const unsigned yr_seen = a.yr ? __hip_atomic_load(a.yr, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : 0u;
  int ep0 = (pn * NS + slice) * BN;                            // first cout of the wave's slice
  asm volatile("" : "+s"(ep0));                                // (loads below the chunk loop, not hoisted above it)
  f32x4 bias_r[NT], scale_r[NT], shift_r[NT];
#pragma unroll
  for (int ni = 0; ni < NT; ++ni) {
    const int cl = ni * 16 + 4 * fg;
    bias_r[ni] = a.bias ? *reinterpret_cast<const f32x4*>(a.bias + ep0 + cl) : (f32x4){0.f, 0.f, 0.f, 0.f};
    scale_r[ni] = a.scale ? *reinterpret_cast<const f32x4*>(a.scale + ep0 + cl) : (f32x4){1.f, 1.f, 1.f, 1.f};
    shift_r[ni] = a.scale ? *reinterpret_cast<const f32x4*>(a.shift + ep0 + cl) : (f32x4){0.f, 0.f, 0.f, 0.f};
  }
  const int Pw = P0 + grp * MT1 * 16 + pc;                     // the lane's pixel of row mi: Pw + 16 mi
  float ym = 0.0f;
  constexpr int EB = 4;                                        // rows per batch of residual loads (64 registers)
#pragma unroll
  for (int m0 = 0; m0 < MT1; m0 += EB) {
    f32x4 res_r[EB][NT];
    if (a.res) {
#pragma unroll
      for (int e = 0; e < EB; ++e)
#pragma unroll
        for (int ni = 0; ni < NT; ++ni) {
          const int P = Pw + 16 * (m0 + e);
          res_r[e][ni] = P < Ptot ? *reinterpret_cast<const f32x4*>(a.res + (size_t)P * a.res_cs + ep0 + ni * 16 + 4 * fg) : (f32x4){0.f, 0.f, 0.f, 0.f};
        }
    }
#pragma unroll
    for (int e = 0; e < EB; ++e) {
      const int P = Pw + 16 * (m0 + e);
      if (P0 + grp * MT1 * 16 + 16 * (m0 + e) >= Ptot) continue;                               // wave-uniform
#pragma unroll
      for (int ni = 0; ni < NT; ++ni) {
        f32x4 v = acc[m0 + e][ni] * inv_s;
        asm("" : "+v"(v));                                     // rounded before the bias, as in conv_x3_kernel: unfenced, the two contract into one FMA
        v += bias_r[ni];
        shdr::act_apply4<0>(v, a.act1);
        if (a.scale) v = v * scale_r[ni] + shift_r[ni];
        if (a.res) v += res_r[e][ni];
        shdr::act_apply4<0>(v, a.act2);
        if (P < Ptot) {
          *reinterpret_cast<f32x4*>(a.y + (size_t)P * a.Cout + ep0 + ni * 16 + 4 * fg) = v;
          if (a.yr) ym = fmaxf(fmaxf(fmaxf(fmaxf(ym, fabsf(v[0])), fabsf(v[1])), fabsf(v[2])), fabsf(v[3]));
        }
      }
    }
  }
  if (a.yr) shdr::range_out(a.yr, ym, lane, wave, yr_seen, x1rw);
}

// ---- wide 3 x 3 layers: one split per chunk for 128 couts ---------------------------------------------------------------------------
// conv_x3_kernel<false, 3, 3> fetches, splits and stages every 32-channel chunk of a tile once per 64-cout slice.  Here a block is the
// same 16 x 16 pixels x TWO slices (128 couts), 512 threads, ONE block per CU at two waves per SIMD: wave w takes slice w >> 2 and the
// pixel rows 4 (w & 3) .. + 3, and inside a tap does what a wave of conv_x3_kernel<false, 3, 3, false, 2> does -- the same fragment reads,
// the same 48 MFMAs per tap in the same order per accumulator, the same epilogue with n0 = 128 pn + 64 slice: the results are
// bit-identical to the sliced kernel.  Per chunk the 18 x 18 raw patch is loaded once by all 512 threads (6 float4 pieces per thread
// instead of 11) and split once; the two fp16 images are DOUBLE-buffered (2 x 41 472 B, which one block per CU leaves room for), so
// chunk c + 1 is split into the other buffer while the taps of chunk c run -- one piece between the MFMA groups of each of the taps
// 3 .. 6 (the wait of tap 2 has sat the patch out: vmcnt retires in order and the unit of tap 4 was issued behind it), the last one
// and the 32-thread remainder behind the wait that ends the chunk -- and the barrier + split phase between two chunks is gone: any time
// after a chunk's first barrier every wave is done with the other buffer, and the first barrier of the next chunk publishes it.
// Each 4-wave half stages its own slice's filter units (the packed layout read as it is, unit base wave-uniform in SGPRs) into its own
// double buffer, in the issue order of LOOK = 2 moved one tap earlier: the fragments of a tap are read from LDS during the tap before
// (see the prologue below).  115.7 KB of LDS.
// UP (the bilinear 2x prologue): the block loads the 10 x 10 low-res patch of the next chunk (two float4 per thread), parks it in the
// 12.5 KB scratch at the top of tap 3 (the barrier of tap 4 publishes it) and expands it to the 18 x 18 patch ONCE for both slices --
// conv_x3_kernel<true, 3, 3>'s expansion, the arithmetic and order of resize2x_kernel -- a piece between the MFMA groups of each of the
// taps 4 .. 7, the rest behind the chunk's last wait, into the other patch buffer.  128.5 KB of LDS.
constexpr int XW_THREADS = 512, XW_BN = 128;
constexpr long XW_UP_MIN_COUT = 128;                           // smallest Cout of an up-sampling layer on the 128-cout blocks (x3_forward)
struct XWG {
  using G = X3G<3, 3>;
  static constexpr int PJ = (G::PPIX * 8 + XW_THREADS - 1) / XW_THREADS;     // float4 pieces per thread and chunk (6; the last: 32 threads)
  static constexpr int RANGE_BYTES = 32;                       // the eight waves' output maxima
  static constexpr int LR_BYTES = LRPIX * 32 * 4;              // UP: the low-res scratch
  static constexpr int LDS_BYTES = (2 * 2 * G::PATCH_HALVES + 2 * 2 * UNIT_HALVES) * 2;
};
template <bool UP>
__global__ __launch_bounds__(XW_THREADS, 2) void conv_x3_wide_kernel(const X3Args a) {
  using G = X3G<3, 3>;
  constexpr int KH = 3, KW = 3, PWID = G::PWID, PPIX = G::PPIX, PJ = XWG::PJ, PATCH_HALVES = G::PATCH_HALVES, NTAPS = 9;
  static_assert((PJ - 1) * XW_THREADS < PPIX * 8 && PJ == 6, "every piece but the last is inside the patch for every thread");
  extern __shared__ __attribute__((aligned(16))) _Float16 xsm[];
#define patch_buf(B) (xsm + (B) * 2 * PATCH_HALVES)            /* [2 buffers][h, l][PATCH_HALVES] */
#define filt (xsm + 4 * PATCH_HALVES)                          /* [2 slices][2 buffers][UNIT_HALVES] */
#define lrs (reinterpret_cast<float*>(xsm + 4 * PATCH_HALVES + 4 * UNIT_HALVES))      /* UP: [LRPIX][32] fp32 */

  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int slice = wave >> 2, wq = wave & 3;                  // cout slice of the wave, its group of four pixel rows
  const int L = shdr::xcd_remap(blockIdx.x, a.nblk_m * a.nblk_n);
  const int pn = L % a.nblk_n;
  int pm = L / a.nblk_n;
  const int tx = pm % a.tiles_x;
  pm /= a.tiles_x;
  const int ty = pm % a.tiles_y;
  const int img = pm / a.tiles_y;
  const int n0 = pn * XW_BN + slice * BN, oh0 = ty * 16, ow0 = tx * 16;

  // ---- patch geometry (fixed per block): piece p = tid + 512 j -> (patch pixel, float4 of the 32-channel chunk) ------------------
  // UP: the low-res 10 x 10 patch instead (PL = 2 pieces per thread), parked in LDS and expanded to the 18 x 18 patch ONCE per chunk for both
  // slices with resize2x_kernel's arithmetic (conv_x3_kernel's expand_store, piece by piece)
  constexpr int PL = UP ? (LRPIX * 8 + XW_THREADS - 1) / XW_THREADS : PJ;      // loaded pieces per thread and chunk
  constexpr int T0 = UP ? 4 : 3;                               // first tap that carries a piece of the next chunk's patch
  int ppix[PL], pdst[PJ];
  int pcnt = 0;                                                // patch loads per chunk this wave is sure to issue (wave-uniform)
  if (UP) {
#pragma unroll
    for (int j = 0; j < PL; ++j) {
      const int p = tid + XW_THREADS * j;
      const int pix = p >> 3;
      const int ly = pix / LRW, lx = pix - ly * LRW;
      const int r = (oh0 >> 1) - 1 + ly, c = (ow0 >> 1) - 1 + lx;
      ppix[j] = (pix < LRPIX && (unsigned)r < (unsigned)a.Hl && (unsigned)c < (unsigned)a.Wl) ? (img * a.Hl + r) * a.Wl + c : -1;
      pcnt += __ballot(ppix[j] >= 0) != 0ull;
    }
  }
#pragma unroll
  for (int j = 0; j < (UP ? 0 : PJ); ++j) {
    const int p = tid + XW_THREADS * j;
    const int pix = p >> 3, q = p & 7;
    const int py = pix / PWID, px = pix - py * PWID;
    const int ih = oh0 + py + a.bh, iw = ow0 + px + a.bw;
    const bool ok = pix < PPIX && (unsigned)ih < (unsigned)a.Hin && (unsigned)iw < (unsigned)a.Win;
    ppix[j] = ok ? (img * a.Hin + ih) * a.Win + iw : -1;
    pdst[j] = pix < PPIX ? pix * 32 + 8 * ((q >> 1) ^ sx(px)) + 4 * (q & 1) : -1;
    pcnt += __ballot(ppix[j] >= 0) != 0ull;
  }
  pcnt = __builtin_amdgcn_readfirstlane(pcnt);
  const int nch1 = a.C1 >> 5, nch = (a.C1 + a.C2) >> 5;
  const int nunits = nch * NTAPS;
  f32x4 pr[PL];
  auto zero_patch = [&]() __attribute__((always_inline)) {     // (in front of the filter unit issued before the prefetch: see conv_x3_kernel)
#pragma unroll
    for (int j = 0; j < PL; ++j) pr[j] = (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int j = 0; j < PL; ++j) asm volatile("" : "+v"(pr[j]));
  };
  auto load_patch = [&](int c, bool zeroed) __attribute__((always_inline)) {
    if (UP) {
#pragma unroll
      for (int j = 0; j < PL; ++j) {
        const int q = (tid + XW_THREADS * j) & 7;
        if (!zeroed) pr[j] = (f32x4){0.f, 0.f, 0.f, 0.f};
        if (ppix[j] >= 0) pr[j] = *reinterpret_cast<const f32x4*>(a.x1 + (size_t)(unsigned)ppix[j] * (unsigned)a.C1 + (c << 5) + 4 * q);
      }
      return;
    }
    const bool second = c >= nch1;
    const float* src = second ? a.x2 : a.x1;
    const int Cs = second ? a.C2 : a.C1;
    const int c0 = (second ? c - nch1 : c) << 5;
#pragma unroll
    for (int j = 0; j < (UP ? 0 : PJ); ++j) {
      const int q = (tid + XW_THREADS * j) & 7;
      if (!zeroed) pr[j] = (f32x4){0.f, 0.f, 0.f, 0.f};
      if (ppix[j] >= 0) pr[j] = *reinterpret_cast<const f32x4*>(src + (size_t)(unsigned)ppix[j] * (unsigned)Cs + c0 + 4 * q);
    }
  };
  float xs = 1.0f, ixs = 1.0f;
  auto park_lr = [&]() __attribute__((always_inline)) {        // UP: registers -> LDS scratch [pixel][32]
#pragma unroll
    for (int j = 0; j < (UP ? PL : 0); ++j)
      if (tid + XW_THREADS * j < LRPIX * 8) *reinterpret_cast<f32x4*>(lrs + 4 * (tid + XW_THREADS * j)) = pr[j];
  };
  // piece j of a chunk's 18 x 18 patch -> 8 bytes in each image of buffer buf: split from the register it was loaded into, or (UP)
  // expanded from the scratch with the arithmetic and order of resize2x_kernel (horizontal first, then vertical) and split
  auto split_store = [&](int buf, int j) __attribute__((always_inline)) {
    f32x4 v = (f32x4){0.f, 0.f, 0.f, 0.f};
    int dst;
    if (UP) {
      const int r0 = (oh0 >> 1) - 1, c0 = (ow0 >> 1) - 1;
      int t0 = tid;
      asm volatile("" : "+v"(t0));                             // the geometry is computed HERE, not held in registers across the taps
      const int p = t0 + XW_THREADS * j;
      const int pix = p >> 3, q = p & 7;
      if (pix >= PPIX) return;
      const int py = pix / PWID, px = pix - py * PWID;
      const int ih = oh0 - 1 + py, iw = ow0 - 1 + px;
      if ((unsigned)ih < (unsigned)a.Hin && (unsigned)iw < (unsigned)a.Win) {
        const int mr = ih >> 1, mc = iw >> 1;
        const int ra = (ih & 1) ? mr : max(mr - 1, 0), rb = (ih & 1) ? min(mr + 1, a.Hl - 1) : mr;
        const int ca = (iw & 1) ? mc : max(mc - 1, 0), cb2 = (iw & 1) ? min(mc + 1, a.Wl - 1) : mc;
        const float* s00 = lrs + ((ra - r0) * LRW + (ca - c0)) * 32 + 4 * q;
        const int dx = (cb2 - ca) * 32, dy = (rb - ra) * LRW * 32;
        const float wx = (iw & 1) ? 0.25f : 0.75f, wy = (ih & 1) ? 0.25f : 0.75f;
        const f32x4 q00 = *reinterpret_cast<const f32x4*>(s00), q01 = *reinterpret_cast<const f32x4*>(s00 + dx);
        const f32x4 q10 = *reinterpret_cast<const f32x4*>(s00 + dy), q11 = *reinterpret_cast<const f32x4*>(s00 + dy + dx);
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const float t = q00[e] + (q01[e] - q00[e]) * wx;
          const float u = q10[e] + (q11[e] - q10[e]) * wx;
          v[e] = t + (u - t) * wy;
        }
      }
      dst = pix * 32 + 8 * ((q >> 1) ^ sx(px)) + 4 * (q & 1);
    } else {
      if (j == PJ - 1 && pdst[j] < 0) return;
      v = pr[UP ? 0 : j];
      dst = pdst[j];
    }
    unsigned h[2], l[2];
    shdr::split4(v, xs, h, l);
    *reinterpret_cast<uint2*>(patch_buf(buf) + dst) = make_uint2(h[0], h[1]);
    *reinterpret_cast<uint2*>(patch_buf(buf) + PATCH_HALVES + dst) = make_uint2(l[0], l[1]);
  };
  // ---- filter units of the wave's slice: 8 KB per tap = 512 pieces of 16 bytes, two per thread of the 4-wave half -----------------
  constexpr int FJ = 2;
  const int ht = tid & 255;
  const _Float16* wbase = a.wp + (size_t)(pn * 2 + slice) * nunits * UNIT_HALVES;
#define fsl (filt + slice * 2 * UNIT_HALVES)                   /* the two unit buffers of the wave's slice */
  int fdst[FJ];
#pragma unroll
  for (int j = 0; j < FJ; ++j) {
    const int p = ht + 256 * j;
    const int im = p >> 8, co = (p & 255) >> 2, slot = p & 3;
    fdst[j] = im * IMG_HALVES + co * 32 + 8 * (slot ^ row_swz(co));
  }
  u32x4 fr[2][FJ];
#pragma unroll
  for (int s = 0; s < 2; ++s)
#pragma unroll
    for (int j = 0; j < FJ; ++j) fr[s][j] = (u32x4){0u, 0u, 0u, 0u};
  const unsigned foff = 16u * (unsigned)ht + 2048u;
  auto issue_filt = [&](int u, int s) __attribute__((always_inline)) {                        // (past the last unit the last unit again: a static load count)
    const _Float16* ub = wbase + (size_t)(u < nunits ? u : nunits - 1) * UNIT_HALVES;
    asm volatile("global_load_dwordx4 %0, %1, %2 offset:-2048" : "+v"(fr[s][0]) : "v"(foff), "s"(ub) : "memory");
    asm volatile("global_load_dwordx4 %0, %1, %2 offset:2048" : "+v"(fr[s][1]) : "v"(foff), "s"(ub) : "memory");
  };
  constexpr int WB = FJ;                                       // loads of the next unit, always behind the one waited for
#define XW_WAIT_VM(N) asm volatile("s_waitcnt vmcnt(%0)" : : "n"(N) : "memory")
  // unit v (slot s) has landed = everything but the FJ loads of the unit behind it and the np patch loads issued after it (np < 0: the
  // prologue); then registers -> the slice's LDS buffer v & 1.  (The wait names no register, one fence ties the slot: conv_x3_kernel.)
  auto wait_store_filt = [&](int v, int s, int np, bool st) __attribute__((always_inline)) {
    static_assert(PL <= 6, "the rungs below cover up to six patch loads per thread");
    if (np < 0) XW_WAIT_VM(0);
    else if (np >= 6) XW_WAIT_VM(WB + 6);
    else if (np >= 5) XW_WAIT_VM(WB + 5);
    else if (np >= 4) XW_WAIT_VM(WB + 4);
    else if (np >= 3) XW_WAIT_VM(WB + 3);
    else if (np >= 2) XW_WAIT_VM(WB + 2);
    else if (np >= 1) XW_WAIT_VM(WB + 1);
    else XW_WAIT_VM(WB);
    asm volatile("" : "+v"(fr[s][0]), "+v"(fr[s][1]) : : "memory");
    if (st) {
#pragma unroll
      for (int j = 0; j < FJ; ++j) *reinterpret_cast<u32x4*>(fsl + (v & 1) * UNIT_HALVES + fdst[j]) = fr[s][j];
    }
  };

  f32x4 acc[MT][NT];
#pragma unroll
  for (int mi = 0; mi < MT; ++mi)
#pragma unroll
    for (int ni = 0; ni < NT; ++ni) acc[mi][ni] = (f32x4){0.f, 0.f, 0.f, 0.f};

  const int fi = lane & 15, fg = lane >> 4;
  int acol[KW], b_rd[NT];
  const int pc = pcol(fi);
#pragma unroll
  for (int kw = 0; kw < KW; ++kw) acol[kw] = (pc + kw) * 32 + 8 * (fg ^ sx(pc + kw));
#pragma unroll
  for (int ni = 0; ni < NT; ++ni) {
    const int row = ni * 16 + fi;
    b_rd[ni] = row * 32 + 8 * (fg ^ row_swz(row));
  }

  static_assert(NT == MT, "one filter fragment pair of the next tap is read in front of each MFMA group");
  load_patch(0, false);
  issue_filt(0, 0);
  issue_filt(1, 1);
  shdr::range_scale(a.xr1, a.xr2, xs, ixs);                    // (behind the first loads: the slot is a dependent scalar load)
  if (UP) {
    park_lr();
    __syncthreads();
  }
#pragma unroll
  for (int j = 0; j < PJ; ++j) {
    split_store(0, j);
    if (UP && (j & 1)) __builtin_amdgcn_sched_barrier(0);      // two pieces' scratch reads in flight, not six
  }
  wait_store_filt(0, 0, -1, true);                             // units 0 and 1 -> the two buffers
  wait_store_filt(1, 1, -1, true);
  issue_filt(2, 0);
  __syncthreads();
  // The filter fragments of a tap are read ONE TAP AHEAD, a pair in front of each MFMA group of the tap before: all eight waves leave a
  // tap's barrier together, and with the fragment reads behind it (80 KB per CU, 640 LDS cycles) no MFMA could issue until they were
  // served -- the sliced kernel's second block per CU covers that phase, one block per CU has nobody to.  So unit u + 1 is in LDS at the
  // barrier of tap u (stored at the end of tap u - 1, issued at the top of tap u - 2), and buffer u & 1, read during tap u - 1, is free.
  f16x8 wh[NT], wl[NT];
#pragma unroll
  for (int ni = 0; ni < NT; ++ni) {
    wh[ni] = *reinterpret_cast<const f16x8*>(fsl + b_rd[ni]);
    wl[ni] = *reinterpret_cast<const f16x8*>(fsl + IMG_HALVES + b_rd[ni]);
  }
#pragma unroll 1
  for (int c = 0; c < nch; ++c) {
    const bool pf = c + 1 < nch;
    const int cb = c & 1;                                      // patch buffer of this chunk; chunk c + 1 is split into cb ^ 1
    zero_patch();
    __builtin_amdgcn_sched_barrier(0);
    issue_filt(c * NTAPS + 3, 1);                              // the unit of tap 3 in FRONT of the patch loads: the waits of taps 0, 1 leave the patch in flight
    __builtin_amdgcn_sched_barrier(0);
    if (pf) load_patch(c + 1, true);
    __builtin_amdgcn_sched_barrier(0);
    const int np = pf ? pcnt : 0;
#pragma unroll
    for (int kh = 0; kh < KH; ++kh) {
#pragma unroll
      for (int kw = 0; kw < KW; ++kw) {
        const int t = kh * KW + kw;                            // the unit of tap t sits in register slot t & 1
        const int u = c * NTAPS + t;
        __syncthreads();                                       // unit u + 1 (and, at tap 0, the patch) is in LDS; filter buffer u & 1 is free
        if (t == 3) {
          // the compiler's own wait for the patch registers (a full one: it counts loads issued under branches no finer) HERE, where only
          // the unit of tap 5 is in flight, a tap old -- between the MFMA groups it would also sit out the unit issued below
#pragma unroll
          for (int j = 0; j < PL; ++j) asm volatile("" : "+v"(pr[j]));
          // UP: the low-res chunk into the scratch (last read by the expansion that ended the chunk before: every wave is past a barrier
          // since), published by the barrier of tap 4
          if (UP && pf) park_lr();
          __builtin_amdgcn_sched_barrier(0);
        }
        if (t > 0) issue_filt(u + 3, (t + 3) & 1);
        const _Float16* F = fsl + ((u + 1) & 1) * UNIT_HALVES;  // the next tap's unit
        const int rowh = (wq * MT + kh) * PWID * 32;

        f16x8 ws[NT], nwh[NT], nwl[NT], ph[2], pl[2];
        auto read_a = [&](int mi, int slot) __attribute__((always_inline)) {
          const int o = rowh + mi * PWID * 32 + acol[kw];
          ph[slot] = *reinterpret_cast<const f16x8*>(patch_buf(cb) + o);
          pl[slot] = *reinterpret_cast<const f16x8*>(patch_buf(cb) + PATCH_HALVES + o);
        };
        read_a(0, 0);
#pragma unroll
        for (int ni = 0; ni < NT; ++ni) ws[ni] = wh[ni] * (_Float16)(1.0f / 2048.0f);
#pragma unroll
        for (int mi = 0; mi < MT; ++mi) {
          if (mi + 1 < MT) read_a(mi + 1, (mi + 1) & 1);
          nwh[mi] = *reinterpret_cast<const f16x8*>(F + b_rd[mi]);
          nwl[mi] = *reinterpret_cast<const f16x8*>(F + IMG_HALVES + b_rd[mi]);
          __builtin_amdgcn_sched_barrier(0);
#pragma unroll
          for (int ni = 0; ni < NT; ++ni) acc[mi][ni] = __builtin_amdgcn_mfma_f32_16x16x32_f16(wh[ni], ph[mi & 1], acc[mi][ni], 0, 0, 0);
#pragma unroll
          for (int ni = 0; ni < NT; ++ni) acc[mi][ni] = __builtin_amdgcn_mfma_f32_16x16x32_f16(ws[ni], pl[mi & 1], acc[mi][ni], 0, 0, 0);
#pragma unroll
          for (int ni = 0; ni < NT; ++ni) acc[mi][ni] = __builtin_amdgcn_mfma_f32_16x16x32_f16(wl[ni], ph[mi & 1], acc[mi][ni], 0, 0, 0);
          __builtin_amdgcn_sched_barrier(0);
          // piece t - T0 of chunk c + 1 behind the second MFMA group of the taps 3 .. 6 (UP: 4 .. 7): it landed with the wait of tap 2
          if (mi == 1 && t >= T0 && t - T0 < PJ - 2) {
            if (pf) split_store(cb ^ 1, t - T0);
            __builtin_amdgcn_sched_barrier(0);
          }
        }
        wait_store_filt(u + 2, t & 1, t < 2 ? np : 0, u + 2 < nunits);
#pragma unroll
        for (int ni = 0; ni < NT; ++ni) {
          wh[ni] = nwh[ni];
          wl[ni] = nwl[ni];
        }
      }
    }
    // every load of the chunk has landed: the unit of the next chunk's tap 2, issued into slot 1 at tap 8, moves to slot 0
    asm volatile("s_waitcnt vmcnt(0)" : "+v"(fr[1][0]), "+v"(fr[1][1]) : : "memory");
#pragma unroll
    for (int j = 0; j < FJ; ++j) fr[0][j] = fr[1][j];
    if (pf) {
      split_store(cb ^ 1, PJ - 2);
      split_store(cb ^ 1, PJ - 1);                             // (the 32 threads that have a sixth piece)
    }
  }
#undef XW_WAIT_VM

  x3_tile_epilogue<8, false>(a, acc, img, oh0 + wq * MT, ow0 + pc, pc, fg, n0, ixs, lane, wave,
                             reinterpret_cast<unsigned*>(reinterpret_cast<char*>(xsm) + XWG::LDS_BYTES + (UP ? XWG::LR_BYTES : 0)));
}
#undef patch_buf
#undef filt
#undef fsl
#undef lrs

// ---- filter preparation ------------------------------------------------------------------------------------------------------------
// max |w| -> *out (bits): one atomicMax per wave, so launched with <= 64 blocks (2048 blocks took 50 us on a 9 MB filter, 64 take 6)
__global__ __launch_bounds__(256) void split_absmax_kernel(const float* __restrict__ w, long n, unsigned* __restrict__ out) {
  float m = 0.f;
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long)gridDim.x * 256) m = fmaxf(m, fabsf(w[i]));
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) m = fmaxf(m, __shfl_xor(m, off, 64));
  if ((threadIdx.x & 63) == 0) atomicMax(out, __float_as_uint(m));          // non-negative floats order like their bit patterns
}
// max |x| of a large tensor into *out (block-level reduction, one atomicMax per block)
__global__ __launch_bounds__(256) void x3_absmax_big_kernel(const float* __restrict__ x, long n4, unsigned* __restrict__ out) {
  __shared__ float part[4];
  float m = 0.f;
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n4; i += (long)gridDim.x * 256) {
    const f32x4 v = reinterpret_cast<const f32x4*>(x)[i];
    m = fmaxf(fmaxf(m, fmaxf(fabsf(v[0]), fabsf(v[1]))), fmaxf(fabsf(v[2]), fabsf(v[3])));
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) m = fmaxf(m, __shfl_xor(m, off, 64));
  if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = m;
  __syncthreads();
  if (threadIdx.x == 0) atomicMax(out, __float_as_uint(fmaxf(fmaxf(part[0], part[1]), fmaxf(part[2], part[3]))));
}
// packed[nb][u = chunk * taps + tap][image][co][k]: w * x2-scale * 2^S split into wh, wl
// taps of the packed filter = the sub-filter w[p0 + step * a][q0 + step * b], a < TH, b < TW, of a KWF-wide filter
__global__ __launch_bounds__(256) void x3_pack_kernel(const float* __restrict__ w, float* __restrict__ hdr, _Float16* __restrict__ out, int Ct,
                                                      int C1, int Cout, float x2_scale, int KWF, int TH, int TW, int p0, int q0, int step) {
  float inv;
  const float s = shdr::weight_scale(hdr, x2_scale, inv);    // max |w'| in [2^13, 2^14)
  if (blockIdx.x == 0 && threadIdx.x == 0) hdr[shdr::kHdrInvScale] = inv;
  const int ntaps = TH * TW;
  const int nunits = (Ct >> 5) * ntaps;
  const long total = (long)((Cout + 63) / 64) * nunits * 64 * 32;      // (a 32-cout layer fills half of its one 64-cout slice with zeros)
  for (long e = (long)blockIdx.x * 256 + threadIdx.x; e < total; e += (long)gridDim.x * 256) {
    const int k = (int)(e & 31), co = (int)((e >> 5) & 63);
    const long t = e >> 11;
    const int u = (int)(t % nunits), nb = (int)(t / nunits);
    const int chunk = u / ntaps, t2 = u - ntaps * chunk;
    const int ta = t2 / TW, tb = t2 - TW * ta;
    const int tap = (p0 + step * ta) * KWF + (q0 + step * tb);
    const int ch = chunk * 32 + k;
    float v = nb * 64 + co < Cout ? w[((size_t)tap * Ct + ch) * Cout + nb * 64 + co] * s : 0.0f;
    if (ch >= C1) v *= x2_scale;
    const _Float16 h = (_Float16)v;
    _Float16* o = out + ((size_t)(nb * nunits + u) * 2) * IMG_HALVES + co * 32 + k;
    o[0] = h;
    o[IMG_HALVES] = (_Float16)(v - (float)h);
  }
}

}  // namespace

void shdr::launch_split_absmax(const float* w, long n, unsigned* out, hipStream_t st) {
  hipLaunchKernelGGL(split_absmax_kernel, dim3(shdr::stream_grid(n) < 64 ? shdr::stream_grid(n) : 64), dim3(256), 0, st, w, n, out);
}

namespace {

struct X3Phase { int th, tw, p0, q0, step, bh, bw; };
// 3 x 3 / stride 1: one "phase" (all nine taps).  7 x 7 / stride 2 (linearization_net.py:91): input pixels of one row / column parity
// meet the filter taps of one parity only, so the layer is the sum of four stride-1 correlations of the parity-subsampled input with
// the 4 x 4, 4 x 3, 3 x 4 and 3 x 3 sub-filters -- exactly the 49 taps, the four phases of the MP kernel.
int x3_phases(const shdr_conv2d_desc* d, X3Phase ph[4]) {
  if (d->stride == 1 || d->KH == 1) {
    // 3 x 3 (pad 1) or 1 x 1 (pad 0): all taps in one launch; the 1 x 1 / stride-2 layer reads input pixel (2 oh, 2 ow)
    ph[0] = X3Phase{d->KH, d->KW, 0, 0, d->stride, -d->pad_t, -d->pad_l};
    return 1;
  }
  int n = 0;
  for (int p0 = 0; p0 < 2; ++p0)
    for (int q0 = 0; q0 < 2; ++q0) ph[n++] = X3Phase{(d->KH - p0 + 1) / 2, (d->KW - q0 + 1) / 2, p0, q0, 2, p0 - d->pad_t, q0 - d->pad_l};
  return n;
}
inline int64_t x3_phase_floats(const X3Phase& p, int Ct, int Cout) { return shdr::kSplitHeaderFloats + (int64_t)p.th * p.tw * Ct * ((Cout + 63) / 64 * 64); }    // two fp16 images

template <bool UP, int KH, int KW, bool MP, int LOOK>
int launch_x3_look(const X3Args& a, hipStream_t st) {
  constexpr int lds = (UP ? X3G<KH, KW>::LDS_BYTES_UP : X3G<KH, KW>::LDS_BYTES) + X3G<KH, KW>::RANGE_BYTES;
  if (int e = shdr::dynamic_lds<&conv_x3_kernel<UP, KH, KW, MP, LOOK>>(lds)) return e;
  const long nblk = (long)a.nblk_m * a.nblk_n;
  if (nblk > 0x7fffffffL) return shdr::fail(SHDR_E_SHAPE, "conv2d_x3: grid of %ld blocks", nblk);
  hipLaunchKernelGGL((conv_x3_kernel<UP, KH, KW, MP, LOOK>), dim3((unsigned)nblk), dim3(256), lds, st, a);
  return shdr::check_launch("conv_x3_kernel");
}
// SHDR_X3_LOOK=1|2: the filter look-ahead (A/B and the second arm of tests/test_gpu_x3_prefetch.py; default 2, the faster by wall time).
template <bool UP, int KH, int KW, bool MP = false>
int launch_x3(const X3Args& a, hipStream_t st) {
  int look = 2;
  if (const char* e = SHDR_ENV("SHDR_X3_LOOK")) look = atoi(e);
  // LOOK = 2 is built for the nine-tap kernels (3 x 3, with and without the up-sampling prologue): the stem is out of registers at
  // LOOK = 1 and a 1 x 1 chunk has no second tap
  constexpr bool look2 = KH == 3 && KW == 3 && !MP;
  if (look >= 2 && look2) return launch_x3_look<UP, KH, KW, MP, look2 ? 2 : 1>(a, st);
  return launch_x3_look<UP, KH, KW, MP, 1>(a, st);
}

// conv_x3_1x1_kernel: 256 couts per block where Cout allows it, else 128 (Cout 64 and 32 keep conv_x3_kernel<false, 1, 1>: its block
// already holds every cout of the layer and splits a chunk once)
int launch_x3_1x1(const X3Args& a0, hipStream_t st) {
  X3Args a = a0;
  const long npix = (long)a.N * a.H * a.W;
  const int ns = a.Cout % 256 == 0 ? 4 : 2;
  a.nblk_m = (int)((npix + X1_BP - 1) / X1_BP);
  a.nblk_n = a.Cout / (64 * ns);
  const long nblk = (long)a.nblk_m * a.nblk_n;
  if (nblk > 0x7fffffffL) return shdr::fail(SHDR_E_SHAPE, "conv2d_x3: grid of %ld blocks", nblk);
  if (ns == 4) hipLaunchKernelGGL((conv_x3_1x1_kernel<4>), dim3((unsigned)nblk), dim3(256), 0, st, a);
  else hipLaunchKernelGGL((conv_x3_1x1_kernel<2>), dim3((unsigned)nblk), dim3(256), 0, st, a);
  return shdr::check_launch("conv_x3_1x1_kernel");
}

// conv_x3_wide_kernel: 128 couts per block, half the blocks of the sliced grid
template <bool UP>
int launch_x3_wide(const X3Args& a0, hipStream_t st) {
  X3Args a = a0;
  a.nblk_n = a.Cout / XW_BN;
  constexpr int lds = XWG::LDS_BYTES + (UP ? XWG::LR_BYTES : 0) + XWG::RANGE_BYTES;
  if (int e = shdr::dynamic_lds<&conv_x3_wide_kernel<UP>>(lds)) return e;
  const long nblk = (long)a.nblk_m * a.nblk_n;
  if (nblk > 0x7fffffffL) return shdr::fail(SHDR_E_SHAPE, "conv2d_x3: grid of %ld blocks", nblk);
  hipLaunchKernelGGL((conv_x3_wide_kernel<UP>), dim3((unsigned)nblk), dim3(XW_THREADS), lds, st, a);
  return shdr::check_launch("conv_x3_wide_kernel");
}

}  // namespace

extern "C" int shdr_conv2d_x3_ok_f32(const shdr_conv2d_desc* d) {
  // Cout 32 (the 64 -> 32 and 32 + 32 -> 32 decoder layers of the U-Nets, dequantization_net.py:17-29): one 64-cout slice, half of it zero
  // filter columns that are neither biased nor stored -- twice the arithmetic of the layer and still 1.3x the exact fp32 kernel
  if (!d || d->C1 <= 0 || d->C1 % 32 || d->C2 % 32 || (d->Cout % 64 && (d->Cout != 32 || d->stride != 1 || SHDR_ENV("SHDR_NO_X3_COUT32")))) return 0;
  const int cv = d->cout_valid > 0 ? d->cout_valid : d->Cout;
  if (cv != d->Cout || d->w_batch_stride != 0 || d->y_pix_stride > 1) return 0;
  if ((long)d->N * d->H * d->W * (d->C1 > d->C2 ? d->C1 : d->C2) >= (1L << 31)) return 0;
  if (SHDR_ENV("SHDR_NO_X3")) return 0;
  if (d->act1 == SHDR_ACT_TANH || d->act2 == SHDR_ACT_TANH) return 0;      // no wide layer of the networks has one: tanhf is not compiled in (act_apply4)
  if (d->stride == 1) {
    const bool k3 = d->KH == 3 && d->KW == 3 && d->pad_t == 1 && d->pad_l == 1;
    // 1 x 1 layers (the skip layers of hallucination_net.py:93-107 on tf.concat of two sources, the bottleneck convs of the ResNet
    // blocks): one tap per chunk, so the patch split is not amortised over nine taps -- still 2-3x the fp32-MFMA kernel from K = 256 on
    int k1_min = 64;                                           // (measured, tools/one_1x1.py: 64 -> 256 at 16 x 128^2 0.171 -> 0.129 ms, 128 -> 512 at 64^2 0.119 -> 0.073)
    if (const char* e = SHDR_ENV("SHDR_X3_1X1_MIN_K")) k1_min = atoi(e);
    const bool k1 = d->KH == 1 && d->KW == 1 && d->pad_t == 0 && d->pad_l == 0 && d->C1 + d->C2 >= k1_min && SHDR_ENV("SHDR_NO_X3_1X1") == nullptr;
    if (!(k3 || k1) || d->Ho != d->H || d->Wo != d->W) return 0;
  } else if (d->stride == 2 && d->KH == 1 && d->KW == 1) {
    // the 1 x 1 / stride-2 projections of the ResNet blocks (linearization_net.py:6-48, res4): the 1 x 1 kernel on every other input pixel
    if (d->pad_t != 0 || d->pad_l != 0 || d->C2 != 0 || d->prologue != SHDR_PROLOGUE_NONE || d->Ho != (d->H + 1) / 2 || d->Wo != (d->W + 1) / 2 ||
        d->C1 < 64 || SHDR_ENV("SHDR_NO_X3_1X1") || SHDR_ENV("SHDR_NO_X3_STRIDE2"))
      return 0;
  } else {
    // the 7 x 7 / stride-2 stem with TF SAME padding (one source, no prologue)
    int ho = 0, wo = 0, pt = 0, pl = 0;
    shdr_same_pad(d->H, 7, 2, &ho, &pt);
    shdr_same_pad(d->W, 7, 2, &wo, &pl);
    if (d->stride != 2 || d->KH != 7 || d->KW != 7 || d->C2 != 0 || d->prologue != SHDR_PROLOGUE_NONE || d->Ho != ho || d->Wo != wo || d->pad_t != pt ||
        d->pad_l != pl || SHDR_ENV("SHDR_NO_X3_STRIDE2"))
      return 0;
  }
  // enough blocks to fill the chip: the deepest, smallest maps stay on the fused Winograd kernel (8 x 16 tiles)
  const long blocks = (long)d->N * ((d->Ho + 15) / 16) * ((d->Wo + 15) / 16) * ((d->Cout + 63) / 64);
  long min_blocks = 192;          // measured (tools/dbg/x3_threshold.py): 256 blocks 1.24-1.28x the fused Winograd kernel, 128 blocks 0.75x
  if (const char* e = SHDR_ENV("SHDR_X3_MIN_BLOCKS")) min_blocks = atol(e);
  return blocks >= min_blocks ? 1 : 0;
}

extern "C" int64_t shdr_conv2d_x3_filter_elems_f32(const shdr_conv2d_desc* d) {
  if (!d || d->C1 <= 0 || (d->C1 + d->C2) % 32 || (d->Cout % 64 && d->Cout != 32) || (d->stride != 1 && d->stride != 2)) return -1;
  X3Phase ph[4];
  const int n = x3_phases(d, ph);
  int64_t total = 0;
  for (int i = 0; i < n; ++i) total += x3_phase_floats(ph[i], d->C1 + d->C2, d->Cout);
  return total;
}

extern "C" int shdr_conv2d_x3_prepare_filter_f32(const shdr_conv2d_desc* d, const float* w, float* prepared, void* stream) {
  return shdr_conv2d_x3_prepare_filter_premax_f32(d, w, prepared, 0, stream);
}
extern "C" int shdr_conv2d_x3_prepare_filter_premax_f32(const shdr_conv2d_desc* d, const float* w, float* prepared, int premax, void* stream) {
  SHDR_REQUIRE(d && w && prepared, SHDR_E_NULL, "conv2d_x3_prepare_filter: null pointer");
  const int Ct = d->C1 + d->C2;
  SHDR_REQUIRE(Ct > 0 && Ct % 32 == 0 && d->C1 % 32 == 0 && d->Cout > 0 && (d->Cout % 64 == 0 || d->Cout == 32), SHDR_E_SHAPE,
               "conv2d_x3_prepare_filter: need C %% 32 == 0, Cout %% 64 == 0 (or Cout 32)");
  SHDR_REQUIRE(shdr::aligned16(prepared), SHDR_E_ALIGN, "conv2d_x3_prepare_filter: prepared must be 16-byte aligned");
  hipStream_t st = shdr::stream_of(stream);
  const float x2s = d->C2 > 0 ? d->x2_scale : 1.0f;
  X3Phase ph[4];
  const int n = x3_phases(d, ph);
  const long nw = (long)d->KH * d->KW * Ct * d->Cout;
  float* out = prepared;
  SHDR_REQUIRE(!premax || n == 1, SHDR_E_SHAPE, "conv2d_x3_prepare_filter: premax is for single-phase (stride-1) layers");
  for (int i = 0; i < n; ++i) {
    if (!premax) {
      if (hipMemsetAsync(out, 0, shdr::kSplitHeaderFloats * sizeof(float), st) != hipSuccess) return shdr::fail(SHDR_E_LAUNCH, "conv2d_x3_prepare_filter: memset");
      shdr::launch_split_absmax(w, nw, reinterpret_cast<unsigned*>(out) + shdr::kHdrMaxW, st);
    }
    const long np = (long)ph[i].th * ph[i].tw * Ct * ((d->Cout + 63) / 64 * 64);
    hipLaunchKernelGGL(x3_pack_kernel, dim3(shdr::stream_grid(np)), dim3(256), 0, st, w, out, reinterpret_cast<_Float16*>(out + shdr::kSplitHeaderFloats), Ct,
                       d->C1, d->Cout, x2s, d->KW, ph[i].th, ph[i].tw, ph[i].p0, ph[i].q0, ph[i].step);
    out += x3_phase_floats(ph[i], Ct, d->Cout);
  }
  return shdr::check_launch("conv2d_x3_prepare_filter");
}

// max |x| of a tensor, atomicMax-ed into a RANGE SLOT (a device word holding the bit pattern of a non-negative float; the caller zeroes
// it, e.g. one memset over a slab of slots per step).  The slot feeds x1_range / x2_range of the ranged convolution calls.
extern "C" int shdr_absmax_f32(const float* x, int64_t n, float* range, void* stream) {
  SHDR_REQUIRE(x && range, SHDR_E_NULL, "absmax: null pointer");
  SHDR_REQUIRE(n > 0, SHDR_E_SHAPE, "absmax: n must be positive");
  hipStream_t st = shdr::stream_of(stream);
  unsigned* slot = reinterpret_cast<unsigned*>(range);
  const int64_t n4 = shdr::aligned16(x) ? n / 4 : 0;
  if (n4 > 0) {
    int grid = shdr::stream_grid(n4);
    if (grid > 1024) grid = 1024;
    hipLaunchKernelGGL(x3_absmax_big_kernel, dim3(grid), dim3(256), 0, st, x, (long)n4, slot);
  }
  if (n - 4 * n4 > 0) shdr::launch_split_absmax(x + 4 * n4, (long)(n - 4 * n4), slot, st);      // the tail (n4 > 0: at most three elements, one block)
  return shdr::check_launch("absmax");
}

// the range slot inside a prepared filter's header (kHdrInputRange): the low-level protocol of desc.prologue = SHDR_PROLOGUE_RANGE_SCALE
extern "C" int shdr_conv2d_x3_input_absmax_f32(const float* x, int64_t n, float* prepared, void* stream) {
  SHDR_REQUIRE(x && prepared, SHDR_E_NULL, "conv2d_x3_input_absmax: null pointer");
  SHDR_REQUIRE(n > 0 && n % 4 == 0 && shdr::aligned16(x), SHDR_E_SHAPE, "conv2d_x3_input_absmax: n must be a positive multiple of 4, x 16-byte aligned");
  return shdr_absmax_f32(x, n, prepared + shdr::kHdrInputRange, stream);
}

static int x3_forward(const shdr_conv2d_desc* d, const float* x1, const float* x2, const float* prepared, const float* bias,
                      const float* scale, const float* shift, const float* residual, float* y, float* y_pool, const float* proj, float* y_proj,
                      const float* x1_range, const float* x2_range, float* y_range, void* stream) {
  SHDR_REQUIRE(d && x1 && prepared && (y || y_pool || y_proj), SHDR_E_NULL, "conv2d_x3: null desc/x1/filter or no output");
  SHDR_REQUIRE((proj == nullptr) == (y_proj == nullptr), SHDR_E_NULL, "conv2d_x3: proj and y_proj come together");
  SHDR_REQUIRE(!proj || (d->Cout == 64 && d->stride == 1 && shdr::aligned16(proj)), SHDR_E_SHAPE,
               "conv2d_x3: the projected output takes a stride-1 layer with 64 output channels (one cout slice per block) and a 16-byte aligned map");
  SHDR_REQUIRE(!y_pool || (d->Ho % 2 == 0 && d->Wo % 2 == 0 && shdr::aligned16(y_pool)), SHDR_E_SHAPE, "conv2d_x3: the fused 2x2 max-pool needs even Ho, Wo");
  const bool up = d->prologue == SHDR_PROLOGUE_BILINEAR2X, rs = d->prologue == SHDR_PROLOGUE_RANGE_SCALE;
  SHDR_REQUIRE(d->prologue == SHDR_PROLOGUE_NONE || rs || (up && d->stride == 1 && d->C2 == 0 && d->H % 2 == 0 && d->W % 2 == 0), SHDR_E_SHAPE,
               "conv2d_x3: the bilinear 2x prologue takes a stride-1 layer, one source and even (up-sampled) H, W");
  SHDR_REQUIRE(shdr_conv2d_x3_ok_f32(d), SHDR_E_SHAPE, "conv2d_x3: layer shape not taken by this kernel");
  SHDR_REQUIRE((d->C2 == 0) == (x2 == nullptr), SHDR_E_NULL, "conv2d_x3: x2 must be given iff C2 > 0");
  SHDR_REQUIRE((scale == nullptr) == (shift == nullptr), SHDR_E_NULL, "conv2d_x3: scale and shift come together");
  SHDR_REQUIRE(shdr::aligned16(x1) && (!x2 || shdr::aligned16(x2)) && shdr::aligned16(prepared) && (!y || shdr::aligned16(y)) &&
                   (!bias || shdr::aligned16(bias)) && (!scale || (shdr::aligned16(scale) && shdr::aligned16(shift))),
               SHDR_E_ALIGN, "conv2d_x3: tensors must be 16-byte aligned");
  SHDR_REQUIRE(!x2 || ((x1_range == nullptr) == (x2_range == nullptr)), SHDR_E_NULL, "conv2d_x3: give the range of both sources or of neither");
  X3Args a{};
  a.x1 = x1; a.x2 = x2 ? x2 : x1;
  a.bias = bias; a.scale = scale; a.shift = shift; a.y = y; a.yp = y_pool;
  a.pool_avg = d->pool == SHDR_POOL_AVG;
  a.N = d->N; a.H = d->Ho; a.W = d->Wo; a.C1 = d->C1; a.C2 = d->C2; a.Cout = d->Cout;
  a.Hin = d->H; a.Win = d->W;
  a.Hl = d->H / 2; a.Wl = d->W / 2;
  a.tiles_x = (a.W + 15) / 16;
  a.tiles_y = (a.H + 15) / 16;
  a.nblk_m = a.N * a.tiles_x * a.tiles_y;
  a.nblk_n = (a.Cout + 63) / 64;
  a.act1 = d->act1; a.act2 = d->act2;
  a.xr1 = reinterpret_cast<const unsigned*>(x1_range);
  a.xr2 = reinterpret_cast<const unsigned*>(x2 ? x2_range : nullptr);
  a.yr = reinterpret_cast<unsigned*>(y_range);
  a.proj = proj; a.yproj = y_proj;
  SHDR_REQUIRE(!residual || (d->stride == 1 && d->res_cstride >= d->Cout && d->res_cstride % 4 == 0 && shdr::aligned16(residual) && !y_pool && !proj), SHDR_E_SHAPE,
               "conv2d_x3: the residual takes a stride-1 layer, res_cstride >= Cout (a multiple of 4), a 16-byte aligned tensor, no pooled / projected output");
  a.res = residual; a.res_cs = d->res_cstride;
  hipStream_t st = shdr::stream_of(stream);
  X3Phase ph[4];
  const int n = x3_phases(d, ph);
  const int Ct = d->C1 + d->C2;
  a.hdr = prepared;
  a.wp = reinterpret_cast<const _Float16*>(prepared + shdr::kSplitHeaderFloats);
  if (rs && !x1_range) a.xr1 = reinterpret_cast<const unsigned*>(prepared) + shdr::kHdrInputRange;      // the header-slot protocol (shdr_conv2d_x3_input_absmax_f32)
  a.in_s = ph[0].step; a.bh = ph[0].bh; a.bw = ph[0].bw;
  if (n == 4) {
    // the stride-2 stem in ONE launch: the phases' packed sub-filters share the scale 2^S (each header's maximum is taken over the whole
    // filter), the partial sums stay in registers
    const float* pk = prepared;
    a.nphase = 4;
    for (int i = 0; i < 4; ++i) {
      SHDR_REQUIRE(ph[i].th <= 4 && ph[i].tw <= 4 && ph[i].step == ph[0].step, SHDR_E_SHAPE, "conv2d_x3: unexpected phase geometry");
      a.pth[i] = ph[i].th; a.ptw[i] = ph[i].tw; a.pbh[i] = ph[i].bh; a.pbw[i] = ph[i].bw;
      a.pwp[i] = reinterpret_cast<const _Float16*>(pk + shdr::kSplitHeaderFloats);
      pk += x3_phase_floats(ph[i], Ct, d->Cout);
    }
    return launch_x3<false, 4, 4, true>(a, st);
  }
  if (ph[0].th == 3 && ph[0].tw == 3) {
    // the 128-cout blocks (conv_x3_wide_kernel<UP>) take the stride-1 layers with a multiple of 128 couts and at least 256 blocks: with
    // the up-sampling prologue from 128 couts on, plain from 512 couts on; a projected output (Cout = 64) and SHDR_X3_SLICED=1 (A/B,
    // tests/test_gpu_x3_wide.py) run the 64-cout kernel.  Measured (tools/x3_wide_ab.py, profiles/r06_x3_wide_layers_ab.txt; sliced / wide
    // by the medians of five rounds, batch 16 and 8):
    //   up-sampling, >= 256 blocks: 64^2 x2 512 -> 256 1.109 and 1.102, 128^2 x2 256 -> 128 1.089 and 1.088, 32^2 x2 256 -> 128 1.121 at
    //   batch 16 -- the ranges apart everywhere (the expansion and the split run once per 128 couts, under the MFMAs);
    //   plain, 512 couts: 64^2 1.018 - 1.020 and 1.029 - 1.033, 32^2 at batch 16 (256 blocks) 1.053, the ranges apart (an earlier session
    //   on another box: 64^2 256 -> 512 at batch 16 1.017 with the ranges overlapping);
    //   plain, 256 couts: 0.985 - 1.012 and 1.002 - 1.018, 128 couts: 0.980 - 1.039 and 0.960 - 0.994, ranges overlapping: they stay sliced;
    //   128 blocks and fewer (half the CUs idle): 0.74 - 0.87, plain and up-sampling alike.
    long wide_min_blocks = 256, wide_min_cout = up ? XW_UP_MIN_COUT : 512;
    if (const char* e = SHDR_ENV("SHDR_X3_WIDE_MIN_BLOCKS")) wide_min_blocks = atol(e);
    if (const char* e = SHDR_ENV("SHDR_X3_WIDE_MIN_COUT")) wide_min_cout = atol(e);
    const bool wide = d->stride == 1 && d->Cout % XW_BN == 0 && d->Cout >= wide_min_cout && !proj &&
                      (long)a.nblk_m * (d->Cout / XW_BN) >= wide_min_blocks && SHDR_ENV("SHDR_X3_SLICED") == nullptr;
    return wide ? (up ? launch_x3_wide<true>(a, st) : launch_x3_wide<false>(a, st)) : up ? launch_x3<true, 3, 3>(a, st) : launch_x3<false, 3, 3>(a, st);
  }
  if (ph[0].th == 1 && ph[0].tw == 1) {
    // the wide-block kernel takes 128- and 256-cout multiples with a plain output; a pooled or projected output (no network has one
    // on a 1 x 1 layer), the narrow layers and SHDR_X3_1X1_SLICED=1 (A/B) run the 64-cout instantiation
    const bool wide = d->Cout % 128 == 0 && y && !y_pool && !proj && !up && SHDR_ENV("SHDR_X3_1X1_SLICED") == nullptr;
    return wide ? launch_x3_1x1(a, st) : launch_x3<false, 1, 1>(a, st);
  }
  return shdr::fail(SHDR_E_SHAPE, "conv2d_x3: no kernel for a %d x %d layer", ph[0].th, ph[0].tw);
}

extern "C" int shdr_conv2d_fwd_x3_ranged_f32(const shdr_conv2d_desc* d, const float* x1, const float* x2, const float* prepared, const float* bias,
                                             const float* scale, const float* shift, float* y, float* y_pool, const float* x1_range,
                                             const float* x2_range, float* y_range, void* stream) {
  SHDR_REQUIRE(y || y_pool, SHDR_E_NULL, "conv2d_x3: neither y nor y_pool");
  return x3_forward(d, x1, x2, prepared, bias, scale, shift, nullptr, y, y_pool, nullptr, nullptr, x1_range, x2_range, y_range, stream);
}

// The same with a residual: y = act2(affine(act1(conv + bias)) + residual), residual [N,Ho,Wo,res_cstride] -- the joins of the ResNet
// blocks (linearization_net.py:6-48: relu(norm(conv) + shortcut)) on the 1x1 layers this kernel takes
extern "C" int shdr_conv2d_fwd_x3_residual_f32(const shdr_conv2d_desc* d, const float* x1, const float* x2, const float* prepared, const float* bias,
                                               const float* scale, const float* shift, const float* residual, float* y, const float* x1_range,
                                               const float* x2_range, float* y_range, void* stream) {
  SHDR_REQUIRE(y, SHDR_E_NULL, "conv2d_x3: null y");
  return x3_forward(d, x1, x2, prepared, bias, scale, shift, residual, y, nullptr, nullptr, nullptr, x1_range, x2_range, y_range, stream);
}

// The same launch with a PROJECTED output: y_proj[n,h,w,j] = sum_c proj[j][c] * y[n,h,w,c] (proj: [3][64] floats, j < 3), written from
// the epilogue that holds y in registers; y itself (and / or its pooled copy) is written only if asked for.  The tail of the
// Hallucination-Net (hallucination_net.py:179-185: the 1x1 skip layer s1 on concat[u1, d1 / 255] followed by the 1x1 conv2 -- two linear
// maps in a row) needs nothing but such a projection of u1's and of d1's 64 channels: their full-resolution tensors (1 GB each at
// 16 x 512^2) are then never written nor read back.
extern "C" int shdr_conv2d_fwd_x3_projected_f32(const shdr_conv2d_desc* d, const float* x1, const float* x2, const float* prepared,
                                                const float* bias, const float* scale, const float* shift, const float* proj, float* y_proj,
                                                float* y, float* y_pool, const float* x1_range, const float* x2_range, float* y_range,
                                                void* stream) {
  SHDR_REQUIRE(proj && y_proj, SHDR_E_NULL, "conv2d_x3_projected: null proj / y_proj");
  return x3_forward(d, x1, x2, prepared, bias, scale, shift, nullptr, y, y_pool, proj, y_proj, x1_range, x2_range, y_range, stream);
}

// The low-level entry point without range slots: the input is split as it stands (|x| must stay inside the fp16 range) unless
// desc.prologue = SHDR_PROLOGUE_RANGE_SCALE names the header slot written by shdr_conv2d_x3_input_absmax_f32.  Hosts go through
// shdr_conv2d_fwd_prepared_f32 / _ranged_f32, which never run a split-operand launch without a range.
extern "C" int shdr_conv2d_fwd_x3_f32(const shdr_conv2d_desc* d, const float* x1, const float* x2, const float* prepared, const float* bias,
                                      const float* scale, const float* shift, float* y, float* y_pool, void* stream) {
  return shdr_conv2d_fwd_x3_ranged_f32(d, x1, x2, prepared, bias, scale, shift, y, y_pool, nullptr, nullptr, nullptr, stream);
}

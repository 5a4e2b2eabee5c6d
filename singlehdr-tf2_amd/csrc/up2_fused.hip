// Conv2D 3x3 (SAME, stride 1) of tf.image.resize(x, 2x, BILINEAR) for 64, 32 or 16 output channels in ONE launch: the low-res channel mix of
// up2_lowres.hip (z_t = x W[t] for the nine taps) and its stencil pass fused, so that the tap planes z -- 2.7 GB for the Hallucination-Net's
// u1 at batch 16, written and read back by the two-launch form -- never leave the CU, and with a projected output neither does the
// 64-channel result.
//
// Block = one low-res PATCH of R rows x 16 columns (clamped at the image border), whose interior (R - 2) x 14 it finishes: 4 waves, wave
// cw takes the couts 16 cw .. 16 cw + 15 of all R patch rows.  The patch (<= 128 channels) is fetched and split ONCE into two fp16 images
// resident in LDS; only the filter fragments stream (from L2 into registers, the packed filter of up2_lowres read as it is: slice t of the
// [Cin, 9 x 64 (+ pad)] 1x1 filter is tap t).  An MFMA pixel tile is the 16 columns of one patch row, D[cout][pixel]: a lane holds patch
// column lane & 15 and four couts, so
//   - the horizontal fold needs the neighbouring LANES of a 16-lane row: DPP row shifts, no LDS;
//   - the vertical fold is between accumulators of the same lane;
//   - lanes 0 and 15 and patch rows 0 and R - 1 are halo.
// The GEMM runs as three passes over ty (3 R accumulators live instead of 9 R); the vertical fold's terms come in ty order, so the passes
// keep the stencil pass's summation order.  Registers at R = 8: 96 tap accumulators + 96 output sums + 36 of the three taps' filter
// fragments (wh, wh 2^-11, wl) + the patch row in flight = the 256 of two waves per SIMD (eight spilled, outside the loops), so the
// fragments of the next chunk are NOT prefetched: the other wave of the SIMD covers their L2 latency.  69.6 KB of LDS, two blocks per CU.
// Arithmetic: z has the bits of conv_x3_1x1_kernel (same 2^T, same packed filter under one 2^S,
// per accumulator the chunks in order and per chunk wh xh, (wh 2^-11) xl, wl xh, then 2^-S 2^-T), the folds are the explicit multiply / FMA
// sequences of up2_lowres_stencil_kernel with its border rules, the epilogue is its `finish`: y is bit-identical to
// shdr_conv2d_fwd_up2_lowres_f32.  A/B switch SHDR_NO_UP2_FUSED=1.
// The text above is the 64-cout form (CW = 4).  With 32 or 16 couts (the `up` blocks of the Dequantization-Net; A/B switch
// SHDR_NO_UP2_NARROW=1) a patch takes CW = 2 or 1 waves, each doing exactly the work above for its 16 couts, and the four waves of a block
// finish 2 or 4 patches, each with its own pair of images in LDS.
#include <hip/hip_fp16.h>
#include <stdlib.h>

#include <type_traits>

#include "split.h"

namespace {

using shdr::fma4;
using shdr::fma4v;
using shdr::mul4;

constexpr int UF_IMG_HALVES = 64 * 32, UF_UNIT_HALVES = 2 * UF_IMG_HALVES;      // one (slice, chunk) unit: wh, wl images [64 couts][32 channels]
constexpr int UF_R = 8;                                         // patch rows: interior 6 x 14 of a 8 x 16 patch
constexpr int UF_COLS = 14;                                     // interior columns of the 16 lanes
constexpr int UF_MAX_CIN = 128;
constexpr int UF_THREADS = 256;
// halves per patch pixel of an instantiation that holds up to CMAX input channels: 16 bytes of padding spread the pixels over the banks;
// none at 32 channels, where four patches with it would be 80 KB + the static range words, past two blocks per CU (reads 2-way, 1/4 of
// the MFMA time of a patch row)
constexpr int uf_stride(int CMAX) { return CMAX == 32 ? 32 : CMAX + 8; }

struct UpFusedArgs {
  const float* x;          // [N, h, w, C1] low-res
  const _Float16* wp;      // packed 1x1 filter [9 (+ pad) slices][C1 / 32 chunks][wh, wl][64][32]
  const float* hdr;        // hdr[kHdrInvScale] = 2^-S
  const float* bias;
  const float* scale;
  const float* shift;
  const float* proj;       // [3][64] or null
  float* y;                // [N, 2h, 2w, 64] or null
  float* yproj;            // [N, 2h, 2w, 3] or null
  const unsigned* xr;      // the input's range slot
  unsigned* yr;            // the output's, or null
  int N, h, w, C1, nty, ntx, act1, act2;
  int npatch;              // N nty ntx
};

// the value of the lane one to the left / right inside the 16-lane row (DPP row_shr:1 / row_shl:1; the row's first / last lane reads zero:
// those are the halo lanes, whose sums are not used)
__device__ __forceinline__ f32x4 from_left(f32x4 a) {
  f32x4 r;
#pragma unroll
  for (int e = 0; e < 4; ++e) r[e] = __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(a[e]), 0x111, 0xf, 0xf, true));
  return r;
}
__device__ __forceinline__ f32x4 from_right(f32x4 a) {
  f32x4 r;
#pragma unroll
  for (int e = 0; e < 4; ++e) r[e] = __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(a[e]), 0x101, 0xf, 0xf, true));
  return r;
}


// CW = Cout / 16 waves finish one patch (wave cw of them the couts 16 cw .. 16 cw + 15), so the four waves of a block finish PPB = 4 / CW
// patches, each with its own pair of images in LDS; a patch past the end of the grid leaves its waves idle (they still reach every barrier).
// CMAX: the most input channels the images hold.  Per wave the work is that of CW = 4 whatever CW is.
template <int R, int CW, int CMAX>
__global__ __launch_bounds__(UF_THREADS, 2) void up2_fused_kernel(const UpFusedArgs a) {
  constexpr int UF_STRIDE = uf_stride(CMAX);
  constexpr int COUT = 16 * CW, PPB = 4 / CW, GT = 64 * CW;      // couts; patches per block; threads per patch
  constexpr int NPIX = 16 * R, IMG = NPIX * UF_STRIDE;           // halves of one fp16 image of the patch
  constexpr int RO = R - 2;                                      // interior rows
  extern __shared__ __attribute__((aligned(16))) _Float16 fsm_all[];      // [patch][h, l][NPIX][UF_STRIDE]; behind the GEMM: the waves' projected partial sums

  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int ps = PPB == 1 ? 0 : wave / CW;                       // the wave's patch of the block
  const int cw = PPB == 1 ? wave : wave % CW;
  const int tid = PPB == 1 ? threadIdx.x : threadIdx.x & (GT - 1);        // among the threads of the patch
  _Float16* const fsm = fsm_all + ps * (2 * IMG);
  const float* const projp = CW == 4 ? a.proj : nullptr;         // the projection is the 64-cout form's
  int L = shdr::xcd_remap(blockIdx.x, gridDim.x) * PPB + ps;
  const bool patch_ok = PPB == 1 || L < a.npatch;                // wave-uniform
  if (!patch_ok) L = 0;
  const int tx_ = L % a.ntx; L /= a.ntx;
  const int ty_ = L % a.nty;
  const int n = L / a.nty;
  const int m_start = ty_ * RO, j_start = tx_ * UF_COLS;         // first interior low-res row / column; patch (q, p) = (m_start - 1 + q, j_start - 1 + p), clamped
  const int nch = a.C1 >> 5;

  // ---- the patch: every piece = one float4 of one patch pixel, fetched, split and stored once --------------------------------------
  float xs, ixs;
  {
    const int f4n = a.C1 >> 2, total = NPIX * f4n;
    const float* xb = a.x + (size_t)n * a.h * a.w * a.C1;
    shdr::range_scale(a.xr, nullptr, xs, ixs);
#pragma unroll 1
    for (int id0 = patch_ok ? tid : total; id0 < total; id0 += 4 * GT) {
      f32x4 v[4];
      int dst[4];
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const int id = id0 + k * GT;
        dst[k] = -1;
        if (id < total) {
          const int pp = id / f4n, f = id - pp * f4n;
          const int row = min(max(m_start - 1 + (pp >> 4), 0), a.h - 1), col = min(max(j_start - 1 + (pp & 15), 0), a.w - 1);
          v[k] = *reinterpret_cast<const f32x4*>(xb + ((size_t)row * a.w + col) * a.C1 + 4 * f);
          dst[k] = pp * UF_STRIDE + 4 * f;
        }
      }
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        if (dst[k] >= 0) {
          unsigned h[2], l[2];
          shdr::split4(v[k], xs, h, l);
          *reinterpret_cast<uint2*>(fsm + dst[k]) = make_uint2(h[0], h[1]);
          *reinterpret_cast<uint2*>(fsm + IMG + dst[k]) = make_uint2(l[0], l[1]);
        }
      }
    }
  }
  __syncthreads();

  // ---- lane geometry ---------------------------------------------------------------------------------------------------------------
  const int p = lane & 15, fg = lane >> 4;                       // patch column; k group of the operands = cout quad of the result
  const int j0 = j_start - 1 + p;                                // the lane's low-res column (interior lanes: 1 <= p <= 14)
  const bool lane_ok = p >= 1 && p <= UF_COLS && j0 < a.w;
  // taps whose hi-res column falls outside the image drop out (up2_lowres_stencil_kernel)
  const float wl0 = j0 >= 1 ? 0.75f : 0.0f, wl1 = j0 >= 1 ? 0.25f : 0.0f;
  const float wr0 = j0 + 1 < a.w ? 0.25f : 0.0f, wr1 = j0 + 1 < a.w ? 0.75f : 0.0f;
  const float inv_s = a.hdr[shdr::kHdrInvScale] * ixs;
  const _Float16* wlane = a.wp + p * 32 + 8 * fg;                // A operand: row (lane & 15) of the wave's 16 couts, channels 8 fg .. 8 fg + 7 of the chunk
  const _Float16* xlane = fsm + p * UF_STRIDE + 8 * fg;          // B operand: patch pixel (q, p), the same channels; + 16 q UF_STRIDE, + 32 c

  f32x4 out[RO][2][2];                                           // [interior row][hi-res row 2 m0 + a][hi-res column 2 j0 + s]

  auto pass = [&](auto tyc) __attribute__((always_inline)) {
    constexpr int TY = decltype(tyc)::value;
    f32x4 z[3][R];
#pragma unroll
    for (int t = 0; t < 3; ++t)
#pragma unroll
      for (int q = 0; q < R; ++q) z[t][q] = (f32x4){0.f, 0.f, 0.f, 0.f};
    // the GEMM of the three taps (TY, 0 .. 2): per chunk the wave's fragments of the three taps, each patch row read once for nine MFMAs
    // tap t of cout group cw starts at column t COUT + 16 cw of the packed [Cin, 9 COUT (+ pad)] filter: slice column / 64, row column % 64
    size_t wo[3];
#pragma unroll
    for (int t = 0; t < 3; ++t) {
      const int col = (3 * TY + t) * COUT + 16 * cw;
      wo[t] = (size_t)(col >> 6) * nch * UF_UNIT_HALVES + (col & 63) * 32;
    }
#pragma unroll 1
    for (int c = 0; c < nch; ++c) {
      f16x8 wh[3], wl[3], ws[3];
#pragma unroll
      for (int t = 0; t < 3; ++t) {
        const _Float16* g = wlane + wo[t] + (size_t)c * UF_UNIT_HALVES;
        wh[t] = *reinterpret_cast<const f16x8*>(g);
        wl[t] = *reinterpret_cast<const f16x8*>(g + UF_IMG_HALVES);
      }
#pragma unroll
      for (int t = 0; t < 3; ++t) ws[t] = wh[t] * (_Float16)(1.0f / 2048.0f);      // exact (as in conv_x3_kernel)
      const _Float16* xc = xlane + 32 * c;
#pragma unroll
      for (int q = 0; q < R; ++q) {
        const f16x8 ph = *reinterpret_cast<const f16x8*>(xc + q * 16 * UF_STRIDE);
        const f16x8 pl = *reinterpret_cast<const f16x8*>(xc + IMG + q * 16 * UF_STRIDE);
#pragma unroll
        for (int t = 0; t < 3; ++t) z[t][q] = __builtin_amdgcn_mfma_f32_16x16x32_f16(wh[t], ph, z[t][q], 0, 0, 0);
#pragma unroll
        for (int t = 0; t < 3; ++t) z[t][q] = __builtin_amdgcn_mfma_f32_16x16x32_f16(ws[t], pl, z[t][q], 0, 0, 0);
#pragma unroll
        for (int t = 0; t < 3; ++t) z[t][q] = __builtin_amdgcn_mfma_f32_16x16x32_f16(wl[t], ph, z[t][q], 0, 0, 0);
      }
    }
    // the folds, patch row by patch row: z -> the bits conv_x3_1x1_kernel stores (acc 2^-S 2^-T, then + 0 for its absent bias), the
    // horizontal fold of up2_lowres_stencil_kernel's hrow, and the two terms this (ty, row) contributes to the vertical sums of `emit`
#pragma unroll
    for (int q = 0; q < R; ++q) {
      // (a row at a time, pinned by the volatile fences here and below: left to itself the compiler scales and shifts every row first and
      //  spills the accumulators)
      asm volatile("" : "+v"(z[0][q]), "+v"(z[1][q]), "+v"(z[2][q]));
      f32x4 zz[3];
#pragma unroll
      for (int t = 0; t < 3; ++t)
#pragma unroll
        for (int e = 0; e < 4; ++e) zz[t][e] = __fadd_rn(__fmul_rn(z[t][q][e], inv_s), 0.0f);
      const f32x4 v0 = from_left(zz[0]), v2 = from_left(zz[1]), v4 = from_right(zz[1]), v6 = from_right(zz[2]);
      f32x4 H[2];
      f32x4 t = mul4(v0, wl0);
      t = fma4(zz[0], wl1, t);
      t = fma4(v2, 0.25f, t);
      t = fma4(zz[1], 0.75f, t);
      t = fma4(zz[2], 0.75f, t);
      t = fma4(v6, 0.25f, t);
      H[0] = t;
      f32x4 u = mul4(v0, 0.25f);
      u = fma4(zz[0], 0.75f, u);
      u = fma4(zz[1], 0.75f, u);
      u = fma4(v4, 0.25f, u);
      u = fma4(zz[2], wr0, u);
      u = fma4(v6, wr1, u);
      H[1] = u;
      // patch row q is row P (m0 - 1) of interior row q + 1, row Q (m0) of interior row q and row R (m0 + 1) of interior row q - 1;
      // interior row qo is low-res row m0 = m_start + qo - 1 and out[qo - 1]
      const int mq = m_start + q - 1;                            // m0 of interior row q
#pragma unroll
      for (int s = 0; s < 2; ++s) {
        if (TY == 0) {
          if (q + 1 <= RO) {                                     // first terms of interior row q + 1 (m0 = mq + 1)
            out[q][0][s] = mul4(H[s], mq + 1 >= 1 ? 0.75f : 0.0f);
            out[q][1][s] = mul4(H[s], 0.25f);
          }
          if (q >= 1 && q <= RO) {
            out[q - 1][0][s] = fma4(H[s], mq >= 1 ? 0.25f : 0.0f, out[q - 1][0][s]);
            out[q - 1][1][s] = fma4(H[s], 0.75f, out[q - 1][1][s]);
          }
        } else if (TY == 1) {
          if (q >= 2) out[q - 2][1][s] = fma4(H[s], 0.25f, out[q - 2][1][s]);                 // R[1] of interior row q - 1
          if (q + 1 <= RO) out[q][0][s] = fma4(H[s], 0.25f, out[q][0][s]);                    // P[1] of interior row q + 1
          if (q >= 1 && q <= RO) {
            out[q - 1][0][s] = fma4(H[s], 0.75f, out[q - 1][0][s]);                           // Q[1]
            out[q - 1][1][s] = fma4(H[s], 0.75f, out[q - 1][1][s]);
          }
        } else {
          if (q >= 2) {                                          // R[2] of interior row q - 1 (m0 = mq - 1)
            out[q - 2][0][s] = fma4(H[s], 0.25f, out[q - 2][0][s]);
            out[q - 2][1][s] = fma4(H[s], mq < a.h ? 0.75f : 0.0f, out[q - 2][1][s]);
          }
          if (q >= 1 && q <= RO) {                               // Q[2]
            out[q - 1][0][s] = fma4(H[s], 0.75f, out[q - 1][0][s]);
            out[q - 1][1][s] = fma4(H[s], mq + 1 < a.h ? 0.25f : 0.0f, out[q - 1][1][s]);
          }
        }
      }
      if (q >= 1 && q <= RO) asm volatile("" : "+v"(out[q - 1][0][0]), "+v"(out[q - 1][0][1]), "+v"(out[q - 1][1][0]), "+v"(out[q - 1][1][1]));
      if (q + 1 <= RO) asm volatile("" : "+v"(out[q][0][0]), "+v"(out[q][0][1]), "+v"(out[q][1][0]), "+v"(out[q][1][1]));
      if (q >= 2) asm volatile("" : "+v"(out[q - 2][0][0]), "+v"(out[q - 2][0][1]), "+v"(out[q - 2][1][0]), "+v"(out[q - 2][1][1]));
    }
  };
  if (patch_ok) {
    pass(std::integral_constant<int, 0>{});
    pass(std::integral_constant<int, 1>{});
    pass(std::integral_constant<int, 2>{});
  }

  // ---- epilogue: up2_lowres_stencil_kernel's `finish` per output, y and / or this wave's share of the projected pixel ---------------------
  const int c = 16 * cw + 4 * fg;
  auto ld = [](const float* q) __attribute__((always_inline)) { return *reinterpret_cast<const f32x4*>(q); };
  const f32x4 bias_r = a.bias ? ld(a.bias + c) : (f32x4){0.f, 0.f, 0.f, 0.f};
  const f32x4 scale_r = a.scale ? ld(a.scale + c) : (f32x4){1.f, 1.f, 1.f, 1.f};
  const f32x4 shift_r = a.scale ? ld(a.shift + c) : (f32x4){0.f, 0.f, 0.f, 0.f};
  f32x4 pq[3];
#pragma unroll
  for (int j = 0; j < 3; ++j) pq[j] = projp ? ld(projp + j * 64 + c) : (f32x4){0.f, 0.f, 0.f, 0.f};
  if (projp) __syncthreads();                                    // every wave is done with the patch images: their LDS takes the partial sums
  float* part = reinterpret_cast<float*>(fsm);                   // [4 waves][RO * 64 slots][3], slot = (qo * 2 + a) * 32 + 2 p + s
  float ym = 0.0f;
#pragma unroll
  for (int qo = 0; qo < RO; ++qo) {
    const int m0 = m_start + qo;
    const bool row_ok = patch_ok && m0 < a.h;                    // wave-uniform
#pragma unroll
    for (int r = 0; r < 2; ++r)
#pragma unroll
      for (int s = 0; s < 2; ++s) {
        f32x4 v = out[qo][r][s];
        v += bias_r;
        shdr::act_apply4<0>(v, a.act1);
        if (a.scale) v = fma4v(v, scale_r, shift_r);
        shdr::act_apply4<0>(v, a.act2);
        if (a.y && row_ok && lane_ok) {
          *reinterpret_cast<f32x4*>(a.y + (((size_t)n * 2 * a.h + 2 * m0 + r) * 2 * a.w + 2 * j0 + s) * COUT + c) = v;
          ym = fmaxf(fmaxf(fmaxf(fmaxf(ym, fabsf(v[0])), fabsf(v[1])), fabsf(v[2])), fabsf(v[3]));
        }
        if (projp) {
#pragma unroll
          for (int j = 0; j < 3; ++j) {
            float t = v[0] * pq[j][0] + v[1] * pq[j][1] + v[2] * pq[j][2] + v[3] * pq[j][3];
            t += __shfl_xor(t, 16, 64);                          // the four lane groups fg hold four couts each of the same pixel
            t += __shfl_xor(t, 32, 64);
            if (fg == 0) part[(cw * RO * 64 + (qo * 2 + r) * 32 + 2 * p + s) * 3 + j] = t;
          }
        }
      }
  }
  if (projp) {
    __syncthreads();
    for (int slot = tid; slot < RO * 64; slot += UF_THREADS) {
      const int s = slot & 1, pp = (slot >> 1) & 15, r = (slot >> 5) & 1, qo = slot >> 6;
      const int m0 = m_start + qo, jj = j_start - 1 + pp;
      if (m0 < a.h && pp >= 1 && pp <= UF_COLS && jj < a.w) {
        float* o = a.yproj + (((size_t)n * 2 * a.h + 2 * m0 + r) * 2 * a.w + 2 * jj + s) * 3;
#pragma unroll
        for (int j = 0; j < 3; ++j)
          o[j] = ((part[slot * 3 + j] + part[(RO * 64 + slot) * 3 + j]) + part[(2 * RO * 64 + slot) * 3 + j]) + part[(3 * RO * 64 + slot) * 3 + j];
      }
    }
  }
  if (a.y && a.yr) shdr::range_out_block256(a.yr, ym);           // one atomicMax per block, every thread calls
}

constexpr int uf_lds_bytes(int R, int CW, int CMAX) { return (4 / CW) * 2 * 16 * R * uf_stride(CMAX) * 2; }

bool uf_geometry_ok(const shdr_conv2d_desc* d) {
  return d && d->N > 0 && d->H > 0 && d->W > 0 && d->H % 2 == 0 && d->W % 2 == 0 && d->KH == 3 && d->KW == 3 && d->stride == 1 && d->pad_t == 1 &&
         d->pad_l == 1 && d->Ho == d->H && d->Wo == d->W && d->C2 == 0 && d->C1 % 32 == 0 && d->C1 <= UF_MAX_CIN;
}
// the 64-cout form (the Hallucination-Net's u1, the Dequantization-Net's u3)
bool uf_shape_ok(const shdr_conv2d_desc* d) { return uf_geometry_ok(d) && d->C1 >= 64 && d->Cout == 64; }
// the narrow forms: 32 couts (two patches per block), 16 couts (four patches per block, whose images fit up to 64 input channels)
bool uf_narrow_shape_ok(const shdr_conv2d_desc* d) {
  return uf_geometry_ok(d) && d->C1 >= 32 && (d->Cout == 32 || (d->Cout == 16 && d->C1 <= 64));
}
// columns of the narrow forms' packed filter: 9 Cout rounded up to the pack's 64-cout slices (16 -> 192, 32 -> 320)
inline int uf_narrow_columns(int Cout) { return (9 * Cout + 63) / 64 * 64; }
bool uf_narrow_gemm_desc(const shdr_conv2d_desc* d, shdr_conv2d_desc* g) {
  if (!uf_narrow_shape_ok(d)) return false;
  *g = shdr_conv2d_desc{};
  g->N = d->N; g->H = d->H / 2; g->W = d->W / 2; g->C1 = d->C1; g->C2 = 0;
  g->Cout = uf_narrow_columns(d->Cout);
  g->KH = 1; g->KW = 1; g->stride = 1; g->pad_t = 0; g->pad_l = 0; g->Ho = g->H; g->Wo = g->W;
  g->x2_scale = 1.0f; g->act1 = SHDR_ACT_NONE; g->act2 = SHDR_ACT_NONE; g->algo = SHDR_ALGO_AUTO; g->cout_valid = g->Cout; g->y_cstride = g->Cout;
  return true;
}
// up2_lowres.hip's staging: st[ci][t * Cout + co] = w[t][ci][co] (t = 3 ty + tx), zero in the padded columns
__global__ __launch_bounds__(256) void up2_fused_filter_kernel(const float* __restrict__ w, float* __restrict__ st, int Cin, int Cout, int Cp) {
  const long total = (long)Cin * Cp;
  for (long e = (long)blockIdx.x * 256 + threadIdx.x; e < total; e += (long)gridDim.x * 256) {
    const int col = (int)(e % Cp), ci = (int)(e / Cp);
    const int t = col / Cout, co = col - t * Cout;
    st[e] = t < 9 ? w[((size_t)t * Cin + ci) * Cout + co] : 0.0f;
  }
}

template <int CW, int CMAX>
int uf_launch(const UpFusedArgs& a, hipStream_t st) {
  constexpr int lds = uf_lds_bytes(UF_R, CW, CMAX), PPB = 4 / CW;
  static_assert(lds <= 160 * 1024 - 64, "the patch images of a block must fit the CU's LDS");
  if (int e = shdr::dynamic_lds<&up2_fused_kernel<UF_R, CW, CMAX>>(lds)) return e;
  const long nblk = ((long)a.npatch + PPB - 1) / PPB;
  hipLaunchKernelGGL((up2_fused_kernel<UF_R, CW, CMAX>), dim3((unsigned)nblk), dim3(UF_THREADS), lds, st, a);
  return shdr::check_launch("up2_fused_kernel");
}

}  // namespace

// 1 unless SHDR_NO_UP2_NARROW=1 (the A/B arm of the narrow forms and of the Dequantization-Net's use of the low-res forms: under it every
// launch of an inference step is the one from before they existed)
extern "C" int shdr_conv2d_up2_narrow_enabled(void) { return SHDR_ENV("SHDR_NO_UP2_NARROW") == nullptr ? 1 : 0; }

// 1 if shdr_conv2d_fwd_up2_fused_f32 takes the layer `d` (the descriptor of shdr_conv2d_up2_lowres_ok_f32): fp32 3x3 / stride 1 / SAME on the
// bilinear prologue, one source, even H and W, no TANH, the split-operand kernels not switched off, and
//   64 couts, Cin = 64, 96 or 128 (the patch of every input channel is resident in LDS), or
//   32 couts, Cin = 32 .. 128, or 16 couts, Cin = 32 or 64 (the narrow forms; not under SHDR_NO_UP2_NARROW=1).
// SHDR_NO_UP2_FUSED=1: never (the A/B arm).
extern "C" int shdr_conv2d_up2_fused_ok_f32(const shdr_conv2d_desc* d) {
  const bool narrow = uf_narrow_shape_ok(d) && shdr_conv2d_up2_narrow_enabled();
  if (!(uf_shape_ok(d) || narrow) || SHDR_ENV("SHDR_NO_UP2_FUSED") != nullptr || SHDR_ENV("SHDR_NO_UP2_LOWRES") != nullptr ||
      SHDR_ENV("SHDR_NO_WINOGRAD") != nullptr || SHDR_ENV("SHDR_NO_X3") != nullptr)
    return 0;
  if (d->algo != SHDR_ALGO_AUTO || d->prologue != SHDR_PROLOGUE_BILINEAR2X) return 0;
  if ((d->cout_valid != 0 && d->cout_valid != d->Cout) || d->w_batch_stride != 0 || d->y_pix_stride > 1 || (d->y_cstride != 0 && d->y_cstride != d->Cout)) return 0;
  if (d->act1 == SHDR_ACT_TANH || d->act2 == SHDR_ACT_TANH) return 0;
  const long nblk = (long)d->N * ((d->H / 2 + UF_R - 3) / (UF_R - 2)) * ((d->W / 2 + UF_COLS - 1) / UF_COLS);
  return nblk <= 0x7fffffffL - (narrow ? 4 : 0) ? 1 : 0;     // (a narrow block numbers its patches past the last one)
}

// 64 couts: the prepared filter is the two-launch form's (its packed [Cin, 9 Cout (+ pad)] filter: slice t = tap t); the narrow forms: the
// same pack of the [Cin, 9 Cout] matrix padded to whole 64-column slices, then its fp32 staging copy
extern "C" int64_t shdr_conv2d_up2_fused_filter_elems_f32(const shdr_conv2d_desc* d) {
  if (uf_shape_ok(d)) return shdr_conv2d_up2_lowres_filter_elems_f32(d);
  shdr_conv2d_desc g;
  if (!uf_narrow_gemm_desc(d, &g)) return -1;
  const int64_t packed = shdr_conv2d_x3_filter_elems_f32(&g);
  return packed < 0 ? -1 : packed + (int64_t)g.C1 * g.Cout;
}
extern "C" int shdr_conv2d_up2_fused_prepare_filter_f32(const shdr_conv2d_desc* d, const float* w, float* prepared, void* stream) {
  if (uf_shape_ok(d)) return shdr_conv2d_up2_lowres_prepare_filter_f32(d, w, prepared, stream);
  SHDR_REQUIRE(d && w && prepared, SHDR_E_NULL, "up2_fused_prepare_filter: null pointer");
  shdr_conv2d_desc g;
  SHDR_REQUIRE(uf_narrow_gemm_desc(d, &g), SHDR_E_SHAPE,
               "up2_fused_prepare_filter: need a 3x3 layer with one source, even H and W, and Cin 64 / 96 / 128 -> 64, Cin 32 .. 128 -> 32 or Cin 32 / 64 -> 16");
  const int64_t packed = shdr_conv2d_x3_filter_elems_f32(&g);
  SHDR_REQUIRE(packed > 0, SHDR_E_SHAPE, "up2_fused_prepare_filter: the 1x1 form of this layer has no packed filter");
  float* staged = prepared + packed;
  const long total = (long)g.C1 * g.Cout;
  hipLaunchKernelGGL(up2_fused_filter_kernel, dim3(shdr::stream_grid(total)), dim3(256), 0, shdr::stream_of(stream), w, staged, g.C1, d->Cout, g.Cout);
  if (int rc = shdr::check_launch("up2_fused_filter")) return rc;
  return shdr_conv2d_x3_prepare_filter_f32(&g, staged, prepared, stream);
}

// x the LOW-RES tensor [N, H/2, W/2, Cin]; y [N, H, W, Cout] = act2(affine(act1(conv3x3(resize2x(x)) + bias))) and / or, at 64 couts,
// y_proj [N, H, W, 3][j] = sum_c proj[j][c] y[c]; one launch on `stream`.  x_range: the input's range slot; y_range (or NULL): receives
// max |y| when y is written (atomicMax, the caller zeroes it).
extern "C" int shdr_conv2d_fwd_up2_fused_f32(const shdr_conv2d_desc* d, const float* x, const float* prepared, const float* bias, const float* scale,
                                             const float* shift, const float* proj, float* y_proj, float* y, const float* x_range, float* y_range,
                                             void* stream) {
  SHDR_REQUIRE(d && x && prepared && x_range, SHDR_E_NULL, "conv2d_up2_fused: null desc / x / prepared filter / x_range");
  SHDR_REQUIRE(y || y_proj, SHDR_E_NULL, "conv2d_up2_fused: neither y nor y_proj");
  SHDR_REQUIRE((proj == nullptr) == (y_proj == nullptr), SHDR_E_NULL, "conv2d_up2_fused: proj and y_proj come together");
  SHDR_REQUIRE(shdr_conv2d_up2_fused_ok_f32(d), SHDR_E_SHAPE, "conv2d_up2_fused: layer not taken (shdr_conv2d_up2_fused_ok_f32)");
  SHDR_REQUIRE(!proj || d->Cout == 64, SHDR_E_SHAPE, "conv2d_up2_fused: the projected output is the 64-cout form's");
  SHDR_REQUIRE((scale == nullptr) == (shift == nullptr), SHDR_E_NULL, "conv2d_up2_fused: scale and shift come together");
  SHDR_REQUIRE(shdr::aligned16(x) && shdr::aligned16(prepared) && (!y || shdr::aligned16(y)) && (!bias || shdr::aligned16(bias)) &&
                   (!scale || (shdr::aligned16(scale) && shdr::aligned16(shift))) && (!proj || shdr::aligned16(proj)),
               SHDR_E_ALIGN, "conv2d_up2_fused: tensors must be 16-byte aligned");
  UpFusedArgs a{};
  a.x = x; a.hdr = prepared; a.wp = reinterpret_cast<const _Float16*>(prepared + shdr::kSplitHeaderFloats);
  a.bias = bias; a.scale = scale; a.shift = shift; a.proj = proj; a.y = y; a.yproj = y_proj;
  a.xr = reinterpret_cast<const unsigned*>(x_range); a.yr = reinterpret_cast<unsigned*>(y_range);
  a.N = d->N; a.h = d->H / 2; a.w = d->W / 2; a.C1 = d->C1; a.act1 = d->act1; a.act2 = d->act2;
  a.nty = (a.h + UF_R - 3) / (UF_R - 2);
  a.ntx = (a.w + UF_COLS - 1) / UF_COLS;
  a.npatch = (int)((long)a.N * a.nty * a.ntx);
  hipStream_t st = shdr::stream_of(stream);
  if (d->Cout == 64) return uf_launch<4, 128>(a, st);
  if (d->Cout == 32) return d->C1 <= 64 ? uf_launch<2, 64>(a, st) : uf_launch<2, 128>(a, st);
  return d->C1 <= 32 ? uf_launch<1, 32>(a, st) : uf_launch<1, 64>(a, st);
}

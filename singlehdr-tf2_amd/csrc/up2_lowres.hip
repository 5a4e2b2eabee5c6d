// Conv2D 3x3 (SAME, stride 1) of tf.image.resize(x, 2x, BILINEAR) with the channel mix done at LOW resolution (the `up` blocks of
// hallucination_net.py:77-91).  The bilinear resize acts on every channel on its own, so it commutes with the channel mix of each filter
// tap.  With W[t] the Cin x Cout matrix of tap t = (ty, tx) and B_r(m) the two bilinear row weights of hi-res row r (half-pixel centres,
// clamped indices: resize2x_kernel of pool.hip):
//     z_t(m, j, :)                   = x(m, j, :) W[t]                                        a 1x1 convolution Cin -> 9 Cout on h x w pixels
//     conv3x3(resize2x(x))(r, s, :)  = sum_t [(r + ty - 1, s + tx - 1) inside 2h x 2w] sum_{m, j} B_{r+ty-1}(m) B_{s+tx-1}(j) z_t(m, j, :)
// exact algebra, zero padding and edge clamp included.  The GEMM runs on h w pixels instead of 4 h w: four times fewer MFMAs.  Two launches:
//   A  conv_x3_1x1_kernel (conv_x3.hip, unchanged) on the low-res input with the filter laid out [1, 1, Cin, 9 Cout (+ pad)], column
//      t Cout + c, all nine taps under one scale 2^S; no bias, no activation; z goes to the caller's workspace;
//   B  up2_lowres_stencil_kernel below: the sum above per hi-res pixel and channel quad, then the conv epilogue act2(affine(act1(v + bias))),
//      16-byte stores and the output's range slot.
// Not bit-identical to resize2x + conv (other roundings, the same accuracy class): an opt-in path (Python: conv2d_up2(lowres=True)),
// A/B switch SHDR_NO_UP2_LOWRES=1.
#include <stdlib.h>

#include "split.h"

namespace {

typedef float f32x4 __attribute__((ext_vector_type(4)));

using shdr::fma4;
using shdr::fma4v;
using shdr::kRangeScratch;
using shdr::mul4;
using shdr::up256;

// z columns: 9 Cout rounded up to the blocks of launch_x3_1x1 -- 256 couts per block (each input chunk split once per 256 couts) where
// that pads at most an eighth (9 x 128 = 1152 -> 1280: 128^2 x 256 -> 1152 at batch 16 0.74 -> 0.655 ms, the layer 1.09 - 1.13 -> 1.00 - 1.03),
// else 128 (9 x 64 = 576 -> 640); SHDR_UP2_LOWRES_PAD=128|256 forces one (A/B)
inline int z_columns(int Cout) {
  const int cols = 9 * Cout, c128 = (cols + 127) / 128 * 128, c256 = (cols + 255) / 256 * 256;
  if (const char* e = SHDR_ENV("SHDR_UP2_LOWRES_PAD")) return atoi(e) == 256 ? c256 : c128;
  return (c256 - cols) * 8 <= cols ? c256 : c128;
}

// ---- filter staging: st[ci][t * Cout + co] = w[t][ci][co] (t = 3 ty + tx), zero in the padded columns ----------------------------------
__global__ __launch_bounds__(256) void up2_lowres_filter_kernel(const float* __restrict__ w, float* __restrict__ st, int Cin, int Cout, int Cp) {
  const long total = (long)Cin * Cp;
  for (long e = (long)blockIdx.x * 256 + threadIdx.x; e < total; e += (long)gridDim.x * 256) {
    const int col = (int)(e % Cp), ci = (int)(e / Cp);
    const int t = col / Cout, co = col - t * Cout;
    st[e] = t < 9 ? w[((size_t)t * Cin + ci) * Cout + co] : 0.0f;
  }
}

// ---- the stencil pass ------------------------------------------------------------------------------------------------------------------
// Layout of the work (the choice the design notes record): NO LDS staging.  A thread owns one low-res COLUMN j0 and one channel quad and
// walks down the low-res rows of its block's row segment.  Per low-res row m it loads the 21 float4 of z it needs -- taps (ty, tx) at
// the columns tx reaches: (j0 - 1, j0), (j0 - 1, j0, j0 + 1), (j0, j0 + 1) -- and folds them HORIZONTALLY at once into H[ty][s], s = the
// two hi-res columns 2 j0, 2 j0 + 1 (6 multiply-adds each).  Three such rows (m0 - 1, m0, m0 + 1, clamped) live in registers; the VERTICAL
// fold of them (6 multiply-adds per output) gives the hi-res rows 2 m0, 2 m0 + 1: 15 multiply-adds per output element, every z row loaded
// once per block, the sums in one fixed order.  A staged tile with its halo would hold (T + 2)^2 pixels x 9 Cout floats -- at 64 couts
// 2.3 KB per pixel, so 64 KB buys a 3 x 3 tile with 2.8x halo traffic -- while the walk has no vertical halo inside a segment and its
// horizontal halo (the neighbouring column strips read columns j0 +- 1 too) is served by L2: blocks of neighbouring strips run on the same XCD
// at the same time (xcd_remap).  Block = 16 columns x 16 quads (64 couts: 256 contiguous bytes per pixel and tap), lanes along the quads.
constexpr int UL_COLS = 16, UL_QUADS = 16;
struct UpLowArgs {
  const float* z;
  const float* bias;
  const float* scale;
  const float* shift;
  float* y;
  unsigned* yr;
  int N, h, w, Cout, Cp, rows, nseg, nstrip, ncs, act1, act2;
};

__global__ __launch_bounds__(256, 2) void up2_lowres_stencil_kernel(const UpLowArgs a) {
  const int tid = threadIdx.x;
  int L = shdr::xcd_remap(blockIdx.x, gridDim.x);
  const int cs = L % a.ncs; L /= a.ncs;
  const int strip = L % a.nstrip; L /= a.nstrip;
  const int seg = L % a.nseg;
  const int n = L / a.nseg;
  const int c = cs * (4 * UL_QUADS) + 4 * (tid & (UL_QUADS - 1));
  const int j0 = strip * UL_COLS + (tid >> 4);
  const bool active = j0 < a.w;
  const int m_begin = seg * a.rows, m_end = min(m_begin + a.rows, a.h);
  float ym = 0.0f;
  if (active) {
    const int jm = max(j0 - 1, 0), jp = min(j0 + 1, a.w - 1);
    // taps whose hi-res column falls outside the image drop out: tx = 0 of column 2 j0 at j0 = 0, tx = 2 of column 2 j0 + 1 at j0 = w - 1
    const float wl0 = j0 >= 1 ? 0.75f : 0.0f, wl1 = j0 >= 1 ? 0.25f : 0.0f;
    const float wr0 = j0 + 1 < a.w ? 0.25f : 0.0f, wr1 = j0 + 1 < a.w ? 0.75f : 0.0f;
    const float* zb = a.z + (size_t)n * a.h * a.w * a.Cp + c;
    const int C = a.Cout;
    auto ld = [](const float* p) __attribute__((always_inline)) { return *reinterpret_cast<const f32x4*>(p); };
    auto hrow = [&](int m, f32x4 (&H)[3][2]) __attribute__((always_inline)) {
      const float* zr = zb + (size_t)m * a.w * a.Cp;
      const float* pm = zr + (size_t)jm * a.Cp;
      const float* p0 = zr + (size_t)j0 * a.Cp;
      const float* pp = zr + (size_t)jp * a.Cp;
      f32x4 v[3][7];
#pragma unroll
      for (int ty = 0; ty < 3; ++ty) {
        const int t0 = 3 * ty * C;
        v[ty][0] = ld(pm + t0); v[ty][1] = ld(p0 + t0);
        v[ty][2] = ld(pm + t0 + C); v[ty][3] = ld(p0 + t0 + C); v[ty][4] = ld(pp + t0 + C);
        v[ty][5] = ld(p0 + t0 + 2 * C); v[ty][6] = ld(pp + t0 + 2 * C);
      }
#pragma unroll
      for (int ty = 0; ty < 3; ++ty) {
        // hi-res column 2 j0: tx = 0 -> 2 j0 - 1 = (j0 - 1, j0) x (.75, .25); tx = 1 -> 2 j0 = (j0 - 1, j0) x (.25, .75); tx = 2 -> 2 j0 + 1 = (j0, j0 + 1) x (.75, .25)
        f32x4 t = mul4(v[ty][0], wl0);
        t = fma4(v[ty][1], wl1, t);
        t = fma4(v[ty][2], 0.25f, t);
        t = fma4(v[ty][3], 0.75f, t);
        t = fma4(v[ty][5], 0.75f, t);
        t = fma4(v[ty][6], 0.25f, t);
        H[ty][0] = t;
        // hi-res column 2 j0 + 1: tx = 0 -> 2 j0; tx = 1 -> 2 j0 + 1; tx = 2 -> 2 j0 + 2 = (j0, j0 + 1) x (.25, .75)
        f32x4 u = mul4(v[ty][0], 0.25f);
        u = fma4(v[ty][1], 0.75f, u);
        u = fma4(v[ty][3], 0.75f, u);
        u = fma4(v[ty][4], 0.25f, u);
        u = fma4(v[ty][5], wr0, u);
        u = fma4(v[ty][6], wr1, u);
        H[ty][1] = u;
      }
    };
    const f32x4 bias_r = a.bias ? ld(a.bias + c) : (f32x4){0.f, 0.f, 0.f, 0.f};
    const f32x4 scale_r = a.scale ? ld(a.scale + c) : (f32x4){1.f, 1.f, 1.f, 1.f};
    const f32x4 shift_r = a.scale ? ld(a.shift + c) : (f32x4){0.f, 0.f, 0.f, 0.f};
    float* yb = a.y + ((size_t)n * 2 * a.h * 2 * a.w + 2 * j0) * C + c;
    auto finish = [&](f32x4 v, int r, int s) __attribute__((always_inline)) {      // the order of x3_tile_epilogue
      v += bias_r;
      shdr::act_apply4<0>(v, a.act1);
      if (a.scale) v = fma4v(v, scale_r, shift_r);
      shdr::act_apply4<0>(v, a.act2);
      *reinterpret_cast<f32x4*>(yb + ((size_t)r * 2 * a.w + s) * C) = v;
      ym = fmaxf(fmaxf(fmaxf(fmaxf(ym, fabsf(v[0])), fabsf(v[1])), fabsf(v[2])), fabsf(v[3]));
    };
    auto emit = [&](int m0, const f32x4 (&P)[3][2], const f32x4 (&Q)[3][2], const f32x4 (&R)[3][2]) __attribute__((always_inline)) {
      // rows P = m0 - 1, Q = m0, R = m0 + 1 (clamped).  Hi-res row 2 m0: ty = 0 -> 2 m0 - 1 (outside at m0 = 0), ty = 1 -> 2 m0, ty = 2 -> 2 m0 + 1;
      // hi-res row 2 m0 + 1: ty = 0 -> 2 m0, ty = 1 -> 2 m0 + 1, ty = 2 -> 2 m0 + 2 (outside at m0 = h - 1)
      const float wt0 = m0 >= 1 ? 0.75f : 0.0f, wt1 = m0 >= 1 ? 0.25f : 0.0f;
      const float wb0 = m0 + 1 < a.h ? 0.25f : 0.0f, wb1 = m0 + 1 < a.h ? 0.75f : 0.0f;
#pragma unroll
      for (int s = 0; s < 2; ++s) {
        f32x4 t = mul4(P[0][s], wt0);
        t = fma4(Q[0][s], wt1, t);
        t = fma4(P[1][s], 0.25f, t);
        t = fma4(Q[1][s], 0.75f, t);
        t = fma4(Q[2][s], 0.75f, t);
        t = fma4(R[2][s], 0.25f, t);
        finish(t, 2 * m0, s);
        f32x4 u = mul4(P[0][s], 0.25f);
        u = fma4(Q[0][s], 0.75f, u);
        u = fma4(Q[1][s], 0.75f, u);
        u = fma4(R[1][s], 0.25f, u);
        u = fma4(Q[2][s], wb0, u);
        u = fma4(R[2][s], wb1, u);
        finish(u, 2 * m0 + 1, s);
      }
    };
    f32x4 Hw[3][3][2];
    hrow(max(m_begin - 1, 0), Hw[0]);
    hrow(m_begin, Hw[1]);
#pragma unroll 1
    for (int m0 = m_begin; m0 < m_end; m0 += 3) {
#pragma unroll
      for (int u = 0; u < 3; ++u) {
        if (m0 + u < m_end) {                                    // block-uniform
          hrow(min(m0 + u + 1, a.h - 1), Hw[(u + 2) % 3]);
          emit(m0 + u, Hw[u % 3], Hw[(u + 1) % 3], Hw[(u + 2) % 3]);
        }
      }
    }
  }
  if (a.yr) shdr::range_out_block256(a.yr, ym);                  // one atomicMax per block, every thread calls
}

// the 1x1 convolution of launch A on the low-res image
bool gemm_desc(const shdr_conv2d_desc* d, shdr_conv2d_desc* g) {
  if (!d || d->Cout <= 0 || d->H <= 0 || d->W <= 0 || d->H % 2 || d->W % 2) return false;
  *g = shdr_conv2d_desc{};
  g->N = d->N; g->H = d->H / 2; g->W = d->W / 2; g->C1 = d->C1; g->C2 = 0;
  g->Cout = z_columns(d->Cout);
  g->KH = 1; g->KW = 1; g->stride = 1; g->pad_t = 0; g->pad_l = 0; g->Ho = g->H; g->Wo = g->W;
  g->x2_scale = 1.0f; g->act1 = SHDR_ACT_NONE; g->act2 = SHDR_ACT_NONE; g->algo = SHDR_ALGO_AUTO; g->cout_valid = g->Cout; g->y_cstride = g->Cout;
  return true;
}

}  // namespace

// 1 if shdr_conv2d_fwd_up2_lowres_f32 takes the layer `d` (the descriptor of the convolution on the up-sampled image, prologue
// SHDR_PROLOGUE_BILINEAR2X as for shdr_conv2d_fwd_prepared_f32): fp32 3x3 / stride 1 / SAME, one source, even H and W, Cin % 32 == 0 and
// >= 64, Cout % 64 == 0, and the low-res 1x1 GEMM on the split-operand plan (shdr_conv2d_x3_ok_f32: SHDR_X3_MIN_BLOCKS and the SHDR_NO_X3*
// switches hold here too).  SHDR_NO_UP2_LOWRES=1: never (the A/B arm).
extern "C" int shdr_conv2d_up2_lowres_ok_f32(const shdr_conv2d_desc* d) {
  shdr_conv2d_desc g;
  if (!gemm_desc(d, &g) || SHDR_ENV("SHDR_NO_UP2_LOWRES") != nullptr || SHDR_ENV("SHDR_NO_WINOGRAD") != nullptr) return 0;
  if (d->algo != SHDR_ALGO_AUTO || d->prologue != SHDR_PROLOGUE_BILINEAR2X || d->KH != 3 || d->KW != 3 || d->stride != 1 || d->pad_t != 1 || d->pad_l != 1 ||
      d->Ho != d->H || d->Wo != d->W || d->C2 != 0 || d->C1 % 32 || d->C1 < 64 || d->Cout % 64)
    return 0;
  if ((d->cout_valid != 0 && d->cout_valid != d->Cout) || d->w_batch_stride != 0 || d->y_pix_stride > 1 || (d->y_cstride != 0 && d->y_cstride != d->Cout)) return 0;
  if (d->act1 == SHDR_ACT_TANH || d->act2 == SHDR_ACT_TANH) return 0;
  if ((long)g.N * g.H * g.W >= (1L << 30)) return 0;           // (the GEMM kernel counts pixels in an int; the stencil pass indexes in size_t)
  return shdr_conv2d_x3_ok_f32(&g);
}

// floats of the prepared filter: the packed split-operand 1x1 filter [Cin, 9 Cout (+ pad)], then its fp32 staging copy
extern "C" int64_t shdr_conv2d_up2_lowres_filter_elems_f32(const shdr_conv2d_desc* d) {
  shdr_conv2d_desc g;
  if (!gemm_desc(d, &g) || d->C1 <= 0 || d->C1 % 32 || d->Cout % 64) return -1;
  const int64_t packed = shdr_conv2d_x3_filter_elems_f32(&g);
  return packed < 0 ? -1 : packed + (int64_t)g.C1 * g.Cout;
}

// w: the HWIO filter [3, 3, Cin, Cout] -> prepared (shdr_conv2d_up2_lowres_filter_elems_f32 floats, 16-byte aligned); once per filter version
extern "C" int shdr_conv2d_up2_lowres_prepare_filter_f32(const shdr_conv2d_desc* d, const float* w, float* prepared, void* stream) {
  SHDR_REQUIRE(d && w && prepared, SHDR_E_NULL, "up2_lowres_prepare_filter: null pointer");
  shdr_conv2d_desc g;
  SHDR_REQUIRE(gemm_desc(d, &g) && d->KH == 3 && d->KW == 3 && d->C2 == 0 && d->C1 > 0 && d->C1 % 32 == 0 && d->Cout % 64 == 0, SHDR_E_SHAPE,
               "up2_lowres_prepare_filter: need a 3x3 layer with one source, Cin %% 32 == 0, Cout %% 64 == 0, even H and W");
  const int64_t packed = shdr_conv2d_x3_filter_elems_f32(&g);
  SHDR_REQUIRE(packed > 0, SHDR_E_SHAPE, "up2_lowres_prepare_filter: the 1x1 form of this layer has no packed filter");
  float* staged = prepared + packed;
  const long total = (long)g.C1 * g.Cout;
  hipLaunchKernelGGL(up2_lowres_filter_kernel, dim3(shdr::stream_grid(total)), dim3(256), 0, shdr::stream_of(stream), w, staged, g.C1, d->Cout, g.Cout);
  if (int rc = shdr::check_launch("up2_lowres_filter")) return rc;
  return shdr_conv2d_x3_prepare_filter_f32(&g, staged, prepared, stream);
}

// bytes of workspace of one forward call: z [N, H/2, W/2, 9 Cout (+ pad)] and the scratch slot of an input without a range
extern "C" int64_t shdr_conv2d_up2_lowres_workspace_bytes_f32(const shdr_conv2d_desc* d) {
  shdr_conv2d_desc g;
  if (!gemm_desc(d, &g)) return -1;
  return (int64_t)(up256((size_t)g.N * g.H * g.W * g.Cout * sizeof(float)) + kRangeScratch);
}

// y [N, H, W, Cout] = act2(affine(act1(conv3x3(resize2x(x)) + bias))), x the LOW-RES tensor [N, H/2, W/2, Cin]: launch A (the GEMM into the
// workspace) and launch B (the stencil pass) on `stream`.  x_range: the input's range slot (NULL: measured into the workspace's tail);
// y_range (or NULL): receives max |y| (atomicMax, the caller zeroes it).
extern "C" int shdr_conv2d_fwd_up2_lowres_f32(const shdr_conv2d_desc* d, const float* x, const float* prepared, const float* bias, const float* scale,
                                              const float* shift, float* y, void* workspace, const float* x_range, float* y_range, void* stream) {
  SHDR_REQUIRE(d && x && prepared && y && workspace, SHDR_E_NULL, "conv2d_up2_lowres: null desc / x / prepared filter / y / workspace");
  SHDR_REQUIRE(shdr_conv2d_up2_lowres_ok_f32(d), SHDR_E_SHAPE, "conv2d_up2_lowres: layer not taken (shdr_conv2d_up2_lowres_ok_f32)");
  SHDR_REQUIRE((scale == nullptr) == (shift == nullptr), SHDR_E_NULL, "conv2d_up2_lowres: scale and shift come together");
  SHDR_REQUIRE(shdr::aligned16(x) && shdr::aligned16(prepared) && shdr::aligned16(workspace) && shdr::aligned16(y) && (!bias || shdr::aligned16(bias)) && (!scale || (shdr::aligned16(scale) && shdr::aligned16(shift))),
               SHDR_E_ALIGN, "conv2d_up2_lowres: tensors must be 16-byte aligned");
  shdr_conv2d_desc g;
  gemm_desc(d, &g);
  float* z = reinterpret_cast<float*>(workspace);
  if (!x_range) {
    float* slot = reinterpret_cast<float*>(reinterpret_cast<char*>(workspace) + shdr_conv2d_up2_lowres_workspace_bytes_f32(d) - kRangeScratch);
    if (hipMemsetAsync(slot, 0, sizeof(float), shdr::stream_of(stream)) != hipSuccess) return shdr::fail(SHDR_E_LAUNCH, "conv2d_up2_lowres: memset failed");
    if (int rc = shdr_absmax_f32(x, (int64_t)g.N * g.H * g.W * g.C1, slot, stream)) return rc;
    x_range = slot;
  }
  if (int rc = shdr_conv2d_fwd_x3_ranged_f32(&g, x, nullptr, prepared, nullptr, nullptr, nullptr, z, nullptr, x_range, nullptr, nullptr, stream)) return rc;
  UpLowArgs a{};
  a.z = z; a.bias = bias; a.scale = scale; a.shift = shift; a.y = y; a.yr = reinterpret_cast<unsigned*>(y_range);
  a.N = g.N; a.h = g.H; a.w = g.W; a.Cout = d->Cout; a.Cp = g.Cout; a.act1 = d->act1; a.act2 = d->act2;
  a.nstrip = (a.w + UL_COLS - 1) / UL_COLS;
  a.ncs = a.Cout / (4 * UL_QUADS);
  // rows per segment: every row of a segment beyond its first costs one row of loads, the first three; 16 where that still leaves
  // four blocks per CU, else 8, else 4 (the result does not depend on it: the sums of a pixel are the same in any segment)
  a.rows = 16;
  while (a.rows > 4 && (long)a.N * ((a.h + a.rows - 1) / a.rows) * a.nstrip * a.ncs < 1024) a.rows >>= 1;
  if (const char* e = SHDR_ENV("SHDR_UP2_LOWRES_ROWS")) a.rows = atoi(e) > 0 ? atoi(e) : a.rows;
  a.nseg = (a.h + a.rows - 1) / a.rows;
  const long nblk = (long)a.N * a.nseg * a.nstrip * a.ncs;
  if (nblk > 0x7fffffffL) return shdr::fail(SHDR_E_SHAPE, "conv2d_up2_lowres: grid of %ld blocks", nblk);
  hipLaunchKernelGGL(up2_lowres_stencil_kernel, dim3((unsigned)nblk), dim3(256), 0, shdr::stream_of(stream), a);
  return shdr::check_launch("up2_lowres_stencil_kernel");
}

// The channel-vector tape kernels, once for both precisions: pooling, bilinear 2x resize, global average
// pooling, their input gradients and the BatchNorm finalisers on NHWC tensors.  pool.hip (forward) and bwd.hip (backward) instantiate
// them for fp32, elem_f16.hip for the native-fp16 activation layout of BASELINE configs[4].
//
// All HBM-bound: one thread per 16-byte channel vector -- four fp32 or eight fp16 channels, C % L == 0 -- grid-stride over
// shdr::stream_grid, coalesced along the channel axis (a wavefront touches 1 KiB contiguous).  All arithmetic is fp32 in registers;
// only the stored tensors are fp16 in the fp16 instantiations (half the bytes).  The semantics that must not drift apart -- the tie
// rule of the max-pools, the border taps of the bilinear resize, the 32-bit index decode -- are written here and nowhere else.
//
// A header, not a translation unit: elem_f16.hip is built with -ffp-contract=off, pool.hip and bwd.hip with the compiler's default,
// so the lerps of resize2x, the weighted sums of resize2x_bwd and the moving-average update of bn_finalize may be fused in the
// fp32 files and are not in the fp16 one.  Every instantiation keeps the flags of the file that makes it.
#pragma once
#include "shdr_internal.h"

namespace shdr {

// ---- the channel vector -----------------------------------------------------------------------------------------------------------------
template <int L>
struct Lanes {
  float v[L];
};
// L consecutive fp32 values as 16-byte accesses (16-byte aligned address)
template <int L>
__device__ __forceinline__ Lanes<L> ldf(const float* p) {
  Lanes<L> r;
#pragma unroll
  for (int i = 0; i < L; i += 4) {
    const float4 t = *reinterpret_cast<const float4*>(p + i);
    r.v[i] = t.x; r.v[i + 1] = t.y; r.v[i + 2] = t.z; r.v[i + 3] = t.w;
  }
  return r;
}
template <int L>
__device__ __forceinline__ void stf(float* p, const Lanes<L>& a) {
#pragma unroll
  for (int i = 0; i < L; i += 4) *reinterpret_cast<float4*>(p + i) = make_float4(a.v[i], a.v[i + 1], a.v[i + 2], a.v[i + 3]);
}

// Vec<T>: L lanes of T in 16 bytes; ld widens into fp32 lanes, st narrows.  The constants are the places where the two precisions
// really differ, in bits or in load schedule (tests/golden/nhwc_family_bits.json pins the bits of both):
//   kResizeInFlight   input vectors (nine loads each) resize2x keeps in flight per trip
//   kGapFoldFromZero  gap's fold over the 16 LDS partials starts from 0.f and adds all sixteen, else from the first partial: the two
//                     differ in the sign of a sum whose terms are all -0
//   kGapBwdDivides    gap_bwd divides by HW (one rounding), else multiplies by 1.0f / HW
template <int N>
struct VecBase {
  static constexpr int L = N, SH = N == 4 ? 2 : 3;           // lanes, log2(lanes): vectors per pixel = C >> SH
  using V = Lanes<N>;
  static __device__ __forceinline__ V zero() { return V{}; }
};
template <typename T>
struct Vec;
template <>
struct Vec<float> : VecBase<4> {
  static __device__ __forceinline__ V ld(const float* p) { return ldf<4>(p); }
  static __device__ __forceinline__ void st(float* p, const V& a) { stf<4>(p, a); }
  static constexpr int kResizeInFlight = 2;
  static constexpr bool kGapFoldFromZero = false, kGapBwdDivides = true;
};
template <>
struct Vec<_Float16> : VecBase<8> {
  static __device__ __forceinline__ V ld(const _Float16* p) {
    const f16x8 t = *reinterpret_cast<const f16x8*>(p);
    V r;
#pragma unroll
    for (int i = 0; i < 8; ++i) r.v[i] = (float)t[i];
    return r;
  }
  static __device__ __forceinline__ void st(_Float16* p, const V& a) {
    f16x8 t;
#pragma unroll
    for (int i = 0; i < 8; ++i) t[i] = (_Float16)a.v[i];
    *reinterpret_cast<f16x8*>(p) = t;
  }
  static constexpr int kResizeInFlight = 1;
  static constexpr bool kGapFoldFromZero = true, kGapBwdDivides = false;
};

// ---- index decode -------------------------------------------------------------------------------------------------------------------------
// e -> (q, w, h, n) of a [N, Hd, Wd, L * Q] tensor
// (e < 2^32 for every tensor below 64 GB: three 32-bit divisions -- about 25 instructions each -- instead of three emulated
//  64-bit ones, which cost more than the whole rest of these HBM-bound kernels; wider indices keep the 64-bit path)
#define SHDR_DECODE_VEC(e, Q, Wd, Hd, q, w, h, n)                      \
  int q, w, h;                                                          \
  long n;                                                               \
  if ((unsigned long)(e) <= 0xffffffffUL) {                             \
    unsigned _t = (unsigned)(e);                                        \
    q = (int)(_t % (unsigned)(Q)); _t /= (unsigned)(Q);                 \
    w = (int)(_t % (unsigned)(Wd)); _t /= (unsigned)(Wd);               \
    h = (int)(_t % (unsigned)(Hd)); n = (long)(_t / (unsigned)(Hd));    \
  } else {                                                              \
    long _t = (e);                                                      \
    q = (int)(_t % (Q)); _t /= (Q);                                     \
    w = (int)(_t % (Wd)); _t /= (Wd);                                   \
    h = (int)(_t % (Hd)); n = _t / (Hd);                                \
  }

// ---- 2x2 pooling --------------------------------------------------------------------------------------------------------------------------
// AveragePooling2D(2,2) VALID (dequantization_net.py:10); MAX: MaxPool2D(2,2,SAME), even dims -> no padding
// (hallucination_net.py:49, vgg16.py:54).  One thread per OUTPUT vector.
template <typename T, bool MAX>
__global__ __launch_bounds__(256) void pool2_kernel(const T* __restrict__ x, T* __restrict__ y, int N, int H, int W, int C) {
  using VT = Vec<T>;
  constexpr int L = VT::L;
  const int Ho = H >> 1, Wo = W >> 1, Q = C >> VT::SH;
  const long total = (long)N * Ho * Wo * Q;
  for (long e = (long)blockIdx.x * 256 + threadIdx.x; e < total; e += (long)gridDim.x * 256) {
    SHDR_DECODE_VEC(e, Q, Wo, Ho, q, ow, oh, n)
    const T* p = x + (((n * H + 2 * oh) * W + 2 * ow) * (long)C + L * q);
    const auto a = VT::ld(p), b = VT::ld(p + C), c = VT::ld(p + (long)W * C), d = VT::ld(p + (long)W * C + C);
    typename VT::V r;
#pragma unroll
    for (int j = 0; j < L; ++j)
      r.v[j] = MAX ? fmaxf(fmaxf(a.v[j], b.v[j]), fmaxf(c.v[j], d.v[j])) : ((a.v[j] + b.v[j]) + (c.v[j] + d.v[j])) * 0.25f;
    VT::st(y + e * L, r);
  }
}
// the backward kernels are in gather form: one thread per INPUT vector
template <typename T>
__global__ __launch_bounds__(256) void avgpool2_bwd_kernel(const T* __restrict__ dy, T* __restrict__ dx, int N, int H, int W, int C) {
  using VT = Vec<T>;
  constexpr int L = VT::L;
  const int Ho = H >> 1, Wo = W >> 1, Q = C >> VT::SH;
  const long total = (long)N * H * W * Q;
  for (long e = (long)blockIdx.x * 256 + threadIdx.x; e < total; e += (long)gridDim.x * 256) {
    SHDR_DECODE_VEC(e, Q, W, H, q, w, h, n)
    auto g = VT::zero();
    if ((h >> 1) < Ho && (w >> 1) < Wo) {
      g = VT::ld(dy + (((n * Ho + (h >> 1)) * Wo + (w >> 1)) * (long)C + L * q));
#pragma unroll
      for (int j = 0; j < L; ++j) g.v[j] *= 0.25f;
    }
    VT::st(dx + e * L, g);
  }
}
// MaxPool 2x2/2: the gradient goes to the FIRST maximum of the window in row-major scan order (one thread per window)
template <typename T>
__global__ __launch_bounds__(256) void maxpool2_bwd_kernel(const T* __restrict__ x, const T* __restrict__ dy, T* __restrict__ dx,
                                                           int N, int H, int W, int C) {
  using VT = Vec<T>;
  constexpr int L = VT::L;
  const int Ho = H >> 1, Wo = W >> 1, Q = C >> VT::SH;
  const long total = (long)N * Ho * Wo * Q;
  for (long e = (long)blockIdx.x * 256 + threadIdx.x; e < total; e += (long)gridDim.x * 256) {
    SHDR_DECODE_VEC(e, Q, Wo, Ho, q, ow, oh, n)
    const long base = ((n * H + 2 * oh) * W + 2 * ow) * (long)C + L * q;
    const long off[4] = {0, (long)C, (long)W * C, (long)W * C + C};
    typename VT::V v[4], r[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) v[k] = VT::ld(x + base + off[k]);
    const auto g = VT::ld(dy + e * L);
#pragma unroll
    for (int c = 0; c < L; ++c) {
      int arg = 0;
      float m = v[0].v[c];
#pragma unroll
      for (int k = 1; k < 4; ++k)
        if (v[k].v[c] > m) { m = v[k].v[c]; arg = k; }
#pragma unroll
      for (int k = 0; k < 4; ++k) r[k].v[c] = (k == arg) ? g.v[c] : 0.f;
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) VT::st(dx + base + off[k], r[k]);
  }
}

// ---- MaxPool2D(3,3,stride 2,SAME) -----------------------------------------------------------------------------------------------------------
// Ho = ceil(H/2); pad_total = max((Ho-1)*2+3-H, 0), pad_before = pad_total/2; padded cells never win (linearization_net.py:94).
template <typename T>
__global__ __launch_bounds__(256) void maxpool3s2_kernel(const T* __restrict__ x, T* __restrict__ y, int N, int H, int W, int C, int Ho,
                                                         int Wo, int pt, int pl) {
  using VT = Vec<T>;
  constexpr int L = VT::L;
  const int Q = C >> VT::SH;
  const long total = (long)N * Ho * Wo * Q;
  for (long e = (long)blockIdx.x * 256 + threadIdx.x; e < total; e += (long)gridDim.x * 256) {
    SHDR_DECODE_VEC(e, Q, Wo, Ho, q, ow, oh, n)
    typename VT::V m;
#pragma unroll
    for (int j = 0; j < L; ++j) m.v[j] = -__builtin_huge_valf();
#pragma unroll
    for (int i = 0; i < 3; ++i) {
      const int ih = 2 * oh - pt + i;
      if ((unsigned)ih >= (unsigned)H) continue;
#pragma unroll
      for (int k = 0; k < 3; ++k) {
        const int iw = 2 * ow - pl + k;
        if ((unsigned)iw >= (unsigned)W) continue;
        const auto t = VT::ld(x + (((n * H + ih) * W + iw) * (long)C + L * q));
#pragma unroll
        for (int j = 0; j < L; ++j) m.v[j] = fmaxf(m.v[j], t.v[j]);
      }
    }
    VT::st(y + e * L, m);
  }
}
// Overlapping windows: one thread per input vector gathers from every window that contains it and whose first maximum it is.  With
// the pooled output at hand an element is a candidate only where it equals the window's maximum (one load per window), and only the
// elements BEFORE it in the window's scan order can still take the gradient from it (the tie rule).
template <typename T>
__global__ __launch_bounds__(256) void maxpool3s2_bwd_kernel(const T* __restrict__ x, const T* __restrict__ y, const T* __restrict__ dy,
                                                             T* __restrict__ dx, int N, int H, int W, int C, int Ho, int Wo, int pt,
                                                             int pl) {
  using VT = Vec<T>;
  constexpr int L = VT::L;
  const int Q = C >> VT::SH;
  const long total = (long)N * H * W * Q;
  for (long e = (long)blockIdx.x * 256 + threadIdx.x; e < total; e += (long)gridDim.x * 256) {
    SHDR_DECODE_VEC(e, Q, W, H, q, w, h, n)
    const auto mine = VT::ld(x + e * L);
    auto acc = VT::zero();
    for (int oh = max(0, (h + pt - 1) / 2); oh <= min(Ho - 1, (h + pt) / 2); ++oh) {
      for (int ow = max(0, (w + pl - 1) / 2); ow <= min(Wo - 1, (w + pl) / 2); ++ow) {
        const int h0 = 2 * oh - pt, w0 = 2 * ow - pl;
        if (h < h0 || h > h0 + 2 || w < w0 || w > w0 + 2) continue;
        const long widx = ((n * Ho + oh) * Wo + ow) * (long)C + L * q;
        const auto m = VT::ld(y + widx);
        unsigned win = 0;                                      // bit c: lane c is this window's first maximum
#pragma unroll
        for (int c = 0; c < L; ++c) win |= (unsigned)(mine.v[c] == m.v[c]) << c;
        if (!win) continue;
        for (int ih = max(h0, 0); ih <= h; ++ih) {
          const int wend = (ih == h) ? w : min(w0 + 3, W);
          for (int iw = max(w0, 0); iw < wend; ++iw) {
            const auto t = VT::ld(x + (((n * H + ih) * W + iw) * (long)C + L * q));
#pragma unroll
            for (int c = 0; c < L; ++c) win &= ~((unsigned)(t.v[c] == mine.v[c]) << c);
          }
        }
        if (!win) continue;
        const auto g = VT::ld(dy + widx);
#pragma unroll
        for (int c = 0; c < L; ++c)
          if (win >> c & 1) acc.v[c] += g.v[c];
      }
    }
    VT::st(dx + e * L, acc);
  }
}

// ---- bilinear 2x resize ---------------------------------------------------------------------------------------------------------------------
// tf.image.resize(2x, BILINEAR), half-pixel centres (dequantization_net.py:25):
// src = (dst+0.5)/2 - 0.5 -> even dst: taps (m-1, m) lerp .75; odd dst: (m, m+1) lerp .25,
// indices clamped; value = top + (bot - top)*ly with top = l + (r - l)*lx.
// One thread owns one INPUT vector and writes its 2x2 output vectors from the 3x3 input neighbourhood (9 loads per 4 stores instead
// of 16), kResizeInFlight input vectors per trip.
template <typename T>
__global__ __launch_bounds__(256) void resize2x_kernel(const T* __restrict__ x, T* __restrict__ y, int N, int H, int W, int C) {
  using VT = Vec<T>;
  using V = typename VT::V;
  constexpr int L = VT::L, IF = VT::kResizeInFlight;
  static_assert(IF == 1 || IF == 2, "the tail below finishes at most one vector");
  const int Q = C >> VT::SH;
  const long total = (long)N * H * W * Q;
  const long orow = (long)2 * W * C;
  auto lerp = [](const V& t, const V& u, float f) {
    V r;
#pragma unroll
    for (int j = 0; j < L; ++j) r.v[j] = t.v[j] + (u.v[j] - t.v[j]) * f;
    return r;
  };
  // the 9 loads of one input vector
  auto load9 = [&](long e, V (&v)[3][3], T*& o) {
    SHDR_DECODE_VEC(e, Q, W, H, q, w, h, n)
    const int hm = max(h - 1, 0), hp = min(h + 1, H - 1), wm = max(w - 1, 0), wp = min(w + 1, W - 1);
    const T* b = x + (n * H * (long)W) * C + L * q;
    const int rows[3] = {hm, h, hp};
#pragma unroll
    for (int r = 0; r < 3; ++r) {
      const T* rp = b + (long)rows[r] * W * C;
      v[r][0] = VT::ld(rp + (long)wm * C); v[r][1] = VT::ld(rp + (long)w * C); v[r][2] = VT::ld(rp + (long)wp * C);
    }
    o = y + ((n * 2 * H + 2 * h) * (long)(2 * W) + 2 * w) * C + L * q;
  };
  auto emit = [&](const V (&v)[3][3], T* o) {
    V lo[3], hi[3];   // horizontally interpolated: lo = output column 2w, hi = output column 2w+1
#pragma unroll
    for (int r = 0; r < 3; ++r) {
      lo[r] = lerp(v[r][0], v[r][1], 0.75f);
      hi[r] = lerp(v[r][1], v[r][2], 0.25f);
    }
    VT::st(o, lerp(lo[0], lo[1], 0.75f));
    VT::st(o + C, lerp(hi[0], hi[1], 0.75f));
    VT::st(o + orow, lerp(lo[1], lo[2], 0.25f));
    VT::st(o + orow + C, lerp(hi[1], hi[2], 0.25f));
  };
  const long step = (long)gridDim.x * 256;
  long e = (long)blockIdx.x * 256 + threadIdx.x;
  for (; e + (IF - 1) * step < total; e += IF * step) {       // IF input vectors (9 loads each) in flight
    V v[IF][3][3];
    T* o[IF];
#pragma unroll
    for (int u = 0; u < IF; ++u) load9(e + u * step, v[u], o[u]);
#pragma unroll
    for (int u = 0; u < IF; ++u) emit(v[u], o[u]);
  }
  if (IF > 1 && e < total) {
    V v[3][3];
    T* o;
    load9(e, v, o);
    emit(v, o);
  }
}
// backward: per axis, input m receives {.25,.75,.75,.25} from outputs {2m-1,2m,2m+1,2m+2};
// the clamped borders fold the missing tap onto output 0 / 2H-1 (weight 1.0).
__device__ __forceinline__ void resize_taps(int m, int n_in, int* idx, float* wt, int* cnt) {
  int k = 0;
  if (m > 0) { idx[k] = 2 * m - 1; wt[k] = 0.25f; ++k; }
  idx[k] = 2 * m; wt[k] = (m == 0) ? 1.0f : 0.75f; ++k;
  idx[k] = 2 * m + 1; wt[k] = (m == n_in - 1) ? 1.0f : 0.75f; ++k;
  if (m < n_in - 1) { idx[k] = 2 * m + 2; wt[k] = 0.25f; ++k; }
  *cnt = k;
}
// RANGE: max |dx| goes to the range slot xr when xr is not null (fp32: the consumer is the input gradient of a split-operand conv)
template <typename T, bool RANGE>
__global__ __launch_bounds__(256) void resize2x_bwd_kernel(const T* __restrict__ dy, T* __restrict__ dx, int N, int H, int W, int C,
                                                           unsigned* __restrict__ xr) {
  using VT = Vec<T>;
  constexpr int L = VT::L;
  const int Q = C >> VT::SH, Ho = 2 * H, Wo = 2 * W;
  const long total = (long)N * H * W * Q;
  float dm = 0.f;
  for (long e = (long)blockIdx.x * 256 + threadIdx.x; e < total; e += (long)gridDim.x * 256) {
    SHDR_DECODE_VEC(e, Q, W, H, q, w, h, n)
    int yi[4], xi[4], ny, nx;
    float yw[4], xw[4];
    resize_taps(h, H, yi, yw, &ny);
    resize_taps(w, W, xi, xw, &nx);
    auto s = VT::zero();
    for (int a = 0; a < ny; ++a)
      for (int b = 0; b < nx; ++b) {
        const auto g = VT::ld(dy + (((n * Ho + yi[a]) * Wo + xi[b]) * (long)C + L * q));
        const float wgt = yw[a] * xw[b];
#pragma unroll
        for (int j = 0; j < L; ++j) s.v[j] += wgt * g.v[j];
      }
    VT::st(dx + e * L, s);
    if constexpr (RANGE) {
#pragma unroll
      for (int j = 0; j < L; ++j) dm = fmaxf(dm, fabsf(s.v[j]));
    }
  }
  if constexpr (RANGE) {
    if (xr) range_out_block256(xr, dm);                      // (a sum of up to nine weighted taps: not bounded by max |dy|)
  }
}
// dx[n, 2*oh, 2*ow, :] = dy[n, oh, ow, :], zero elsewhere (input gradient of a 1x1 stride-2 conv after the 1x1 dgrad has been
// evaluated on the coarse grid)
template <typename T>
__global__ __launch_bounds__(256) void upsample_zero2_kernel(const T* __restrict__ dy, T* __restrict__ dx, int N, int H, int W, int C) {
  using VT = Vec<T>;
  constexpr int L = VT::L;
  const int Q = C >> VT::SH, Ho = (H + 1) >> 1, Wo = (W + 1) >> 1;
  const long total = (long)N * H * W * Q;
  for (long e = (long)blockIdx.x * 256 + threadIdx.x; e < total; e += (long)gridDim.x * 256) {
    SHDR_DECODE_VEC(e, Q, W, H, q, w, h, n)
    auto g = VT::zero();
    if (((h | w) & 1) == 0) g = VT::ld(dy + (((n * Ho + (h >> 1)) * Wo + (w >> 1)) * (long)C + L * q));
    VT::st(dx + e * L, g);
  }
}

// ---- global average pooling -----------------------------------------------------------------------------------------------------------------
// tf.reduce_mean(x,[1,2]) (linearization_net.py:118): x [N,HW,C] -> fp32 y [N,C].
// grid (ceil(C / (16 L)), N); thread = (channel vector 0..15, pixel lane 0..15).
template <typename T>
__global__ __launch_bounds__(256) void gap_kernel(const T* __restrict__ x, float* __restrict__ y, int HW, int C) {
  using VT = Vec<T>;
  constexpr int L = VT::L;
  __shared__ __attribute__((aligned(16))) float part[16][16][L];
  const int q = threadIdx.x & 15, g = threadIdx.x >> 4;
  const int c0 = blockIdx.x * (16 * L) + L * q;
  const long n = blockIdx.y;
  auto s = VT::zero();
  if (c0 < C) {
    // four independent loads in flight per thread: the sequential form ran at the latency of 16 dependent loads (0.12 ms for
    // the 33 MB of the Linearization-Net's 16 x 256 x 2048 tensor)
    const T* xb = x + n * HW * (long)C + c0;
    auto s1 = s, s2 = s, s3 = s;
    int p = g;
    for (; p + 48 < HW; p += 64) {
      const auto a = VT::ld(xb + (long)p * C), b = VT::ld(xb + (long)(p + 16) * C), c = VT::ld(xb + (long)(p + 32) * C),
                 d = VT::ld(xb + (long)(p + 48) * C);
#pragma unroll
      for (int j = 0; j < L; ++j) { s.v[j] += a.v[j]; s1.v[j] += b.v[j]; s2.v[j] += c.v[j]; s3.v[j] += d.v[j]; }
    }
    for (; p < HW; p += 16) {
      const auto a = VT::ld(xb + (long)p * C);
#pragma unroll
      for (int j = 0; j < L; ++j) s.v[j] += a.v[j];
    }
#pragma unroll
    for (int j = 0; j < L; ++j) s.v[j] = (s.v[j] + s1.v[j]) + (s2.v[j] + s3.v[j]);
  }
#pragma unroll
  for (int j = 0; j < L; ++j) part[g][q][j] = s.v[j];
  __syncthreads();
  if (g == 0 && c0 < C) {
    const float hw = (float)HW;         // one correctly rounded division per output (sum * (1 / HW) rounds twice: 1.41 ulp at HW = 63)
#pragma unroll
    for (int j = 0; j < L; ++j) {
      float t = VT::kGapFoldFromZero ? 0.f : part[0][q][j];
#pragma unroll
      for (int i = VT::kGapFoldFromZero ? 0 : 1; i < 16; ++i) t += part[i][q][j];
      y[n * C + c0 + j] = t / hw;
    }
  }
}
// dx[n, p, :] = dy[n, :] / HW; dy is fp32 in both precisions
template <typename T>
__global__ __launch_bounds__(256) void gap_bwd_kernel(const float* __restrict__ dy, T* __restrict__ dx, long total_v, int HW, int C) {
  using VT = Vec<T>;
  constexpr int L = VT::L;
  const int Q = C >> VT::SH;
  const float hw = (float)HW, inv = 1.0f / hw;       // dy / HW, one rounding (dy * (1 / HW) rounds twice)
  for (long e = (long)blockIdx.x * 256 + threadIdx.x; e < total_v; e += (long)gridDim.x * 256) {
    const int q = (int)(e % Q);
    const long n = e / ((long)Q * HW);
    auto g = ldf<L>(dy + n * C + L * q);
#pragma unroll
    for (int j = 0; j < L; ++j) g.v[j] = VT::kGapBwdDivides ? g.v[j] / hw : g.v[j] * inv;
    VT::st(dx + e * L, g);
  }
}

// ---- BatchNormalization, training mode: what follows the per-precision reduction kernels (no operand of the tensor's type) ---------------------
// ws[col] = sum over the g partial rows ws[(1 + b) * 2C + col]: one wave per column, lanes stride over the rows
__global__ __launch_bounds__(256) static void bn_fold_kernel(double* __restrict__ ws, int C, int g) {
  const int col = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (col >= 2 * C) return;
  double t = 0.0;
  for (int b = lane; b < g; b += 64) t += ws[(size_t)(1 + b) * 2 * C + col];
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) t += __shfl_xor(t, off, 64);
  if (lane == 0) ws[col] = t;
}
// mean/var (biased) from the double sums; optional Keras moving-average update
// (momentum m: moving = moving*m + batch*(1-m); the variance update uses the unbiased estimate)
__global__ static void bn_finalize_kernel(const double* __restrict__ ws, float* __restrict__ mean, float* __restrict__ var,
                                          float* __restrict__ mov_mean, float* __restrict__ mov_var, long npix, int C, float momentum) {
  const int c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= C) return;
  const double mu = ws[c] / (double)npix;
  double v = ws[C + c] / (double)npix - mu * mu;
  if (v < 0.0) v = 0.0;
  mean[c] = (float)mu;
  var[c] = (float)v;
  if (mov_mean) {
    const double unbiased = npix > 1 ? v * (double)npix / (double)(npix - 1) : v;
    mov_mean[c] = mov_mean[c] * momentum + (float)mu * (1.0f - momentum);
    mov_var[c] = mov_var[c] * momentum + (float)unbiased * (1.0f - momentum);
  }
}
__global__ static void bn_bwd_finalize_kernel(const double* __restrict__ ws, const float* __restrict__ var, float* __restrict__ dgamma,
                                              float* __restrict__ dbeta, int C, float eps) {
  const int c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= C) return;
  dbeta[c] += (float)ws[c];
  dgamma[c] += (float)(ws[C + c] * (double)rsqrtf(var[c] + eps));
}

// ---- host side ----------------------------------------------------------------------------------------------------------------------------
// the checks every entry of the family makes on its first and last tensor: L channels per 16-byte vector
template <int L>
inline int check_nhwc(const char* op, const void* a, const void* b, int N, int H, int W, int C) {
  SHDR_REQUIRE(a && b, SHDR_E_NULL, "%s: null pointer", op);
  SHDR_REQUIRE(N > 0 && H > 0 && W > 0 && C > 0, SHDR_E_SHAPE, "%s: non-positive dimension", op);
  SHDR_REQUIRE(C % L == 0, SHDR_E_ALIGN, "%s: C=%d must be a multiple of %d (16-byte channel vectors)", op, C, L);
  SHDR_REQUIRE(aligned16(a) && aligned16(b), SHDR_E_ALIGN, "%s: tensors must be 16-byte aligned", op);
  return SHDR_OK;
}
// one thread per channel vector: stream_grid(total) blocks of 256 threads on the stream of the C ABI
template <typename... P, typename... A>
inline int launch_vec(const char* op, void (*kernel)(P...), long total, void* stream, A... args) {
  hipLaunchKernelGGL(kernel, dim3(stream_grid(total)), dim3(256), 0, stream_of(stream), static_cast<P>(args)...);
  return check_launch(op);
}

}  // namespace shdr

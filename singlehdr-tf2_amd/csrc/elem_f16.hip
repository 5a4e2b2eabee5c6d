// fp16 twins of the HBM-bound tape ops, for the native-fp16 activation layout of BASELINE configs[4] (csrc/conv_f16.hip): every
// feature map of the fine-tuning chain is NHWC fp16 with C % 8 == 0, so one thread moves 16 bytes = 8 channels; all arithmetic
// is fp32 in registers, reductions are fp32 / fp64, only the stored tensors are fp16 (half the bytes of the fp32 kernels in
// bwd.hip / glue.hip / frontend.hip, whose semantics -- BatchNorm statistics in double -- they restate).  Pooling, resize, global
// average pooling and the BatchNorm finalisers are the fp16 instantiations of nhwc_vec.h.  Image-like tensors (3 channels) stay fp32.
// Replaces the same TF op call sites as their _f32 counterparts (include/shdr.h).
#include <hip/hip_fp16.h>
#include <stdlib.h>

#include "nhwc_vec.h"

using shdr::bn_bwd_finalize_kernel;
using shdr::bn_finalize_kernel;
using shdr::bn_fold_kernel;
using shdr::launch_vec;

namespace {

typedef _Float16 hf;
using VH = shdr::Vec<hf>;            // a channel octet: 8 fp16 in 16 bytes, fp32 lanes in registers
using V8 = VH::V;

__device__ __forceinline__ float act_grad(float g, float y, int act) {
  switch (act) {
    case SHDR_ACT_RELU: return y > 0.f ? g : 0.f;
    case SHDR_ACT_LRELU: return y > 0.f ? g : 0.1f * g;
    case SHDR_ACT_TANH: return g * (1.0f - y * y);
    default: return g;
  }
}

// ---- casts / packing ----------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void cast_f32_f16_kernel(const float* __restrict__ x, hf* __restrict__ y, long n) {
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long)gridDim.x * 256) y[i] = (hf)x[i];
}
__global__ __launch_bounds__(256) void cast_f16_f32_kernel(const hf* __restrict__ x, float* __restrict__ y, long n) {
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long)gridDim.x * 256) y[i] = (float)x[i];
}
// y[p][c] = c < Cin ? x[p][c] : 0 with a dtype change (fp32 [npix, Cin] -> fp16 [npix, Cout] and back, Cout % 8 == 0 on the fp16 side)
template <typename TI, typename TO>
__global__ __launch_bounds__(256) void pad_cast_kernel(const TI* __restrict__ x, TO* __restrict__ y, long npix, int Cin, int Cout) {
  const long total = npix * Cout;
  for (long e = (long)blockIdx.x * 256 + threadIdx.x; e < total; e += (long)gridDim.x * 256) {
    const long p = e / Cout;
    const int c = (int)(e - p * Cout);
    y[e] = c < Cin ? (TO)(float)x[p * Cin + c] : (TO)0.f;
  }
}
struct Src4 {
  const float* s[4];
};
// concat of up to four 3-channel fp32 images -> fp16 [npix, OC] (zero-padded), optionally with the VGG preprocessing of
// hallucination_net.py:149-153 on source 0 (x*255, RGB -> BGR, minus mean)
__global__ __launch_bounds__(256) void pack3_h_kernel(Src4 src, int nsrc, hf* __restrict__ y, int OC, long npix, int vgg) {
  const int O = OC >> 3;
  const long total = npix * O;
  for (long e = (long)blockIdx.x * 256 + threadIdx.x; e < total; e += (long)gridDim.x * 256) {
    const long p = e / O;
    const int o = (int)(e - p * O);
    V8 r;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const int ch = 8 * o + j, s = ch / 3, c = ch - 3 * s;
      float v = 0.f;
      if (s < nsrc) {
        const float* sp = s == 0 ? src.s[0] : (s == 1 ? src.s[1] : (s == 2 ? src.s[2] : src.s[3]));
        if (vgg) {
          const float mean = c == 0 ? 103.939f : (c == 1 ? 116.779f : 123.68f);
          v = sp[3 * p + (2 - c)] * 255.0f - mean;
        } else {
          v = sp[3 * p + c];
        }
      }
      r.v[j] = v;
    }
    VH::st(y + e * 8, r);
  }
}
struct Dst4 {
  float* d[4];
};
// inverse: the first `nout` 3-channel slices of an fp16 [npix, C] tensor -> fp32 images; vgg: the backward of the preprocessing
__global__ __launch_bounds__(256) void unpack3_h_kernel(const hf* __restrict__ y, Dst4 out, int nout, int C, long npix, int vgg) {
  const long total = npix * 3 * nout;
  for (long e = (long)blockIdx.x * 256 + threadIdx.x; e < total; e += (long)gridDim.x * 256) {
    const long p = e / (3 * nout);
    const int ch = (int)(e - p * 3 * nout), s = ch / 3, c = ch - 3 * s;
    float* op = s == 0 ? out.d[0] : (s == 1 ? out.d[1] : (s == 2 ? out.d[2] : out.d[3]));
    if (vgg) op[3 * p + c] = (float)y[p * C + (2 - c)] * 255.0f;
    else op[3 * p + c] = (float)y[p * C + ch];
  }
}

// ---- activation backward + bias gradient -----------------------------------------------------------------------------------
// dz = dy * act'(y) (skipped when act == NONE: dz == dy), db[c] += sum_p dz[p][c] (skipped when db == null).  A thread's channel
// octet is fixed over its grid-stride loop (the launcher makes gridDim * 256 a multiple of O), partial sums go through LDS
// atomics, one global atomic per block and channel.
__global__ __launch_bounds__(256) void act_bwd_bias_h_kernel(const hf* __restrict__ dy, const hf* __restrict__ y, hf* __restrict__ dz,
                                                             float* __restrict__ db, float* __restrict__ ws, long nvec, int O, int act) {
  extern __shared__ float sdb[];                              // [8 * O]
  if (db) {
    for (int i = threadIdx.x; i < 8 * O; i += 256) sdb[i] = 0.f;
    __syncthreads();
  }
  float s[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  const long step = (long)gridDim.x * 256;
  long e = (long)blockIdx.x * 256 + threadIdx.x;
  const int o = (int)(e % O);
  auto one = [&](long i, const V8& g, const V8& yv) {
    V8 d = g;
    if (act != SHDR_ACT_NONE) {
#pragma unroll
      for (int j = 0; j < 8; ++j) d.v[j] = act_grad(g.v[j], yv.v[j], act);
      VH::st(dz + 8 * i, d);
    }
#pragma unroll
    for (int j = 0; j < 8; ++j) s[j] += d.v[j];
  };
  for (; e + 3 * step < nvec; e += 4 * step) {                // four vectors per operand in flight
    V8 g[4], yv[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      g[u] = VH::ld(dy + 8 * (e + u * step));
      yv[u] = g[u];
      if (act != SHDR_ACT_NONE) yv[u] = VH::ld(y + 8 * (e + u * step));
    }
#pragma unroll
    for (int u = 0; u < 4; ++u) one(e + u * step, g[u], yv[u]);
  }
  for (; e < nvec; e += step) {
    const V8 g0 = VH::ld(dy + 8 * e);
    V8 y0 = g0;
    if (act != SHDR_ACT_NONE) y0 = VH::ld(y + 8 * e);
    one(e, g0, y0);
  }
  if (db) {
#pragma unroll
    for (int j = 0; j < 8; ++j) atomicAdd(&sdb[8 * o + j], s[j]);
    __syncthreads();
    if (ws) {                                                  // this block's partial row (folded by shdr::col_fold_kernel)
      for (int i = threadIdx.x; i < 8 * O; i += 256) ws[(size_t)blockIdx.x * 8 * O + i] = sdb[i];
    } else {
      for (int i = threadIdx.x; i < 8 * O; i += 256) atomicAdd(db + i, sdb[i]);
    }
  }
}

// y = act(a + b): the fan-in joins of the tape (residual adds, gradient accumulation at fan-out points)
__global__ __launch_bounds__(256) void add_h_kernel(const hf* __restrict__ a, const hf* __restrict__ b, hf* __restrict__ y, long nvec,
                                                    int relu) {
  for (long e = (long)blockIdx.x * 256 + threadIdx.x; e < nvec; e += (long)gridDim.x * 256) {
    const V8 x0 = VH::ld(a + 8 * e), x1 = VH::ld(b + 8 * e);
    V8 r;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      r.v[j] = x0.v[j] + x1.v[j];
      if (relu) r.v[j] = fmaxf(r.v[j], 0.f);
    }
    VH::st(y + 8 * e, r);
  }
}

// ---- BatchNormalization, training mode (statistics in double, as bn_reduce4_kernel) -------------------------------------------
//   mode 0 : ws[c] += sum x,   ws[C + c] += sum x*x
//   mode 1 : ws[c] += sum dy', ws[C + c] += sum dy' * (x - mean),   dy' = dy masked by y > 0 when y != null
__global__ __launch_bounds__(256) void bn_reduce_h_kernel(const hf* __restrict__ a, const hf* __restrict__ x, const hf* __restrict__ y,
                                                          const float* __restrict__ mean, double* __restrict__ ws, long npix, int C, int mode) {
  __shared__ double part[16][256];
  const int O = C >> 3;
  int OL = 1;
  while (OL < O && OL < 256) OL <<= 1;
  const int PL = 256 / OL;
  const int ol = threadIdx.x % OL, pl = threadIdx.x / OL;
  for (int o0 = 0; o0 < O; o0 += OL) {
    const int o = o0 + ol;
    double s1[8], s2[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) { s1[j] = 0.0; s2[j] = 0.0; }
    if (o < O) {
      V8 mu = VH::zero();
      if (mode) mu = shdr::ldf<8>(mean + 8 * o);
      const long step = (long)gridDim.x * PL;
      // fp32 partial sums over short runs (<= 16 pixels: their rounding is 2^-24 relative, far below the fp16 input), folded into
      // the double accumulators once per run -- the double adds of every element made the kernel VALU-bound at ~2 TB/s
      float f1[8], f2[8];
#pragma unroll
      for (int j = 0; j < 8; ++j) { f1[j] = 0.f; f2[j] = 0.f; }
      int run = 0;
      auto acc = [&](const V8& av, const V8& xv, const V8& yv) {
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          if (mode == 0) {
            f1[j] += av.v[j]; f2[j] += av.v[j] * av.v[j];
          } else {
            const float gg = (y && !(yv.v[j] > 0.f)) ? 0.f : av.v[j];
            f1[j] += gg; f2[j] += gg * (xv.v[j] - mu.v[j]);
          }
        }
      };
      auto fold = [&]() {
#pragma unroll
        for (int j = 0; j < 8; ++j) { s1[j] += (double)f1[j]; s2[j] += (double)f2[j]; f1[j] = 0.f; f2[j] = 0.f; }
        run = 0;
      };
      long p = (long)blockIdx.x * PL + pl;
      if (mode == 0) {
        for (; p + 7 * step < npix; p += 8 * step) {         // statistics pass: eight 16-byte loads in flight per thread
          V8 av[8];
#pragma unroll
          for (int u = 0; u < 8; ++u) av[u] = VH::ld(a + (p + u * step) * C + 8 * o);
#pragma unroll
          for (int u = 0; u < 8; ++u) acc(av[u], av[u], av[u]);
          run += 8;
          if (run >= 16) fold();
        }
      }
      for (; p + 3 * step < npix; p += 4 * step) {           // four vectors per operand in flight
        V8 av[4], xv[4], yv[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
          const long i = (p + u * step) * C + 8 * o;
          av[u] = VH::ld(a + i);
          xv[u] = av[u]; yv[u] = av[u];
          if (mode) {
            xv[u] = VH::ld(x + i);
            if (y) yv[u] = VH::ld(y + i);
          }
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) acc(av[u], xv[u], yv[u]);
        run += 4;
        if (run >= 16) fold();
      }
      for (; p < npix; p += step) {
        const long i = p * C + 8 * o;
        const V8 a0 = VH::ld(a + i);
        V8 x0 = a0, y0 = a0;
        if (mode) {
          x0 = VH::ld(x + i);
          if (y) y0 = VH::ld(y + i);
        }
        acc(a0, x0, y0);
      }
      fold();
    }
#pragma unroll
    for (int j = 0; j < 8; ++j) { part[j][threadIdx.x] = s1[j]; part[8 + j][threadIdx.x] = s2[j]; }
    __syncthreads();
    if (pl == 0 && o < O) {
      double* wp = ws + (size_t)(1 + blockIdx.x) * 2 * C;       // this block's partial row; summed by bn_fold_kernel (no atomics, no memset)
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        double t1 = s1[j], t2 = s2[j];
        for (int k = 1; k < PL; ++k) { t1 += part[j][k * OL + ol]; t2 += part[8 + j][k * OL + ol]; }
        wp[8 * o + j] = t1;
        wp[C + 8 * o + j] = t2;
      }
    }
    __syncthreads();
  }
}
// forward apply (mode 0): y = [relu]((x - mean) * rstd * gamma + beta);  backward apply (mode 1):
// dx = gamma * rstd * (dy' - mean(dy') - xhat * mean(dy' * xhat)).  The launcher makes gridDim * 256 a multiple of O, so the
// per-channel factors are computed once per thread.
__global__ __launch_bounds__(256) void bn_apply_h_kernel(const hf* __restrict__ a, const hf* __restrict__ x, const hf* __restrict__ y,
                                                         const float* __restrict__ mean, const float* __restrict__ var,
                                                         const float* __restrict__ gamma, const float* __restrict__ beta,
                                                         const double* __restrict__ ws, hf* __restrict__ out, long nvec, long npix, int C,
                                                         float eps, int relu, int mode) {
  const int O = C >> 3;
  const int o = (int)(((long)blockIdx.x * 256 + threadIdx.x) % O);
  float rstd[8], mu[8], k0[8], k1[8], k2[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    const int c = 8 * o + j;
    rstd[j] = rsqrtf(var[c] + eps);
    mu[j] = mean[c];
    if (mode == 0) {
      k0[j] = rstd[j] * gamma[c];
      k1[j] = beta[c];
      k2[j] = 0.f;
    } else {
      k0[j] = gamma[c] * rstd[j];
      k1[j] = (float)(ws[c] / (double)npix);
      k2[j] = (float)(ws[C + c] / (double)npix) * rstd[j];
    }
  }
  for (long e = (long)blockIdx.x * 256 + threadIdx.x; e < nvec; e += (long)gridDim.x * 256) {
    V8 r;
    if (mode == 0) {
      const V8 xv = VH::ld(a + 8 * e);
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        r.v[j] = (xv.v[j] - mu[j]) * k0[j] + k1[j];
        if (relu) r.v[j] = fmaxf(r.v[j], 0.f);
      }
    } else {
      V8 g = VH::ld(a + 8 * e);
      const V8 xv = VH::ld(x + 8 * e);
      if (y) {
        const V8 yv = VH::ld(y + 8 * e);
#pragma unroll
        for (int j = 0; j < 8; ++j)
          if (!(yv.v[j] > 0.f)) g.v[j] = 0.f;
      }
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const float xh = (xv.v[j] - mu[j]) * rstd[j];
        r.v[j] = k0[j] * (g.v[j] - k1[j] - xh * k2[j]);
      }
    }
    VH::st(out + 8 * e, r);
  }
}

// ---- Linearization-Net front end (linearization_net.py:310-322, 336-350) -> fp16 [N,H,W,96] and its backward --------------------
// channel layout as lin_frontend_rows_kernel: [img 3 | sobel 6 (c*2 + {dy,dx}) | hist4 12 | hist8 24 | hist16 48 | 0 0 0]
__device__ __forceinline__ float lin_feature(const float* __restrict__ img, long n, int h, int w, int H, int W, int ch) {
  const long base = (n * H + h) * (long)W + w;
  if (ch < 3) return img[3 * base + ch];
  if (ch < 9) {
    const int c = (ch - 3) >> 1, k = (ch - 3) & 1;            // k = 0: dy kernel [[-1,-2,-1],[0,0,0],[1,2,1]], 1: its transpose
    auto at = [&](int hh, int ww) {                           // REFLECT padding by one
      hh = hh < 0 ? -hh : (hh >= H ? 2 * H - 2 - hh : hh);
      ww = ww < 0 ? -ww : (ww >= W ? 2 * W - 2 - ww : ww);
      return img[3 * ((n * H + hh) * (long)W + ww) + c];
    };
    if (k == 0)
      return (at(h + 1, w - 1) + 2.f * at(h + 1, w) + at(h + 1, w + 1)) - (at(h - 1, w - 1) + 2.f * at(h - 1, w) + at(h - 1, w + 1));
    return (at(h - 1, w + 1) + 2.f * at(h, w + 1) + at(h + 1, w + 1)) - (at(h - 1, w - 1) + 2.f * at(h, w - 1) + at(h + 1, w - 1));
  }
  if (ch >= 93) return 0.f;
  int B, r;
  if (ch < 21) { B = 4; r = ch - 9; } else if (ch < 45) { B = 8; r = ch - 21; } else { B = 16; r = ch - 45; }
  const int bin = r / 3 + 1, c = r - 3 * (r / 3);
  const float xv = img[3 * base + c];
  const float centre = (float)(2 * bin - 1) / (float)(2 * B);
  const float d = fabsf(xv - centre);
  return d < 1.0f / (float)B ? 1.0f - d * (float)B : 0.0f;
}
// Block roles (no divergence inside a wave): every sixth block writes the two leading octets (image, sobel, first histogram channels:
// the general per-channel form, 18 neighbour loads per pixel and colour), the others the ten pure-histogram octets -- a thread owns ONE
// of them for all its pixels, so bin centre, bin count and colour index of its eight channels are computed once, then 3 loads + 8 hat
// functions + one 16-byte store per pixel (the element-major form decoded the channel per value: 0.92 ms for 4 x 1024^2).  YC = 96.
__global__ __launch_bounds__(256) void lin_frontend_h_kernel(const float* __restrict__ img, hf* __restrict__ y, int N, int H, int W, int YC) {
  const int O = YC >> 3;
  const long npix = (long)N * H * W;
  const bool lead = blockIdx.x % 6 == 0;
  if (!lead) {
    const int OH = O - 2;                                      // histogram octets 2 .. O-1
    const long bid = blockIdx.x - blockIdx.x / 6 - 1, nb = gridDim.x - (gridDim.x + 5) / 6;       // index among the histogram blocks
    const long t0 = bid * 256 + threadIdx.x, nthr = nb * 256;  // nthr is a multiple of OH (launcher)
    const int o = 2 + (int)(t0 % OH);
    int cj[8];
    float centre[8], fB[8], wB[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const int ch = 8 * o + j;
      int B = 4, r = ch - 9;
      if (ch >= 45) { B = 16; r = ch - 45; } else if (ch >= 21) { B = 8; r = ch - 21; }
      const int bin = r / 3 + 1;
      cj[j] = ch < 93 ? r - 3 * (r / 3) : -1;
      centre[j] = (float)(2 * bin - 1) / (float)(2 * B);
      fB[j] = (float)B;
      wB[j] = 1.0f / (float)B;
    }
    for (long p = t0 / OH; p < npix; p += nthr / OH) {
      const float x3[3] = {img[3 * p], img[3 * p + 1], img[3 * p + 2]};
      V8 r;
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const float xv = cj[j] == 1 ? x3[1] : (cj[j] == 2 ? x3[2] : x3[0]);
        const float d = fabsf(xv - centre[j]);
        r.v[j] = (cj[j] >= 0 && d < wB[j]) ? 1.0f - d * fB[j] : 0.0f;
      }
      VH::st(y + (p * O + o) * 8, r);
    }
  } else {
    const long bid = blockIdx.x / 6, nb = (gridDim.x + 5) / 6;
    const long t0 = bid * 256 + threadIdx.x, nthr = nb * 256;
    const int o = (int)(t0 & 1);
    for (long p = t0 >> 1; p < npix; p += nthr >> 1) {
      const int w = (int)(p % W);
      const long t = p / W;
      const int h = (int)(t % H);
      const long n = t / H;
      V8 r;
#pragma unroll
      for (int j = 0; j < 8; ++j) r.v[j] = lin_feature(img, n, h, w, H, W, 8 * o + j);
      VH::st(y + (p * O + o) * 8, r);
    }
  }
}
// dimg[n,h,w,c] = dF[c] + sum of the sobel transposes + sum_bins dF[hist] * (-+B inside the bin support); gather form, no atomics
__global__ __launch_bounds__(256) void lin_frontend_bwd_h_kernel(const float* __restrict__ img, const hf* __restrict__ dF,
                                                                 float* __restrict__ dimg, int N, int H, int W, int YC) {
  const long total = (long)N * H * W * 3;
  for (long e = (long)blockIdx.x * 256 + threadIdx.x; e < total; e += (long)gridDim.x * 256) {
    const int c = (int)(e % 3);
    const long pix = e / 3;
    const int w = (int)(pix % W);
    const long t = pix / W;
    const int h = (int)(t % H);
    const long n = t / H;
    const hf* g = dF + pix * YC;
    float acc = (float)g[c];
    const float xv = img[e];
    // histogram slopes: h = 1 - |x - centre| * B inside the support
    const int Bs[3] = {4, 8, 16}, offs[3] = {9, 21, 45};
#pragma unroll
    for (int s = 0; s < 3; ++s) {
      const int B = Bs[s];
      for (int bin = 1; bin <= B; ++bin) {
        const float centre = (float)(2 * bin - 1) / (float)(2 * B);
        const float d = xv - centre;
        if (fabsf(d) < 1.0f / (float)B) acc += (float)g[offs[s] + 3 * (bin - 1) + c] * (d > 0.f ? -(float)B : (d < 0.f ? (float)B : 0.f));
      }
    }
    // sobel transpose: output pixel (hh, ww) read input (reflect(hh+i-1), reflect(ww+j-1)) with weight k[i][j]; gather every
    // output pixel whose reflected tap lands on (h, w)
    for (int hh = h - 2; hh <= h + 2; ++hh) {
      if (hh < 0 || hh >= H) continue;
      for (int ww = w - 2; ww <= w + 2; ++ww) {
        if (ww < 0 || ww >= W) continue;
        float wy = 0.f, wx = 0.f;
#pragma unroll
        for (int i = -1; i <= 1; ++i) {
          int rh = hh + i;
          rh = rh < 0 ? -rh : (rh >= H ? 2 * H - 2 - rh : rh);
          if (rh != h) continue;
#pragma unroll
          for (int j = -1; j <= 1; ++j) {
            int rw = ww + j;
            rw = rw < 0 ? -rw : (rw >= W ? 2 * W - 2 - rw : rw);
            if (rw != w) continue;
            wy += (float)i * (j == 0 ? 2.f : 1.f);           // dy kernel: rows -1 / +1 weighted (1,2,1)
            wx += (float)j * (i == 0 ? 2.f : 1.f);           // dx kernel: its transpose
          }
        }
        if (wy != 0.f || wx != 0.f) {
          const hf* go = dF + ((n * H + hh) * (long)W + ww) * YC + 3 + 2 * c;
          acc += wy * (float)go[0] + wx * (float)go[1];
        }
      }
    }
    dimg[e] = acc;
  }
}

// grid whose thread count is a multiple of O (a thread keeps its channel octet), at most `cap` blocks
inline int octet_grid(long nvec, int O, int cap) {
  long g = (nvec + 255) / 256;
  if (g > cap) g = cap;
  if (g < 1) g = 1;
  int unit = O;
  for (int d = 256; d > 1; d >>= 1)
    if (unit % 2 == 0 && d > 1) { unit /= 2; } else break;      // unit = O / gcd(O, 256)
  g = (g + unit - 1) / unit * unit;
  return (int)g;
}
typedef const hf* HP;
typedef hf* HM;

}  // namespace

#define H_(p) reinterpret_cast<HP>(p)
#define HM_(p) reinterpret_cast<HM>(p)

extern "C" int shdr_cast_f32_to_f16(const float* x, void* y, int64_t n, void* stream) {
  SHDR_REQUIRE(x && y && n > 0, SHDR_E_NULL, "cast: bad arguments");
  hipLaunchKernelGGL(cast_f32_f16_kernel, dim3(shdr::stream_grid(n)), dim3(256), 0, shdr::stream_of(stream), x, HM_(y), (long)n);
  return shdr::check_launch("cast_f32_to_f16");
}
extern "C" int shdr_cast_f16_to_f32(const void* x, float* y, int64_t n, void* stream) {
  SHDR_REQUIRE(x && y && n > 0, SHDR_E_NULL, "cast: bad arguments");
  hipLaunchKernelGGL(cast_f16_f32_kernel, dim3(shdr::stream_grid(n)), dim3(256), 0, shdr::stream_of(stream), H_(x), y, (long)n);
  return shdr::check_launch("cast_f16_to_f32");
}
extern "C" int shdr_pad_channels_f32_to_f16(const float* x, void* y, int64_t npix, int Cin, int Cout, void* stream) {
  SHDR_REQUIRE(x && y, SHDR_E_NULL, "pad_channels: null pointer");
  SHDR_REQUIRE(npix > 0 && Cin > 0 && Cout >= Cin, SHDR_E_SHAPE, "pad_channels: need Cout >= Cin > 0");
  hipLaunchKernelGGL((pad_cast_kernel<float, hf>), dim3(shdr::stream_grid(npix * Cout)), dim3(256), 0, shdr::stream_of(stream), x, HM_(y), (long)npix, Cin, Cout);
  return shdr::check_launch("pad_channels_f32_to_f16");
}
extern "C" int shdr_pack3_f16(const float* s0, const float* s1, const float* s2, const float* s3, int nsrc, void* y, int out_channels,
                              int64_t npix, int vgg_preprocess, void* stream) {
  SHDR_REQUIRE(y && s0, SHDR_E_NULL, "pack3_f16: null pointer");
  SHDR_REQUIRE(nsrc >= 1 && nsrc <= 4 && out_channels >= 3 * nsrc && out_channels % 8 == 0 && npix > 0, SHDR_E_SHAPE,
               "pack3_f16: need 1 <= nsrc <= 4, out_channels >= 3 * nsrc, out_channels %% 8 == 0");
  SHDR_REQUIRE(!vgg_preprocess || nsrc == 1, SHDR_E_SHAPE, "pack3_f16: the VGG preprocessing takes one source");
  SHDR_REQUIRE(shdr::aligned16(y), SHDR_E_ALIGN, "pack3_f16: y must be 16-byte aligned");
  const float* s[4] = {s0, s1, s2, s3};
  for (int i = 0; i < nsrc; ++i) SHDR_REQUIRE(s[i], SHDR_E_NULL, "pack3_f16: source %d is null", i);
  Src4 src{{s0, s1, s2, s3}};
  hipLaunchKernelGGL(pack3_h_kernel, dim3(shdr::stream_grid(npix * (out_channels / 8))), dim3(256), 0, shdr::stream_of(stream), src, nsrc, HM_(y),
                     out_channels, (long)npix, vgg_preprocess);
  return shdr::check_launch("pack3_f16");
}
extern "C" int shdr_unpack3_f16(const void* y, float* o0, float* o1, float* o2, float* o3, int nout, int channels, int64_t npix,
                                int vgg_preprocess_bwd, void* stream) {
  SHDR_REQUIRE(y && o0, SHDR_E_NULL, "unpack3_f16: null pointer");
  SHDR_REQUIRE(nout >= 1 && nout <= 4 && channels >= 3 * nout && npix > 0, SHDR_E_SHAPE, "unpack3_f16: need 1 <= nout <= 4, channels >= 3 * nout");
  float* o[4] = {o0, o1, o2, o3};
  for (int i = 0; i < nout; ++i) SHDR_REQUIRE(o[i], SHDR_E_NULL, "unpack3_f16: output %d is null", i);
  Dst4 dst{{o0, o1, o2, o3}};
  hipLaunchKernelGGL(unpack3_h_kernel, dim3(shdr::stream_grid(npix * 3 * nout)), dim3(256), 0, shdr::stream_of(stream), H_(y), dst, nout, channels,
                     (long)npix, vgg_preprocess_bwd);
  return shdr::check_launch("unpack3_f16");
}
extern "C" int shdr_act_bwd_bias_f16(const void* dy, const void* y, void* dz, float* db, float* ws, int64_t npix, int C, int act, void* stream) {
  SHDR_REQUIRE(dy, SHDR_E_NULL, "act_bwd_bias_f16: null pointer");
  SHDR_REQUIRE(act == SHDR_ACT_NONE || (y && dz), SHDR_E_NULL, "act_bwd_bias_f16: y and dz are needed with an activation");
  SHDR_REQUIRE(npix > 0 && C > 0 && C % 8 == 0 && C <= 4096 && act >= 0 && act <= 3, SHDR_E_SHAPE, "act_bwd_bias_f16: bad arguments (C %% 8 == 0)");
  SHDR_REQUIRE(shdr::aligned16(dy) && (!y || shdr::aligned16(y)) && (!dz || shdr::aligned16(dz)), SHDR_E_ALIGN,
               "act_bwd_bias_f16: tensors must be 16-byte aligned");
  const int O = C / 8;
  const long nvec = (long)npix * O;
  const bool rows = db && ws && nvec >= (1L << 22);   // partial rows + fold instead of atomics on the same C addresses (pays from ~64 MB on)
  const int cap = db && !rows ? (nvec >= (1L << 23) ? 512 : 256) : 2048;
  int grid = octet_grid(nvec, O, cap);
  if (rows && grid > shdr::kBiasMaxBlocks) grid = octet_grid(nvec, O, shdr::kBiasMaxBlocks / 2);       // the rounding up to the octet unit stays below the row count
  if (db) shdr::count_order_dependent();                  // (fp32 atomics into the block's LDS sums, then into db or through the fold)
  hipLaunchKernelGGL(act_bwd_bias_h_kernel, dim3(grid), dim3(256), db ? 8 * O * sizeof(float) : 0, shdr::stream_of(stream), H_(dy),
                     H_(y), HM_(dz), db, rows ? ws : (float*)nullptr, nvec, O, act);
  if (rows) shdr::launch_col_fold(ws, db, grid, C, shdr::stream_of(stream));
  return shdr::check_launch("act_bwd_bias_f16");
}
extern "C" int shdr_add_f16(const void* a, const void* b, void* y, int64_t n, int relu, void* stream) {
  SHDR_REQUIRE(a && b && y, SHDR_E_NULL, "add_f16: null pointer");
  SHDR_REQUIRE(n > 0 && n % 8 == 0, SHDR_E_SHAPE, "add_f16: n must be a positive multiple of 8");
  SHDR_REQUIRE(shdr::aligned16(a) && shdr::aligned16(b) && shdr::aligned16(y), SHDR_E_ALIGN, "add_f16: tensors must be 16-byte aligned");
  hipLaunchKernelGGL(add_h_kernel, dim3(shdr::stream_grid(n / 8)), dim3(256), 0, shdr::stream_of(stream), H_(a), H_(b), HM_(y), (long)(n / 8), relu);
  return shdr::check_launch("add_f16");
}
// pooling / resize / global average pooling: nhwc_vec.h (launch_vec turns the ABI's void pointers into the kernel's)
extern "C" int shdr_avgpool2_fwd_f16(const void* x, void* y, int N, int H, int W, int C, void* stream) {
  if (int rc = shdr::check_nhwc<8>("avgpool2_f16", x, y, N, H, W, C)) return rc;
  SHDR_REQUIRE(H >= 2 && W >= 2, SHDR_E_SHAPE, "avgpool2_f16: H, W must be >= 2");
  return launch_vec("avgpool2_f16", shdr::pool2_kernel<hf, false>, (long)N * (H / 2) * (W / 2) * (C / 8), stream, x, y, N, H, W, C);
}
extern "C" int shdr_maxpool2_fwd_f16(const void* x, void* y, int N, int H, int W, int C, void* stream) {
  if (int rc = shdr::check_nhwc<8>("maxpool2_f16", x, y, N, H, W, C)) return rc;
  SHDR_REQUIRE((H & 1) == 0 && (W & 1) == 0, SHDR_E_SHAPE, "maxpool2_f16: H, W must be even");
  return launch_vec("maxpool2_f16", shdr::pool2_kernel<hf, true>, (long)N * (H / 2) * (W / 2) * (C / 8), stream, x, y, N, H, W, C);
}
extern "C" int shdr_avgpool2_bwd_f16(const void* dy, void* dx, int N, int H, int W, int C, void* stream) {
  if (int rc = shdr::check_nhwc<8>("avgpool2_bwd_f16", dy, dx, N, H, W, C)) return rc;
  return launch_vec("avgpool2_bwd_f16", shdr::avgpool2_bwd_kernel<hf>, (long)N * H * W * (C / 8), stream, dy, dx, N, H, W, C);
}
extern "C" int shdr_maxpool2_bwd_f16(const void* x, const void* dy, void* dx, int N, int H, int W, int C, void* stream) {
  if (int rc = shdr::check_nhwc<8>("maxpool2_bwd_f16", x, dx, N, H, W, C)) return rc;
  SHDR_REQUIRE(dy && shdr::aligned16(dy), SHDR_E_NULL, "maxpool2_bwd_f16: dy null or unaligned");
  SHDR_REQUIRE((H & 1) == 0 && (W & 1) == 0, SHDR_E_SHAPE, "maxpool2_bwd_f16: H, W must be even");
  return launch_vec("maxpool2_bwd_f16", shdr::maxpool2_bwd_kernel<hf>, (long)N * (H / 2) * (W / 2) * (C / 8), stream, x, dy, dx, N, H, W, C);
}
extern "C" int shdr_maxpool3s2_fwd_f16(const void* x, void* y, int N, int H, int W, int C, void* stream) {
  if (int rc = shdr::check_nhwc<8>("maxpool3s2_f16", x, y, N, H, W, C)) return rc;
  int Ho, Wo, pt, pl;
  shdr_same_pad(H, 3, 2, &Ho, &pt);
  shdr_same_pad(W, 3, 2, &Wo, &pl);
  return launch_vec("maxpool3s2_f16", shdr::maxpool3s2_kernel<hf>, (long)N * Ho * Wo * (C / 8), stream, x, y, N, H, W, C, Ho, Wo, pt, pl);
}
extern "C" int shdr_maxpool3s2_bwd_f16(const void* x, const void* y, const void* dy, void* dx, int N, int H, int W, int C, void* stream) {
  if (int rc = shdr::check_nhwc<8>("maxpool3s2_bwd_f16", x, dx, N, H, W, C)) return rc;
  SHDR_REQUIRE(dy && shdr::aligned16(dy), SHDR_E_NULL, "maxpool3s2_bwd_f16: dy null or unaligned");
  SHDR_REQUIRE(y && shdr::aligned16(y), SHDR_E_NULL, "maxpool3s2_bwd_f16: y (the pooled output) null or unaligned");
  int Ho, Wo, pt, pl;
  shdr_same_pad(H, 3, 2, &Ho, &pt);
  shdr_same_pad(W, 3, 2, &Wo, &pl);
  return launch_vec("maxpool3s2_bwd_f16", shdr::maxpool3s2_bwd_kernel<hf>, (long)N * H * W * (C / 8), stream, x, y, dy, dx, N, H, W, C, Ho,
                    Wo, pt, pl);
}
extern "C" int shdr_resize2x_fwd_f16(const void* x, void* y, int N, int H, int W, int C, void* stream) {
  if (int rc = shdr::check_nhwc<8>("resize2x_f16", x, y, N, H, W, C)) return rc;
  return launch_vec("resize2x_f16", shdr::resize2x_kernel<hf>, (long)N * H * W * (C / 8), stream, x, y, N, H, W, C);
}
extern "C" int shdr_resize2x_bwd_f16(const void* dy, void* dx, int N, int H, int W, int C, void* stream) {
  if (int rc = shdr::check_nhwc<8>("resize2x_bwd_f16", dy, dx, N, H, W, C)) return rc;
  return launch_vec("resize2x_bwd_f16", shdr::resize2x_bwd_kernel<hf, false>, (long)N * H * W * (C / 8), stream, dy, dx, N, H, W, C, nullptr);
}
extern "C" int shdr_upsample_zero2_f16(const void* dy, void* dx, int N, int H, int W, int C, void* stream) {
  if (int rc = shdr::check_nhwc<8>("upsample_zero2_f16", dy, dx, N, H, W, C)) return rc;
  return launch_vec("upsample_zero2_f16", shdr::upsample_zero2_kernel<hf>, (long)N * H * W * (C / 8), stream, dy, dx, N, H, W, C);
}
extern "C" int shdr_gap_fwd_f16(const void* x, float* y, int N, int HW, int C, void* stream) {
  if (int rc = shdr::check_nhwc<8>("gap_f16", x, y, N, HW, 1, C)) return rc;
  hipLaunchKernelGGL(shdr::gap_kernel<hf>, dim3((C + 127) / 128, N), dim3(256), 0, shdr::stream_of(stream), H_(x), y, HW, C);
  return shdr::check_launch("gap_f16");
}
extern "C" int shdr_gap_bwd_f16(const float* dy, void* dx, int N, int HW, int C, void* stream) {
  if (int rc = shdr::check_nhwc<8>("gap_bwd_f16", dy, dx, N, HW, 1, C)) return rc;
  const long tv = (long)N * HW * (C / 8);
  return launch_vec("gap_bwd_f16", shdr::gap_bwd_kernel<hf>, tv, stream, dy, dx, tv, HW, C);
}
namespace {
inline void launch_bn_reduce_h(hipStream_t st, HP a, HP x, HP y, const float* mean, double* ws, long npix, int C, int mode) {
  const int O = C / 8;
  int OL = 1;
  while (OL < O && OL < 256) OL <<= 1;
  const long PL = 256 / OL;
  long g = (npix + PL * 16 - 1) / (PL * 16);
  g = g < 1 ? 1 : (g > SHDR_BN_MAX_BLOCKS ? SHDR_BN_MAX_BLOCKS : g);       // every block owns a partial row of the workspace
  hipLaunchKernelGGL(bn_reduce_h_kernel, dim3((unsigned)g), dim3(256), 0, st, a, x, y, mean, ws, npix, C, mode);
  hipLaunchKernelGGL(bn_fold_kernel, dim3((unsigned)((2 * C + 3) / 4)), dim3(256), 0, st, ws, C, (int)g);
}
}  // namespace
extern "C" int shdr_bn_stats_f16(const void* x, double* ws, float* mean, float* var, float* moving_mean, float* moving_var, int64_t npix,
                                 int C, float momentum, void* stream) {
  SHDR_REQUIRE(x && ws && mean && var, SHDR_E_NULL, "bn_stats_f16: null pointer");
  SHDR_REQUIRE((moving_mean == nullptr) == (moving_var == nullptr), SHDR_E_NULL, "bn_stats_f16: moving stats come in pairs");
  SHDR_REQUIRE(npix > 0 && C > 0 && C % 8 == 0, SHDR_E_SHAPE, "bn_stats_f16: bad shape (C %% 8 == 0)");
  SHDR_REQUIRE(shdr::aligned16(x), SHDR_E_ALIGN, "bn_stats_f16: x must be 16-byte aligned");
  hipStream_t st = shdr::stream_of(stream);
  launch_bn_reduce_h(st, H_(x), nullptr, nullptr, nullptr, ws, (long)npix, C, 0);
  hipLaunchKernelGGL(bn_finalize_kernel, dim3((C + 255) / 256), dim3(256), 0, st, ws, mean, var, moving_mean, moving_var, (long)npix, C, momentum);
  return shdr::check_launch("bn_stats_f16");
}
extern "C" int shdr_bn_train_apply_f16(const void* x, const float* mean, const float* var, const float* gamma, const float* beta, void* y,
                                       int64_t npix, int C, float eps, int relu, void* stream) {
  SHDR_REQUIRE(x && mean && var && gamma && beta && y, SHDR_E_NULL, "bn_train_apply_f16: null pointer");
  SHDR_REQUIRE(npix > 0 && C > 0 && C % 8 == 0, SHDR_E_SHAPE, "bn_train_apply_f16: bad shape (C %% 8 == 0)");
  SHDR_REQUIRE(shdr::aligned16(x) && shdr::aligned16(y), SHDR_E_ALIGN, "bn_train_apply_f16: x and y must be 16-byte aligned");
  const long nvec = (long)npix * (C / 8);
  hipLaunchKernelGGL(bn_apply_h_kernel, dim3(octet_grid(nvec, C / 8, 2048)), dim3(256), 0, shdr::stream_of(stream), H_(x), (HP) nullptr, (HP) nullptr, mean, var,
                     gamma, beta, (const double*)nullptr, HM_(y), nvec, (long)npix, C, eps, relu, 0);
  return shdr::check_launch("bn_train_apply_f16");
}
extern "C" int shdr_bn_bwd_f16(const void* dy, const void* x, const void* y_relu, const float* mean, const float* var, const float* gamma,
                               double* ws, float* dgamma, float* dbeta, void* dx, int64_t npix, int C, float eps, void* stream) {
  SHDR_REQUIRE(dy && x && mean && var && gamma && ws && dgamma && dbeta && dx, SHDR_E_NULL, "bn_bwd_f16: null pointer");
  SHDR_REQUIRE(npix > 0 && C > 0 && C % 8 == 0, SHDR_E_SHAPE, "bn_bwd_f16: bad shape (C %% 8 == 0)");
  SHDR_REQUIRE(shdr::aligned16(dy) && shdr::aligned16(x) && (!y_relu || shdr::aligned16(y_relu)) && shdr::aligned16(dx) && shdr::aligned16(mean),
               SHDR_E_ALIGN, "bn_bwd_f16: dy, x, y_relu, dx and mean (read as float4) must be 16-byte aligned");
  hipStream_t st = shdr::stream_of(stream);
  launch_bn_reduce_h(st, H_(dy), H_(x), H_(y_relu), mean, ws, (long)npix, C, 1);
  hipLaunchKernelGGL(bn_bwd_finalize_kernel, dim3((C + 255) / 256), dim3(256), 0, st, ws, var, dgamma, dbeta, C, eps);
  const long nvec = (long)npix * (C / 8);
  hipLaunchKernelGGL(bn_apply_h_kernel, dim3(octet_grid(nvec, C / 8, 2048)), dim3(256), 0, st, H_(dy), H_(x), H_(y_relu), mean, var, gamma,
                     (const float*)nullptr, ws, HM_(dx), nvec, (long)npix, C, eps, 0, 1);
  return shdr::check_launch("bn_bwd_f16");
}
extern "C" int shdr_lin_frontend_fwd_f16(const float* img, void* y, int N, int H, int W, int y_channels, void* stream) {
  SHDR_REQUIRE(img && y, SHDR_E_NULL, "lin_frontend_f16: null pointer");
  SHDR_REQUIRE(N > 0 && H >= 2 && W >= 2 && y_channels >= 93 && y_channels % 8 == 0, SHDR_E_SHAPE,
               "lin_frontend_f16: need H, W >= 2 and y_channels >= 93, a multiple of 8");
  SHDR_REQUIRE(shdr::aligned16(y), SHDR_E_ALIGN, "lin_frontend_f16: y must be 16-byte aligned");
  SHDR_REQUIRE(y_channels == 96, SHDR_E_SHAPE, "lin_frontend_f16: built for the 96-channel (93 + 3 zero) layout");
  // 6 blocks per group: one leading-octet block + five histogram blocks (5 * 256 threads = a multiple of the 10 histogram octets)
  long groups = ((long)N * H * W * 12 + 6 * 256 - 1) / (6 * 256);
  groups = groups < 1 ? 1 : (groups > 342 ? 342 : groups);
  hipLaunchKernelGGL(lin_frontend_h_kernel, dim3((unsigned)(6 * groups)), dim3(256), 0, shdr::stream_of(stream), img, HM_(y), N, H, W, y_channels);
  return shdr::check_launch("lin_frontend_f16");
}
extern "C" int shdr_lin_frontend_bwd_f16(const float* img, const void* dF, float* dimg, int N, int H, int W, int y_channels, void* stream) {
  SHDR_REQUIRE(img && dF && dimg, SHDR_E_NULL, "lin_frontend_bwd_f16: null pointer");
  SHDR_REQUIRE(N > 0 && H >= 2 && W >= 2 && y_channels >= 93, SHDR_E_SHAPE, "lin_frontend_bwd_f16: bad shape");
  hipLaunchKernelGGL(lin_frontend_bwd_h_kernel, dim3(shdr::stream_grid((long)N * H * W * 3)), dim3(256), 0, shdr::stream_of(stream), img, H_(dF), dimg, N, H, W,
                     y_channels);
  return shdr::check_launch("lin_frontend_bwd_f16");
}

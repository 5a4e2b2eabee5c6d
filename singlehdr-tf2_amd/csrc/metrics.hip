// Validation metrics of an HDR estimate against its ground truth (include/shdr.h "validation metrics"; DESIGN.md "Validation
// metrics"): PSNR-L, PSNR-mu, SSIM-mu and the fine-tuning loss, per image, without leaving the device.
//
//   shdr_pair_moments_f32   sum(pred), sum(gt), max(gt), min(gt) per image -> the two mean-normalisation scales and the peak
//   shdr_hdr_metrics_f32    ONE pass over both images: a block owns a tile of TH x TW SSIM windows, stages the (TH+10) x (TW+10)
//                           pixels under them through LDS (tone-mapped once per staged pixel), adds the three pointwise sums over the
//                           pixels it owns, filters the five SSIM moments with the separable 11-tap Gaussian in LDS and adds SSIM
//                           over its windows
//   shdr_tonemap_u8_f32     the same tone curve to 8 bits with a 2.2 gamma, for previews
//
// Every reduction has two stages and no floating-point atomics: the blocks write float64 partial sums into the caller's workspace,
// one block per image adds them in a fixed order.  The same inputs give the same bits.
#include <math.h>

#include "shdr_internal.h"

namespace {

constexpr int TH = SHDR_METRICS_TILE_H, TW = SHDR_METRICS_TILE_W;   // windows per tile
constexpr int TAPS = 11, HALO = TAPS - 1;
constexpr int SR = TH + HALO, SC = TW + HALO;                       // staged pixels: 26 x 42
// LDS pitches.  ds_read_b32 / ds_write_b32 bank = dword address mod 32, per half wave.
//   staged planes: the horizontal pass gives 8 lanes to a row (4 outputs each, so lane addresses 4 apart) and the next 8 lanes to the
//   next row: a pitch of 3 mod 4 puts the four rows of a half wave on the four residues mod 4 -> 32 different banks.
//   the staging writes walk c fastest (NHWC): a plane stride of 11 mod 32 keeps the three channels of the ~11 pixels a half wave
//   covers on different banks.
//   moment planes: written with the same 8-lanes-per-row pattern (pitch 3 mod 4), read down a column by 32 lanes with consecutive x.
constexpr int SP = 43, SPLANE = 1131;                               // 26 * 43 = 1118 -> 1131 = 11 mod 32
constexpr int HP = 35;
constexpr int MGRID_MAX = 64;                                       // blocks per image of the moments pass
static_assert(SC <= SP && SR * SP <= SPLANE && TW <= HP && TW % 4 == 0 && TH % 4 == 0 && (TW / 4) * SR <= 256 && (TH / 4) * TW <= 256,
              "tile constants");

struct Gauss { float w[TAPS]; };

__device__ __forceinline__ double wave_sum_d(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}
// sum of NV values over the 256 threads of a block, in a fixed order; valid in thread 0.  sred: 4 * NV doubles of LDS
template <int NV>
__device__ __forceinline__ void block_sum_d(double (&v)[NV], double* sred) {
#pragma unroll
  for (int k = 0; k < NV; ++k) v[k] = wave_sum_d(v[k]);
  if ((threadIdx.x & 63) == 0) {
#pragma unroll
    for (int k = 0; k < NV; ++k) sred[(threadIdx.x >> 6) * NV + k] = v[k];
  }
  __syncthreads();
#pragma unroll
  for (int k = 0; k < NV; ++k) v[k] = (sred[k] + sred[NV + k]) + (sred[2 * NV + k] + sred[3 * NV + k]);
}

// ---- moments ------------------------------------------------------------------------------------------------------------
// part[(n * grid + b) * 4 + {0,1,2,3}] = sum(pred), sum(gt), max(gt), min(gt) over block b's share of image n
__global__ __launch_bounds__(256) void pair_moments_kernel(const float* __restrict__ pred, const float* __restrict__ gt, int64_t n_per,
                                                           int vec, double* __restrict__ part) {
  __shared__ double sred[4 * 2];
  __shared__ float smax[4], smin[4];
  const int n = blockIdx.y;
  const float* P = pred + (int64_t)n * n_per;
  const float* G = gt + (int64_t)n * n_per;
  double s[2] = {0.0, 0.0};
  float mx = -INFINITY, mn = INFINITY;
  if (vec) {                                   // n_per % 4 == 0 and 16-byte aligned bases: every image starts on a 16-byte boundary
    const float4* P4 = reinterpret_cast<const float4*>(P);
    const float4* G4 = reinterpret_cast<const float4*>(G);
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n_per / 4; i += (int64_t)gridDim.x * 256) {
      const float4 a = P4[i], b = G4[i];
      s[0] += ((double)a.x + (double)a.y) + ((double)a.z + (double)a.w);
      s[1] += ((double)b.x + (double)b.y) + ((double)b.z + (double)b.w);
      mx = fmaxf(fmaxf(mx, fmaxf(b.x, b.y)), fmaxf(b.z, b.w));
      mn = fminf(fminf(mn, fminf(b.x, b.y)), fminf(b.z, b.w));
    }
  } else {
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n_per; i += (int64_t)gridDim.x * 256) {
      const float b = G[i];
      s[0] += (double)P[i];
      s[1] += (double)b;
      mx = fmaxf(mx, b);
      mn = fminf(mn, b);
    }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    mx = fmaxf(mx, __shfl_xor(mx, o, 64));
    mn = fminf(mn, __shfl_xor(mn, o, 64));
  }
  if ((threadIdx.x & 63) == 0) { smax[threadIdx.x >> 6] = mx; smin[threadIdx.x >> 6] = mn; }
  block_sum_d<2>(s, sred);                     // (its barrier publishes smax / smin as well)
  if (threadIdx.x == 0) {
    double* o = part + ((int64_t)n * gridDim.x + blockIdx.x) * 4;
    o[0] = s[0];
    o[1] = s[1];
    o[2] = (double)fmaxf(fmaxf(smax[0], smax[1]), fmaxf(smax[2], smax[3]));
    o[3] = (double)fminf(fminf(smin[0], smin[1]), fminf(smin[2], smin[3]));
  }
}

// one wave per image: the `grid` partials in ascending order
__global__ __launch_bounds__(64) void pair_moments_final_kernel(const double* __restrict__ part, int grid, int64_t n_per, int normalise,
                                                                double* __restrict__ scale_pred, double* __restrict__ scale_gt,
                                                                double* __restrict__ peak) {
  if (threadIdx.x != 0) return;
  const int n = blockIdx.x;
  const double* p = part + (int64_t)n * grid * 4;
  double sp = 0.0, sg = 0.0, mx = -INFINITY, mn = INFINITY;
  for (int b = 0; b < grid; ++b) {
    sp += p[4 * b];
    sg += p[4 * b + 1];
    mx = fmax(mx, p[4 * b + 2]);
    mn = fmin(mn, p[4 * b + 3]);
  }
  // the scales multiply float32 pixels: they ARE float32 numbers (as in shdr_mean_norm_fwd_f32), stored widened
  const float fp = normalise ? (float)(0.5 / (1e-6 + sp / (double)n_per)) : 1.0f;
  const float fg = normalise ? (float)(0.5 / (1e-6 + sg / (double)n_per)) : 1.0f;
  scale_pred[n] = (double)fp;
  scale_gt[n] = (double)fg;
  // max over the image of max(s_g * gt, 0): s_g * max(gt) for a positive scale, s_g * min(gt) for a negative one (a gt of negative mean)
  peak[n] = fmax((double)fg * (fg >= 0.0f ? mx : mn), 0.0);
}

// ---- the fused pass -----------------------------------------------------------------------------------------------------
// fminf drops a NaN operand: tone_sat maps 0 / 0 (a black pixel under a peak of 0) to T = 1, which the preview keeps (a defined
// code).  The metrics use tone, which lets the NaN through: an all-black ground truth must not report SSIM = 1.  For every other
// quotient the two give the same bits.
__device__ __forceinline__ float tone_sat(float x, float peak, float mu, float inv_log) {
  return log1pf(mu * fminf(x / peak, 1.0f)) * inv_log;
}
__device__ __forceinline__ float tone(float x, float peak, float mu, float inv_log) {
  const float q = x / peak;
  return log1pf(mu * (q > 1.0f ? 1.0f : q)) * inv_log;
}

// part[(n * tiles + tile) * 4 + {0,1,2,3}] = sum (p-g)^2, sum (T(p)-T(g))^2, sum |logc(p)-logc(g)| over the tile's own pixels,
// sum of SSIM over its windows and the three channels
__global__ __launch_bounds__(256) void hdr_metrics_kernel(const float* __restrict__ pred, const float* __restrict__ gt, int H, int W,
                                                          int tiles_x, int tiles_y, float mu, float inv_log,
                                                          const double* __restrict__ scale_pred, const double* __restrict__ scale_gt,
                                                          const double* __restrict__ peak, Gauss gw, double* __restrict__ part) {
  __shared__ float sa[3 * SPLANE], sb[3 * SPLANE];     // T(p) - shift_p, T(g) - shift_g, one plane per channel
  __shared__ float hm[5 * SR * HP];                    // rows of the five moments after the horizontal pass, one channel at a time
  __shared__ double sred[4 * 4];
  __shared__ float shift[2][3];

  const int tiles = tiles_x * tiles_y;
  const int n = blockIdx.x / tiles, tile = blockIdx.x - n * tiles;
  const int ty = tile / tiles_x, tx = tile - ty * tiles_x;
  const int oy0 = ty * TH, ox0 = tx * TW;              // first window = first staged pixel of the tile: inside the image
  const bool last_y = ty == tiles_y - 1, last_x = tx == tiles_x - 1;
  const float sp = (float)scale_pred[n], sg = (float)scale_gt[n], pk = (float)peak[n];
  const float* P = pred + (int64_t)n * H * W * 3;
  const float* G = gt + (int64_t)n * H * W * 3;
  const int tid = threadIdx.x;

  // The second moments are formed about a per-tile, per-channel shift (the tile's first staged value): a window's variance is then
  // the difference of numbers of the size of the tile's contrast, not of 1 (raw fp32 moments lose 4e-6 of SSIM on a flat 0.9 image)
  if (tid < 3) {
    const int64_t off = ((int64_t)oy0 * W + ox0) * 3 + tid;
    shift[0][tid] = tone(fmaxf(sp * P[off], 0.0f), pk, mu, inv_log);
    shift[1][tid] = tone(fmaxf(sg * G[off], 0.0f), pk, mu, inv_log);
  }
  __syncthreads();

  // ---- stage: a staged row is SC * 3 consecutive floats of the image.  A pixel is OWNED by the tile whose TH x TW window origins
  //      cover it; the last tile row / column also owns the 10 pixels beyond its windows: every pixel is counted exactly once ----
  double acc[4] = {0.0, 0.0, 0.0, 0.0};
  for (int i = tid; i < SR * SC * 3; i += 256) {
    const int r = i / (SC * 3), j = i - r * (SC * 3);
    const int q = j / 3, c = j - 3 * q;
    const int y = oy0 + r, x = ox0 + q;
    float ta = 0.0f, tb = 0.0f;
    if (y < H && x < W) {
      const int64_t off = ((int64_t)y * W + x) * 3 + c;
      const float p = fmaxf(sp * P[off], 0.0f), g = fmaxf(sg * G[off], 0.0f);
      const float tp = tone(p, pk, mu, inv_log), tg = tone(g, pk, mu, inv_log);
      if ((r < TH || last_y) && (q < TW || last_x)) {
        // The three pointwise terms are differences of nearly equal numbers when the estimate is good (a flat 0.9 +- 1e-3 image:
        // T(p) - T(g) ~ 2e-4 between values rounded at 6e-8).  Each is formed from the difference of the ARGUMENTS instead:
        //   p - g with the rounding of the two scalings taken back (fma residuals),
        //   log(1 + k p) - log(1 + k g) = log1p(k (p - g) / (1 + k g)),
        // which keeps every term to a few ulp of ITSELF.
        float d = p - g;
        if (p > 0.0f && g > 0.0f) d = fmaf(sp, P[off], -g) - fmaf(sg, G[off], -g);
        const float t_g = g / pk;                                                  // <= 1: peak is max(g)
        const float dt = p <= pk ? d / pk : (pk - g) / pk;                         // min(p / peak, 1) - g / peak
        const float dm = log1pf(mu * dt / (1.0f + mu * t_g)) * inv_log;
        const float dl = log1pf(10.0f * d / (1.0f + 10.0f * g)) * 0.41703239f;     // 1 / log(11)
        acc[0] += (double)(d * d);
        acc[1] += (double)(dm * dm);
        acc[2] += (double)fabsf(dl);
      }
      ta = tp - shift[0][c];
      tb = tg - shift[1][c];
    }
    sa[c * SPLANE + r * SP + q] = ta;
    sb[c * SPLANE + r * SP + q] = tb;
  }
  __syncthreads();

  for (int c = 0; c < 3; ++c) {
    // ---- horizontal pass: thread = (staged row, 4 adjacent outputs); 14 + 14 LDS reads feed 4 x 5 x 11 multiply-adds ----
    if (tid < SR * (TW / 4)) {
      const int r = tid / (TW / 4), x0 = (tid - r * (TW / 4)) * 4;
      const float* ra = sa + c * SPLANE + r * SP + x0;
      const float* rb = sb + c * SPLANE + r * SP + x0;
      float a[14], b[14], aa[14], bb[14], ab[14];
#pragma unroll
      for (int k = 0; k < 14; ++k) {
        a[k] = ra[k];
        b[k] = rb[k];
        aa[k] = a[k] * a[k];
        bb[k] = b[k] * b[k];
        ab[k] = a[k] * b[k];
      }
      float m[5][4];
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        float m0 = 0.f, m1 = 0.f, m2 = 0.f, m3 = 0.f, m4 = 0.f;
#pragma unroll
        for (int k = 0; k < TAPS; ++k) {
          const float w = gw.w[k];
          m0 = fmaf(w, a[j + k], m0);
          m1 = fmaf(w, b[j + k], m1);
          m2 = fmaf(w, aa[j + k], m2);
          m3 = fmaf(w, bb[j + k], m3);
          m4 = fmaf(w, ab[j + k], m4);
        }
        m[0][j] = m0; m[1][j] = m1; m[2][j] = m2; m[3][j] = m3; m[4][j] = m4;
      }
#pragma unroll
      for (int q = 0; q < 5; ++q)
#pragma unroll
        for (int j = 0; j < 4; ++j) hm[(q * SR + r) * HP + x0 + j] = m[q][j];
    }
    __syncthreads();
    // ---- vertical pass + SSIM: thread = (column, 4 windows down it); 32 lanes read 32 consecutive floats of a row ----
    if (tid < (TH / 4) * TW) {
      const int x = tid & (TW - 1), y0 = (tid / TW) * 4;
      float m[5][4];
#pragma unroll
      for (int q = 0; q < 5; ++q) {
        float v[14];
#pragma unroll
        for (int k = 0; k < 14; ++k) v[k] = hm[(q * SR + y0 + k) * HP + x];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          float t = 0.f;
#pragma unroll
          for (int k = 0; k < TAPS; ++k) t = fmaf(gw.w[k], v[j + k], t);
          m[q][j] = t;
        }
      }
      const float C1 = 1e-4f, C2 = 9e-4f;
      const float sha = shift[0][c], shb = shift[1][c];
      float ss = 0.f;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        if (oy0 + y0 + j < H - HALO && ox0 + x < W - HALO) {
          const float ma = m[0][j], mb = m[1][j];
          const float va = m[2][j] - ma * ma, vb = m[3][j] - mb * mb, cab = m[4][j] - ma * mb;
          const float mua = ma + sha, mub = mb + shb;
          ss += ((2.0f * mua * mub + C1) * (2.0f * cab + C2)) / ((mua * mua + mub * mub + C1) * (va + vb + C2));
        }
      }
      acc[3] += (double)ss;
    }
    __syncthreads();                                   // hm is rewritten by the next channel
  }
  block_sum_d<4>(acc, sred);
  if (tid == 0) {
    double* o = part + (int64_t)blockIdx.x * 4;
    o[0] = acc[0]; o[1] = acc[1]; o[2] = acc[2]; o[3] = acc[3];
  }
}

// one block per image: thread t adds tiles t, t + 256, ... in ascending order, then the fixed tree of block_sum_d
__global__ __launch_bounds__(256) void hdr_metrics_final_kernel(const double* __restrict__ part, int tiles, int H, int W,
                                                                const double* __restrict__ peak, double* __restrict__ mse_l,
                                                                double* __restrict__ mse_mu, double* __restrict__ l1_logc,
                                                                double* __restrict__ ssim_mu) {
  __shared__ double sred[4 * 4];
  const int n = blockIdx.x;
  const double* p = part + (int64_t)n * tiles * 4;
  double acc[4] = {0.0, 0.0, 0.0, 0.0};
  for (int t = threadIdx.x; t < tiles; t += 256) {
#pragma unroll
    for (int k = 0; k < 4; ++k) acc[k] += p[4 * t + k];
  }
  block_sum_d<4>(acc, sred);
  if (threadIdx.x == 0) {
    const double cnt = (double)H * (double)W * 3.0, pk = peak[n];
    mse_l[n] = acc[0] / cnt / (pk * pk);
    mse_mu[n] = acc[1] / cnt;
    l1_logc[n] = acc[2] / cnt;
    ssim_mu[n] = acc[3] / ((double)(H - HALO) * (double)(W - HALO) * 3.0);
  }
}

// ---- preview ------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void tonemap_u8_kernel(const float* __restrict__ x, const double* __restrict__ scale,
                                                         const double* __restrict__ peak, uint8_t* __restrict__ y, int64_t npix_per,
                                                         int64_t npix, float mu, float inv_log, int reverse) {
  for (int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x; p < npix; p += (int64_t)gridDim.x * 256) {
    const int64_t n = p / npix_per;
    const float s = scale ? (float)scale[n] : 1.0f, pk = (float)peak[n];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      const float v = fmaxf(s * x[3 * p + (reverse ? 2 - c : c)], 0.0f);
      y[3 * p + c] = (uint8_t)rintf(255.0f * powf(tone_sat(v, pk, mu, inv_log), 1.0f / 2.2f));
    }
  }
}

inline int moments_grid(int H, int W) {
  const int64_t g = ((int64_t)H * W * 3 + 256 * 16 - 1) / (256 * 16);           // ~16 values per thread, at most MGRID_MAX blocks
  return (int)(g < 1 ? 1 : (g > MGRID_MAX ? MGRID_MAX : g));
}
inline int64_t tiles_of(int H, int W) { return (int64_t)((H - HALO + TH - 1) / TH) * ((W - HALO + TW - 1) / TW); }
inline bool shape_ok(int N, int H, int W) { return N > 0 && H >= TAPS && W >= TAPS; }

}  // namespace

// the two launches use the workspace one after the other on one stream: it holds the larger of the two partial tables
extern "C" int64_t shdr_metrics_workspace_bytes(int N, int H, int W) {
  if (!shape_ok(N, H, W)) {
    shdr::set_error("metrics_workspace_bytes: need N > 0, H >= 11, W >= 11 (got %d, %d, %d)", N, H, W);
    return SHDR_E_SHAPE;
  }
  const int64_t a = (int64_t)moments_grid(H, W), b = tiles_of(H, W);
  return (int64_t)N * (a > b ? a : b) * 4 * (int64_t)sizeof(double);
}

extern "C" int shdr_pair_moments_f32(const float* pred, const float* gt, int N, int H, int W, int normalise, double* scale_pred,
                                     double* scale_gt, double* peak, void* workspace, void* stream) {
  SHDR_REQUIRE(pred && gt && scale_pred && scale_gt && peak && workspace, SHDR_E_NULL, "pair_moments: null pointer");
  SHDR_REQUIRE(shape_ok(N, H, W), SHDR_E_SHAPE, "pair_moments: need N > 0, H >= 11, W >= 11 (got %d, %d, %d)", N, H, W);
  SHDR_REQUIRE(N <= 65535, SHDR_E_SHAPE, "pair_moments: at most 65535 images per call (got %d)", N);
  SHDR_REQUIRE((reinterpret_cast<uintptr_t>(workspace) & 7u) == 0, SHDR_E_ALIGN, "pair_moments: workspace must be 8-byte aligned");
  const int64_t n_per = (int64_t)H * W * 3;
  const int grid = moments_grid(H, W);
  const int vec = (n_per % 4 == 0) && shdr::aligned16(pred) && shdr::aligned16(gt);
  double* part = static_cast<double*>(workspace);
  hipLaunchKernelGGL(pair_moments_kernel, dim3(grid, N), dim3(256), 0, shdr::stream_of(stream), pred, gt, n_per, vec, part);
  hipLaunchKernelGGL(pair_moments_final_kernel, dim3(N), dim3(64), 0, shdr::stream_of(stream), part, grid, n_per, normalise, scale_pred, scale_gt,
                     peak);
  return shdr::check_launch("pair_moments");
}

extern "C" int shdr_hdr_metrics_f32(const float* pred, const float* gt, int N, int H, int W, float mu, const double* scale_pred,
                                    const double* scale_gt, const double* peak, double* mse_l, double* mse_mu, double* l1_logc,
                                    double* ssim_mu, void* workspace, void* stream) {
  SHDR_REQUIRE(pred && gt && scale_pred && scale_gt && peak && mse_l && mse_mu && l1_logc && ssim_mu && workspace, SHDR_E_NULL,
               "hdr_metrics: null pointer");
  SHDR_REQUIRE(shape_ok(N, H, W), SHDR_E_SHAPE, "hdr_metrics: need N > 0, H >= 11, W >= 11 (got %d, %d, %d)", N, H, W);
  SHDR_REQUIRE(mu > 0.0f, SHDR_E_SHAPE, "hdr_metrics: mu must be positive");
  SHDR_REQUIRE((reinterpret_cast<uintptr_t>(workspace) & 7u) == 0, SHDR_E_ALIGN, "hdr_metrics: workspace must be 8-byte aligned");
  const int tiles_y = (H - HALO + TH - 1) / TH, tiles_x = (W - HALO + TW - 1) / TW;
  const int64_t blocks = (int64_t)N * tiles_y * tiles_x;
  SHDR_REQUIRE(blocks <= 0x7fffffff, SHDR_E_SHAPE, "hdr_metrics: %lld tiles exceed the grid", (long long)blocks);
  Gauss gw;
  double g[TAPS], sum = 0.0;
  for (int k = 0; k < TAPS; ++k) sum += g[k] = exp(-(double)((k - 5) * (k - 5)) / (2.0 * 1.5 * 1.5));
  for (int k = 0; k < TAPS; ++k) gw.w[k] = (float)(g[k] / sum);
  double* part = static_cast<double*>(workspace);
  hipLaunchKernelGGL(hdr_metrics_kernel, dim3((unsigned)blocks), dim3(256), 0, shdr::stream_of(stream), pred, gt, H, W, tiles_x, tiles_y, mu,
                     (float)(1.0 / log1p((double)mu)), scale_pred, scale_gt, peak, gw, part);
  hipLaunchKernelGGL(hdr_metrics_final_kernel, dim3(N), dim3(256), 0, shdr::stream_of(stream), part, tiles_y * tiles_x, H, W, peak, mse_l, mse_mu,
                     l1_logc, ssim_mu);
  return shdr::check_launch("hdr_metrics");
}

extern "C" int shdr_tonemap_u8_f32(const float* x, const double* scale, const double* peak, uint8_t* y, int N, int H, int W, float mu,
                                   int reverse_channels, void* stream) {
  SHDR_REQUIRE(x && peak && y, SHDR_E_NULL, "tonemap_u8: null pointer");
  SHDR_REQUIRE(shape_ok(N, H, W), SHDR_E_SHAPE, "tonemap_u8: need N > 0, H >= 11, W >= 11 (got %d, %d, %d)", N, H, W);
  SHDR_REQUIRE(mu > 0.0f, SHDR_E_SHAPE, "tonemap_u8: mu must be positive");
  const int64_t npix_per = (int64_t)H * W, npix = npix_per * N;
  hipLaunchKernelGGL(tonemap_u8_kernel, dim3(shdr::stream_grid(npix)), dim3(256), 0, shdr::stream_of(stream), x, scale, peak, y, npix_per, npix, mu,
                     (float)(1.0 / log1p((double)mu)), reverse_channels);
  return shdr::check_launch("tonemap_u8");
}

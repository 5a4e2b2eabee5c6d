// Device side of the training-set reader (dataset.py of the reference).  The reference builds
// every patch on the host (cv2.imread, cv2.resize, np.mean, np.rot90, np.flip in 24 worker processes); here the files are
// decoded once, resized into one resident arena, and a batch is ONE launch over that arena.
//
// cv2.resize(src, dsize, cv2.INTER_AREA) at dataset.py:190 and :225 passes the flag as `dst`, so the interpolation in effect is
// the default INTER_LINEAR.  Restated from OpenCV's resize.cpp (generic path, float32; cv2 is not available to run):
//   scale = 1 / (dsize / ssize) in double;  f = (float)((d + 0.5) * scale - 0.5);  s = floor(f);  f -= s;
//   horizontal: s < 0 -> s = 0, f = 0;  s >= ssize - 1 -> s = ssize - 1, f = 0;  value = S[s] * (1 - f) + S[s + 1] * f
//   vertical:   rows s and s + 1, each clamped to [0, ssize - 1], weights (1 - f, f); horizontal pass first.
// Same-size resizes are copies, which weights (1, 0) reproduce exactly.  OpenCV routes an exact 2x downscale to its INTER_AREA
// fast path (a 2 x 2 average); the bilinear weights are then (0.5, 0.5), the same value up to the order of the sums.
// Compiled with -ffp-contract=off: every product and sum is rounded where numpy / OpenCV round it.
#include "shdr_internal.h"
#include "linear_resize.h"

namespace {

using shdr::linear::Taps;
using shdr::linear::bilinear3;
using shdr::linear::linear_taps;

constexpr int kWin = 512;          // PatchHDRDataset's crop side (dataset.py:216-219)

// Ward's RGBE -> float, as hdr_io.rgbe_decode: byte * 2^(e - 136), e == 0 -> 0; channel c of the result is the file's 2 - c
// (cv2.imread's BGR; the [:,:,::-1] and np.flip(hdr, -1) of dataset.py:183-184 cancel), clip(0, None) (:185) is the identity
__device__ __forceinline__ float3 rgbe_bgr(uchar4 p) {
  const float sc = p.w == 0 ? 0.0f : ldexpf(1.0f, (int)p.w - 136);
  return make_float3((float)p.z * sc, (float)p.y * sc, (float)p.x * sc);
}

// (a) load: one thread per output pixel; the four taps are decoded from the RGBE bytes (4 B per source pixel read, no
//     full-resolution float copy)
__global__ __launch_bounds__(256) void hdr_load_resize_kernel(const uchar4* __restrict__ src, float* __restrict__ y, int H0,
                                                              int W0, int H, int W, double sy, double sx) {
  const long total = (long)H * W;
  for (long p = (long)blockIdx.x * 256 + threadIdx.x; p < total; p += (long)gridDim.x * 256) {
    const int oy = (int)(p / W), ox = (int)(p - (long)oy * W);
    const float3 v = bilinear3(oy, ox, H0, W0, sy, sx, [&](int r, int c) { return rgbe_bgr(src[(long)r * W0 + c]); });
    y[3 * p] = v.x;
    y[3 * p + 1] = v.y;
    y[3 * p + 2] = v.z;
  }
}

// top-left corner of the 512 x 512 crop of file (H, W), parity p (dataset.py:216-219: rows if h > w, else columns)
__device__ __forceinline__ long window_origin(int H, int W, int parity) {
  const int r0 = (H > W && parity) ? H - kWin : 0;
  const int c0 = (H <= W && parity) ? W - kWin : 0;
  return ((long)r0 * W + c0) * 3;
}

// (b) means: block (w, g) sums rows 8g .. 8g+7 of window w (16 pixels = 48 values per thread, then an LDS tree); a second
//     launch folds the 64 partials of each window in the same tree order
constexpr int kMeanBlocks = kWin / 8;

__device__ __forceinline__ float block_sum_256(float v, float* lds) {
  lds[threadIdx.x] = v;
  __syncthreads();
  for (int s = 128; s > 0; s >>= 1) {
    if ((int)threadIdx.x < s) lds[threadIdx.x] += lds[threadIdx.x + s];
    __syncthreads();
  }
  return lds[0];
}

__global__ __launch_bounds__(256) void hdr_window_partials_kernel(const float* __restrict__ arena, const int64_t* __restrict__ offsets,
                                                                  const int* __restrict__ dims, float* __restrict__ partials) {
  __shared__ float lds[256];
  const int w = blockIdx.x, f = w >> 1, g = blockIdx.y;
  const int H = dims[2 * f], W = dims[2 * f + 1];
  const float* base = arena + offsets[f] + window_origin(H, W, w & 1);
  float acc = 0.0f;
  for (int r = 8 * g; r < 8 * g + 8; ++r) {
    const float* row = base + (long)r * W * 3;
    for (int c = threadIdx.x; c < kWin; c += 256) acc += (row[3 * c] + row[3 * c + 1]) + row[3 * c + 2];
  }
  const float s = block_sum_256(acc, lds);
  if (threadIdx.x == 0) partials[(long)w * kMeanBlocks + g] = s;
}

__global__ __launch_bounds__(64) void hdr_window_fold_kernel(const float* __restrict__ partials, float* __restrict__ means) {
  __shared__ float lds[kMeanBlocks];
  const int w = blockIdx.x;
  lds[threadIdx.x] = partials[(long)w * kMeanBlocks + threadIdx.x];
  __syncthreads();
  for (int s = kMeanBlocks / 2; s > 0; s >>= 1) {
    if ((int)threadIdx.x < s) lds[threadIdx.x] += lds[threadIdx.x + s];
    __syncthreads();
  }
  if (threadIdx.x == 0) means[w] = lds[0] / (float)(kWin * kWin * 3);
}

// (c) the batch: block = one 16 x 16 tile of one sample's output.  The tile's taps come from a compact region of the window
//     for every k (a 16-pixel output row maps to a source column when k is odd), so a block reads a few dozen lines however the
//     sample is rotated.  Output pixel (i, j) is traced back through flip(axis 1), flip(axis 0) and rot90(k) to (ci, cj) of the
//     S x S image, (y0 + ci, x0 + cj), then to cv2's taps in the window; taps are normalised, then blended.
__global__ __launch_bounds__(256) void hdr_patch_sample_kernel(const float* __restrict__ arena, const int64_t* __restrict__ offsets,
                                                               const int* __restrict__ dims, const float* __restrict__ means,
                                                               const int* __restrict__ params, int stride, int n_files, int P,
                                                               float* __restrict__ y) {
  const int n = blockIdx.z;
  const int* prm = params + (long)n * stride;
  const int idx = prm[0];
  const int f = min(max(idx >> 1, 0), n_files - 1), parity = idx & 1;
  const int Sz = max(prm[1], 1), y0 = prm[2], x0 = prm[3], k = prm[4] & 3, flip0 = prm[5], flip1 = prm[6];
  const int i = blockIdx.y * 16 + (threadIdx.x >> 4), j = blockIdx.x * 16 + (threadIdx.x & 15);
  const int L = P - 1;
  const int a = flip0 ? L - i : i;                           // flips were applied last: undo them first
  const int b = flip1 ? L - j : j;
  int ci, cj;                                                // np.rot90(m, k)[a][b] = m[ci][cj]
  switch (k) {
    case 1: ci = b; cj = L - a; break;
    case 2: ci = L - a; cj = L - b; break;
    case 3: ci = L - b; cj = a; break;
    default: ci = a; cj = b; break;
  }
  const double scale = 1.0 / ((double)Sz / (double)kWin);
  const Taps ty = linear_taps(y0 + ci, scale, kWin, false), tx = linear_taps(x0 + cj, scale, kWin, true);
  const int H = dims[2 * f], W = dims[2 * f + 1];
  const float* win = arena + offsets[f] + window_origin(H, W, parity);
  const float denom = means[2 * f + parity] + 1e-6f;                // hdr_mean + 1e-6 (:268)
  const long rs = (long)W * 3;
  const float* r0 = win + ty.s0 * rs;
  const float* r1 = win + ty.s1 * rs;
  float v[3];
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    const float t00 = (0.5f * r0[3 * tx.s0 + c]) / denom, t01 = (0.5f * r0[3 * tx.s1 + c]) / denom;
    const float t10 = (0.5f * r1[3 * tx.s0 + c]) / denom, t11 = (0.5f * r1[3 * tx.s1 + c]) / denom;
    const float g = 1.0f - tx.f, h = 1.0f - ty.f;
    const float h0 = t00 * g + t01 * tx.f, h1 = t10 * g + t11 * tx.f;
    v[c] = h0 * h + h1 * ty.f;
  }
  float* o = y + (((long)n * P + i) * P + j) * 3;
  o[0] = v[0];
  o[1] = v[1];
  o[2] = v[2];
}

}  // namespace

extern "C" int shdr_hdr_load_resize_f32(const uint8_t* rgbe, float* y, int H0, int W0, int H, int W, void* stream) {
  SHDR_REQUIRE(rgbe && y, SHDR_E_NULL, "hdr_load_resize: null pointer");
  SHDR_REQUIRE(H0 > 0 && W0 > 0 && H > 0 && W > 0, SHDR_E_SHAPE, "hdr_load_resize: non-positive dimension");
  SHDR_REQUIRE((reinterpret_cast<uintptr_t>(rgbe) & 3u) == 0, SHDR_E_ALIGN, "hdr_load_resize: rgbe must be 4-byte aligned");
  const long total = (long)H * W;
  hipLaunchKernelGGL(hdr_load_resize_kernel, dim3(shdr::stream_grid(total)), dim3(256), 0, shdr::stream_of(stream),
                     reinterpret_cast<const uchar4*>(rgbe), y, H0, W0, H, W, 1.0 / ((double)H / H0), 1.0 / ((double)W / W0));
  return shdr::check_launch("hdr_load_resize");
}

extern "C" int shdr_hdr_window_means_f32(const float* arena, const int64_t* offsets, const int32_t* dims, int n_files, float* partials,
                                         float* means, void* stream) {
  SHDR_REQUIRE(arena && offsets && dims && partials && means, SHDR_E_NULL, "hdr_window_means: null pointer");
  SHDR_REQUIRE(n_files > 0 && n_files < (1 << 30), SHDR_E_SHAPE, "hdr_window_means: %d files", n_files);
  hipLaunchKernelGGL(hdr_window_partials_kernel, dim3(2 * n_files, kMeanBlocks), dim3(256), 0, shdr::stream_of(stream), arena, offsets, dims,
                     partials);
  int rc = shdr::check_launch("hdr_window_means");
  if (rc != SHDR_OK) return rc;
  hipLaunchKernelGGL(hdr_window_fold_kernel, dim3(2 * n_files), dim3(kMeanBlocks), 0, shdr::stream_of(stream), partials, means);
  return shdr::check_launch("hdr_window_means");
}

extern "C" int shdr_hdr_patch_sample_f32(const float* arena, const int64_t* offsets, const int32_t* dims, const float* means,
                                         const int32_t* params, int param_stride, int N, int n_files, int P, float* y, void* stream) {
  SHDR_REQUIRE(arena && offsets && dims && means && params && y, SHDR_E_NULL, "hdr_patch_sample: null pointer");
  SHDR_REQUIRE(N > 0 && N <= 65535 && n_files > 0 && param_stride >= 7, SHDR_E_SHAPE,
               "hdr_patch_sample: N %d, n_files %d, param_stride %d", N, n_files, param_stride);
  SHDR_REQUIRE(P > 0 && P % 16 == 0 && P <= kWin * 4, SHDR_E_SHAPE, "hdr_patch_sample: P %d must be a multiple of 16", P);
  hipLaunchKernelGGL(hdr_patch_sample_kernel, dim3(P / 16, P / 16, N), dim3(256), 0, shdr::stream_of(stream), arena, offsets, dims, means,
                     params, param_stride, n_files, P, y);
  return shdr::check_launch("hdr_patch_sample");
}

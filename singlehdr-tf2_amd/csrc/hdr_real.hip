// Device side of the HDR-Real folder reader (hdr_real.py; convert_to_tf_record.py and finetune_real_dataset.py:34-61 of the
// reference).  The reference cuts every HDR_gt / LDR_in pair into 256 x 256 patches at stride 64 on the
// host, stores each patch twice as float32 in GZIP TFRecords and normalises / augments them again per batch.  Here every pair is
// resident once -- LDR as uint8 RGB (3 B / pixel), HDR as float32 RGB -- in two flat arenas that share ONE pixel-offset table:
//   images  int64 [n_images, 3]   (first pixel of the image in both arenas, H, W)
//   patches int32 [n_patches, 3]  (image, h1, w1): the top-left corner of a size x size patch
//   samples int32 [b, 3]          (patch, flip, rot) of one batch
// (a) statistics, once: one workgroup per patch counts the extreme pixels of convert_to_tf_record.py:54-55 and sums the HDR patch
//     in float64 (the mean of finetune_real_dataset.py:47);
// (b) a batch: one launch crops, flips, rotates and normalises both patches of every sample.
// Compiled with -ffp-contract=off: the grey value is three rounded products and two rounded sums, left to right.
#include "shdr_internal.h"

namespace {

constexpr int kMaxSize = 16384;          // size * size stays an int

// ---- (a) -----------------------------------------------------------------------------------------------------------
// Thread t visits pixels t, t + 256, ... of the patch in row-major order, then the 256 partial sums meet in a fixed LDS tree: the
// result depends on nothing but the data.  A uint8 row starts at byte 3 * (y * W + w1), any alignment: bytes are read one by one.
__global__ __launch_bounds__(256) void pair_patch_stats_kernel(const uint8_t* __restrict__ ldr, const float* __restrict__ hdr,
                                                               const int64_t* __restrict__ images, const int* __restrict__ patches,
                                                               int size, int* __restrict__ count, float* __restrict__ mean) {
  __shared__ double sums[256];
  __shared__ int cnts[256];
  const int p = blockIdx.x, t = threadIdx.x;
  const int img = patches[3 * p], h1 = patches[3 * p + 1], w1 = patches[3 * p + 2];
  const long W = images[3 * img + 2];
  const long base = images[3 * img] + h1 * W + w1;
  const int npx = size * size;
  double acc = 0.0;
  int cnt = 0;
  for (int e = t; e < npx; e += 256) {
    const int y = e / size, x = e - y * size;
    const long px = 3 * (base + y * W + x);
    const float r = (float)ldr[px], g = (float)ldr[px + 1], b = (float)ldr[px + 2];
    const float gray = r * 0.299f + g * 0.587f + b * 0.114f;
    cnt += (gray >= 249.0f || gray <= 6.0f) ? 1 : 0;
    acc += ((double)hdr[px] + (double)hdr[px + 1]) + (double)hdr[px + 2];
  }
  sums[t] = acc;
  cnts[t] = cnt;
  __syncthreads();
  for (int s = 128; s > 0; s >>= 1) {
    if (t < s) {
      sums[t] += sums[t + s];
      cnts[t] += cnts[t + s];
    }
    __syncthreads();
  }
  if (t == 0) {
    count[p] = cnts[0];
    mean[p] = (float)(sums[0] / (double)((long)npx * 3));
  }
}

// ---- (b) -----------------------------------------------------------------------------------------------------------
// Block = one 32 x 32 tile of one sample's OUTPUT.  Its pixels come from a 32 x 32 square of the patch whatever the flip and the
// rotation; the square is read row by row (96 contiguous floats / bytes per row) into LDS and the output is written row by row
// (96 contiguous floats), so a rotation by 90 or 270 degrees -- an output row is a source column -- strides through LDS, not through
// memory.  LDS rows are 99 floats apart: the 32 lanes of a ds_read_b32 group hold output elements 3 j + c of consecutive (j, c),
// which for a column walk sit at j * 99 + c + const, bank (3 j + c) mod 32 -- 32 different banks; a pitch of 96 or 97 puts them on
// 3 or 13.  Row walks (rotations 0 and 2) are contiguous in either direction.
constexpr int kT = 32, kPitch = 3 * kT + 3;

// the pixel (si, sj) of the un-augmented patch that lands on output pixel (i, j): np.rot90(m, k)[i][j], m = the flipped patch
// (flip_rot90_kernel of imageio.hip)
__device__ __forceinline__ void source_pixel(int i, int j, int L, int rot, int flip, int& si, int& sj) {
  switch (rot) {
    case 1: si = j; sj = L - i; break;
    case 2: si = L - i; sj = L - j; break;
    case 3: si = L - j; sj = i; break;
    default: si = i; sj = j; break;
  }
  if (flip) sj = L - sj;
}

__global__ __launch_bounds__(256) void pair_patch_gather_kernel(const uint8_t* __restrict__ ldr, const float* __restrict__ hdr,
                                                                const int64_t* __restrict__ images, const int* __restrict__ patches,
                                                                const float* __restrict__ mean, const int* __restrict__ samples,
                                                                int size, float* __restrict__ out_ldr, float* __restrict__ out_hdr) {
  __shared__ float tile_h[kT * kPitch];
  __shared__ float tile_l[kT * kPitch];
  const int n = blockIdx.z, t = threadIdx.x;
  const int p = samples[3 * n], flip = samples[3 * n + 1], rot = samples[3 * n + 2] & 3;          // rot 4 is rot 0
  const int img = patches[3 * p], h1 = patches[3 * p + 1], w1 = patches[3 * p + 2];
  const long W = images[3 * img + 2];
  const long base = images[3 * img] + h1 * W + w1;
  const int i0 = blockIdx.y * kT, j0 = blockIdx.x * kT, L = size - 1;
  const int oh = min(kT, size - i0), ow = min(kT, size - j0);          // the tile's part of the output
  int ai, aj, bi, bj;                                                  // the sources of two opposite corners span the source square
  source_pixel(i0, j0, L, rot, flip, ai, aj);
  source_pixel(i0 + oh - 1, j0 + ow - 1, L, rot, flip, bi, bj);
  const int sr0 = min(ai, bi), sc0 = min(aj, bj);
  const int sh = abs(ai - bi) + 1, sw3 = 3 * (abs(aj - bj) + 1);
  for (int e = t; e < sh * sw3; e += 256) {
    const int r = e / sw3, x = e - r * sw3;
    const long a = 3 * (base + (sr0 + r) * W + sc0) + x;
    tile_h[r * kPitch + x] = hdr[a];
    tile_l[r * kPitch + x] = (float)ldr[a];
  }
  __syncthreads();
  const float denom = 1e-6f + mean[p];
  const int ow3 = 3 * ow;
  for (int e = t; e < oh * ow3; e += 256) {
    const int i = e / ow3, x = e - i * ow3, j = x / 3, c = x - 3 * j;
    int si, sj;
    source_pixel(i0 + i, j0 + j, L, rot, flip, si, sj);
    const int l = (si - sr0) * kPitch + 3 * (sj - sc0) + c;
    const long o = (((long)n * size + i0 + i) * size + j0) * 3 + x;
    out_ldr[o] = tile_l[l] / 255.0f;                                   // ref_LDR / 255.0           (finetune_real_dataset.py:49)
    out_hdr[o] = tile_h[l] / denom * 0.5f;                             // ref_HDR / (1e-6 + mean) * 0.5   (:47)
  }
}

// ---- host-side checks of the host tables: nothing below launches with an index that leaves a table or an arena ---------------
int check_image(const char* what, const int64_t* images, int img, int64_t arena_pixels) {
  const int64_t off = images[3 * img], H = images[3 * img + 1], W = images[3 * img + 2];
  SHDR_REQUIRE(H > 0 && W > 0 && H <= INT32_MAX && W <= INT32_MAX, SHDR_E_SHAPE, "%s: image %d is %lld x %lld", what, img, (long long)H,
               (long long)W);
  SHDR_REQUIRE(off >= 0 && off <= arena_pixels && H <= (arena_pixels - off) / W, SHDR_E_SHAPE,
               "%s: image %d (%lld x %lld at pixel %lld) leaves the arenas of %lld pixels", what, img, (long long)H, (long long)W,
               (long long)off, (long long)arena_pixels);
  return SHDR_OK;
}

int check_patch(const char* what, const int64_t* images, int n_images, const int32_t* patches, int p, int size, int64_t arena_pixels) {
  const int img = patches[3 * p], h1 = patches[3 * p + 1], w1 = patches[3 * p + 2];
  SHDR_REQUIRE(img >= 0 && img < n_images, SHDR_E_SHAPE, "%s: patch %d names image %d of %d", what, p, img, n_images);
  const int rc = check_image(what, images, img, arena_pixels);
  if (rc != SHDR_OK) return rc;
  const int64_t H = images[3 * img + 1], W = images[3 * img + 2];
  SHDR_REQUIRE(h1 >= 0 && w1 >= 0 && (int64_t)h1 + size <= H && (int64_t)w1 + size <= W, SHDR_E_SHAPE,
               "%s: patch %d (%d x %d at row %d, column %d) leaves its %lld x %lld image", what, p, size, size, h1, w1, (long long)H,
               (long long)W);
  return SHDR_OK;
}

}  // namespace

extern "C" int shdr_pair_patch_stats(const uint8_t* ldr, const float* hdr, int64_t arena_pixels, const int64_t* images_host,
                                     const int64_t* images, int n_images, const int32_t* patches_host, const int32_t* patches,
                                     int n_patches, int size, int32_t* count, float* mean, void* stream) {
  SHDR_REQUIRE(size > 0 && size <= kMaxSize, SHDR_E_SHAPE, "pair_patch_stats: size %d (1 .. %d)", size, kMaxSize);
  SHDR_REQUIRE(ldr && hdr && images_host && images && patches_host && patches && count && mean, SHDR_E_NULL,
               "pair_patch_stats: null pointer");
  SHDR_REQUIRE(n_images > 0 && n_patches > 0 && arena_pixels > 0, SHDR_E_SHAPE, "pair_patch_stats: %d images, %d patches, %lld pixels",
               n_images, n_patches, (long long)arena_pixels);
  for (int p = 0; p < n_patches; ++p) {
    const int rc = check_patch("pair_patch_stats", images_host, n_images, patches_host, p, size, arena_pixels);
    if (rc != SHDR_OK) return rc;
  }
  hipLaunchKernelGGL(pair_patch_stats_kernel, dim3(n_patches), dim3(256), 0, shdr::stream_of(stream), ldr, hdr, images, patches, size, count, mean);
  return shdr::check_launch("pair_patch_stats");
}

extern "C" int shdr_pair_patch_gather_f32(const uint8_t* ldr, const float* hdr, int64_t arena_pixels, const int64_t* images_host,
                                          const int64_t* images, int n_images, const int32_t* patches_host, const int32_t* patches,
                                          int n_patches, const float* mean, const int32_t* samples_host, const int32_t* samples, int b,
                                          int size, float* out_ldr, float* out_hdr, void* stream) {
  SHDR_REQUIRE(size > 0 && size <= kMaxSize, SHDR_E_SHAPE, "pair_patch_gather: size %d (1 .. %d)", size, kMaxSize);
  SHDR_REQUIRE(b > 0 && b <= 65535, SHDR_E_SHAPE, "pair_patch_gather: batch of %d (1 .. 65535)", b);
  SHDR_REQUIRE(ldr && hdr && images_host && images && patches_host && patches && mean && samples_host && samples && out_ldr && out_hdr,
               SHDR_E_NULL, "pair_patch_gather: null pointer");
  SHDR_REQUIRE(n_images > 0 && n_patches > 0 && arena_pixels > 0, SHDR_E_SHAPE, "pair_patch_gather: %d images, %d patches, %lld pixels",
               n_images, n_patches, (long long)arena_pixels);
  for (int n = 0; n < b; ++n) {
    const int p = samples_host[3 * n], flip = samples_host[3 * n + 1], rot = samples_host[3 * n + 2];
    SHDR_REQUIRE(p >= 0 && p < n_patches, SHDR_E_SHAPE, "pair_patch_gather: sample %d names patch %d of %d", n, p, n_patches);
    SHDR_REQUIRE(flip == 0 || flip == 1, SHDR_E_SHAPE, "pair_patch_gather: sample %d has flip %d (0 or 1)", n, flip);
    SHDR_REQUIRE(rot >= 0 && rot <= 4, SHDR_E_SHAPE, "pair_patch_gather: sample %d has rot %d (0 .. 4)", n, rot);
    const int rc = check_patch("pair_patch_gather", images_host, n_images, patches_host, p, size, arena_pixels);
    if (rc != SHDR_OK) return rc;
  }
  const int tiles = (size + kT - 1) / kT;
  hipLaunchKernelGGL(pair_patch_gather_kernel, dim3(tiles, tiles, b), dim3(256), 0, shdr::stream_of(stream), ldr, hdr, images, patches, mean, samples,
                     size, out_ldr, out_hdr);
  return shdr::check_launch("pair_patch_gather");
}

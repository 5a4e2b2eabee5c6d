// OpenEXR output (exr.py encode_exr): float32 images [H][W][3] -> the planar scanline bytes of every chunk and, for ZIP / ZIPS,
// the predicted bytes that get deflated -- the encode side of csrc/exr.hip, for a BATCH of images of different sizes in one launch.
//
// One block per chunk (`lines` scanlines of one image).  Byte j of a chunk's scanline bytes is byte (j mod sample size) of one sample:
// row j / row_bytes, channel plane (B, G, R) and column from the remainder -- a pure gather.  The predictor is a gather too on this
// side: with h = (n + 1) / 2,  t[i] = a[2 i] for i < h, a[2 (i - h) + 1] after it,  d[0] = t[0], d[i] = t[i] - t[i - 1] + 128 mod 256
// (tests/exr_ref.py predict), so every output byte reads at most two samples and nothing is carried across threads.  The pixels are
// read three times (once for the planar byte, twice for the predicted one) and the vector L1 / L2 serve the repeats.
// HALF conversion: exr_half.h, integer arithmetic, no floating-point contraction or rounding mode involved.
#include "shdr_internal.h"
#include "batch.h"
#include "exr_half.h"

namespace {

constexpr int kThreads = 256;
constexpr int64_t kMaxSide = 1 << 20, kMaxPixels = (int64_t)1 << 28;      // exr.py's reader refuses larger data windows

struct Pack {
  const float* pixels;
  int64_t pixel0;                                                // first pixel of the image
  int y0, W, row_bytes, plane_bytes, shift;                      // shift: log2 of the sample size
  bool half, reverse, saturate;
};

__device__ __forceinline__ uint32_t planar_byte(const Pack& p, int j) {
  const int r = j / p.row_bytes, q = j - r * p.row_bytes;
  const int k = q / p.plane_bytes, t = q - k * p.plane_bytes;    // k: 0 B, 1 G, 2 R
  const int x = t >> p.shift, b = t & ((1 << p.shift) - 1);
  const int ch = p.reverse ? k : 2 - k;
  uint32_t f = __float_as_uint(p.pixels[(p.pixel0 + (int64_t)(p.y0 + r) * p.W + x) * 3 + ch]);
  if (p.half) f = shdr_half_bits(p.saturate ? shdr_half_saturate(f) : f);
  return (f >> (8 * b)) & 255u;
}

__global__ __launch_bounds__(kThreads) void exr_pack_kernel(const float* __restrict__ pixels, const int64_t* __restrict__ table, int n_img,
                                                            int64_t n_chunks, int64_t total_bytes, int64_t total_pixels, int lines,
                                                            int sample_shift, int reverse, int saturate,
                                                            const int64_t* __restrict__ chunk_off, uint8_t* __restrict__ planar,
                                                            uint8_t* __restrict__ predicted) {
  const int64_t c = blockIdx.x;
  const int64_t* chunk0 = table;
  const int lo = (int)shdr::last_le(chunk0, n_img, c);           // the image of this chunk
  const int64_t hw = table[2 * (n_img + 1) + lo];
  const int H = (int)(hw >> 32), W = (int)(hw & 0xffffffff);
  Pack p;
  p.pixels = pixels;
  p.pixel0 = table[(n_img + 1) + lo];
  p.y0 = (int)(c - chunk0[lo]) * lines;
  p.W = W;
  p.shift = sample_shift;
  p.plane_bytes = W << sample_shift;
  p.row_bytes = 3 * p.plane_bytes;
  p.half = sample_shift == 1;
  p.reverse = reverse != 0;
  p.saturate = saturate != 0;
  if (p.y0 < 0 || p.y0 >= H || W < 1) return;
  const int rows = min(lines, H - p.y0);
  const int n = rows * p.row_bytes;
  const int64_t base = chunk_off[c];
  // (never with the tables of shdr_exr_pack_sizes: the chunk lies in the buffers and its pixels in the batch)
  if (base < 0 || base + n > total_bytes || p.pixel0 < 0 || p.pixel0 + (int64_t)(p.y0 + rows) * W > total_pixels) return;
  const int h = (n + 1) >> 1;
  for (int j = threadIdx.x; j < n; j += kThreads) {
    planar[base + j] = (uint8_t)planar_byte(p, j);
    if (predicted) {
      const uint32_t t = planar_byte(p, j < h ? 2 * j : 2 * (j - h) + 1);
      uint32_t d = t;
      if (j > 0) d = t - planar_byte(p, j - 1 < h ? 2 * (j - 1) : 2 * (j - 1 - h) + 1) + 128u;
      predicted[base + j] = (uint8_t)d;
    }
  }
}

__device__ __forceinline__ void store_le(uint8_t* p, uint64_t v, int bytes) {
  for (int b = 0; b < bytes; ++b) p[b] = (uint8_t)(v >> (8 * b));
}

__global__ __launch_bounds__(kThreads) void exr_finish_kernel(uint8_t* __restrict__ records, uint8_t* __restrict__ tables,
                                                              const int64_t* __restrict__ out_offsets, const int64_t* __restrict__ table,
                                                              const int64_t* __restrict__ header_len, int n_img, int64_t n_chunks, int lines) {
  const int64_t c = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  if (c >= n_chunks) return;
  const int lo = (int)shdr::last_le(table, n_img, c);
  const int64_t c0 = table[lo], c1 = table[lo + 1];
  const int64_t at = out_offsets[c], size = out_offsets[c + 1] - at - 8;
  store_le(records + at, (uint64_t)(uint32_t)((c - c0) * lines), 4);
  store_le(records + at + 4, (uint64_t)(uint32_t)size, 4);
  store_le(tables + 8 * c, (uint64_t)(header_len[lo] + 8 * (c1 - c0) + at - out_offsets[c0]), 8);
}

int check_shapes(const char* what, const int32_t* shapes, int n, int pixel_type, int lines, int64_t* chunks, int64_t* bytes, int64_t* pixels) {
  SHDR_REQUIRE(shapes, SHDR_E_NULL, "%s: null shape table", what);
  SHDR_REQUIRE(n > 0, SHDR_E_SHAPE, "%s: the number of images must be positive, got %d", what, n);
  SHDR_REQUIRE(pixel_type == SHDR_EXR_HALF || pixel_type == SHDR_EXR_FLOAT, SHDR_E_SHAPE, "%s: pixel type %d is neither HALF (1) nor FLOAT (2)",
               what, pixel_type);
  SHDR_REQUIRE(lines == 1 || lines == 16 || lines == 32, SHDR_E_SHAPE, "%s: a chunk holds 1, 16 or 32 scanlines, got %d", what, lines);
  const int64_t sample = pixel_type == SHDR_EXR_HALF ? 2 : 4;
  int64_t c = 0, b = 0, p = 0;
  for (int i = 0; i < n; ++i) {
    const int64_t h = shapes[2 * i], w = shapes[2 * i + 1];
    SHDR_REQUIRE(h > 0 && w > 0 && h <= kMaxSide && w <= kMaxSide && h * w <= kMaxPixels, SHDR_E_SHAPE,
                 "%s: image %d is %lld x %lld (H x W): sides are 1 .. 2^20 and an image has at most 2^28 pixels", what, i, (long long)h,
                 (long long)w);
    c += (h + lines - 1) / lines;
    b += h * w * 3 * sample;
    p += h * w;
  }
  SHDR_REQUIRE(c < ((int64_t)1 << 31), SHDR_E_SHAPE, "%s: %lld chunks in one call, the limit is 2^31 - 1", what, (long long)c);
  *chunks = c;
  *bytes = b;
  *pixels = p;
  return SHDR_OK;
}

}  // namespace

extern "C" int shdr_exr_pack_sizes(const int32_t* shapes, int n_images, int pixel_type, int lines, int64_t* n_chunks, int64_t* bytes,
                                   int64_t* table, int64_t* chunk_off) {
  int64_t chunks = 0, total = 0, pixels = 0;
  if (int rc = check_shapes("exr_pack_sizes", shapes, n_images, pixel_type, lines, &chunks, &total, &pixels)) return rc;
  if (n_chunks) *n_chunks = chunks;
  if (bytes) *bytes = total;
  const int64_t sample = pixel_type == SHDR_EXR_HALF ? 2 : 4, stride = n_images + 1;
  int64_t c = 0, b = 0, p = 0;
  for (int i = 0; i < n_images; ++i) {
    const int64_t h = shapes[2 * i], w = shapes[2 * i + 1];
    if (table) {
      table[i] = c;
      table[stride + i] = p;
      table[2 * stride + i] = (h << 32) | w;
    }
    for (int64_t y = 0; y < h; y += lines) {
      if (chunk_off) chunk_off[c] = b;
      b += (h - y < lines ? h - y : lines) * w * 3 * sample;
      ++c;
    }
    p += h * w;
  }
  if (table) {
    table[n_images] = c;
    table[stride + n_images] = p;
    table[2 * stride + n_images] = 0;
  }
  if (chunk_off) chunk_off[c] = b;
  return SHDR_OK;
}

extern "C" int shdr_exr_pack_f32(const float* pixels, const int32_t* shapes, int n_images, int pixel_type, int lines, int reverse_channels,
                                 int saturate, const int64_t* table_dev, const int64_t* chunk_off, uint8_t* planar, uint8_t* predicted,
                                 void* stream) {
  const char* what = "exr_pack_f32";
  SHDR_REQUIRE(pixels && table_dev && chunk_off && planar, SHDR_E_NULL, "%s: null pointer", what);
  int64_t chunks = 0, total = 0, npix = 0;
  if (int rc = check_shapes(what, shapes, n_images, pixel_type, lines, &chunks, &total, &npix)) return rc;
  SHDR_REQUIRE((reinterpret_cast<uintptr_t>(pixels) & 3u) == 0, SHDR_E_ALIGN, "%s: pixels must be 4-byte aligned", what);
  SHDR_REQUIRE((reinterpret_cast<uintptr_t>(table_dev) & 7u) == 0 && (reinterpret_cast<uintptr_t>(chunk_off) & 7u) == 0, SHDR_E_ALIGN,
               "%s: table_dev and chunk_off must be 8-byte aligned", what);
  hipLaunchKernelGGL(exr_pack_kernel, dim3((unsigned)chunks), dim3(kThreads), 0, shdr::stream_of(stream), pixels, table_dev, n_images, chunks, total, npix,
                     lines, pixel_type == SHDR_EXR_HALF ? 1 : 2, reverse_channels, saturate, chunk_off, planar, predicted);
  return shdr::check_launch(what);
}

extern "C" int shdr_exr_finish_chunks(uint8_t* records, uint8_t* tables, const int64_t* out_offsets, const int64_t* table_dev,
                                      const int64_t* header_len, int n_images, int64_t n_chunks, int lines, void* stream) {
  const char* what = "exr_finish_chunks";
  SHDR_REQUIRE(records && tables && out_offsets && table_dev && header_len, SHDR_E_NULL, "%s: null pointer", what);
  SHDR_REQUIRE(n_images > 0 && n_chunks > 0 && n_chunks < ((int64_t)1 << 31), SHDR_E_SHAPE, "%s: %d images, %lld chunks", what, n_images,
               (long long)n_chunks);
  SHDR_REQUIRE(lines == 1 || lines == 16 || lines == 32, SHDR_E_SHAPE, "%s: a chunk holds 1, 16 or 32 scanlines, got %d", what, lines);
  hipLaunchKernelGGL(exr_finish_kernel, dim3((unsigned)((n_chunks + kThreads - 1) / kThreads)), dim3(kThreads), 0, shdr::stream_of(stream), records, tables,
                     out_offsets, table_dev, header_len, n_images, n_chunks, lines);
  return shdr::check_launch(what);
}

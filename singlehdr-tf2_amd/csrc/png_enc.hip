// PNG files of a BATCH of 8-bit images of different sizes and channel counts on the device: byte for byte what the host twin
// shdr_png_encode_host writes (png.h holds what both share: the filters, the segment cuts, the framing, the checksums' algebra).
//
// Launches (stream-ordered, no global atomics, no host wait; the same input gives the same bytes):
//   1  png_tables_kernel   ONE block: scans of the images' pixels, stream bytes, rows and segments, then every segment's offset in the
//                          filtered arena, its flags (first / last of its image) and its image
//      png_filter_kernel   one 64-lane wave per row, four rows per block: every byte with its three neighbours (x, a, b, c straight from
//                          the pixels, byte loads that the lanes of a wave coalesce), the five candidates' costs, a wave reduction, the
//                          type; then the row is read again -- the caches hold it -- filtered with that type and stored.  (Rows of up
//                          to 2048 bytes kept in registers in between, 32 words per lane, took twice as long: 194 VGPRs, two waves per
//                          SIMD)  A fixed filter skips the costing
//   2-4  the three launches of csrc/deflate_batch.h over the segments (run_segments of the chosen encoder): sizes and Adler-32 per
//                          segment, the scan that places every segment in the files, the blocks or stored blocks themselves
//   5  png_frame_kernel    one block per segment: signature and IHDR in front of an image's first, the IDAT's length and tag, the zlib
//                          bytes, the Adler-32 of the image (adler_combine over its segments' sums of pass 2), IEND; then the chunk's
//                          CRC-32: every lane runs the table over its slice, shifts it by the bytes behind it (crc_shift) and the
//                          block XORs the results.  The image's file offset goes to `offsets`
#include "shdr_internal.h"
#include "batch.h"
#include "png.h"
#include "deflate_batch.h"

namespace {

using namespace shdr_png;

constexpr int kThreads = 256;
constexpr int kRowsPerBlock = kThreads / 64;

struct Tables {                               // carved out of the caller's workspace, every part 16-byte aligned
  uint8_t* arena;                             // [stream] the filtered streams back to back
  int64_t* img_pix;                           // [n + 1] first pixel byte of image i
  int64_t* img_stream;                        // [n + 1] first byte of its filtered stream
  int64_t* img_row;                           // [n + 1] its first row among all rows
  int64_t* img_seg;                           // [n + 1] its first segment
  int64_t* seg_off;                           // [S + 1] a segment's first byte in the arena
  int64_t* out_off;                           // [S + 1] where its front begins in the output
  int32_t* seg_img;                           // [S]
  uint8_t* seg_flags;                         // [S]
  uint8_t* coded;                             // [S]
  void* deflate;                              // the encoder's workspace
  int64_t bytes;
};
Tables carve_tables(void* ws, int64_t n, int64_t stream, int64_t segs, int64_t deflate_bytes) {
  Tables t;
  shdr::Carver cut(ws);
  t.arena = cut.take<uint8_t>(stream);
  t.img_pix = cut.take<int64_t>(n + 1);
  t.img_stream = cut.take<int64_t>(n + 1);
  t.img_row = cut.take<int64_t>(n + 1);
  t.img_seg = cut.take<int64_t>(n + 1);
  t.seg_off = cut.take<int64_t>(segs + 1);
  t.out_off = cut.take<int64_t>(segs + 1);
  t.seg_img = cut.take<int32_t>(segs);
  t.seg_flags = cut.take<uint8_t>(segs);
  t.coded = cut.take<uint8_t>(segs);
  t.deflate = cut.take<uint8_t>(deflate_bytes);
  t.bytes = cut.bytes();
  return t;
}

// what the host sums up from the shapes; the kernels clamp what they derive from the device copy to these
struct Totals {
  int64_t pixels, stream, rows, segs;
};

struct Shape {
  int64_t h, w, c;
};
__device__ __forceinline__ Shape shape_of(const int32_t* __restrict__ images, int64_t i) {
  Shape s{images[4 * i], images[4 * i + 1], images[4 * i + 2]};
  if (!shape_ok(s.h, s.w, s.c)) s = Shape{1, 1, 1};              // never with the shapes the host checked
  return s;
}

__global__ __launch_bounds__(1024) void png_tables_kernel(const int32_t* __restrict__ images, int64_t n, Totals tot, Tables t) {
  auto scan = [&](int64_t* dst, auto value) {
    const int64_t all = shdr::scan_array<1024, 1>(
        n, [&](int64_t i) { return (int64_t)value(shape_of(images, i)); }, [&](int64_t i, int64_t before) { dst[i] = before; });
    if (threadIdx.x == 0) dst[n] = all;
  };
  scan(t.img_pix, [](Shape s) { return s.h * s.w * s.c; });
  scan(t.img_stream, [](Shape s) { return stream_bytes(s.h, s.w, s.c); });
  scan(t.img_row, [](Shape s) { return s.h; });
  scan(t.img_seg, [](Shape s) { return segments(stream_bytes(s.h, s.w, s.c)); });
  __syncthreads();
  for (int64_t s = threadIdx.x; s < tot.segs; s += 1024) {
    const int64_t i = shdr::last_le(t.img_seg, n, s), k = s - t.img_seg[i];
    t.seg_off[s] = t.img_stream[i] + k * kPngSegment;
    t.seg_img[s] = (int32_t)i;
    t.seg_flags[s] = (uint8_t)((k == 0 ? kFirst : 0) | (s + 1 == t.img_seg[i + 1] ? kLast : 0));
  }
  if (threadIdx.x == 0) t.seg_off[tot.segs] = t.img_stream[n];
}

__device__ __forceinline__ uint64_t wave_sum(uint64_t v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
  return v;
}

__global__ __launch_bounds__(kThreads) void png_filter_kernel(const uint8_t* __restrict__ pixels, const int32_t* __restrict__ images, int64_t n,
                                                              int filter, Totals tot, Tables t) {
  const int lane = threadIdx.x & 63;
  const int64_t r = (int64_t)blockIdx.x * kRowsPerBlock + (threadIdx.x >> 6);
  if (r >= tot.rows) return;                                     // (no barrier below: a wave is on its own)
  const int64_t i = shdr::last_le(t.img_row, n, r), y = r - t.img_row[i];
  const Shape s = shape_of(images, i);
  const int64_t len = s.w * s.c, src_at = t.img_pix[i] + y * len, dst_at = t.img_stream[i] + y * (len + 1);
  if (y >= s.h || src_at < (y ? len : 0) || src_at + len > tot.pixels || dst_at < 0 || dst_at + len + 1 > tot.stream) return;   // as above
  const uint8_t* row = pixels + src_at;
  const uint8_t* above = y ? row - len : nullptr;
  const int bpp = (int)s.c;
  int type = filter;
  if (filter == kAdaptive) {
    uint64_t costs[5] = {0, 0, 0, 0, 0};
    for (int64_t k = lane; k < len; k += 64) {
      const int x = row[k], a = k >= bpp ? row[k - bpp] : 0, b = above ? above[k] : 0, c = above && k >= bpp ? above[k - bpp] : 0;
#pragma unroll
      for (int f = 0; f < 5; ++f) costs[f] += cost(filtered(f, x, a, b, c));
    }
#pragma unroll
    for (int f = 0; f < 5; ++f) costs[f] = wave_sum(costs[f]);
    type = cheapest(costs);
  }
  uint8_t* dst = t.arena + dst_at;
  if (lane == 0) dst[0] = (uint8_t)type;
  for (int64_t k = lane; k < len; k += 64) {
    const int x = row[k], a = k >= bpp ? row[k - bpp] : 0, b = above ? above[k] : 0, c = above && k >= bpp ? above[k - bpp] : 0;
    dst[1 + k] = filtered(type, x, a, b, c);
  }
}

__global__ __launch_bounds__(kThreads) void png_frame_kernel(const int32_t* __restrict__ images, int64_t n, Totals tot, Tables t,
                                                             const uint32_t* __restrict__ adler, uint8_t* __restrict__ out, int64_t capacity,
                                                             int64_t* __restrict__ offsets) {
  __shared__ uint32_t table[256];
  __shared__ uint32_t part[kThreads / 64];
  const int tid = threadIdx.x;
  const int64_t s = blockIdx.x;
  const int flags = t.seg_flags[s];
  const int64_t i = t.seg_img[s];
  const int64_t base = t.out_off[s], end = t.out_off[s + 1];
  table[tid] = crc_entry((uint32_t)tid);
  const int front = seg_front(flags), back = seg_back(flags);
  const bool ok = i >= 0 && i < n && base >= 0 && end <= capacity && end - base >= front + back;   // never false with the sizes the host checked
  const int64_t chunk = ok ? base + front - 8 - ((flags & kFirst) ? 2 : 0) : 0;                    // where the IDAT's length stands
  const int64_t crc_at = ok ? end - back + ((flags & kLast) ? 4 : 0) : 0;                          // where its CRC goes
  __syncthreads();
  if (ok && tid == 0) {
    const Shape sh = shape_of(images, i);
    if (flags & kFirst) {
      put_head(out + base, sh.h, sh.w, (int)sh.c, table);
      out[chunk + 8] = 0x78;
      out[chunk + 9] = 0x01;
      offsets[i] = base;
    }
    put_be32(out + chunk, (uint32_t)(crc_at - chunk - 8));
    out[chunk + 4] = 'I';
    out[chunk + 5] = 'D';
    out[chunk + 6] = 'A';
    out[chunk + 7] = 'T';
    if (flags & kLast) {
      const int64_t s0 = t.img_seg[i];
      uint32_t a = 1;                                            // of no bytes
      for (int64_t k = s0 < 0 ? s : s0; k <= s; ++k) a = adler_combine(a, adler[k], t.seg_off[k + 1] - t.seg_off[k]);
      put_be32(out + crc_at - 4, a);
      put_iend(out + crc_at + 4);
    }
    if (s + 1 == tot.segs) offsets[n] = end;
  }
  __syncthreads();                                               // the block's stores to `out` are visible to the block
  uint32_t reg = 0;
  if (ok) {
    const uint8_t* p = out + chunk + 4;
    const int64_t len = crc_at - chunk - 4, per = (len + kThreads - 1) / kThreads;
    const int64_t lo = per * tid < len ? per * tid : len, hi = lo + per < len ? lo + per : len;
    reg = crc_shift(crc_bytes(tid == 0 ? 0xFFFFFFFFu : 0u, p + lo, hi - lo, table), len - hi);
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) reg ^= __shfl_xor(reg, off, 64);
  if ((tid & 63) == 0) part[tid >> 6] = reg;
  __syncthreads();
  if (ok && tid == 0) put_be32(out + crc_at, ~(part[0] ^ part[1] ^ part[2] ^ part[3]));
}

// the shapes' sums, or the refusal of a shape
int sum_shapes(const char* what, const int32_t* images, int n, Totals* tot, int64_t* out_bytes) {
  SHDR_REQUIRE(images, SHDR_E_NULL, "%s: null images", what);
  SHDR_REQUIRE(n > 0, SHDR_E_SHAPE, "%s: the number of images must be positive, got %d", what, n);
  *tot = Totals{0, 0, 0, 0};
  *out_bytes = 0;
  for (int i = 0; i < n; ++i) {
    const int64_t h = images[4 * i], w = images[4 * i + 1], c = images[4 * i + 2];
    SHDR_REQUIRE(colour_type((int)c) >= 0, SHDR_E_SHAPE, "%s: image %d has %lld channels (1 grey, 3 RGB and 4 RGBA are supported)", what, i,
                 (long long)c);
    SHDR_REQUIRE(shape_ok(h, w, c), SHDR_E_SHAPE, "%s: image %d is %lld x %lld x %lld: H >= 1, W >= 1 and H (W C + 1) < 2^31 are supported", what,
                 i, (long long)h, (long long)w, (long long)c);
    const int64_t stream = stream_bytes(h, w, c);
    tot->pixels += h * w * c;
    tot->stream += stream;
    tot->rows += h;
    tot->segs += segments(stream);
    *out_bytes += file_bound(stream);
  }
  SHDR_REQUIRE(tot->segs < ((int64_t)1 << 31) && (tot->rows + kRowsPerBlock - 1) / kRowsPerBlock < ((int64_t)1 << 31), SHDR_E_SHAPE,
               "%s: %lld rows in %lld segments are more than one launch takes", what, (long long)tot->rows, (long long)tot->segs);
  return SHDR_OK;
}

int check_options(const char* what, int filter, int deflate) {
  SHDR_REQUIRE(filter >= kNone && filter <= kAdaptive, SHDR_E_SHAPE, "%s: filter must be SHDR_PNG_FILTER_NONE .. _ADAPTIVE, got %d", what, filter);
  SHDR_REQUIRE(deflate == kHuffman || deflate == kLz, SHDR_E_SHAPE, "%s: deflate must be SHDR_PNG_DEFLATE_HUFFMAN or _LZ, got %d", what, deflate);
  return SHDR_OK;
}

shdr_deflate_batch::SegmentCoder coder_of(int deflate) {
  return deflate == kLz ? shdr_deflate_batch::lz_segments() : shdr_deflate_batch::huffman_segments();
}

static_assert(kPngSegment == SHDR_PNG_SEGMENT && kAdaptive == SHDR_PNG_FILTER_ADAPTIVE && kPaeth == SHDR_PNG_FILTER_PAETH &&
                  kLz == SHDR_PNG_DEFLATE_LZ && kHuffman == SHDR_PNG_DEFLATE_HUFFMAN,
              "shdr.h names the segment size and the options");

}  // namespace

extern "C" uint32_t shdr_crc32(const void* data, uint64_t n, uint32_t crc) {
  return crc32_host(static_cast<const uint8_t*>(data), (int64_t)n, crc);
}

extern "C" int64_t shdr_png_filter_host(const uint8_t* pixels, int h, int w, int c, int filter, uint8_t* out, int64_t capacity) {
  if (!pixels || !out) return shdr::fail(SHDR_E_NULL, "png_filter_host: null pointer");
  if (!shape_ok(h, w, c)) return shdr::fail(SHDR_E_SHAPE, "png_filter_host: %d x %d x %d is outside the writer's scope (C 1, 3 or 4; H (W C + 1) < 2^31)", h, w, c);
  if (int rc = check_options("png_filter_host", filter, kLz)) return rc;
  const int64_t stream = stream_bytes(h, w, c);
  if (capacity < stream) return shdr::fail(SHDR_E_SHAPE, "png_filter_host: output buffer too small (%lld < %lld)", (long long)capacity, (long long)stream);
  for (int64_t y = 0; y < h; ++y) filter_row_host(pixels, y, w, c, filter, out + y * ((int64_t)w * c + 1));
  return stream;
}

extern "C" int64_t shdr_png_encode_host(const uint8_t* pixels, int h, int w, int c, int filter, int deflate, uint8_t* out, int64_t capacity) {
  if (!pixels || !out) return shdr::fail(SHDR_E_NULL, "png_encode_host: null pointer");
  if (!shape_ok(h, w, c)) return shdr::fail(SHDR_E_SHAPE, "png_encode_host: %d x %d x %d is outside the writer's scope (C 1, 3 or 4; H (W C + 1) < 2^31)", h, w, c);
  if (int rc = check_options("png_encode_host", filter, deflate)) return rc;
  int64_t need = 0;
  const int64_t r = encode_host(pixels, h, w, c, filter, deflate, out, capacity, &need);
  if (r == -2) return shdr::fail(SHDR_E_SHAPE, "png_encode_host: output buffer too small (%lld < %lld)", (long long)capacity, (long long)need);
  if (r < 0) return shdr::fail(SHDR_E_SHAPE, "png_encode_host: no memory for an image of %d x %d x %d", h, w, c);
  return r;
}

extern "C" int shdr_png_encode_batch_sizes(const int32_t* images, int n_images, int deflate, int64_t* pixel_bytes, int64_t* out_bytes,
                                           int64_t* n_segments, int64_t* workspace_bytes) {
  Totals tot;
  int64_t bound = 0;
  if (int rc = sum_shapes("png_encode_batch_sizes", images, n_images, &tot, &bound)) return rc;
  if (int rc = check_options("png_encode_batch_sizes", kAdaptive, deflate)) return rc;
  if (pixel_bytes) *pixel_bytes = tot.pixels;
  if (out_bytes) *out_bytes = bound;
  if (n_segments) *n_segments = tot.segs;
  if (workspace_bytes) *workspace_bytes = carve_tables(nullptr, n_images, tot.stream, tot.segs, coder_of(deflate).workspace_bytes(tot.segs, tot.stream)).bytes;
  return SHDR_OK;
}

extern "C" int shdr_png_encode_batch(const uint8_t* pixels, const int32_t* images, const int32_t* images_dev, int n_images, int filter,
                                     int deflate, uint8_t* out, int64_t out_capacity, int64_t* offsets, void* workspace, void* stream,
                                     float* stage_ms) {
  const char* what = "png_encode_batch";
  SHDR_REQUIRE(pixels && images_dev && out && offsets && workspace, SHDR_E_NULL, "%s: null pointer", what);
  Totals tot;
  int64_t bound = 0;
  if (int rc = sum_shapes(what, images, n_images, &tot, &bound)) return rc;
  if (int rc = check_options(what, filter, deflate)) return rc;
  SHDR_REQUIRE((reinterpret_cast<uintptr_t>(images_dev) & 3u) == 0 && (reinterpret_cast<uintptr_t>(offsets) & 7u) == 0, SHDR_E_ALIGN,
               "%s: images_dev must be 4-byte and offsets 8-byte aligned", what);
  SHDR_REQUIRE(shdr::aligned16(workspace), SHDR_E_ALIGN, "%s: workspace must be 16-byte aligned", what);
  SHDR_REQUIRE(out_capacity >= bound, SHDR_E_SHAPE, "%s: output buffer too small (%lld < %lld)", what, (long long)out_capacity, (long long)bound);
  const shdr_deflate_batch::SegmentCoder coder = coder_of(deflate);
  const Tables t = carve_tables(workspace, n_images, tot.stream, tot.segs, coder.workspace_bytes(tot.segs, tot.stream));
  hipStream_t st = shdr::stream_of(stream);
  using Timer = shdr::StageTimer<SHDR_PNG_STAGES>;
  Timer timer(stage_ms, st);
  hipLaunchKernelGGL(png_tables_kernel, dim3(1), dim3(1024), 0, st, images_dev, (int64_t)n_images, tot, t);
  hipLaunchKernelGGL(png_filter_kernel, dim3((unsigned)((tot.rows + kRowsPerBlock - 1) / kRowsPerBlock)), dim3(kThreads), 0, st, pixels, images_dev,
                     (int64_t)n_images, filter, tot, t);
  timer.mark();
  const uint32_t* adler = nullptr;
  coder.run(t.arena, t.seg_off, tot.segs, tot.stream, t.seg_flags, out, out_capacity, t.out_off, t.coded, t.deflate, st, &adler,
            [](void* p) { static_cast<Timer*>(p)->mark(); }, &timer);
  hipLaunchKernelGGL(png_frame_kernel, dim3((unsigned)tot.segs), dim3(kThreads), 0, st, images_dev, (int64_t)n_images, tot, t, adler, out,
                     out_capacity, offsets);
  timer.mark();
  return shdr::check_launch(what);
}

// The scan regions of a BATCH of JPEG files prepared on the device for the decoder of jpeg.hip: the rules are those of jpeg_scan.h, the
// very code of the host twin shdr_jpeg_scan_host.  Two stream-ordered calls with the host's layout (jpeg.py) between them:
//
// shdr_jpeg_scan: where every region ends, how many bytes are kept and how many restart markers lie before that end, and per marker
// the number of kept bytes before it.
//      init      end = none per image, no fill byte seen
//      end       the smallest marker position per image: a minimum per tile, one atomicMin per tile that has a marker
//      count     kept bytes and restart markers per tile before `end`; the fill flag
//      prefix    the tile totals summed over the whole batch, two levels (the pattern of scan_local / scan_partials of jpeg.hip):
//                an image's figure is the difference of two entries
//      bounds    the boundary of every restart marker that has a slot;  report: a few words per image
// shdr_jpeg_compact: kept byte j of segment s to arena[seg_dword[s] * 4 + (j - boundary of s)], into an arena filled with FF.
//
// A tile is kTile = 4096 raw bytes, a lane loads 16 of them in one aligned load (the regions start on multiples of 16) and re-reads
// the byte before and the byte after its 16 from global memory: no tile needs another.  Counts inside a tile are popcounts of the
// lanes' 16-bit masks, summed with shuffles.  The compaction writes its bytes with byte stores (first form: see DESIGN.md section 9
// for what they cost).  Every boundary store goes through bound_slot and every arena store through arena_index of jpeg_scan.h,
// whatever the bytes are: a file with more markers than its header implies is counted and writes nothing outside its slots.
// atomicMin on the ends and a store of 1 to the fill flag are the only cross-tile writes: the same input gives the same bits.
#include "shdr_internal.h"
#include "batch.h"
#include "jpeg_scan.h"

namespace {

using namespace jpegscan;

constexpr int WG = 256;
static_assert(kTile == WG * 16 && kScanChunk == WG, "a lane owns 16 bytes of a tile, and one tile total of a prefix chunk");
static_assert(sizeof(Image) == sizeof(shdr_jpeg_scan_image) && sizeof(Report) == sizeof(shdr_jpeg_scan_report), "mirrors of shdr.h");
constexpr int64_t kNoEnd = INT64_MAX;


struct Workspace {                                               // every part starts on a multiple of 16
  int64_t* end;                                                  // [n_images] kNoEnd or the end
  int32_t* fill;                                                 // [n_images]
  uint32_t* tile_count;                                          // [n_tiles] kept | restarts << 16
  int64_t* pre_kept;                                             // [n_tiles + 1] exclusive inside its chunk of kScanChunk
  int64_t* pre_rst;
  int64_t* part_kept;                                            // [chunks] exclusive over the chunks
  int64_t* part_rst;
  int64_t bytes;
};
Workspace carve(void* base, int n_images, int64_t n_tiles) {
  const int64_t m = n_tiles + 1, chunks = (m + kScanChunk - 1) / kScanChunk;
  shdr::Carver cut(base);
  Workspace w;
  w.end = cut.take<int64_t>(n_images);
  w.fill = cut.take<int32_t>(n_images);
  w.tile_count = cut.take<uint32_t>(n_tiles);
  w.pre_kept = cut.take<int64_t>(m);
  w.pre_rst = cut.take<int64_t>(m);
  w.part_kept = cut.take<int64_t>(chunks);
  w.part_rst = cut.take<int64_t>(chunks);
  w.bytes = cut.bytes();
  return w;
}

// the image of a tile: the last one whose first_tile is not beyond it (images without tiles share theirs with the next)
__device__ __forceinline__ int image_of(const Image* __restrict__ images, int n_images, int64_t tile) {
  int lo = 0, hi = n_images - 1;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (images[mid].first_tile <= tile) lo = mid; else hi = mid - 1;
  }
  return lo;
}

// a lane's 16 bytes of its tile and what they are: bit k of a mask speaks of region byte p0 + k
struct Lane {
  int64_t p0;
  uint8_t b[16];
  uint32_t valid, marker, restart, fill, dropped;
};
__device__ __forceinline__ Lane load_lane(const uint8_t* __restrict__ src, const Image& im, int64_t tile) {
  Lane L;
  const uint8_t* r = src + im.offset;
  const int64_t n = im.length;
  L.p0 = (tile - im.first_tile) * kTile + (int64_t)threadIdx.x * 16;
  L.valid = L.marker = L.restart = L.fill = L.dropped = 0;
  if (L.p0 >= n) return L;
  if (L.p0 + 16 <= n) {
    const uint4 v = *reinterpret_cast<const uint4*>(r + L.p0);    // offset, tile and lane are multiples of 16
    const uint32_t w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
    for (int k = 0; k < 16; ++k) L.b[k] = (uint8_t)(w[k >> 2] >> (8 * (k & 3)));
  } else {
#pragma unroll
    for (int k = 0; k < 16; ++k) L.b[k] = L.p0 + k < n ? r[L.p0 + k] : (uint8_t)0;
  }
  int prev = L.p0 > 0 ? (int)r[L.p0 - 1] : -1;
  const int after = L.p0 + 16 < n ? (int)r[L.p0 + 16] : -1;
#pragma unroll
  for (int k = 0; k < 16; ++k) {
    if (L.p0 + k < n) {
      const int next = k < 15 ? (L.p0 + k + 1 < n ? (int)L.b[k + 1] : -1) : after;
      const uint32_t c = byte_class(prev, L.b[k], next);
      L.valid |= 1u << k;
      if (c & kMarker) L.marker |= 1u << k;
      if (c & kRestart) L.restart |= 1u << k;
      if (c & kFill) L.fill |= 1u << k;
      if (c & kDropped) L.dropped |= 1u << k;
      prev = L.b[k];
    }
  }
  return L;
}
// the bits of a lane's masks that lie before `end`
__device__ __forceinline__ uint32_t before(const Lane& L, int64_t end) {
  const int64_t k = end - L.p0;
  return k <= 0 ? 0u : k >= 16 ? 0xFFFFu : (1u << k) - 1u;
}

__global__ __launch_bounds__(WG) void init_kernel(int64_t* __restrict__ end, int32_t* __restrict__ fill, int n_images) {
  const int i = blockIdx.x * WG + threadIdx.x;
  if (i < n_images) {
    end[i] = kNoEnd;
    fill[i] = 0;
  }
}

__global__ __launch_bounds__(WG) void end_kernel(const uint8_t* __restrict__ src, const Image* __restrict__ images, int n_images,
                                                 int64_t* __restrict__ end) {
  __shared__ unsigned long long wmin[WG / 64];
  const int64_t tile = blockIdx.x;
  const int i = image_of(images, n_images, tile);
  const Image im = images[i];
  const Lane L = load_lane(src, im, tile);
  unsigned long long m = L.marker ? (unsigned long long)(L.p0 + __builtin_ctz(L.marker)) : (unsigned long long)kNoEnd;
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    const unsigned long long u = __shfl_xor(m, off, 64);
    m = u < m ? u : m;
  }
  if ((threadIdx.x & 63) == 0) wmin[threadIdx.x >> 6] = m;
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int k = 1; k < WG / 64; ++k) m = wmin[k] < m ? wmin[k] : m;
    if (m != (unsigned long long)kNoEnd) atomicMin(reinterpret_cast<unsigned long long*>(end + i), m);
  }
}

__global__ __launch_bounds__(WG) void count_kernel(const uint8_t* __restrict__ src, const Image* __restrict__ images, int n_images,
                                                   const int64_t* __restrict__ end, int32_t* __restrict__ fill,
                                                   uint32_t* __restrict__ tile_count) {
  __shared__ uint32_t wsum[WG / 64];
  __shared__ uint32_t wfill[WG / 64];
  const int64_t tile = blockIdx.x;
  const int i = image_of(images, n_images, tile);
  const Image im = images[i];
  const Lane L = load_lane(src, im, tile);
  const uint32_t in = L.valid & before(L, end[i]);
  uint32_t c = (uint32_t)__builtin_popcount(in & ~L.dropped) | (uint32_t)__builtin_popcount(in & L.restart) << 16;
  uint32_t f = (in & L.fill) ? 1u : 0u;
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    c += (uint32_t)__shfl_xor((int)c, off, 64);                  // at most 4096 kept and 2048 restarts per tile: the halves do not meet
    f |= (uint32_t)__shfl_xor((int)f, off, 64);
  }
  if ((threadIdx.x & 63) == 0) {
    wsum[threadIdx.x >> 6] = c;
    wfill[threadIdx.x >> 6] = f;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int k = 1; k < WG / 64; ++k) {
      c += wsum[k];
      f |= wfill[k];
    }
    tile_count[tile] = c;
    if (f) fill[i] = 1;                                          // (every writer stores the same value)
  }
}

// tile totals -> per chunk of kScanChunk tiles their exclusive prefix sums and the chunk's totals; m = n_tiles + 1 entries, the last 0
__global__ __launch_bounds__(WG) void prefix_local_kernel(const uint32_t* __restrict__ tile_count, int64_t n_tiles, int64_t* __restrict__ pre_kept,
                                                          int64_t* __restrict__ pre_rst, int64_t* __restrict__ part_kept,
                                                          int64_t* __restrict__ part_rst) {
  __shared__ uint64_t wsum[WG / 64];
  const int64_t t = (int64_t)blockIdx.x * kScanChunk + threadIdx.x;
  const uint32_t c = t < n_tiles ? tile_count[t] : 0u;
  const uint64_t k = c & 0xFFFFu, r = c >> 16;
  const uint64_t ek = shdr::block_scan<WG>(k, wsum), er = shdr::block_scan<WG>(r, wsum);
  if (t <= n_tiles) {
    pre_kept[t] = (int64_t)ek;
    pre_rst[t] = (int64_t)er;
  }
  if (threadIdx.x == WG - 1) {
    part_kept[blockIdx.x] = (int64_t)(ek + k);
    part_rst[blockIdx.x] = (int64_t)(er + r);
  }
}

// one workgroup: the chunk totals -> their exclusive prefix sums, in place
__global__ __launch_bounds__(WG) void prefix_partials_kernel(int64_t* __restrict__ part_kept, int64_t* __restrict__ part_rst, int64_t chunks) {
  __shared__ uint64_t wsum[WG / 64];
  uint64_t run_k = 0, run_r = 0;
  for (int64_t i0 = 0; i0 < chunks; i0 += WG) {                  // (not scan_array: both arrays in one walk, one LDS array)
    const int64_t i = i0 + threadIdx.x;
    const uint64_t k = i < chunks ? (uint64_t)part_kept[i] : 0u, r = i < chunks ? (uint64_t)part_rst[i] : 0u;
    uint64_t all_k, all_r;
    const uint64_t ek = shdr::block_scan<WG>(k, wsum, all_k), er = shdr::block_scan<WG>(r, wsum, all_r);
    if (i < chunks) {
      part_kept[i] = (int64_t)(run_k + ek);
      part_rst[i] = (int64_t)(run_r + er);
    }
    run_k += all_k;
    run_r += all_r;
  }
}

__device__ __forceinline__ int64_t summed(const int64_t* __restrict__ pre, const int64_t* __restrict__ part, int64_t t) {
  return pre[t] + part[t / kScanChunk];
}

// what lies before a lane's 16 bytes in its image: kept bytes and restart markers (both before `end`)
struct Before {
  int64_t kept, rst;
};
__device__ __forceinline__ Before lane_prefix(const Lane& L, uint32_t in, const Image& im, int64_t tile, const int64_t* __restrict__ pre_kept,
                                              const int64_t* __restrict__ pre_rst, const int64_t* __restrict__ part_kept,
                                              const int64_t* __restrict__ part_rst, uint64_t* wsum) {
  const uint64_t c = (uint64_t)__builtin_popcount(in & ~L.dropped) | (uint64_t)__builtin_popcount(in & L.restart) << 32;
  const uint64_t excl = shdr::block_scan<WG>(c, wsum);
  Before b;
  b.kept = summed(pre_kept, part_kept, tile) - summed(pre_kept, part_kept, im.first_tile) + (int64_t)(excl & 0xFFFFFFFFu);
  b.rst = summed(pre_rst, part_rst, tile) - summed(pre_rst, part_rst, im.first_tile) + (int64_t)(excl >> 32);
  return b;
}

__global__ __launch_bounds__(WG) void bounds_kernel(const uint8_t* __restrict__ src, const Image* __restrict__ images, int n_images,
                                                    const int64_t* __restrict__ end, const int64_t* __restrict__ pre_kept,
                                                    const int64_t* __restrict__ pre_rst, const int64_t* __restrict__ part_kept,
                                                    const int64_t* __restrict__ part_rst, int64_t* __restrict__ bounds) {
  __shared__ uint64_t wsum[WG / 64];
  const int64_t tile = blockIdx.x;
  const int i = image_of(images, n_images, tile);
  const Image im = images[i];
  const Lane L = load_lane(src, im, tile);
  const uint32_t in = L.valid & before(L, end[i]);
  const Before at = lane_prefix(L, in, im, tile, pre_kept, pre_rst, part_kept, part_rst, wsum);
  uint32_t marks = in & L.restart;
  if (!marks) return;
  int64_t kept = at.kept, rst = at.rst;
  for (int k = 0; k < 16 && (marks >> k); ++k) {
    if ((marks >> k) & 1u) {
      const int64_t slot = bound_slot(im, rst);
      if (slot >= 0) bounds[slot] = kept;
      ++rst;
    }
    if (((in & ~L.dropped) >> k) & 1u) ++kept;
  }
}

__global__ __launch_bounds__(WG) void report_kernel(const uint8_t* __restrict__ src, const Image* __restrict__ images, int n_images,
                                                    const int64_t* __restrict__ end, const int32_t* __restrict__ fill,
                                                    const int64_t* __restrict__ pre_kept, const int64_t* __restrict__ pre_rst,
                                                    const int64_t* __restrict__ part_kept, const int64_t* __restrict__ part_rst,
                                                    Report* __restrict__ report) {
  const int i = blockIdx.x * WG + threadIdx.x;
  if (i >= n_images) return;
  const Image im = images[i];
  const int64_t t0 = im.first_tile, t1 = t0 + (im.length + kTile - 1) / kTile;
  const int64_t e = end[i];
  Report r;
  r.end = e == kNoEnd ? kNone : e;
  r.kept = summed(pre_kept, part_kept, t1) - summed(pre_kept, part_kept, t0);
  r.n_rst = (int32_t)(summed(pre_rst, part_rst, t1) - summed(pre_rst, part_rst, t0));
  r.fill = fill[i];
  r.end_marker = e == kNoEnd ? -1 : (int)src[im.offset + e + 1];  // a marker position has e + 1 < length
  r.reserved = 0;
  report[i] = r;
}

__global__ __launch_bounds__(WG) void compact_kernel(const uint8_t* __restrict__ src, const Image* __restrict__ images, int n_images,
                                                     const int64_t* __restrict__ end, const int64_t* __restrict__ pre_kept,
                                                     const int64_t* __restrict__ pre_rst, const int64_t* __restrict__ part_kept,
                                                     const int64_t* __restrict__ part_rst, const int64_t* __restrict__ bounds,
                                                     const int32_t* __restrict__ seg_dword, int seg_stride, uint8_t* __restrict__ arena,
                                                     int64_t arena_bytes) {
  __shared__ uint64_t wsum[WG / 64];
  const int64_t tile = blockIdx.x;
  const int i = image_of(images, n_images, tile);
  const Image im = images[i];
  const Lane L = load_lane(src, im, tile);
  const uint32_t in = L.valid & before(L, end[i]);
  const Before at = lane_prefix(L, in, im, tile, pre_kept, pre_rst, part_kept, part_rst, wsum);
  const uint32_t keep = in & ~L.dropped, marks = in & L.restart;
  if (!keep) return;
  int64_t kept = at.kept, rst = at.rst;
  int64_t seg = segment_of(im, rst);
  int64_t dword = seg_dword[seg * seg_stride], start = segment_start(im, seg, bounds);
  for (int k = 0; k < 16 && (keep >> k); ++k) {
    if ((keep >> k) & 1u) {
      const int64_t o = arena_index(dword, start, kept, arena_bytes);
      if (o >= 0) arena[o] = L.b[k];
      ++kept;
    }
    if ((marks >> k) & 1u) {                                      // (its two bytes are not kept: the next kept byte opens the segment)
      ++rst;
      seg = segment_of(im, rst);
      dword = seg_dword[seg * seg_stride];
      start = segment_start(im, seg, bounds);
    }
  }
}

int check(const char* what, const shdr_jpeg_scan_image* images, int n_images, int64_t src_bytes, int64_t n_bounds, int64_t n_segs,
          int64_t* n_tiles) {
  SHDR_REQUIRE(images, SHDR_E_NULL, "%s: null descriptors", what);
  int bad = -1;
  const int c = check_images(reinterpret_cast<const Image*>(images), n_images, src_bytes, n_bounds, n_segs, n_tiles, &bad);
  SHDR_REQUIRE(c == kOk, SHDR_E_SHAPE, "%s: image %d: %s", what, bad, check_text(c));
  return SHDR_OK;
}

}  // namespace

extern "C" int64_t shdr_jpeg_scan_workspace_bytes(int n_images, int64_t n_tiles) {
  if (n_images < 1 || n_images > kMaxImages || n_tiles < 0 || n_tiles > kMaxBytes / kTile + kMaxImages) {
    shdr::set_error("jpeg_scan_workspace_bytes: bad sizes (%d images, %lld tiles)", n_images, (long long)n_tiles);
    return -1;
  }
  return carve(nullptr, n_images, n_tiles).bytes;
}

extern "C" int shdr_jpeg_scan(const uint8_t* src, int64_t src_bytes, const shdr_jpeg_scan_image* images,
                              const shdr_jpeg_scan_image* images_dev, int n_images, shdr_jpeg_scan_report* report, int64_t* bounds,
                              int64_t n_bounds, void* workspace, void* stream, float* stage_ms) {
  const char* what = "jpeg_scan";
  SHDR_REQUIRE(images_dev && report && workspace && (src || !src_bytes) && (bounds || !n_bounds), SHDR_E_NULL, "%s: null pointer", what);
  SHDR_REQUIRE(n_bounds >= 0, SHDR_E_SHAPE, "%s: %lld boundary slots", what, (long long)n_bounds);
  int64_t n_tiles = 0;
  if (int rc = check(what, images, n_images, src_bytes, n_bounds, -1, &n_tiles)) return rc;
  SHDR_REQUIRE(shdr::aligned16(src) && shdr::aligned16(workspace) && (reinterpret_cast<uintptr_t>(images_dev) & 7u) == 0 &&
                   (reinterpret_cast<uintptr_t>(report) & 7u) == 0 && (reinterpret_cast<uintptr_t>(bounds) & 7u) == 0,
               SHDR_E_ALIGN, "%s: the source and the workspace must be 16-byte aligned, descriptors, report and boundaries 8-byte aligned", what);
  hipStream_t st = shdr::stream_of(stream);
  const Workspace w = carve(workspace, n_images, n_tiles);
  const Image* im = reinterpret_cast<const Image*>(images_dev);
  const int64_t chunks = (n_tiles + 1 + kScanChunk - 1) / kScanChunk;
  const unsigned img_grid = (unsigned)((n_images + WG - 1) / WG);
  {
    shdr::StageTimer<1> timer(stage_ms, st);                     // the whole call is the one stage
    if (n_bounds) SHDR_REQUIRE(hipMemsetAsync(bounds, 0xFF, 8 * (size_t)n_bounds, st) == hipSuccess, SHDR_E_LAUNCH, "%s: hipMemsetAsync failed", what);
    hipLaunchKernelGGL(init_kernel, dim3(img_grid), dim3(WG), 0, st, w.end, w.fill, n_images);
    if (n_tiles) {
      hipLaunchKernelGGL(end_kernel, dim3((unsigned)n_tiles), dim3(WG), 0, st, src, im, n_images, w.end);
      hipLaunchKernelGGL(count_kernel, dim3((unsigned)n_tiles), dim3(WG), 0, st, src, im, n_images, w.end, w.fill, w.tile_count);
    }
    hipLaunchKernelGGL(prefix_local_kernel, dim3((unsigned)chunks), dim3(WG), 0, st, w.tile_count, n_tiles, w.pre_kept, w.pre_rst, w.part_kept,
                       w.part_rst);
    hipLaunchKernelGGL(prefix_partials_kernel, dim3(1), dim3(WG), 0, st, w.part_kept, w.part_rst, chunks);
    if (n_tiles && n_bounds)
      hipLaunchKernelGGL(bounds_kernel, dim3((unsigned)n_tiles), dim3(WG), 0, st, src, im, n_images, w.end, w.pre_kept, w.pre_rst, w.part_kept,
                         w.part_rst, bounds);
    hipLaunchKernelGGL(report_kernel, dim3(img_grid), dim3(WG), 0, st, src, im, n_images, w.end, w.fill, w.pre_kept, w.pre_rst, w.part_kept,
                       w.part_rst, reinterpret_cast<Report*>(report));
    timer.mark();
  }
  return shdr::check_launch(what);
}

extern "C" int shdr_jpeg_compact(const uint8_t* src, int64_t src_bytes, const shdr_jpeg_scan_image* images,
                                 const shdr_jpeg_scan_image* images_dev, int n_images, const int64_t* bounds, int64_t n_bounds,
                                 const int32_t* seg_dword, int seg_stride, int64_t n_segs, uint8_t* arena, int64_t arena_bytes,
                                 const void* workspace, void* stream, float* stage_ms) {
  const char* what = "jpeg_compact";
  SHDR_REQUIRE(images_dev && seg_dword && workspace && (src || !src_bytes) && (bounds || !n_bounds) && (arena || !arena_bytes), SHDR_E_NULL,
               "%s: null pointer", what);
  SHDR_REQUIRE(n_bounds >= 0 && n_segs > 0 && seg_stride >= 1 && seg_stride <= 64 && arena_bytes >= 0 && arena_bytes < kMaxBytes, SHDR_E_SHAPE,
               "%s: bad sizes (%lld boundary slots, %lld segments of stride %d, an arena of %lld bytes)", what, (long long)n_bounds,
               (long long)n_segs, seg_stride, (long long)arena_bytes);
  int64_t n_tiles = 0;
  if (int rc = check(what, images, n_images, src_bytes, n_bounds, n_segs, &n_tiles)) return rc;
  SHDR_REQUIRE(shdr::aligned16(src) && shdr::aligned16(workspace) && (reinterpret_cast<uintptr_t>(images_dev) & 7u) == 0 &&
                   (reinterpret_cast<uintptr_t>(bounds) & 7u) == 0 && (reinterpret_cast<uintptr_t>(seg_dword) & 3u) == 0,
               SHDR_E_ALIGN, "%s: the source and the workspace must be 16-byte aligned, descriptors and boundaries 8-byte, seg_dword 4-byte", what);
  hipStream_t st = shdr::stream_of(stream);
  const Workspace w = carve(const_cast<void*>(workspace), n_images, n_tiles);
  {
    shdr::StageTimer<1> timer(stage_ms, st);                     // the whole call is the one stage
    if (arena_bytes)
      SHDR_REQUIRE(hipMemsetAsync(arena, 0xFF, (size_t)arena_bytes, st) == hipSuccess, SHDR_E_LAUNCH, "%s: hipMemsetAsync failed", what);
    if (n_tiles)
      hipLaunchKernelGGL(compact_kernel, dim3((unsigned)n_tiles), dim3(WG), 0, st, src, reinterpret_cast<const Image*>(images_dev), n_images, w.end,
                         w.pre_kept, w.pre_rst, w.part_kept, w.part_rst, bounds, seg_dword, seg_stride, arena, arena_bytes);
    timer.mark();
  }
  return shdr::check_launch(what);
}

extern "C" int shdr_jpeg_scan_host(const uint8_t* src, int64_t src_bytes, const shdr_jpeg_scan_image* images, int n_images,
                                   shdr_jpeg_scan_report* report, int64_t* bounds, int64_t n_bounds, const int32_t* seg_dword,
                                   int seg_stride, int64_t n_segs, uint8_t* arena, int64_t arena_bytes) {
  const char* what = "jpeg_scan_host";
  SHDR_REQUIRE(report && (src || !src_bytes) && (bounds || !n_bounds), SHDR_E_NULL, "%s: null pointer", what);
  SHDR_REQUIRE(n_bounds >= 0, SHDR_E_SHAPE, "%s: %lld boundary slots", what, (long long)n_bounds);
  if (seg_dword) {
    SHDR_REQUIRE(arena || !arena_bytes, SHDR_E_NULL, "%s: null arena", what);
    SHDR_REQUIRE(n_segs > 0 && seg_stride >= 1 && seg_stride <= 64 && arena_bytes >= 0 && arena_bytes < kMaxBytes, SHDR_E_SHAPE,
                 "%s: bad sizes (%lld segments of stride %d, an arena of %lld bytes)", what, (long long)n_segs, seg_stride, (long long)arena_bytes);
  }
  int64_t n_tiles = 0;
  if (int rc = check(what, images, n_images, src_bytes, n_bounds, seg_dword ? n_segs : -1, &n_tiles)) return rc;
  const Image* im = reinterpret_cast<const Image*>(images);
  Report* rep = reinterpret_cast<Report*>(report);
  for (int i = 0; i < n_images; ++i) scan_host(src, im[i], rep + i, bounds);
  if (seg_dword) {
    for (int64_t k = 0; k < arena_bytes; ++k) arena[k] = 0xFF;
    for (int i = 0; i < n_images; ++i) compact_host(src, im[i], rep[i].end, bounds, seg_dword, seg_stride, arena, arena_bytes);
  }
  return SHDR_OK;
}

// Gain maps on the device (ultrahdr.py; include/shdr.h "gain maps"; DESIGN.md "Gain maps").  Every rule is csrc/gainmap.h, which the
// host twins compile too: a kernel below only says which lane computes which pixel, cell or map byte.  A batch of images of different
// sizes goes through ONE descriptor table; a block finds its image by a binary search of the table's block0 column.
//   encode  (1) statistics: one block per part of an image (gainmap.h rule 3) -> one Stat per block; the image's first block also clears
//               its min / max slots.  With the scales given only the slots are cleared.
//           (2) cells: 1024 cells per block, lane t takes cells t, t + 256, ... (neighbouring lanes read neighbouring pixels).  Every
//               block first folds its image's parts (at most 256, from L2) into s, in the fixed tree.  g goes to the workspace as fp32;
//               the block's extremes meet in LDS and one lane issues an atomicMin and an atomicMax on ordered integer keys.
//           (3) quantise: the same blocks; 3072 map bytes each, and the image's first block writes the meta record.
//   apply   1024 pixels per block, lane t takes pixels t, t + 256, ...: 3 bytes in, the four map texels around it (L2), 12 bytes out.
// The sRGB table is copied to LDS by every block: its index differs from lane to lane.
// Compiled with -ffp-contract=off (gainmap.h).
#include "batch.h"
#include "gainmap.h"

namespace {

using namespace shdr_gainmap;

static_assert(kCellsPerBlock == SHDR_GAINMAP_CELLS_PER_BLOCK && kPixelsPerBlock == SHDR_GAINMAP_PIXELS_PER_BLOCK, "shdr.h names the block sizes");
static_assert(sizeof(shdr_gainmap_image) == 40 && sizeof(shdr_gainmap_meta) == 24 && sizeof(shdr_gainmap_apply_image) == 72 && sizeof(Stat) == 24,
              "the records of shdr.h as _ops.py mirrors them");

struct Workspace {
  float* g;                                    // [3 * cells of all images]
  Stat* parts;                                 // [statistics blocks]
  uint32_t* minmax;                            // [n][2] ordered keys
  int64_t bytes;
};

Workspace carve(void* base, int n, const EncodeTotals& t) {
  shdr::Carver c(base);
  Workspace w;
  w.g = c.take<float>(3 * t.cells);
  w.parts = c.take<Stat>(t.stat_blocks);
  w.minmax = c.take<uint32_t>(2 * (int64_t)n);
  w.bytes = c.bytes();
  return w;
}

// the last image whose first block is <= b
template <class D, class F>
__device__ __forceinline__ int image_of_block(const D* __restrict__ images, int n, int b, F block0) {
  int lo = 0, hi = n;
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if (block0(images[mid]) <= b) lo = mid; else hi = mid;
  }
  return lo;
}

__device__ __forceinline__ void load_table(float* tab) {
  tab[threadIdx.x] = kSrgbToLinear[threadIdx.x];
  __syncthreads();
}

// the halving tree of gainmap.h over the block's 256 lanes; every lane calls it and gets the total.  lanes: LDS [256], free again on return
__device__ __forceinline__ Stat stat_tree(Stat v, Stat* lanes) {
  const int t = threadIdx.x;
  lanes[t] = v;
  __syncthreads();
  for (int s = kLanes / 2; s > 0; s >>= 1) {
    if (t < s) stat_add(lanes[t], lanes[t + s]);
    __syncthreads();
  }
  const Stat all = lanes[0];
  __syncthreads();
  return all;
}

// the image's parts folded: lane t brings part t
__device__ __forceinline__ Stat image_stat(const shdr_gainmap_image& im, const Stat* __restrict__ parts, Stat* lanes) {
  const int64_t np = stat_parts((int64_t)im.height * im.width);
  Stat v = {0.0, 0.0, 0};
  if (threadIdx.x < np) v = parts[im.stat_block0 + threadIdx.x];
  return stat_tree(v, lanes);
}

__global__ __launch_bounds__(kLanes) void gainmap_stats_kernel(const uint8_t* __restrict__ sdr, const float* __restrict__ hdr,
                                                               const shdr_gainmap_image* __restrict__ images, int n, int reverse,
                                                               Stat* __restrict__ parts, uint32_t* __restrict__ minmax) {
  __shared__ float tab[256];
  __shared__ Stat lanes[kLanes];
  load_table(tab);
  const int b = blockIdx.x;
  const int i = image_of_block(images, n, b, [](const shdr_gainmap_image& im) { return im.stat_block0; });
  const shdr_gainmap_image im = images[i];
  const int part = b - im.stat_block0;
  const Stat all = stat_tree(stat_lane(sdr, hdr, im.pix_off, (int64_t)im.height * im.width, part, threadIdx.x, reverse, tab), lanes);
  if (threadIdx.x == 0) {
    parts[b] = all;
    if (part == 0) {
      minmax[2 * i] = kKeyMinInit;
      minmax[2 * i + 1] = kKeyMaxInit;
    }
  }
}

__global__ __launch_bounds__(kLanes) void gainmap_clear_kernel(int n, uint32_t* __restrict__ minmax) {
  const int i = blockIdx.x * kLanes + threadIdx.x;
  if (i < n) {
    minmax[2 * i] = kKeyMinInit;
    minmax[2 * i + 1] = kKeyMaxInit;
  }
}

__global__ __launch_bounds__(kLanes) void gainmap_cells_kernel(const uint8_t* __restrict__ sdr, const float* __restrict__ hdr,
                                                               const shdr_gainmap_image* __restrict__ images, int n,
                                                               const float* __restrict__ scales, float lo, float hi, int reverse,
                                                               const Stat* __restrict__ parts, float* __restrict__ g,
                                                               uint32_t* __restrict__ minmax) {
  __shared__ float tab[256];
  __shared__ Stat lanes[kLanes];
  __shared__ uint32_t wave_min[kLanes / 64], wave_max[kLanes / 64];
  load_table(tab);
  const int b = blockIdx.x, t = threadIdx.x;
  const int i = image_of_block(images, n, b, [](const shdr_gainmap_image& im) { return im.cell_block0; });
  const shdr_gainmap_image im = images[i];
  const float s = scales ? scales[i] : scale_of(image_stat(im, parts, lanes));
  const uint32_t mw = (uint32_t)map_side(im.width, im.factor), cells = (uint32_t)map_side(im.height, im.factor) * mw;
  const uint32_t first = (uint32_t)(b - im.cell_block0) * kCellsPerBlock;
  uint32_t kmin = kKeyMinInit, kmax = kKeyMaxInit;
  for (int k = 0; k < kCellsPerBlock / kLanes; ++k) {
    const uint32_t cell = first + (uint32_t)(k * kLanes + t);
    if (cell < cells) {
      const uint32_t cy = cell / mw, cx = cell - cy * mw;
      float o[3];
      cell_gain(sdr, hdr, im.pix_off, im.height, im.width, im.factor, (int)cy, (int)cx, s, lo, hi, reverse, tab, o);
      float* dst = g + 3 * (im.cell_off + cell);
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        dst[c] = o[c];
        const uint32_t key = ordered_key(o[c]);
        kmin = key < kmin ? key : kmin;
        kmax = key > kmax ? key : kmax;
      }
    }
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    const uint32_t a = __shfl_xor(kmin, off, 64), c = __shfl_xor(kmax, off, 64);
    kmin = a < kmin ? a : kmin;
    kmax = c > kmax ? c : kmax;
  }
  if ((t & 63) == 0) {
    wave_min[t >> 6] = kmin;
    wave_max[t >> 6] = kmax;
  }
  __syncthreads();
  if (t == 0) {
    for (int w = 1; w < kLanes / 64; ++w) {
      kmin = wave_min[w] < kmin ? wave_min[w] : kmin;
      kmax = wave_max[w] > kmax ? wave_max[w] : kmax;
    }
    atomicMin(minmax + 2 * i, kmin);
    atomicMax(minmax + 2 * i + 1, kmax);
  }
}

__global__ __launch_bounds__(kLanes) void gainmap_quantise_kernel(const shdr_gainmap_image* __restrict__ images, int n,
                                                                  const float* __restrict__ scales, const Stat* __restrict__ parts,
                                                                  const float* __restrict__ g, const uint32_t* __restrict__ minmax,
                                                                  uint8_t* __restrict__ maps, shdr_gainmap_meta* __restrict__ meta) {
  __shared__ Stat lanes[kLanes];
  const int b = blockIdx.x, t = threadIdx.x;
  const int i = image_of_block(images, n, b, [](const shdr_gainmap_image& im) { return im.cell_block0; });
  const shdr_gainmap_image im = images[i];
  const float mn = ordered_value(minmax[2 * i]), mx = widened_max(mn, ordered_value(minmax[2 * i + 1]));
  if (b == im.cell_block0) {                   // the whole block takes this branch or none of it
    Stat all = {0.0, 0.0, 0};
    float s;
    if (scales) {
      s = scales[i];
    } else {
      all = image_stat(im, parts, lanes);
      s = scale_of(all);
    }
    if (t == 0) {
      shdr_gainmap_meta m;
      m.gain_min = mn;
      m.gain_max = mx;
      m.scale = s;
      m.reserved = 0;
      m.count = all.n;
      meta[i] = m;
    }
  }
  const int64_t total = 3 * cells_of(im);
  const int64_t first = (int64_t)(b - im.cell_block0) * (3 * kCellsPerBlock);
  const float* src = g + 3 * im.cell_off;
  uint8_t* dst = maps + 3 * im.cell_off;
  for (int k = 0; k < 3 * kCellsPerBlock / kLanes; ++k) {
    const int64_t e = first + k * kLanes + t;
    if (e < total) dst[e] = quantise(src[e], mn, mx);
  }
}

__global__ __launch_bounds__(kLanes) void gainmap_apply_kernel(const uint8_t* __restrict__ sdr, const uint8_t* __restrict__ maps,
                                                               const shdr_gainmap_apply_image* __restrict__ images, int n,
                                                               float* __restrict__ out) {
  __shared__ float tab[256];
  load_table(tab);
  const int b = blockIdx.x, t = threadIdx.x;
  const int i = image_of_block(images, n, b, [](const shdr_gainmap_apply_image& im) { return im.block0; });
  const shdr_gainmap_apply_image im = images[i];
  const ApplyParams p = params_of(im);
  const uint32_t w = (uint32_t)im.width, pixels = (uint32_t)im.height * w;          // 65535^2 < 2^32
  const uint32_t first = (uint32_t)(b - im.block0) * kPixelsPerBlock;
  for (int k = 0; k < kPixelsPerBlock / kLanes; ++k) {
    const uint32_t e = first + (uint32_t)(k * kLanes + t);
    if (e < pixels) {
      const uint32_t y = e / w, x = e - y * w;
      const int64_t px = im.pix_off + e;
      float o[3];
      apply_pixel(sdr + 3 * px, maps + im.map_off, p, (int)y, (int)x, tab, o);
      out[3 * px] = o[0];
      out[3 * px + 1] = o[1];
      out[3 * px + 2] = o[2];
    }
  }
}

int refuse(const char* what, int rc, const char* why) { return shdr::fail(rc, "%s: %s", what, why); }

}  // namespace

extern "C" int shdr_gainmap_math_host(int op, const float* x, int64_t n, float* y) {
  SHDR_REQUIRE(y && (x || op == 2), SHDR_E_NULL, "gainmap_math_host: null pointer");
  SHDR_REQUIRE(op >= 0 && op <= 2 && n >= 0 && (op != 2 || n <= 256), SHDR_E_SHAPE, "gainmap_math_host: op %d with %lld values", op, (long long)n);
  for (int64_t i = 0; i < n; ++i) y[i] = op == 0 ? log2_poly(x[i]) : op == 1 ? exp2_poly(x[i]) : kSrgbToLinear[i];
  return SHDR_OK;
}

extern "C" int shdr_gainmap_encode_sizes(shdr_gainmap_image* images, int n_images, int64_t* map_bytes, int64_t* workspace_bytes) {
  char why[kWhy];
  EncodeTotals tot;
  if (int rc = fill_encode(images, n_images, &tot, why)) return refuse("gainmap_encode_sizes", rc, why);
  if (map_bytes) *map_bytes = 3 * tot.cells;
  if (workspace_bytes) *workspace_bytes = carve(nullptr, n_images, tot).bytes;
  return SHDR_OK;
}

extern "C" int shdr_gainmap_encode_host(const uint8_t* sdr, const float* hdr, int64_t arena_pixels, const shdr_gainmap_image* images,
                                        int n_images, const float* scales, float lo, float hi, int reverse_channels, uint8_t* maps,
                                        int64_t map_capacity, shdr_gainmap_meta* meta, int64_t meta_capacity) {
  char why[kWhy];
  if (int rc = encode_host(sdr, hdr, arena_pixels, images, n_images, scales, lo, hi, reverse_channels != 0, maps, map_capacity, meta,
                           meta_capacity, why))
    return refuse("gainmap_encode_host", rc, why);
  return SHDR_OK;
}

extern "C" int shdr_gainmap_encode(const uint8_t* sdr, const float* hdr, int64_t arena_pixels, const shdr_gainmap_image* images,
                                   const shdr_gainmap_image* images_dev, int n_images, const float* scales, const float* scales_dev, float lo,
                                   float hi, int reverse_channels, uint8_t* maps, int64_t map_capacity, shdr_gainmap_meta* meta,
                                   int64_t meta_capacity, void* workspace, void* stream, float* stage_ms) {
  const char* what = "gainmap_encode";
  SHDR_REQUIRE(sdr && hdr && images_dev && maps && meta && workspace, SHDR_E_NULL, "%s: null pointer", what);
  SHDR_REQUIRE((scales == nullptr) == (scales_dev == nullptr), SHDR_E_NULL, "%s: scales and scales_dev go together", what);
  char why[kWhy];
  EncodeTotals tot;
  if (int rc = check_encode(images, n_images, arena_pixels, scales, lo, hi, &tot, why)) return refuse(what, rc, why);
  SHDR_REQUIRE(map_capacity >= 3 * tot.cells, SHDR_E_SHAPE, "%s: the maps need %lld bytes, the destination has %lld", what,
               (long long)(3 * tot.cells), (long long)map_capacity);
  SHDR_REQUIRE(meta_capacity >= n_images, SHDR_E_SHAPE, "%s: %d meta records are needed, the destination has %lld", what, n_images,
               (long long)meta_capacity);
  SHDR_REQUIRE(shdr::aligned16(workspace), SHDR_E_ALIGN, "%s: workspace must be 16-byte aligned", what);
  SHDR_REQUIRE((reinterpret_cast<uintptr_t>(images_dev) & 7u) == 0 && (reinterpret_cast<uintptr_t>(meta) & 7u) == 0 &&
                   (reinterpret_cast<uintptr_t>(hdr) & 3u) == 0 && (reinterpret_cast<uintptr_t>(scales_dev) & 3u) == 0,
               SHDR_E_ALIGN, "%s: images_dev and meta must be 8-byte, hdr and scales_dev 4-byte aligned", what);
  const Workspace w = carve(workspace, n_images, tot);
  const int reverse = reverse_channels != 0;
  hipStream_t st = shdr::stream_of(stream);
  shdr::StageTimer<SHDR_GAINMAP_STAGES> timer(stage_ms, st);
  if (scales_dev)
    hipLaunchKernelGGL(gainmap_clear_kernel, dim3((unsigned)((n_images + kLanes - 1) / kLanes)), dim3(kLanes), 0, st, n_images, w.minmax);
  else
    hipLaunchKernelGGL(gainmap_stats_kernel, dim3((unsigned)tot.stat_blocks), dim3(kLanes), 0, st, sdr, hdr, images_dev, n_images, reverse, w.parts,
                       w.minmax);
  timer.mark();
  hipLaunchKernelGGL(gainmap_cells_kernel, dim3((unsigned)tot.cell_blocks), dim3(kLanes), 0, st, sdr, hdr, images_dev, n_images, scales_dev, lo, hi,
                     reverse, w.parts, w.g, w.minmax);
  timer.mark();
  hipLaunchKernelGGL(gainmap_quantise_kernel, dim3((unsigned)tot.cell_blocks), dim3(kLanes), 0, st, images_dev, n_images, scales_dev, w.parts, w.g,
                     w.minmax, maps, meta);
  timer.mark();
  return shdr::check_launch(what);
}

extern "C" int shdr_gainmap_apply_sizes(shdr_gainmap_apply_image* images, int n_images, int64_t* n_blocks) {
  char why[kWhy];
  if (int rc = check_apply(images, n_images, true, 0, 0, 0, n_blocks, why)) return refuse("gainmap_apply_sizes", rc, why);
  return SHDR_OK;
}

extern "C" int shdr_gainmap_apply_host(const uint8_t* sdr, int64_t arena_pixels, const uint8_t* maps, int64_t map_bytes,
                                       const shdr_gainmap_apply_image* images, int n_images, float* out, int64_t out_capacity) {
  char why[kWhy];
  if (int rc = apply_host(sdr, arena_pixels, maps, map_bytes, images, n_images, out, out_capacity, why)) return refuse("gainmap_apply_host", rc, why);
  return SHDR_OK;
}

extern "C" int shdr_gainmap_apply(const uint8_t* sdr, int64_t arena_pixels, const uint8_t* maps, int64_t map_bytes,
                                  const shdr_gainmap_apply_image* images, const shdr_gainmap_apply_image* images_dev, int n_images, float* out,
                                  int64_t out_capacity, void* stream) {
  const char* what = "gainmap_apply";
  SHDR_REQUIRE(sdr && maps && images_dev && out, SHDR_E_NULL, "%s: null pointer", what);
  char why[kWhy];
  int64_t blocks = 0;
  if (int rc = check_apply(const_cast<shdr_gainmap_apply_image*>(images), n_images, false, arena_pixels, map_bytes, out_capacity, &blocks, why))
    return refuse(what, rc, why);
  SHDR_REQUIRE((reinterpret_cast<uintptr_t>(images_dev) & 7u) == 0 && (reinterpret_cast<uintptr_t>(out) & 3u) == 0, SHDR_E_ALIGN,
               "%s: images_dev must be 8-byte and out 4-byte aligned", what);
  hipLaunchKernelGGL(gainmap_apply_kernel, dim3((unsigned)blocks), dim3(kLanes), 0, shdr::stream_of(stream), sdr, maps, images_dev, n_images, out);
  return shdr::check_launch(what);
}

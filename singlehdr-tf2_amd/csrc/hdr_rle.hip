// Radiance .hdr scanline encoder on the device: the adaptive RLE of shdr_rgbe_rle_encode (csrc/api.cpp), byte for byte, for a
// BATCH of RGBE images of different sizes.
//
// The host routine is a greedy loop, but what it writes for one component of one line depends on the bytes only through
//   stretches   maximal runs of equal bytes,
//   capped runs each stretch cut from its head into runs of 127 and a remainder,
//   tokens      a capped run of >= 4 is LONG: (128 + len, byte).  A GAP is a maximal sequence of short runs between long runs or
//               the line's ends; a gap that is one run of 2 or 3 is (128 + len, byte), any other gap is literal chunks of <= 128
//               counted from the gap's first byte, each with its length in front
// (tests/hdr_rle_ref.py states this in NumPy and tests/test_hdr_rle_ref.py holds it byte-equal to the host loop).  In that form
// every byte POSITION can decide what it contributes from two forward scans and six bytes of lookahead:
//   scan 1  the head of its stretch (and whether that stretch has >= 4 bytes, which the head sees in its next 3 bytes);
//   short   whether it lies in a short capped run: its stretch is short, or it lies in a remainder < 4 -- then the stretch ends
//           within 3 bytes, so the stretch length is known locally;
//   scan 2  the first byte of its gap (a short position whose left neighbour is not short);
//   a long run is coded by its LAST byte (2 bytes: the length is the offset in the run + 1), a one-run gap by its last byte (2 bytes),
//   a literal byte contributes itself, plus the count byte if it is the first of its chunk; the count is stored by the chunk's LAST
//   byte, which knows it.  An exclusive prefix sum of the contributions is where each position writes.
// All three are forward scans, so a wave streams along the line 64 positions at a time with three carried values.
//
// Passes (stream-ordered, no atomics, no host wait; the same input gives the same bytes):
//   0  rle_setup_kernel    first row and first pixel of every image                               (1 thread, N steps)
//   1  rle_rows_kernel<0>  coded size of every (row, component): one block per row, one wave per component
//   2  rle_scan_kernel     exclusive int64 scan of the row sizes over all rows of all images, and the per-image offsets (1 block)
//   3  rle_rows_kernel<1>  the same walk again, writing at the scanned offsets
// A block reads its row's pixels as 32-bit words straight from global memory: the four waves pick their byte out of the same 256 B,
// which the vector L1 serves after the first touch, so HBM sees the pixels once per pass.  LDS holds only the 80-position window
// (64 + 1 back + 6 ahead, rounded) of each wave, 1.25 KB per block, at any width.
#include "shdr_internal.h"
#include "batch.h"

namespace {

using shdr::wave_scan;

constexpr int kMaxRun = 127, kMinRun = 4, kMaxLiteral = 128;
constexpr int kWin = 80;                       // window of a wave: positions base - 1 .. base + 78
constexpr int kMaxWidth = 1 << 28;             // 4 * W fits an int32 with room

inline bool rle_width(int w) { return w >= 8 && w <= 32767; }

struct RleWorkspace {                          // carved out of the caller's workspace, every part 16-byte aligned
  int64_t* rowstart;                           // [N + 1] first row of image n among all rows
  int64_t* pixoff;                             // [N + 1] first pixel of image n
  int32_t* sizes;                              // [R][4]  coded bytes of (row, component); component 0 includes the 4-byte line header;
                                               //         a flat row is {4 W, 0, 0, 0}
  int64_t* rowoff;                             // [R + 1] first output byte of every row
  int64_t bytes;
};
inline RleWorkspace carve(void* ws, int64_t n, int64_t rows) {
  RleWorkspace w;
  shdr::Carver cut(ws);
  w.rowstart = cut.take<int64_t>(n + 1);
  w.pixoff = cut.take<int64_t>(n + 1);
  w.sizes = cut.take<int32_t>(4 * rows);
  w.rowoff = cut.take<int64_t>(rows + 1);
  w.bytes = cut.bytes();
  return w;
}

__global__ void rle_setup_kernel(const int32_t* __restrict__ shapes, int n, int64_t* __restrict__ rowstart, int64_t* __restrict__ pixoff) {
  if (blockIdx.x != 0 || threadIdx.x != 0) return;
  int64_t r = 0, p = 0;
  for (int i = 0; i < n; ++i) {
    rowstart[i] = r;
    pixoff[i] = p;
    r += shapes[2 * i];
    p += (int64_t)shapes[2 * i] * shapes[2 * i + 1];
  }
  rowstart[n] = r;
  pixoff[n] = p;
}

// One block per row of the batch, wave c codes component c.  WRITE = false: sizes[row][c]; WRITE = true: the bytes at rowoff[row].
template <bool WRITE>
__global__ __launch_bounds__(256) void rle_rows_kernel(const uint32_t* __restrict__ pixels, const int32_t* __restrict__ shapes, int n_img,
                                                       const int64_t* __restrict__ rowstart, const int64_t* __restrict__ pixoff,
                                                       int32_t* __restrict__ sizes, const int64_t* __restrict__ rowoff,
                                                       uint8_t* __restrict__ out, int64_t capacity) {
  __shared__ int win[4][kWin];
  const int64_t row = blockIdx.x;
  const int lo = (int)shdr::last_le(rowstart, n_img, row);       // the image of this row
  const int W = shapes[2 * lo + 1];
  const uint32_t* line = pixels + pixoff[lo] + (row - rowstart[lo]) * (int64_t)W;
  const int c = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const bool flat = W < 8 || W > 32767;

  int64_t row_at = 0;
  int csize = 0, cbase = 0;                                      // WRITE: size and offset in the row of this wave's component
  if constexpr (WRITE) {
    row_at = rowoff[row];
    if (rowoff[row + 1] > capacity) return;                      // never reached with the sizes the host checked
    const int4 sz = *reinterpret_cast<const int4*>(sizes + 4 * row);
    csize = c == 0 ? sz.x - 4 : c == 1 ? sz.y : c == 2 ? sz.z : sz.w;
    cbase = c == 0 ? 4 : c == 1 ? sz.x : c == 2 ? sz.x + sz.y : sz.x + sz.y + sz.z;
  }
  if (flat) {                                                    // the format stores such lines as they are
    if constexpr (WRITE) {
      const uint8_t* src = reinterpret_cast<const uint8_t*>(line);
      for (int64_t i = threadIdx.x; i < 4 * (int64_t)W; i += 256) out[row_at + i] = src[i];
    } else if (threadIdx.x == 0) {
      *reinterpret_cast<int4*>(sizes + 4 * row) = make_int4(4 * W, 0, 0, 0);
    }
    return;
  }
  uint8_t* dst = out + row_at + cbase;
  if constexpr (WRITE) {
    if (threadIdx.x == 0) {
      out[row_at] = 2; out[row_at + 1] = 2; out[row_at + 2] = (uint8_t)(W >> 8); out[row_at + 3] = (uint8_t)(W & 255);
    }
  }

  const int shift = 8 * c;
  int carry_key = -1, carry_gap = -1, carry_short = 0, carry_p = 0;
  for (int base = 0; base < W; base += 64) {
    // the window: win[i] = byte at base - 1 + i; -1 before the line, -2 after it (so both ends start a "stretch")
    for (int i = lane; i < kWin; i += 64) {
      const int pos = base - 1 + i;
      win[c][i] = pos < 0 ? -1 : pos >= W ? -2 : (int)((line[pos] >> shift) & 255u);
    }
    __syncthreads();
    int D[8];                                                    // D[k + 1] = byte at x + k, k = -1 .. 6
#pragma unroll
    for (int k = 0; k < 8; ++k) D[k] = win[c][lane + k];
    __syncthreads();
    const int x = base + lane;
    bool hd[7];                                                  // hd[k]: position x + k starts a stretch
#pragma unroll
    for (int k = 0; k < 7; ++k) hd[k] = D[k + 1] != D[k];
    // scan 1: (head of the stretch of x) * 2 + (that stretch has >= 4 bytes)
    const bool lh0 = D[1] >= 0 && D[1] == D[2] && D[1] == D[3] && D[1] == D[4];
    int key = hd[0] ? x * 2 + (lh0 ? 1 : 0) : -1;
    key = max(wave_scan(key, shdr::maximum()), carry_key);
    carry_key = __shfl(key, 63, 64);
    const int s0 = key >> 1;
    int sk = s0;
    bool longk = key & 1;
    bool sh[4];                                                  // sh[k]: position x + k lies in a short capped run
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      if (k > 0 && hd[k]) {
        sk = x + k;
        longk = D[k + 1] >= 0 && D[k + 1] == D[k + 2] && D[k + 1] == D[k + 3] && D[k + 1] == D[k + 4];
      }
      const int e = hd[k + 1] ? x + k + 1 : hd[k + 2] ? x + k + 2 : hd[k + 3] ? x + k + 3 : -1;      // the stretch's end, if near
      const int len = e - sk, rem = len % kMaxRun;
      const bool short_rest = e >= 0 && rem < kMinRun && x + k - sk >= len - rem;
      sh[k] = D[k + 1] >= 0 && (!longk || short_rest);
    }
    // scan 2: the first byte of the gap of x
    const unsigned long long shmask = __ballot(sh[0]);
    const bool prev_short = lane == 0 ? carry_short != 0 : ((shmask >> (lane - 1)) & 1ull) != 0;
    carry_short = (int)(shmask >> 63);
    int g = sh[0] && !prev_short ? x : -1;
    g = max(wave_scan(g, shdr::maximum()), carry_gap);
    carry_gap = __shfl(g, 63, 64);
    const int rel = x - g;
    // a gap that is one run of 2 or 3 bytes
    const int yl = !sh[1] ? 0 : !sh[2] ? 1 : !sh[3] ? 2 : 9;
    const int glen = rel + yl + 1;
    const bool tok = sh[0] && glen >= 2 && glen <= 3 && s0 <= g && (yl < 1 || !hd[1]) && (yl < 2 || !hd[2]);
    const bool gap_last = !sh[1];
    const int o = (x - s0) % kMaxRun;
    const bool run_last = o == kMaxRun - 1 || hd[1];
    const int chunk = rel & (kMaxLiteral - 1);
    int contrib;
    if (D[1] < 0) contrib = 0;                                   // past the end of the line
    else if (!sh[0]) contrib = run_last ? 2 : 0;
    else if (tok) contrib = gap_last ? 2 : 0;
    else contrib = 1 + (chunk == 0 ? 1 : 0);
    const int incl = wave_scan(contrib);
    const int p = carry_p + incl - contrib;
    carry_p += __shfl(incl, 63, 64);
    if constexpr (WRITE) {
      if (contrib != 0 && p + contrib <= csize) {                // (the bound holds whenever pass 1 saw the same pixels)
        if (!sh[0]) {
          dst[p] = (uint8_t)(128 + o + 1);
          dst[p + 1] = (uint8_t)D[1];
        } else if (tok) {
          dst[p] = (uint8_t)(128 + glen);
          dst[p + 1] = (uint8_t)D[1];
        } else {
          dst[p + (chunk == 0 ? 1 : 0)] = (uint8_t)D[1];
          if (gap_last || chunk == kMaxLiteral - 1) dst[p - chunk - (chunk != 0 ? 1 : 0)] = (uint8_t)(chunk + 1);
        }
      }
    }
  }
  if constexpr (!WRITE) {
    if (lane == 0) sizes[4 * row + c] = carry_p + (c == 0 ? 4 : 0);
  }
}

// rowoff[r] = sum of the sizes of the rows before r (int64), rowoff[R] = the total; offsets[n] = rowoff[rowstart[n]].  One block:
// R is the number of scanlines of the batch, a few thousand.
__global__ __launch_bounds__(1024) void rle_scan_kernel(const int32_t* __restrict__ sizes, int64_t rows, int64_t* __restrict__ rowoff,
                                                        const int64_t* __restrict__ rowstart, int n_img, int64_t* __restrict__ offsets) {
  const int64_t all = shdr::scan_array<1024, 1>(
      rows,
      [&](int64_t r) {
        const int4 sz = *reinterpret_cast<const int4*>(sizes + 4 * r);
        return (int64_t)sz.x + sz.y + sz.z + sz.w;
      },
      [&](int64_t r, int64_t before) { rowoff[r] = before; });
  if (threadIdx.x == 0) rowoff[rows] = all;
  __syncthreads();                                              // the block's own global writes are visible to it after the barrier
  for (int n = threadIdx.x; n <= n_img; n += 1024) offsets[n] = rowoff[rowstart[n]];
}

// shapes as the ABI takes them: validated on the host, totals returned
int check_shapes(const char* what, const int32_t* shapes, int n, int64_t* rows, int64_t* bound) {
  SHDR_REQUIRE(shapes, SHDR_E_NULL, "%s: null shape table", what);
  SHDR_REQUIRE(n > 0, SHDR_E_SHAPE, "%s: the number of images must be positive, got %d", what, n);
  int64_t r = 0, b = 0;
  for (int i = 0; i < n; ++i) {
    const int64_t h = shapes[2 * i], w = shapes[2 * i + 1];
    SHDR_REQUIRE(h > 0 && w > 0, SHDR_E_SHAPE, "%s: image %d is %lld x %lld (H x W): sizes must be positive", what, i, (long long)h, (long long)w);
    SHDR_REQUIRE(w <= kMaxWidth, SHDR_E_SHAPE, "%s: image %d is %lld wide, the limit is %d", what, i, (long long)w, kMaxWidth);
    r += h;
    b += h * (rle_width((int)w) ? 4 + 4 * (w + w / 127 + 2) : 4 * w);
  }
  SHDR_REQUIRE(r < ((int64_t)1 << 31), SHDR_E_SHAPE, "%s: %lld scanlines in one call, the limit is 2^31 - 1", what, (long long)r);
  *rows = r;
  *bound = b;
  return SHDR_OK;
}

}  // namespace

extern "C" int shdr_rgbe_rle_encode_batch_sizes(const int32_t* shapes, int n_images, int64_t* out_bytes, int64_t* workspace_bytes) {
  int64_t rows = 0, bound = 0;
  if (int rc = check_shapes("rgbe_rle_encode_batch_sizes", shapes, n_images, &rows, &bound)) return rc;
  if (out_bytes) *out_bytes = bound;
  if (workspace_bytes) *workspace_bytes = carve(nullptr, n_images, rows).bytes;
  return SHDR_OK;
}

namespace {
int encode_batch(const uint8_t* rgbe, const int32_t* shapes, const int32_t* shapes_dev, int n_images, uint8_t* out, int64_t out_capacity,
                 int64_t* offsets, void* workspace, void* stream, float* stage_ms) {
  const char* what = "rgbe_rle_encode_batch";
  SHDR_REQUIRE(rgbe && shapes_dev && out && offsets && workspace, SHDR_E_NULL, "%s: null pointer", what);
  int64_t rows = 0, bound = 0;
  if (int rc = check_shapes(what, shapes, n_images, &rows, &bound)) return rc;
  SHDR_REQUIRE((reinterpret_cast<uintptr_t>(rgbe) & 3u) == 0, SHDR_E_ALIGN, "%s: rgbe must be 4-byte aligned", what);
  SHDR_REQUIRE((reinterpret_cast<uintptr_t>(shapes_dev) & 3u) == 0, SHDR_E_ALIGN, "%s: shapes_dev must be 4-byte aligned", what);
  SHDR_REQUIRE((reinterpret_cast<uintptr_t>(offsets) & 7u) == 0, SHDR_E_ALIGN, "%s: offsets must be 8-byte aligned", what);
  SHDR_REQUIRE(shdr::aligned16(workspace), SHDR_E_ALIGN, "%s: workspace must be 16-byte aligned", what);
  SHDR_REQUIRE(out_capacity >= bound, SHDR_E_SHAPE, "%s: output buffer too small (%lld < %lld)", what, (long long)out_capacity,
               (long long)bound);
  const RleWorkspace w = carve(workspace, n_images, rows);
  hipStream_t st = shdr::stream_of(stream);
  const uint32_t* px = reinterpret_cast<const uint32_t*>(rgbe);
  shdr::StageTimer<SHDR_RLE_STAGES> timer(stage_ms, st);
  hipLaunchKernelGGL(rle_setup_kernel, dim3(1), dim3(64), 0, st, shapes_dev, n_images, w.rowstart, w.pixoff);
  timer.mark();
  hipLaunchKernelGGL(rle_rows_kernel<false>, dim3((unsigned)rows), dim3(256), 0, st, px, shapes_dev, n_images, w.rowstart, w.pixoff,
                     w.sizes, w.rowoff, out, out_capacity);
  timer.mark();
  hipLaunchKernelGGL(rle_scan_kernel, dim3(1), dim3(1024), 0, st, w.sizes, rows, w.rowoff, w.rowstart, n_images, offsets);
  timer.mark();
  hipLaunchKernelGGL(rle_rows_kernel<true>, dim3((unsigned)rows), dim3(256), 0, st, px, shapes_dev, n_images, w.rowstart, w.pixoff,
                     w.sizes, w.rowoff, out, out_capacity);
  timer.mark();
  return shdr::check_launch(what);
}
}  // namespace

extern "C" int shdr_rgbe_rle_encode_batch(const uint8_t* rgbe, const int32_t* shapes, const int32_t* shapes_dev, int n_images,
                                          uint8_t* out, int64_t out_capacity, int64_t* offsets, void* workspace, void* stream) {
  return encode_batch(rgbe, shapes, shapes_dev, n_images, out, out_capacity, offsets, workspace, stream, nullptr);
}

extern "C" int shdr_rgbe_rle_encode_batch_timed(const uint8_t* rgbe, const int32_t* shapes, const int32_t* shapes_dev, int n_images,
                                                uint8_t* out, int64_t out_capacity, int64_t* offsets, void* workspace, void* stream,
                                                float* stage_ms) {
  SHDR_REQUIRE(stage_ms, SHDR_E_NULL, "rgbe_rle_encode_batch_timed: null stage_ms");
  return encode_batch(rgbe, shapes, shapes_dev, n_images, out, out_capacity, offsets, workspace, stream, stage_ms);
}

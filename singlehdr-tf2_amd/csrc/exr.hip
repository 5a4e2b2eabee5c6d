// Device side of the OpenEXR reader (exr.py; DESIGN.md "OpenEXR training files").  The host checks the file, inflates ZIP /
// ZIPS chunks and decodes RLE ones (shdr_exr_rle_decode); what reaches the device is one byte buffer of chunks in increasing-y
// order, chunk c at [chunk_off[c], chunk_off[c + 1]).  Two kernels finish the decode:
//
// (a) exr_unpredict_kernel, one workgroup per chunk.  A coded chunk (RLE, ZIPS, ZIP and smaller than its scanlines) holds the
//     scanline bytes interleaved (even bytes first, then odd) and delta-coded; undoing the predictor is
//         t[0] = d[0],  t[i] = (t[i-1] + d[i] - 128) & 0xFF
//     i.e. an inclusive prefix sum mod 256 of e[0] = d[0], e[i] = d[i] + 128, and the scanline bytes are
//         out[2k] = t[k],  out[2k+1] = t[h + k],  h = (n + 1) / 2.
//     Both halves are scanned in the same pass: a first sweep sums e over [0, h) (t[h-1], the second half's start value), then
//     pair k is produced from the two running sums.  Steps of 256 threads x 8 pairs carry their totals to the next step; wave
//     sums are shuffle scans, the four waves meet in LDS.  uint32 sums wrap mod 2^32, a multiple of 256, so nothing is masked
//     until a byte is stored.  No atomics: the result does not depend on scheduling.  Other chunks are copied.
// (b) exr_load_resize_kernel, one thread per output pixel: the four taps of cv2's bilinear map (linear_resize.h, the
//     arithmetic of hdr_load_resize_kernel) are read straight from the planar scanlines, HALF or FLOAT, in the channel order
//     of the table it is given; optionally clipped at 0 first (np.clip(hdr, 0, None): NaN and +inf pass).  Same-size loads are
//     copies, as cv2.resize makes them: a zero-weight tap would turn a neighbouring inf into NaN and -0 into +0.
// Compiled with -ffp-contract=off.
#include "shdr_internal.h"
#include "batch.h"
#include "linear_resize.h"

namespace {

using shdr::linear::bilinear3;

constexpr int kThreads = 256;
constexpr int kPairs = 8;                        // pairs per thread and step: a step writes 4 KiB of a chunk

// (block_scan of batch.h would add the lanes' prefixes, which nobody reads here: only the wave-level part is shared)
__device__ __forceinline__ uint32_t block_sum(uint32_t v, uint32_t* lds) {
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  v = shdr::wave_scan(v);
  if (lane == 63) lds[wid] = v;
  __syncthreads();
  const uint32_t s = lds[0] + lds[1] + lds[2] + lds[3];
  __syncthreads();
  return s;
}

__device__ __forceinline__ uint32_t pred_e(const uint8_t* d, int64_t i) { return i == 0 ? d[0] : (uint32_t)d[i] + 128u; }

__global__ __launch_bounds__(kThreads) void exr_unpredict_kernel(const uint8_t* __restrict__ src, uint8_t* __restrict__ dst,
                                                                 int64_t size, const int64_t* __restrict__ chunk_off,
                                                                 const uint8_t* __restrict__ coded) {
  __shared__ uint32_t lds[2][4];
  const int c = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const shdr::Span span = shdr::clamped_span(chunk_off, c, size);         // the host checked the table; clamp regardless
  const int64_t n = span.n;
  const uint8_t* d = src + span.lo;
  uint8_t* o = dst + span.lo;
  if (!coded[c]) {
    for (int64_t i = tid; i < n; i += kThreads) o[i] = d[i];
    return;
  }
  const int64_t h = (n + 1) >> 1;
  uint32_t acc = 0;
  for (int64_t i = tid; i < h; i += kThreads) acc += pred_e(d, i);
  uint32_t carry_a = 0, carry_b = block_sum(acc, lds[0]);                 // carry_b = t[h - 1]
  for (int64_t k0 = 0; k0 < h; k0 += (int64_t)kThreads * kPairs) {
    const int64_t kb = k0 + (int64_t)tid * kPairs;
    uint32_t a[kPairs], b[kPairs];
    uint32_t sa = 0, sb = 0;
#pragma unroll
    for (int j = 0; j < kPairs; ++j) {
      const int64_t k = kb + j;
      sa += k < h ? pred_e(d, k) : 0u;
      sb += h + k < n ? pred_e(d, h + k) : 0u;
      a[j] = sa;
      b[j] = sb;
    }
    const uint32_t ia = shdr::wave_scan(sa), ib = shdr::wave_scan(sb);      // (two scans under ONE pair of barriers: no block_scan)
    if (lane == 63) {
      lds[0][wid] = ia;
      lds[1][wid] = ib;
    }
    __syncthreads();
    uint32_t pa = carry_a + ia - sa, pb = carry_b + ib - sb;                // exclusive prefix of this thread
    for (int w = 0; w < 4; ++w) {
      if (w < wid) {
        pa += lds[0][w];
        pb += lds[1][w];
      }
      carry_a += lds[0][w];
      carry_b += lds[1][w];
    }
    __syncthreads();
#pragma unroll
    for (int j = 0; j < kPairs; ++j) {
      const int64_t k = kb + j;
      if (k < h) o[2 * k] = (uint8_t)(pa + a[j]);
      if (h + k < n) o[2 * k + 1] = (uint8_t)(pb + b[j]);
    }
  }
}

// channel table of the load: byte offset of each output channel's run inside a scanline and its sample type
struct ExrChannels {
  int64_t off[3];
  int type[3];
};

// OpenEXR HALF (IEEE binary16) -> float, bit-exact: +-0, subnormals, +-inf and NaN payloads (no quieting) are kept
__device__ __forceinline__ float half_bits_to_float(uint32_t hb) {
  const uint32_t sign = (hb & 0x8000u) << 16, e = (hb >> 10) & 0x1fu, m = hb & 0x3ffu;
  if (e == 0x1f) return __uint_as_float(sign | 0x7f800000u | (m << 13));
  if (e == 0) return __uint_as_float(sign | __float_as_uint((float)m * 5.9604644775390625e-8f));     // m * 2^-24, exact
  return __uint_as_float(sign | ((e + 112u) << 23) | (m << 13));
}

__device__ __forceinline__ float exr_sample(const uint8_t* p, int type) {
  if (type == SHDR_EXR_FLOAT)
    return __uint_as_float((uint32_t)p[0] | (uint32_t)p[1] << 8 | (uint32_t)p[2] << 16 | (uint32_t)p[3] << 24);
  return half_bits_to_float((uint32_t)p[0] | (uint32_t)p[1] << 8);
}

__global__ __launch_bounds__(256) void exr_load_resize_kernel(const uint8_t* __restrict__ planes, int64_t size,
                                                              const int64_t* __restrict__ chunk_off, int lines, int64_t row_bytes,
                                                              ExrChannels ch, int H0, int W0, int H, int W, double sy, double sx,
                                                              int clip, float* __restrict__ y) {
  auto fetch = [&](int r, int x) {
    const int ck = r / lines;
    const int64_t row = chunk_off[ck] + (int64_t)(r - ck * lines) * row_bytes;
    float v[3];
#pragma unroll
    for (int i = 0; i < 3; ++i) {
      const int sz = ch.type[i] == SHDR_EXR_FLOAT ? 4 : 2;
      const int64_t pos = min(max(row + ch.off[i] + (int64_t)x * sz, (int64_t)0), size - sz);   // in bounds whatever the table
      v[i] = exr_sample(planes + pos, ch.type[i]);
      if (clip && v[i] < 0.0f) v[i] = 0.0f;
    }
    return make_float3(v[0], v[1], v[2]);
  };
  const bool same = H == H0 && W == W0;
  const long total = (long)H * W;
  for (long p = (long)blockIdx.x * 256 + threadIdx.x; p < total; p += (long)gridDim.x * 256) {
    const int oy = (int)(p / W), ox = (int)(p - (long)oy * W);
    const float3 v = same ? fetch(oy, ox) : bilinear3(oy, ox, H0, W0, sy, sx, fetch);
    y[3 * p] = v.x;
    y[3 * p + 1] = v.y;
    y[3 * p + 2] = v.z;
  }
}

}  // namespace

extern "C" int shdr_exr_unpredict_u8(const uint8_t* payload, uint8_t* out, int64_t size, const int64_t* chunk_off,
                                     const uint8_t* coded, int n_chunks, void* stream) {
  SHDR_REQUIRE(payload && out && chunk_off && coded, SHDR_E_NULL, "exr_unpredict: null pointer");
  SHDR_REQUIRE(size > 0 && n_chunks > 0 && n_chunks < (1 << 30), SHDR_E_SHAPE, "exr_unpredict: size %lld, %d chunks",
               (long long)size, n_chunks);
  hipLaunchKernelGGL(exr_unpredict_kernel, dim3(n_chunks), dim3(kThreads), 0, shdr::stream_of(stream), payload, out, size, chunk_off, coded);
  return shdr::check_launch("exr_unpredict");
}

extern "C" int shdr_exr_load_resize_f32(const uint8_t* planes, int64_t size, const int64_t* chunk_off, int n_chunks, int lines,
                                        int64_t row_bytes, const int64_t* chan_off, const int32_t* chan_type, int H0, int W0,
                                        float* y, int H, int W, int clip, void* stream) {
  SHDR_REQUIRE(planes && chunk_off && chan_off && chan_type && y, SHDR_E_NULL, "exr_load_resize: null pointer");
  SHDR_REQUIRE(H0 > 0 && W0 > 0 && H > 0 && W > 0 && lines > 0, SHDR_E_SHAPE, "exr_load_resize: non-positive dimension");
  SHDR_REQUIRE(n_chunks == (H0 + lines - 1) / lines, SHDR_E_SHAPE, "exr_load_resize: %d chunks of %d lines for %d rows", n_chunks,
               lines, H0);
  SHDR_REQUIRE(row_bytes > 0 && size >= row_bytes, SHDR_E_SHAPE, "exr_load_resize: row_bytes %lld, size %lld",
               (long long)row_bytes, (long long)size);
  ExrChannels ch;
  for (int i = 0; i < 3; ++i) {
    SHDR_REQUIRE(chan_type[i] == SHDR_EXR_HALF || chan_type[i] == SHDR_EXR_FLOAT, SHDR_E_SHAPE,
                 "exr_load_resize: channel %d has type %d (HALF or FLOAT only)", i, chan_type[i]);
    const int64_t sz = chan_type[i] == SHDR_EXR_FLOAT ? 4 : 2;
    SHDR_REQUIRE(chan_off[i] >= 0 && chan_off[i] + sz * W0 <= row_bytes, SHDR_E_SHAPE,
                 "exr_load_resize: channel %d at byte %lld does not fit a %lld-byte scanline", i, (long long)chan_off[i],
                 (long long)row_bytes);
    ch.off[i] = chan_off[i];
    ch.type[i] = chan_type[i];
  }
  const long total = (long)H * W;
  hipLaunchKernelGGL(exr_load_resize_kernel, dim3(shdr::stream_grid(total)), dim3(256), 0, shdr::stream_of(stream), planes, size, chunk_off,
                     lines, row_bytes, ch, H0, W0, H, W, 1.0 / ((double)H / H0), 1.0 / ((double)W / W0), clip, y);
  return shdr::check_launch("exr_load_resize");
}

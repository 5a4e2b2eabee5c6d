// Huffman-only zlib streams for a BATCH of byte chunks on the device: byte for byte what shdr_deflate_huffman_host writes
// (deflate_huffman.h holds what both share: the code lengths, the canonical codes and the fixed-length block header).
//
// Passes (stream-ordered, no global atomics, no host wait; the same input gives the same bytes):
//   1  deflate_stats_kernel  one block per chunk: byte histogram in LDS (one per wave), Adler-32 as two block reductions, then ONE lane
//                            runs build_lengths on the 257 counts; stores the lengths, the block's size in bits, the checksum and the
//                            stored size of the chunk: its stream if that is strictly smaller than the chunk, else the chunk itself
//   2  deflate_scan_kernel   exclusive int64 scan of the stored sizes (+ `pad` bytes in front of each) -> out_offsets   (1 block;
//                            deflate_batch.h, shared with deflate_lz.hip)
//   3  deflate_write_kernel  one block per chunk: the header, then tiles of kTile symbols: a block prefix sum of the code lengths
//                            gives every symbol its bit, the codes are OR-ed into LDS words and the whole bytes of the tile are
//                            stored; the partial byte and the bit position carry to the next tile; then the tail and the Adler-32.
//                            A chunk that is not coded is copied from `raw` (the caller's uncoded form of the chunk).
// Adler-32: s1 = 1 + sum b[i], s2 = n + sum (n - i) b[i], both mod 65521.  A thread adds (n - i) mod 65521 times b[i] < 2^24 for at
// most 2^22 bytes (a 2^30-byte chunk over 256 threads) into 64 bits, so nothing overflows at any size.
#include "shdr_internal.h"
#include "deflate_huffman.h"
#include "deflate_batch.h"

namespace {

using namespace shdr_deflate;
using namespace shdr_deflate_batch;

constexpr int kThreads = 256;
constexpr int kPerThread = 4;
constexpr int kTile = kThreads * kPerThread;                   // symbols per tile of the writer (shdr.h: SHDR_DEFLATE_TILE)
constexpr int kTileWords = (7 + kTile * kMaxBits) / 32 + 3;      // carried bits + the tile's bits, and the word a shifted code spills into
constexpr int kLenStride = 272;                                  // bytes per chunk of the stored code lengths
static_assert(kTile == SHDR_DEFLATE_TILE, "shdr.h names the tile size");

struct Workspace {                                               // carved out of the caller's workspace, every part 16-byte aligned
  uint8_t* lens;                                                 // [C][kLenStride]
  int64_t* bits;                                                 // [C] bits of the block incl. the two zlib bytes in front
  int64_t* sizes;                                                // [C] pad + stored bytes
  uint32_t* adler;                                               // [C]
  int64_t bytes;
};
inline Workspace carve(void* ws, int64_t c) {
  Workspace w;
  char* p = static_cast<char*>(ws);
  int64_t o = 0;
  w.lens = reinterpret_cast<uint8_t*>(p + o);   o += (int64_t)kLenStride * c;
  w.bits = reinterpret_cast<int64_t*>(p + o);   o += align16(8 * c);
  w.sizes = reinterpret_cast<int64_t*>(p + o);  o += align16(8 * c);
  w.adler = reinterpret_cast<uint32_t*>(p + o); o += align16(4 * c);
  w.bytes = o;
  return w;
}

__device__ __forceinline__ uint64_t block_sum_u64(uint64_t v, uint64_t* part) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = v;
  __syncthreads();
  return part[0] + part[1] + part[2] + part[3];
}

__global__ __launch_bounds__(kThreads) void deflate_stats_kernel(const uint8_t* __restrict__ data, const int64_t* __restrict__ offsets,
                                                                 int64_t total, int pad, uint8_t* __restrict__ lens,
                                                                 int64_t* __restrict__ bits_out, int64_t* __restrict__ sizes,
                                                                 uint32_t* __restrict__ adler, uint8_t* __restrict__ coded) {
  __shared__ uint32_t hist[4][256];
  __shared__ uint32_t freq[kSyms];
  __shared__ uint8_t len[kLenStride];
  __shared__ HuffWork work;
  __shared__ uint64_t part[4];
  const int64_t c = blockIdx.x;
  int64_t lo, n;
  chunk_range(offsets, c, total, lo, n);
  const int tid = threadIdx.x, wave = tid >> 6;
  for (int i = tid; i < 4 * 256; i += kThreads) (&hist[0][0])[i] = 0;
  __syncthreads();
  const uint8_t* src = data + lo;
  uint64_t s1 = 0, s2 = 0;
  for (int64_t i = tid; i < n; i += kThreads) {
    const uint32_t b = src[i];
    atomicAdd(&hist[wave][b], 1u);                               // LDS
    s1 += b;
    s2 += (uint64_t)((n - i) % kAdlerMod) * b;
  }
  s1 = block_sum_u64(s1 % kAdlerMod, part);
  s2 = block_sum_u64(s2 % kAdlerMod, part);
  for (int s = tid; s < kSyms; s += kThreads) freq[s] = s < 256 ? hist[0][s] + hist[1][s] + hist[2][s] + hist[3][s] : 1u;
  __syncthreads();
  if (tid == 0) {
    build_lengths(freq, len, work);
    const int64_t bits = stream_bits(freq, len), stream = stream_bytes(bits);
    const bool use = n > 0 && stream < n;
    bits_out[c] = bits;
    sizes[c] = pad + (use ? stream : n);
    coded[c] = use ? 1 : 0;
    adler[c] = (uint32_t)((((uint64_t)(n % kAdlerMod) + s2) % kAdlerMod) << 16) | (uint32_t)((1 + s1) % kAdlerMod);
  }
  __syncthreads();
  for (int s = tid; s < kLenStride; s += kThreads) lens[c * kLenStride + s] = s < kSyms ? len[s] : 0;
}

__global__ __launch_bounds__(kThreads) void deflate_write_kernel(const uint8_t* __restrict__ data, const uint8_t* __restrict__ raw,
                                                                 const int64_t* __restrict__ offsets, int64_t total, int pad,
                                                                 const uint8_t* __restrict__ lens, const int64_t* __restrict__ bits_in,
                                                                 const uint32_t* __restrict__ adler, const uint8_t* __restrict__ coded,
                                                                 const int64_t* __restrict__ out_offsets, uint8_t* __restrict__ out,
                                                                 int64_t capacity) {
  __shared__ uint8_t len[kLenStride];
  __shared__ uint16_t code[kSyms + 1];
  __shared__ uint8_t hdr[kHeaderBytes + 3];
  __shared__ uint32_t words[kTileWords];
  __shared__ int wave_bits[4];
  const int64_t c = blockIdx.x;
  int64_t lo, n;
  chunk_range(offsets, c, total, lo, n);
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int64_t at = out_offsets[c] + pad, end = out_offsets[c + 1];
  if (at < 0 || end > capacity || end < at) return;              // never with the sizes the host checked
  uint8_t* dst = out + at;
  const int64_t room = end - at;
  if (!coded[c]) {
    const uint8_t* src = raw + lo;
    for (int64_t i = tid; i < n && i < room; i += kThreads) dst[i] = src[i];
    return;
  }
  const int64_t bits = bits_in[c];
  if (stream_bytes(bits) != room) return;                        // (pass 1 stored both)
  for (int s = tid; s < kLenStride; s += kThreads) len[s] = lens[c * kLenStride + s];
  __syncthreads();
  if (tid == 0) {
    build_codes(len, code);
    write_header(len, hdr);
  }
  __syncthreads();
  for (int i = tid; i < kHeaderBytes - 1; i += kThreads) dst[i] = hdr[i];
  const uint8_t* src = data + lo;
  int64_t P = kSymbolsAtBit;                                     // the stream bit of the tile's first symbol; the same in every thread
  uint32_t carry = hdr[kHeaderBytes - 1];                        // the bits of byte P / 8 that are already decided
  for (int64_t base = 0; base <= n; base += kTile) {             // n + 1 symbols: the chunk's bytes, then end-of-block
    for (int i = tid; i < kTileWords; i += kThreads) words[i] = i == 0 ? carry : 0u;
    uint64_t v = 0;
    int nb = 0;
#pragma unroll
    for (int k = 0; k < kPerThread; ++k) {
      const int64_t i = base + (int64_t)tid * kPerThread + k;
      if (i <= n) {
        const int s = i < n ? (int)src[i] : 256;
        v |= (uint64_t)code[s] << nb;
        nb += len[s];
      }
    }
    int incl = nb;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
      const int t = __shfl_up(incl, off, 64);
      if (lane >= off) incl += t;
    }
    if (lane == 63) wave_bits[wave] = incl;
    __syncthreads();                                             // words are cleared, wave_bits are written
    int before = 0;
    for (int w = 0; w < wave; ++w) before += wave_bits[w];
    const int tile_bits = wave_bits[0] + wave_bits[1] + wave_bits[2] + wave_bits[3];
    if (nb) {
      const int rel = (int)(P & 7) + before + incl - nb;         // bit in `words`, whose bit 0 is bit 0 of byte P / 8
      const int w = rel >> 5, sh = rel & 31;
      const uint64_t lo64 = v << sh;                             // v has at most 60 bits
      const uint32_t hi = sh ? (uint32_t)(v >> (64 - sh)) : 0u;
      if ((uint32_t)lo64) atomicOr(&words[w], (uint32_t)lo64);   // LDS; OR commutes, so the order of arrival does not matter
      if ((uint32_t)(lo64 >> 32)) atomicOr(&words[w + 1], (uint32_t)(lo64 >> 32));
      if (hi) atomicOr(&words[w + 2], hi);
    }
    __syncthreads();
    const int64_t first = P >> 3;
    const int have = (int)(P & 7) + tile_bits, whole = have >> 3;
    for (int i = tid; i < whole; i += kThreads) {
      if (first + i < room) dst[first + i] = (uint8_t)(words[i >> 2] >> (8 * (i & 3)));
    }
    carry = (words[whole >> 2] >> (8 * (whole & 3))) & 255u;
    P += tile_bits;
    __syncthreads();                                             // everyone has read `words` and wave_bits
  }
  if (tid == 0) {
    int64_t o = P >> 3;
    if ((P & 7) && o < room) dst[o++] = (uint8_t)carry;
    const uint32_t a = adler[c];
    if (P == bits && o + 4 == room) {
      dst[o] = (uint8_t)(a >> 24); dst[o + 1] = (uint8_t)(a >> 16); dst[o + 2] = (uint8_t)(a >> 8); dst[o + 3] = (uint8_t)a;
    }
  }
}

}  // namespace

extern "C" int64_t shdr_deflate_huffman_host(const uint8_t* src, int64_t n, uint8_t* dst, int64_t capacity) {
  int64_t need = 0;
  const int64_t r = encode_host(src, n, dst, capacity, &need);
  if (r == -1) {
    shdr::set_error("deflate_huffman_host: bad arguments (null pointer, or a chunk outside 1 .. 2^30 bytes)");
    return -1;
  }
  if (r == -2) {
    shdr::set_error("deflate_huffman_host: output buffer too small (%lld < %lld)", (long long)capacity, (long long)need);
    return -1;
  }
  return r;
}

extern "C" int shdr_deflate_huffman_lengths_host(const uint8_t* src, int64_t n, uint8_t* lengths) {
  SHDR_REQUIRE(src && lengths, SHDR_E_NULL, "deflate_huffman_lengths_host: null pointer");
  SHDR_REQUIRE(n >= 1 && n <= kMaxChunk, SHDR_E_SHAPE, "deflate_huffman_lengths_host: a chunk has 1 .. 2^30 bytes, got %lld", (long long)n);
  uint32_t freq[kSyms];
  HuffWork work;
  histogram_host(src, n, freq);
  build_lengths(freq, lengths, work);
  return SHDR_OK;
}

extern "C" int shdr_deflate_huffman_batch_sizes(const int64_t* offsets, int n_chunks, int pad, int64_t* out_bytes, int64_t* workspace_bytes) {
  int64_t total = 0, bound = 0;
  if (int rc = check_offsets("deflate_huffman_batch_sizes", offsets, n_chunks, pad, &total, &bound)) return rc;
  if (out_bytes) *out_bytes = bound;
  if (workspace_bytes) *workspace_bytes = carve(nullptr, n_chunks).bytes;
  return SHDR_OK;
}

extern "C" int shdr_deflate_huffman_batch(const uint8_t* data, const uint8_t* raw, const int64_t* offsets, const int64_t* offsets_dev,
                                          int n_chunks, int pad, uint8_t* out, int64_t out_capacity, int64_t* out_offsets, uint8_t* coded,
                                          void* workspace, void* stream, float* stage_ms) {
  const char* what = "deflate_huffman_batch";
  SHDR_REQUIRE(data && offsets_dev && out && out_offsets && coded && workspace, SHDR_E_NULL, "%s: null pointer", what);
  int64_t total = 0, bound = 0;
  if (int rc = check_offsets(what, offsets, n_chunks, pad, &total, &bound)) return rc;
  SHDR_REQUIRE((reinterpret_cast<uintptr_t>(offsets_dev) & 7u) == 0 && (reinterpret_cast<uintptr_t>(out_offsets) & 7u) == 0, SHDR_E_ALIGN,
               "%s: offsets_dev and out_offsets must be 8-byte aligned", what);
  SHDR_REQUIRE(shdr::aligned16(workspace), SHDR_E_ALIGN, "%s: workspace must be 16-byte aligned", what);
  SHDR_REQUIRE(out_capacity >= bound, SHDR_E_SHAPE, "%s: output buffer too small (%lld < %lld)", what, (long long)out_capacity, (long long)bound);
  const Workspace w = carve(workspace, n_chunks);
  hipStream_t st = S(stream);
  hipEvent_t ev[SHDR_DEFLATE_STAGES + 1] = {};
  if (stage_ms)
    for (auto& e : ev) SHDR_REQUIRE(hipEventCreate(&e) == hipSuccess, SHDR_E_LAUNCH, "%s: hipEventCreate failed", what);
  auto mark = [&](int i) { if (stage_ms) (void)hipEventRecord(ev[i], st); };
  mark(0);
  hipLaunchKernelGGL(deflate_stats_kernel, dim3((unsigned)n_chunks), dim3(kThreads), 0, st, data, offsets_dev, total, pad, w.lens, w.bits,
                     w.sizes, w.adler, coded);
  mark(1);
  hipLaunchKernelGGL(deflate_scan_kernel, dim3(1), dim3(1024), 0, st, w.sizes, (int64_t)n_chunks, out_offsets);
  mark(2);
  hipLaunchKernelGGL(deflate_write_kernel, dim3((unsigned)n_chunks), dim3(kThreads), 0, st, data, raw ? raw : data, offsets_dev, total, pad,
                     w.lens, w.bits, w.adler, coded, out_offsets, out, out_capacity);
  mark(3);
  const int rc = shdr::check_launch(what);
  if (stage_ms) {
    const bool ok = hipEventSynchronize(ev[SHDR_DEFLATE_STAGES]) == hipSuccess;
    for (int i = 0; i < SHDR_DEFLATE_STAGES; ++i)
      if (!ok || hipEventElapsedTime(&stage_ms[i], ev[i], ev[i + 1]) != hipSuccess) stage_ms[i] = -1.0f;
    for (auto& e : ev) (void)hipEventDestroy(e);
  }
  return rc;
}

// Huffman-only zlib streams for a BATCH of byte chunks on the device: byte for byte what shdr_deflate_huffman_host writes
// (deflate_huffman.h holds what both share: the code lengths, the canonical codes and the fixed-length block header).
//
// Passes (stream-ordered, no global atomics, no host wait; the same input gives the same bytes).  This file holds the front of
// pass 1 and what a symbol is (HuffCodec); the rest is csrc/deflate_batch.h, shared with csrc/deflate_lz.hip:
//   1  deflate_stats_kernel  one block per chunk: byte histogram in LDS (one per wave), Adler-32 as two block reductions; then
//                            finish_pass1: ONE lane runs build_lengths on the 257 counts
//   2  deflate_scan_kernel   the stored sizes -> out_offsets
//   3  deflate_write_kernel  write_chunk in tiles of kTile symbols: a thread ORs the codes of its four symbols into one value of at
//                            most 60 bits and deposits it once
// Adler-32: s1 = 1 + sum b[i], s2 = n + sum (n - i) b[i], both mod 65521.  A thread adds (n - i) mod 65521 times b[i] < 2^24 for at
// most 2^22 bytes (a 2^30-byte chunk over 256 threads) into 64 bits, so nothing overflows at any size.
#include "shdr_internal.h"
#include "deflate_huffman.h"
#include "deflate_batch.h"

namespace {

using namespace shdr_deflate;
using namespace shdr_deflate_batch;

static_assert(kTile == SHDR_DEFLATE_TILE, "shdr.h names the tile size");

struct HuffCodec {                                               // the Huffman-only stream, as deflate_batch.h asks for it
  static constexpr bool kTokens = false;                         // nothing is parsed: no tokens in the workspace
  static constexpr int kPass1Threads = kThreads, kDeposits = 1;
  static constexpr int kSyms = shdr_deflate::kSyms, kSymbolsAtBit = shdr_deflate::kSymbolsAtBit;
  static constexpr int kTileWords = (7 + kTile * kMaxBits) / 32 + 3;   // carried bits + the tile's bits, and the word a shifted code spills into
  static const uint8_t* items(const uint8_t* data, const Workspace&) { return data; }   // the writer codes the chunk's bytes
  static __device__ __forceinline__ int64_t build_lengths(const uint32_t* freq, uint8_t* len, HuffWork& work) {   // returns the block's bits
    shdr_deflate::build_lengths(freq, len, work);
    return stream_bits(freq, len);
  }
  static __device__ __forceinline__ void build_codes(const uint8_t* len, uint16_t* code, uint8_t* hdr) {
    shdr_deflate::build_codes(len, code);
    write_header(len, hdr);
  }
  // symbols first .. first + 3 of the n + 1 (the chunk's bytes, then end-of-block) in ONE value of at most 60 bits
  static __device__ __forceinline__ void thread_bits(const uint8_t* __restrict__ src, int64_t n, int64_t first, const uint8_t* len,
                                                     const uint16_t* code, uint64_t (&v)[1], int (&nb)[1]) {
    v[0] = 0;
    nb[0] = 0;
#pragma unroll
    for (int k = 0; k < kPerThread; ++k) {
      const int64_t i = first + k;
      if (i <= n) {
        const int s = i < n ? (int)src[i] : 256;
        v[0] |= (uint64_t)code[s] << nb[0];
        nb[0] += len[s];
      }
    }
  }
};
static_assert(kLenStride<HuffCodec> == 272, "shdr_deflate_huffman_batch_sizes: the workspace's layout");

__device__ __forceinline__ uint64_t block_sum_u64(uint64_t v, uint64_t* part) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = v;
  __syncthreads();
  return part[0] + part[1] + part[2] + part[3];
}

__global__ __launch_bounds__(kThreads) void deflate_stats_kernel(const uint8_t* __restrict__ data, const int64_t* __restrict__ offsets,
                                                                 int64_t total, Framing fr, Workspace w, uint8_t* __restrict__ coded) {
  __shared__ uint32_t hist[4][256];
  __shared__ uint32_t freq[kSyms];
  __shared__ uint8_t len[kLenStride<HuffCodec>];
  __shared__ HuffWork work;
  __shared__ uint64_t part[4];
  const int64_t c = blockIdx.x;
  const shdr::Span span = shdr::clamped_span(offsets, c, total, kMaxChunk);
  const int64_t lo = span.lo, n = span.n;
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
  finish_pass1<HuffCodec>(freq, len, work, tid, kThreads, c, n, fr, s1, s2, w, coded);
}

__global__ __launch_bounds__(kThreads) void deflate_write_kernel(const uint8_t* __restrict__ data, const uint8_t* __restrict__ raw,
                                                                 const int64_t* __restrict__ offsets, int64_t total, Framing fr, Workspace w,
                                                                 const uint8_t* __restrict__ coded, const int64_t* __restrict__ out_offsets,
                                                                 uint8_t* __restrict__ out, int64_t capacity) {
  write_chunk<HuffCodec>(data, raw, offsets, total, fr, w, coded, out_offsets, out, capacity);
}

}  // namespace

// the same kernels over the segments of PNG images (csrc/png_enc.hip; deflate_batch.h: run_segments)
namespace shdr_deflate_batch {
static int64_t segments_workspace(int64_t n_chunks, int64_t total) {
  return carve(nullptr, n_chunks, kLenStride<HuffCodec>, HuffCodec::kTokens ? total : 0).bytes;
}
static void segments_run(const uint8_t* data, const int64_t* offsets_dev, int64_t n_chunks, int64_t total, const uint8_t* seg_dev, uint8_t* out,
                         int64_t out_capacity, int64_t* out_offsets, uint8_t* coded, void* workspace, hipStream_t st, const uint32_t** adler,
                         void (*mark)(void*), void* mark_arg) {
  run_segments<HuffCodec>(deflate_stats_kernel, deflate_write_kernel, data, offsets_dev, n_chunks, total, seg_dev, out, out_capacity, out_offsets, coded, workspace, st,
                      adler, [&] { mark(mark_arg); });
}
SegmentCoder huffman_segments() { return SegmentCoder{segments_workspace, segments_run}; }
}  // namespace shdr_deflate_batch

extern "C" int64_t shdr_deflate_huffman_host(const uint8_t* src, int64_t n, uint8_t* dst, int64_t capacity) {
  int64_t need = 0;
  return host_result("deflate_huffman_host", encode_host(src, n, dst, capacity, &need), n, capacity, need);
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
  return batch_sizes<HuffCodec>("deflate_huffman_batch_sizes", offsets, n_chunks, pad, out_bytes, workspace_bytes);
}

extern "C" int shdr_deflate_huffman_batch(const uint8_t* data, const uint8_t* raw, const int64_t* offsets, const int64_t* offsets_dev,
                                          int n_chunks, int pad, uint8_t* out, int64_t out_capacity, int64_t* out_offsets, uint8_t* coded,
                                          void* workspace, void* stream, float* stage_ms) {
  return run_batch<HuffCodec>("deflate_huffman_batch", deflate_stats_kernel, deflate_write_kernel, data, raw, offsets, offsets_dev, n_chunks, pad,
                              out, out_capacity, out_offsets, coded, workspace, stream, stage_ms);
}

// The batched device encoder behind shdr_deflate_huffman_batch (csrc/deflate.hip) and shdr_deflate_lz_batch (csrc/deflate_lz.hip): all
// of it that does not depend on what a symbol is.  Each of the two files brings the front of its pass 1, two __global__ entry points
// and a `Codec`: a struct with kTokens, kPass1Threads, kDeposits, kSyms, kSymbolsAtBit, kTileWords, items, build_lengths, build_codes
// and thread_bits (HuffCodec, LzCodec).  Here are the workspace, the end of pass 1 (finish_pass1), pass 2 (deflate_scan_kernel, over scan_array of batch.h), the
// body of pass 3 (write_chunk) and the host side (batch_sizes, run_batch).  Every translation unit gets its own copy.
// A second framing (Framing, run_segments) codes the segments of PNG images with the same kernels: the block without the zlib bytes,
// BFINAL per chunk, a sync marker, stored blocks (csrc/png.h has the rules, csrc/png_enc.hip the caller).
#pragma once
#include "shdr_internal.h"
#include "batch.h"
#include "deflate_huffman.h"
#include "png.h"

namespace shdr_deflate_batch {
namespace {                                   // internal linkage: the kernel and its host stub exist once per translation unit

using shdr_deflate::kAdlerMod;
using shdr_deflate::kMaxChunk;
using shdr_deflate::stream_bytes;

constexpr int kThreads = 256;                                    // of a writer block
constexpr int kPerThread = 4;
constexpr int kTile = kThreads * kPerThread;                     // items per tile of the writers (shdr.h: SHDR_DEFLATE_TILE, _LZ_TILE)

template <class Codec>
constexpr int kLenStride = (int)shdr::align16(Codec::kSyms);         // bytes per chunk of the stored code lengths

struct Workspace {                                               // carved out of the caller's workspace, every part 16-byte aligned
  uint8_t* lens;                                                 // [C][kLenStride]
  int64_t* bits;                                                 // [C] bits of the block incl. the two zlib bytes in front
  int64_t* sizes;                                                // [C] pad + stored bytes
  uint32_t* adler;                                               // [C]
  uint32_t* tokens;                                              // [n_tokens] one per input byte where the codec parses, else none
  int64_t bytes;
};
// How a chunk is framed.  seg == NULL: a zlib stream of its own behind `pad` free bytes, or its raw bytes (the entry points of shdr.h).
// seg[c], a PNG segment's flags (png.h): the block alone -- no zlib bytes, BFINAL only with kLast, the sync marker behind every other
// one -- or one stored block if that is not strictly fewer than n + 5 bytes, between seg_front and seg_back free bytes.
struct Framing {
  int pad;
  const uint8_t* seg;
};
inline Workspace carve(void* ws, int64_t c, int len_stride, int64_t n_tokens) {
  Workspace w;
  shdr::Carver cut(ws);
  w.lens = cut.take<uint8_t>((int64_t)len_stride * c);           // (the stride is a multiple of 16)
  w.bits = cut.take<int64_t>(c);
  w.sizes = cut.take<int64_t>(c);
  w.adler = cut.take<uint32_t>(c);
  w.tokens = cut.take<uint32_t>(n_tokens);
  w.bytes = cut.bytes();
  return w;
}

// The end of pass 1 for chunk c of n bytes, by all `threads` threads of its block (this one is `tid`): freq (LDS) holds the counts
// once every thread has arrived, s1 and s2 are the Adler sums mod 65521.  ONE lane builds the lengths and stores the block's size in
// bits, the checksum and the stored size: the stream if that is strictly smaller than the chunk, else the chunk.  All store the lengths.
template <class Codec, class Work>
__device__ __forceinline__ void finish_pass1(const uint32_t* freq, uint8_t* len, Work& work, int tid, int threads, int64_t c,
                                             int64_t n, Framing fr, uint64_t s1, uint64_t s2, const Workspace& w, uint8_t* __restrict__ coded) {
  __syncthreads();
  if (tid == 0) {
    const int64_t bits = Codec::build_lengths(freq, len, work);
    bool use;
    if (fr.seg) {
      const int flags = fr.seg[c];
      const int64_t body = shdr_png::coded_bytes(bits - 16, flags & shdr_png::kLast);
      use = n > 0 && shdr_png::use_coded(body, n);
      w.sizes[c] = shdr_png::seg_front(flags) + (use ? body : n + 5) + shdr_png::seg_back(flags);
    } else {
      const int64_t stream = stream_bytes(bits);
      use = n > 0 && stream < n;
      w.sizes[c] = fr.pad + (use ? stream : n);
    }
    w.bits[c] = bits;
    coded[c] = use ? 1 : 0;
    w.adler[c] = (uint32_t)((((uint64_t)(n % kAdlerMod) + s2) % kAdlerMod) << 16) | (uint32_t)((1 + s1) % kAdlerMod);
  }
  __syncthreads();
  for (int s = tid; s < kLenStride<Codec>; s += threads) w.lens[c * kLenStride<Codec> + s] = s < Codec::kSyms ? len[s] : 0;
}

// out_offsets[c] = sum of the sizes before c, out_offsets[C] = the total.  One block.
__global__ __launch_bounds__(1024) void deflate_scan_kernel(const int64_t* __restrict__ sizes, int64_t count, int64_t* __restrict__ out_offsets) {
  const int64_t all = shdr::scan_array<1024, 1>(
      count, [&](int64_t c) { return sizes[c]; }, [&](int64_t c, int64_t before) { out_offsets[c] = before; });
  if (threadIdx.x == 0) out_offsets[count] = all;
}

// Pass 3 for chunk blockIdx.x, by a block of kThreads: the header, then tiles of kTile items (+ end-of-block behind the last).  The
// codec turns a thread's kPerThread items (the chunk's bytes, or the tokens of pass 1) into Codec::kDeposits values of nb[k] bits, in
// stream order; a block prefix sum of the bit counts gives every thread its bit, each value is OR-ed into the tile's LDS words on
// its own (ONE deposit per thread where the codec can combine its items) and the whole bytes of the tile are stored; the partial
// byte and the bit position carry to the next tile; then the tail and the Adler-32.  A chunk that is not coded is copied from `raw`.
template <class Codec, class Item>
__device__ __forceinline__ void write_chunk(const Item* __restrict__ items, const uint8_t* __restrict__ raw,
                                            const int64_t* __restrict__ offsets, int64_t total, Framing fr, const Workspace& ws,
                                            const uint8_t* __restrict__ coded, const int64_t* __restrict__ out_offsets,
                                            uint8_t* __restrict__ out, int64_t capacity) {
  constexpr int kHeaderBytes = Codec::kSymbolsAtBit / 8 + 1;     // the bytes that hold the bits in front of the symbols
  __shared__ uint8_t len[kLenStride<Codec>];
  __shared__ uint16_t code[Codec::kSyms + (Codec::kSyms & 1)];
  __shared__ uint8_t hdr[kHeaderBytes + 3];
  __shared__ uint32_t words[Codec::kTileWords];
  __shared__ int wave_bits[4];
  const int64_t c = blockIdx.x;
  const shdr::Span span = shdr::clamped_span(offsets, c, total, kMaxChunk);
  const int64_t lo = span.lo, n = span.n;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const bool png = fr.seg != nullptr;
  const int flags = png ? fr.seg[c] : 0;
  const bool last = !png || (flags & shdr_png::kLast);
  const int64_t at = out_offsets[c] + (png ? shdr_png::seg_front(flags) : fr.pad), end = out_offsets[c + 1] - (png ? shdr_png::seg_back(flags) : 0);
  if (at < 0 || end > capacity || end < at) return;              // never with the sizes the host checked
  uint8_t* dst = out + at;
  int64_t room = end - at;
  if (!coded[c]) {
    const uint8_t* src = raw + lo;
    if (png) {                                                   // one stored block
      if (room != n + 5) return;
      if (tid == 0) shdr_png::put_stored_header(dst, n, last);
      dst += 5;
      room -= 5;
    }
    for (int64_t i = tid; i < n && i < room; i += kThreads) dst[i] = src[i];
    return;
  }
  const int64_t bits = ws.bits[c];
  if ((png ? shdr_png::coded_bytes(bits - 16, last) : stream_bytes(bits)) != room) return;   // (pass 1 stored both)
  const int skip = png ? 2 : 0;                                  // the zlib bytes in front: stream byte i goes to dst[i], from `skip` on
  dst -= skip;                                                   // (at least 8 bytes of the segment's front lie there)
  room += skip;
  for (int s = tid; s < kLenStride<Codec>; s += kThreads) len[s] = ws.lens[c * kLenStride<Codec> + s];
  __syncthreads();
  if (tid == 0) {
    Codec::build_codes(len, code, hdr);
    if (!last) hdr[2] &= 0xFEu;                                  // BFINAL
  }
  __syncthreads();
  for (int i = skip + tid; i < kHeaderBytes - 1; i += kThreads) dst[i] = hdr[i];
  const Item* src = items + lo;
  int64_t P = Codec::kSymbolsAtBit;                              // the stream bit of the tile's first item; the same in every thread
  uint32_t carry = hdr[kHeaderBytes - 1];                        // the bits of byte P / 8 that are already decided
  for (int64_t base = 0; base <= n; base += kTile) {             // n items, then end-of-block
    for (int i = tid; i < Codec::kTileWords; i += kThreads) words[i] = i == 0 ? carry : 0u;
    uint64_t v[Codec::kDeposits];
    int nbk[Codec::kDeposits], nb = 0;
    Codec::thread_bits(src, n, base + (int64_t)tid * kPerThread, len, code, v, nbk);
#pragma unroll
    for (int k = 0; k < Codec::kDeposits; ++k) nb += nbk[k];
    const int incl = shdr::wave_scan(nb);                        // (not block_scan: the barrier below also covers `words`)
    if (lane == 63) wave_bits[wave] = incl;
    __syncthreads();                                             // words are cleared, wave_bits are written
    int before = 0;
    for (int w = 0; w < wave; ++w) before += wave_bits[w];
    const int tile_bits = wave_bits[0] + wave_bits[1] + wave_bits[2] + wave_bits[3];
    int rel = (int)(P & 7) + before + incl - nb;                 // bit in `words`, whose bit 0 is bit 0 of byte P / 8
#pragma unroll
    for (int k = 0; k < Codec::kDeposits; ++k) {
      if (!nbk[k]) continue;
      const int word = rel >> 5, sh = rel & 31;
      const uint32_t w0 = (uint32_t)(v[k] << sh);                // up to 64 bits shifted by up to 31: three words at the most
      const uint64_t hi = sh ? v[k] >> (32 - sh) : v[k] >> 32;
      if (w0) atomicOr(&words[word], w0);                        // LDS; OR commutes, so the order of arrival does not matter
      if ((uint32_t)hi) atomicOr(&words[word + 1], (uint32_t)hi);
      if ((uint32_t)(hi >> 32)) atomicOr(&words[word + 2], (uint32_t)(hi >> 32));
      rel += nbk[k];
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
    if (png) {
      if (!last && P == bits) {                                  // the empty stored block: three zero bits, the byte's rest, 00 00 FF FF
        for (const int64_t e = (P + 3 + 7) >> 3; o < e && o < room; ++o) dst[o] = 0;
        if (o + 4 == room) {
          dst[o] = dst[o + 1] = 0;
          dst[o + 2] = dst[o + 3] = 0xFF;
        }
      }
      return;
    }
    const uint32_t a = ws.adler[c];
    if (P == bits && o + 4 == room) {
      dst[o] = (uint8_t)(a >> 24); dst[o + 1] = (uint8_t)(a >> 16); dst[o + 2] = (uint8_t)(a >> 8); dst[o + 3] = (uint8_t)a;
    }
  }
}

// what the two *_host routines return for encode_host's r: the stream's length, or -1 with the error set
inline int64_t host_result(const char* what, int64_t r, int64_t n, int64_t capacity, int64_t need) {
  if (r == -1) shdr::set_error("%s: bad arguments (null pointer, or a chunk outside 1 .. 2^30 bytes)", what);
  if (r == -2) shdr::set_error("%s: output buffer too small (%lld < %lld)", what, (long long)capacity, (long long)need);
  if (r == -3) shdr::set_error("%s: no memory for the tokens of %lld bytes", what, (long long)n);
  return r < 0 ? -1 : r;
}

int check_offsets(const char* what, const int64_t* offsets, int n_chunks, int pad, int64_t* total, int64_t* bound) {
  SHDR_REQUIRE(offsets, SHDR_E_NULL, "%s: null offsets", what);
  SHDR_REQUIRE(n_chunks > 0, SHDR_E_SHAPE, "%s: the number of chunks must be positive, got %d", what, n_chunks);
  SHDR_REQUIRE(pad >= 0 && pad <= 4096, SHDR_E_SHAPE, "%s: pad must be in [0, 4096], got %d", what, pad);
  SHDR_REQUIRE(offsets[0] == 0, SHDR_E_SHAPE, "%s: offsets[0] must be 0", what);
  for (int c = 0; c < n_chunks; ++c) {
    const int64_t n = offsets[c + 1] - offsets[c];
    SHDR_REQUIRE(n >= 1 && n <= kMaxChunk, SHDR_E_SHAPE, "%s: chunk %d has %lld bytes (1 .. 2^30 are supported)", what, c, (long long)n);
  }
  *total = offsets[n_chunks];
  *bound = offsets[n_chunks] + (int64_t)pad * n_chunks;          // a stored chunk is never larger than the chunk
  return SHDR_OK;
}

template <class Codec>
int batch_sizes(const char* what, const int64_t* offsets, int n_chunks, int pad, int64_t* out_bytes, int64_t* workspace_bytes) {
  int64_t total = 0, bound = 0;
  if (int rc = check_offsets(what, offsets, n_chunks, pad, &total, &bound)) return rc;
  if (out_bytes) *out_bytes = bound;
  if (workspace_bytes) *workspace_bytes = carve(nullptr, n_chunks, kLenStride<Codec>, Codec::kTokens ? total : 0).bytes;
  return SHDR_OK;
}

// The three launches.  pass1, write: the codec's kernels, one block of Codec::kPass1Threads and one of kThreads per chunk.
template <class Codec, class Pass1, class Write>
int run_batch(const char* what, Pass1 pass1, Write write, const uint8_t* data, const uint8_t* raw, const int64_t* offsets,
              const int64_t* offsets_dev, int n_chunks, int pad, uint8_t* out, int64_t out_capacity, int64_t* out_offsets, uint8_t* coded,
              void* workspace, void* stream, float* stage_ms) {
  SHDR_REQUIRE(data && offsets_dev && out && out_offsets && coded && workspace, SHDR_E_NULL, "%s: null pointer", what);
  int64_t total = 0, bound = 0;
  if (int rc = check_offsets(what, offsets, n_chunks, pad, &total, &bound)) return rc;
  SHDR_REQUIRE((reinterpret_cast<uintptr_t>(offsets_dev) & 7u) == 0 && (reinterpret_cast<uintptr_t>(out_offsets) & 7u) == 0, SHDR_E_ALIGN,
               "%s: offsets_dev and out_offsets must be 8-byte aligned", what);
  SHDR_REQUIRE(shdr::aligned16(workspace), SHDR_E_ALIGN, "%s: workspace must be 16-byte aligned", what);
  SHDR_REQUIRE(out_capacity >= bound, SHDR_E_SHAPE, "%s: output buffer too small (%lld < %lld)", what, (long long)out_capacity, (long long)bound);
  const Workspace w = carve(workspace, n_chunks, kLenStride<Codec>, Codec::kTokens ? total : 0);
  hipStream_t st = shdr::stream_of(stream);
  shdr::StageTimer<SHDR_DEFLATE_STAGES> timer(stage_ms, st);
  hipLaunchKernelGGL(pass1, dim3((unsigned)n_chunks), dim3(Codec::kPass1Threads), 0, st, data, offsets_dev, total, Framing{pad, nullptr}, w, coded);
  timer.mark();
  hipLaunchKernelGGL(deflate_scan_kernel, dim3(1), dim3(1024), 0, st, w.sizes, (int64_t)n_chunks, out_offsets);
  timer.mark();
  hipLaunchKernelGGL(write, dim3((unsigned)n_chunks), dim3(kThreads), 0, st, Codec::items(data, w), raw ? raw : data, offsets_dev, total,
                     Framing{pad, nullptr}, w, coded, out_offsets, out, out_capacity);
  timer.mark();
  return shdr::check_launch(what);
}

// The same three launches over the segments of PNG images (csrc/png_enc.hip, which has checked every size): chunk c is
// data[offsets_dev[c] .. offsets_dev[c + 1]), at most kPngSegment bytes, framed by seg_dev[c]; out_offsets[c] is where its front begins.
// *adler: the workspace's Adler-32 per segment.  mark: called behind every launch.
template <class Codec, class Pass1, class Write, class Mark>
void run_segments(Pass1 pass1, Write write, const uint8_t* data, const int64_t* offsets_dev, int64_t n_chunks, int64_t total,
                  const uint8_t* seg_dev, uint8_t* out, int64_t out_capacity, int64_t* out_offsets, uint8_t* coded, void* workspace,
                  hipStream_t st, const uint32_t** adler, Mark mark) {
  const Workspace w = carve(workspace, n_chunks, kLenStride<Codec>, Codec::kTokens ? total : 0);
  const Framing fr{0, seg_dev};
  hipLaunchKernelGGL(pass1, dim3((unsigned)n_chunks), dim3(Codec::kPass1Threads), 0, st, data, offsets_dev, total, fr, w, coded);
  mark();
  hipLaunchKernelGGL(deflate_scan_kernel, dim3(1), dim3(1024), 0, st, w.sizes, n_chunks, out_offsets);
  mark();
  hipLaunchKernelGGL(write, dim3((unsigned)n_chunks), dim3(kThreads), 0, st, Codec::items(data, w), data, offsets_dev, total, fr, w, coded,
                     out_offsets, out, out_capacity);
  mark();
  *adler = w.adler;
}

}  // namespace

// Defined by csrc/deflate.hip (huffman_segments) and csrc/deflate_lz.hip (lz_segments) over their codecs, for csrc/png_enc.hip: the workspace that
// run_segments takes for n_chunks segments of `total` bytes, and run_segments itself.
struct SegmentCoder {
  int64_t (*workspace_bytes)(int64_t n_chunks, int64_t total);
  void (*run)(const uint8_t* data, const int64_t* offsets_dev, int64_t n_chunks, int64_t total, const uint8_t* seg_dev, uint8_t* out,
              int64_t out_capacity, int64_t* out_offsets, uint8_t* coded, void* workspace, hipStream_t st, const uint32_t** adler,
              void (*mark)(void*), void* mark_arg);
};
SegmentCoder huffman_segments();
SegmentCoder lz_segments();

}  // namespace shdr_deflate_batch

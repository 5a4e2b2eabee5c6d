// zlib streams with LZ77 matches for a BATCH of byte chunks on the device: byte for byte what shdr_deflate_lz_host writes
// (deflate_lz.h holds what both share: the parse rules, the symbols, the code lengths and the fixed-length block header).
//
// Passes (stream-ordered, no global atomics, no host wait; the same input gives the same bytes).  This file holds the parse of
// pass 1 and what a token is (LzCodec); the rest is csrc/deflate_batch.h, shared with csrc/deflate.hip:
//   1  deflate_lz_parse_kernel  ONE 64-lane wave per chunk walks the chunk in groups of 64 positions: every lane that the greedy walk
//                               can still reach looks its position up in the LDS hash table and compares the first 8 bytes of
//                               candidates A and B (probe_at; the group's own bytes are staged in LDS a window of 1024 ahead),
//                               all lanes insert their position (LDS atomicMax: the highest wins), then the walk runs over the group with wave-uniform state (a ballot of the lanes that hold a match, one step
//                               and one v_readlane per match on the way, the literals between them by mask); a token on the
//                               walk's way whose candidates reach beyond 8 bytes is extended by the whole wave, 8 bytes per lane,
//                               so a long match costs one more round of loads and only where it is taken.  One uint32 token
//                               per position goes to the workspace, the starts are counted into the LDS histogram (286 + 30),
//                               Adler-32 as in deflate.hip; then finish_pass1: ONE lane builds both codes
//   2  deflate_scan_kernel      the stored sizes -> out_offsets
//   3  deflate_lz_write_kernel  write_chunk in tiles of kTile POSITIONS: a position's token is 0..48 bits and is OR-ed into the LDS
//                               words on its own, four deposits per thread
// LDS of pass 1: 16 KiB table + 1264 B counts + 320 B lengths + 5148 B Huffman scratch + 1032 B window = 24 152 B per 64-thread
// block, so the 160 KiB of a CU hold 6 blocks (6 chunks); pass 3: 320 + 632 + 173 + 6156 (words) + 16 B per 256-thread block.
#include "shdr_internal.h"
#include "deflate_lz.h"
#include "deflate_batch.h"

namespace {

using namespace shdr_deflate_lz;
using namespace shdr_deflate_batch;

static_assert(kTile == SHDR_DEFLATE_LZ_TILE, "shdr.h names the tile size");
constexpr int kWindow = 16 * kGroup;                             // bytes of the chunk staged in LDS per round: 16 per lane
static_assert(kGroup == 64, "one lane per position of a group");
static_assert(kLiteral == SHDR_DEFLATE_LZ_LITERAL, "shdr.h names the literal flag of a token");

struct LzCodec {                                                 // the stream with matches, as deflate_batch.h asks for it
  static constexpr bool kTokens = true;
  static constexpr int kPass1Threads = kGroup, kDeposits = kPerThread;
  static constexpr int kSyms = kAllSyms, kSymbolsAtBit = shdr_deflate_lz::kSymbolsAtBit;
  static constexpr int kTileWords = (7 + kTile * kMaxTokenBits) / 32 + 3;   // carried bits + the tile's bits, and the words a shifted token spills into
  static const uint32_t* items(const uint8_t*, const Workspace& w) { return w.tokens; }   // the writer codes the tokens of pass 1
  static __device__ __forceinline__ int64_t build_lengths(const uint32_t* freq, uint8_t* len, LzWork& work) {   // returns the block's bits
    build_all_lengths(freq, len, work);
    return stream_bits(freq, len);
  }
  static __device__ __forceinline__ void build_codes(const uint8_t* len, uint16_t* code, uint8_t* hdr) {
    build_all_codes(len, code);
    write_header(len, hdr);
  }
  // positions first .. first + 3 of the n + 1 (the chunk's tokens, then end-of-block), each on its own: at most 48 bits, none where a match covers it
  static __device__ __forceinline__ void thread_bits(const uint32_t* __restrict__ tok, int64_t n, int64_t first, const uint8_t* len,
                                                     const uint16_t* code, uint64_t (&v)[kPerThread], int (&nb)[kPerThread]) {
#pragma unroll
    for (int k = 0; k < kPerThread; ++k) {
      const int64_t i = first + k;
      const uint32_t t = i < n ? tok[i] : i == n ? kEndOfBlock : 0u;
      v[k] = 0;
      nb[k] = t ? token_bits(t, len, code, v[k]) : 0;
    }
  }
};
static_assert(kLenStride<LzCodec> == 320, "shdr_deflate_lz_batch_sizes: the workspace's layout (316 lengths are used)");

__device__ __forceinline__ uint64_t wave_sum_u64(uint64_t v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
  return v;
}

// 16 bytes of the chunk from position `at` on, zero beyond its end (any alignment)
__device__ __forceinline__ void load16(const uint8_t* __restrict__ src, int64_t n, int64_t at, uint64_t& a, uint64_t& b) {
  a = b = 0;
  if (at + 16 <= n) {
    __builtin_memcpy(&a, src + at, 8);
    __builtin_memcpy(&b, src + at + 8, 8);
  } else {
    for (int k = 0; k < 8; ++k) {
      if (at + k < n) a |= (uint64_t)src[at + k] << (8 * k);
      if (at + 8 + k < n) b |= (uint64_t)src[at + 8 + k] << (8 * k);
    }
  }
}

// token_at's second half for ONE position q, by the whole wave: o holds what probe_at found (da | la << 16 | lb << 20); lanes 0..31
// compare 8 bytes each of candidate A behind the probe, lanes 32..63 of candidate B, and the first lane that differs ends the match.
// The same in every lane.
__device__ __forceinline__ uint32_t extend_in_wave(const uint8_t* __restrict__ src, int64_t n, int64_t q, uint32_t o, uint32_t byte, int lane) {
  const int64_t rest = n - q;
  const int maxlen = rest < kMaxMatch ? (int)rest : kMaxMatch;
  const int da = (int)(o & 0xFFFFu), la0 = (int)(o >> 16) & 15, lb0 = (int)(o >> 20) & 15;
  const bool second = lane >= 32;
  const int at = kProbe + 8 * (lane & 31), dist = second ? 1 : da;
  const bool active = (second ? lb0 : la0) == kProbe && at < maxlen;
  const int want = maxlen - at < 8 ? maxlen - at : 8;
  int eq = 8;
  if (active) eq = match_length(src + q + at, src + q + at - dist, want);
  const uint64_t differ = __ballot(active && eq < want);
  const uint32_t differ_a = (uint32_t)differ, differ_b = (uint32_t)(differ >> 32);
  int la = la0, lb = lb0;
  if (la0 == kProbe) {
    const int f = differ_a ? __builtin_ctz(differ_a) : 0;
    la = differ_a ? kProbe + 8 * f + __builtin_amdgcn_readlane(eq, f) : maxlen;
  }
  if (lb0 == kProbe) {
    const int f = differ_b ? __builtin_ctz(differ_b) : 0;
    lb = differ_b ? kProbe + 8 * f + __builtin_amdgcn_readlane(eq, 32 + f) : maxlen;
  }
  return choose_token(byte, la, da, lb);
}

__global__ __launch_bounds__(kGroup) void deflate_lz_parse_kernel(const uint8_t* __restrict__ data, const int64_t* __restrict__ offsets,
                                                                  int64_t total, Framing fr, Workspace w, uint8_t* __restrict__ coded) {
  __shared__ uint32_t table[kHashSlots];
  __shared__ uint32_t freq[kAllSyms];
  __shared__ uint8_t len[kLenStride<LzCodec>];
  __shared__ LzWork work;
  __shared__ uint64_t stage64[kWindow / 8 + 1];                  // a window of the chunk and the 2 bytes behind it
  uint8_t* stage = reinterpret_cast<uint8_t*>(stage64);
  const int64_t c = blockIdx.x;
  const shdr::Span span = shdr::clamped_span(offsets, c, total, kMaxChunk);
  const int64_t lo = span.lo, n = span.n;
  const int lane = threadIdx.x;
  for (int i = lane; i < kHashSlots; i += kGroup) table[i] = 0;
  for (int i = lane; i < kAllSyms; i += kGroup) freq[i] = i == 256 ? 1u : 0u;
  __syncthreads();
  const uint8_t* src = data + lo;
  uint32_t* tok_out = w.tokens + lo;
  uint64_t s1 = 0, s2 = 0;
  int64_t pos = 0;                                               // where the next token starts: the same in every lane
  // The group's own bytes come through LDS, kWindow at a time and one window ahead: a wave alone on its chunk would otherwise wait
  // for memory once per group.  The candidates' bytes (token_at) are read from memory, which these loads have just touched.
  uint64_t ahead_a, ahead_b;
  uint32_t ahead_c;                                              // lanes 0 and 1: the two bytes behind the window, for its last hashes
  auto fetch = [&](int64_t at) {
    load16(src, n, at + 16 * lane, ahead_a, ahead_b);
    ahead_c = lane < 2 && at + kWindow + lane < n ? src[at + kWindow + lane] : 0u;
  };
  fetch(0);
  int64_t weight = ((n - lane) % kAdlerMod + kAdlerMod) % kAdlerMod;   // (n - p) mod 65521, kept by subtraction
  for (int64_t base = 0; base < n; base += kGroup) {
    const int64_t p = base + lane;
    const int in_window = (int)(base & (kWindow - 1));
    if (in_window == 0) {
      __syncthreads();                                           // the last group's reads of the window are done
      stage64[2 * lane] = ahead_a;
      stage64[2 * lane + 1] = ahead_b;
      if (lane < 2) stage[kWindow + lane] = (uint8_t)ahead_c;
      fetch(base + kWindow);                                     // in flight while this window is parsed
      __syncthreads();
    }
    const uint8_t* at = stage + in_window + lane;
    const uint32_t b0 = at[0], b1 = at[1], b2 = at[2];
    const bool in = p < n, hashable = p + 2 < n;
    const uint32_t h = hash3(b0, b1, b2);
    const uint32_t slot = hashable ? table[h] : 0u;
    if (in) {
      s1 += b0;
      s2 += (uint64_t)weight * b0;
    }
    weight -= kGroup;
    if (weight < 0) weight += kAdlerMod;
    uint32_t tok = 0, open = 0;                                  // open: a position whose candidates go on beyond the probe
    if (in && p >= pos) {                                        // an earlier match covers the others whatever this group finds
      int maxlen, da, la, lb;
      probe_at(src, n, p, slot, maxlen, da, la, lb);
      if (probe_is_open(maxlen, la, lb)) open = (uint32_t)da | (uint32_t)la << 16 | (uint32_t)lb << 20 | 1u << 24;
      else tok = choose_token(b0, la, da, lb);
    }
    __syncthreads();                                             // every lookup of the group comes before its inserts
    if (hashable) atomicMax(&table[h], (uint32_t)(p + 1));       // LDS; positions grow, so the slot keeps the most recent one
    __syncthreads();
    const int64_t end = base + kGroup < n ? base + kGroup : n;
    // The walk, one step per MATCH on its way: the literals between two matches start a token each and need no step of their own.
    const uint64_t matches = __ballot(open != 0 || (tok != 0 && !token_is_literal(tok)));
    const int lim = (int)(end - base);
    uint64_t starts = 0;
    while (pos < end) {
      const int l = __builtin_amdgcn_readfirstlane((int)(pos - base));
      const uint64_t from = ~0ull << l, ahead = matches & from;
      const int m = ahead ? __builtin_ctzll(ahead) : kGroup;     // the next lane with a match, if the group has one
      const int stop = m < lim ? m : lim;
      starts |= from & (stop < kGroup ? (1ull << stop) - 1 : ~0ull);   // lanes l .. stop - 1 are literals
      pos = base + stop;
      if (stop == lim) break;
      uint32_t t = (uint32_t)__builtin_amdgcn_readlane((int)tok, stop);
      const uint32_t o = (uint32_t)__builtin_amdgcn_readlane((int)open, stop);
      if (o) {                                                   // the walk takes this token: all lanes extend its candidates
        t = extend_in_wave(src, n, pos, o, (uint32_t)__builtin_amdgcn_readlane((int)b0, stop), lane);
        if (lane == stop) tok = t;
      }
      starts |= 1ull << stop;
      const int step = token_is_literal(t) ? 1 : token_length(t);
      pos += step > 0 ? step : 1;                                // (a visited lane always holds a token: the walk never stalls)
    }
    const bool start = (starts >> lane) & 1ull;
    if (in) tok_out[p] = start ? tok : 0u;
    if (start) {
      int ls, ds;
      token_symbols(tok, ls, ds);
      atomicAdd(&freq[ls], 1u);                                  // LDS
      if (ds >= 0) atomicAdd(&freq[kLitSyms + ds], 1u);
    }
  }
  s1 = wave_sum_u64(s1 % kAdlerMod);
  s2 = wave_sum_u64(s2 % kAdlerMod);
  finish_pass1<LzCodec>(freq, len, work, lane, kGroup, c, n, fr, s1, s2, w, coded);
}

__global__ __launch_bounds__(kThreads) void deflate_lz_write_kernel(const uint32_t* __restrict__ tokens, const uint8_t* __restrict__ raw,
                                                                    const int64_t* __restrict__ offsets, int64_t total, Framing fr, Workspace w,
                                                                    const uint8_t* __restrict__ coded, const int64_t* __restrict__ out_offsets,
                                                                    uint8_t* __restrict__ out, int64_t capacity) {
  write_chunk<LzCodec>(tokens, raw, offsets, total, fr, w, coded, out_offsets, out, capacity);
}

}  // namespace

// the same kernels over the segments of PNG images (csrc/png_enc.hip; deflate_batch.h: run_segments)
namespace shdr_deflate_batch {
static int64_t segments_workspace(int64_t n_chunks, int64_t total) {
  return carve(nullptr, n_chunks, kLenStride<LzCodec>, LzCodec::kTokens ? total : 0).bytes;
}
static void segments_run(const uint8_t* data, const int64_t* offsets_dev, int64_t n_chunks, int64_t total, const uint8_t* seg_dev, uint8_t* out,
                         int64_t out_capacity, int64_t* out_offsets, uint8_t* coded, void* workspace, hipStream_t st, const uint32_t** adler,
                         void (*mark)(void*), void* mark_arg) {
  run_segments<LzCodec>(deflate_lz_parse_kernel, deflate_lz_write_kernel, data, offsets_dev, n_chunks, total, seg_dev, out, out_capacity, out_offsets, coded, workspace, st,
                      adler, [&] { mark(mark_arg); });
}
SegmentCoder lz_segments() { return SegmentCoder{segments_workspace, segments_run}; }
}  // namespace shdr_deflate_batch

extern "C" int64_t shdr_deflate_lz_host(const uint8_t* src, int64_t n, uint8_t* dst, int64_t capacity) {
  int64_t need = 0;
  return host_result("deflate_lz_host", encode_host(src, n, dst, capacity, &need), n, capacity, need);
}

extern "C" int shdr_deflate_lz_parse_host(const uint8_t* src, int64_t n, uint32_t* tokens) {
  SHDR_REQUIRE(src && tokens, SHDR_E_NULL, "deflate_lz_parse_host: null pointer");
  SHDR_REQUIRE(n >= 1 && n <= kMaxChunk, SHDR_E_SHAPE, "deflate_lz_parse_host: a chunk has 1 .. 2^30 bytes, got %lld", (long long)n);
  uint32_t table[kHashSlots];
  parse_host(src, n, tokens, table);
  return SHDR_OK;
}

extern "C" int shdr_deflate_lz_batch_sizes(const int64_t* offsets, int n_chunks, int pad, int64_t* out_bytes, int64_t* workspace_bytes) {
  return batch_sizes<LzCodec>("deflate_lz_batch_sizes", offsets, n_chunks, pad, out_bytes, workspace_bytes);
}

extern "C" int shdr_deflate_lz_batch(const uint8_t* data, const uint8_t* raw, const int64_t* offsets, const int64_t* offsets_dev,
                                     int n_chunks, int pad, uint8_t* out, int64_t out_capacity, int64_t* out_offsets, uint8_t* coded,
                                     void* workspace, void* stream, float* stage_ms) {
  return run_batch<LzCodec>("deflate_lz_batch", deflate_lz_parse_kernel, deflate_lz_write_kernel, data, raw, offsets, offsets_dev, n_chunks, pad,
                            out, out_capacity, out_offsets, coded, workspace, stream, stage_ms);
}

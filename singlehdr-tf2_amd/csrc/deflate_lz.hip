// zlib streams with LZ77 matches for a BATCH of byte chunks on the device: byte for byte what shdr_deflate_lz_host writes
// (deflate_lz.h holds what both share: the parse rules, the symbols, the code lengths and the fixed-length block header).
//
// Passes (stream-ordered, no global atomics, no host wait; the same input gives the same bytes):
//   1  deflate_lz_parse_kernel  ONE 64-lane wave per chunk walks the chunk in groups of 64 positions: every lane that the greedy walk
//                               can still reach looks its position up in the LDS hash table and compares the first 8 bytes of
//                               candidates A and B (probe_at; the group's own bytes are staged in LDS a window of 1024 ahead),
//                               all lanes insert their position (LDS atomicMax: the highest wins), then the walk runs over the group with wave-uniform state (a ballot of the lanes that hold a match, one step
//                               and one v_readlane per match on the way, the literals between them by mask); a token on the
//                               walk's way whose candidates reach beyond 8 bytes is extended by the whole wave, 8 bytes per lane,
//                               so a long match costs one more round of loads and only where it is taken.  One uint32 token
//                               per position goes to the workspace, the starts are counted into the LDS histogram (286 + 30),
//                               Adler-32 as in deflate.hip; then ONE lane builds both codes and stores the lengths, the block's size
//                               in bits and the stored size: the stream if that is strictly smaller than the chunk, else the chunk
//   2  deflate_scan_kernel      (deflate_batch.h) exclusive int64 scan of the stored sizes (+ `pad` in front of each) -> out_offsets
//   3  deflate_lz_write_kernel  one block per chunk: the header, then tiles of kTile POSITIONS (+ end-of-block behind the last): a
//                               position's token is 0..48 bits, a block prefix sum gives each its bit, every token is OR-ed into
//                               LDS words on its own (at most three words), the whole bytes of the tile are stored; partial byte
//                               and bit position carry to the next tile; then the tail and the Adler-32.  A chunk that is not
//                               coded is copied from `raw`.
// LDS of pass 1: 16 KiB table + 1264 B counts + 320 B lengths + 5148 B Huffman scratch + 1032 B window = 24 152 B per 64-thread
// block, so the 160 KiB of a CU hold 6 blocks (6 chunks); pass 3: 320 + 632 + 173 + 6156 (words) + 16 B per 256-thread block.
#include "shdr_internal.h"
#include "deflate_lz.h"
#include "deflate_batch.h"

namespace {

using namespace shdr_deflate_lz;
using namespace shdr_deflate_batch;

constexpr int kThreads = 256;
constexpr int kPerThread = 4;
constexpr int kTile = kThreads * kPerThread;                     // positions per tile of the writer (shdr.h: SHDR_DEFLATE_LZ_TILE)
constexpr int kTileWords = (7 + kTile * kMaxTokenBits) / 32 + 3; // carried bits + the tile's bits, and the words a shifted token spills into
constexpr int kLenStride = 320;                                  // bytes per chunk of the stored code lengths (316 used)
static_assert(kTile == SHDR_DEFLATE_LZ_TILE, "shdr.h names the tile size");
constexpr int kWindow = 16 * kGroup;                             // bytes of the chunk staged in LDS per round: 16 per lane
static_assert(kGroup == 64, "one lane per position of a group");
static_assert(kLiteral == SHDR_DEFLATE_LZ_LITERAL, "shdr.h names the literal flag of a token");

struct Workspace {                                               // carved out of the caller's workspace, every part 16-byte aligned
  uint8_t* lens;                                                 // [C][kLenStride]
  int64_t* bits;                                                 // [C] bits of the block incl. the two zlib bytes in front
  int64_t* sizes;                                                // [C] pad + stored bytes
  uint32_t* adler;                                               // [C]
  uint32_t* tokens;                                              // [total] one per input byte
  int64_t bytes;
};
inline Workspace carve(void* ws, int64_t c, int64_t total) {
  Workspace w;
  char* p = static_cast<char*>(ws);
  int64_t o = 0;
  w.lens = reinterpret_cast<uint8_t*>(p + o);    o += (int64_t)kLenStride * c;
  w.bits = reinterpret_cast<int64_t*>(p + o);    o += align16(8 * c);
  w.sizes = reinterpret_cast<int64_t*>(p + o);   o += align16(8 * c);
  w.adler = reinterpret_cast<uint32_t*>(p + o);  o += align16(4 * c);
  w.tokens = reinterpret_cast<uint32_t*>(p + o); o += align16(4 * total);
  w.bytes = o;
  return w;
}

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
                                                                  int64_t total, int pad, uint32_t* __restrict__ tokens,
                                                                  uint8_t* __restrict__ lens, int64_t* __restrict__ bits_out,
                                                                  int64_t* __restrict__ sizes, uint32_t* __restrict__ adler,
                                                                  uint8_t* __restrict__ coded) {
  __shared__ uint32_t table[kHashSlots];
  __shared__ uint32_t freq[kAllSyms];
  __shared__ uint8_t len[kLenStride];
  __shared__ LzWork work;
  __shared__ uint64_t stage64[kWindow / 8 + 1];                  // a window of the chunk and the 2 bytes behind it
  uint8_t* stage = reinterpret_cast<uint8_t*>(stage64);
  const int64_t c = blockIdx.x;
  int64_t lo, n;
  chunk_range(offsets, c, total, lo, n);
  const int lane = threadIdx.x;
  for (int i = lane; i < kHashSlots; i += kGroup) table[i] = 0;
  for (int i = lane; i < kAllSyms; i += kGroup) freq[i] = i == 256 ? 1u : 0u;
  __syncthreads();
  const uint8_t* src = data + lo;
  uint32_t* tok_out = tokens + lo;
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
  __syncthreads();
  if (lane == 0) {
    build_all_lengths(freq, len, work);
    const int64_t bits = stream_bits(freq, len), stream = stream_bytes(bits);
    const bool use = n > 0 && stream < n;
    bits_out[c] = bits;
    sizes[c] = pad + (use ? stream : n);
    coded[c] = use ? 1 : 0;
    adler[c] = (uint32_t)((((uint64_t)(n % kAdlerMod) + s2) % kAdlerMod) << 16) | (uint32_t)((1 + s1) % kAdlerMod);
  }
  __syncthreads();
  for (int s = lane; s < kLenStride; s += kGroup) lens[c * kLenStride + s] = s < kAllSyms ? len[s] : 0;
}

__global__ __launch_bounds__(kThreads) void deflate_lz_write_kernel(const uint8_t* __restrict__ raw, const int64_t* __restrict__ offsets,
                                                                    int64_t total, int pad, const uint32_t* __restrict__ tokens,
                                                                    const uint8_t* __restrict__ lens, const int64_t* __restrict__ bits_in,
                                                                    const uint32_t* __restrict__ adler, const uint8_t* __restrict__ coded,
                                                                    const int64_t* __restrict__ out_offsets, uint8_t* __restrict__ out,
                                                                    int64_t capacity) {
  __shared__ uint8_t len[kLenStride];
  __shared__ uint16_t code[kAllSyms];
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
    build_all_codes(len, code);
    write_header(len, hdr);
  }
  __syncthreads();
  for (int i = tid; i < kHeaderBytes - 1; i += kThreads) dst[i] = hdr[i];
  const uint32_t* tok = tokens + lo;
  int64_t P = kSymbolsAtBit;                                     // the stream bit of the tile's first token; the same in every thread
  uint32_t carry = hdr[kHeaderBytes - 1];                        // the bits of byte P / 8 that are already decided
  for (int64_t base = 0; base <= n; base += kTile) {             // n positions, then end-of-block
    for (int i = tid; i < kTileWords; i += kThreads) words[i] = i == 0 ? carry : 0u;
    uint64_t v[kPerThread];
    int nbk[kPerThread];
    int nb = 0;
#pragma unroll
    for (int k = 0; k < kPerThread; ++k) {
      const int64_t i = base + (int64_t)tid * kPerThread + k;
      const uint32_t t = i < n ? tok[i] : i == n ? kEndOfBlock : 0u;
      v[k] = 0;
      nbk[k] = t ? token_bits(t, len, code, v[k]) : 0;
      nb += nbk[k];
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
    int rel = (int)(P & 7) + before + incl - nb;                 // bit in `words`, whose bit 0 is bit 0 of byte P / 8
#pragma unroll
    for (int k = 0; k < kPerThread; ++k) {
      if (!nbk[k]) continue;
      const int w = rel >> 5, sh = rel & 31;
      const uint32_t w0 = (uint32_t)(v[k] << sh);                // v has at most 48 bits: 79 after the shift, three words
      const uint64_t hi = sh ? v[k] >> (32 - sh) : v[k] >> 32;
      if (w0) atomicOr(&words[w], w0);                           // LDS; OR commutes, so the order of arrival does not matter
      if ((uint32_t)hi) atomicOr(&words[w + 1], (uint32_t)hi);
      if ((uint32_t)(hi >> 32)) atomicOr(&words[w + 2], (uint32_t)(hi >> 32));
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
    const uint32_t a = adler[c];
    if (P == bits && o + 4 == room) {
      dst[o] = (uint8_t)(a >> 24); dst[o + 1] = (uint8_t)(a >> 16); dst[o + 2] = (uint8_t)(a >> 8); dst[o + 3] = (uint8_t)a;
    }
  }
}

}  // namespace

extern "C" int64_t shdr_deflate_lz_host(const uint8_t* src, int64_t n, uint8_t* dst, int64_t capacity) {
  int64_t need = 0;
  const int64_t r = encode_host(src, n, dst, capacity, &need);
  if (r == -1) {
    shdr::set_error("deflate_lz_host: bad arguments (null pointer, or a chunk outside 1 .. 2^30 bytes)");
    return -1;
  }
  if (r == -2) {
    shdr::set_error("deflate_lz_host: output buffer too small (%lld < %lld)", (long long)capacity, (long long)need);
    return -1;
  }
  if (r == -3) {
    shdr::set_error("deflate_lz_host: no memory for the tokens of %lld bytes", (long long)n);
    return -1;
  }
  return r;
}

extern "C" int shdr_deflate_lz_parse_host(const uint8_t* src, int64_t n, uint32_t* tokens) {
  SHDR_REQUIRE(src && tokens, SHDR_E_NULL, "deflate_lz_parse_host: null pointer");
  SHDR_REQUIRE(n >= 1 && n <= kMaxChunk, SHDR_E_SHAPE, "deflate_lz_parse_host: a chunk has 1 .. 2^30 bytes, got %lld", (long long)n);
  uint32_t table[kHashSlots];
  parse_host(src, n, tokens, table);
  return SHDR_OK;
}

extern "C" int shdr_deflate_lz_batch_sizes(const int64_t* offsets, int n_chunks, int pad, int64_t* out_bytes, int64_t* workspace_bytes) {
  int64_t total = 0, bound = 0;
  if (int rc = check_offsets("deflate_lz_batch_sizes", offsets, n_chunks, pad, &total, &bound)) return rc;
  if (out_bytes) *out_bytes = bound;
  if (workspace_bytes) *workspace_bytes = carve(nullptr, n_chunks, total).bytes;
  return SHDR_OK;
}

extern "C" int shdr_deflate_lz_batch(const uint8_t* data, const uint8_t* raw, const int64_t* offsets, const int64_t* offsets_dev,
                                     int n_chunks, int pad, uint8_t* out, int64_t out_capacity, int64_t* out_offsets, uint8_t* coded,
                                     void* workspace, void* stream, float* stage_ms) {
  const char* what = "deflate_lz_batch";
  SHDR_REQUIRE(data && offsets_dev && out && out_offsets && coded && workspace, SHDR_E_NULL, "%s: null pointer", what);
  int64_t total = 0, bound = 0;
  if (int rc = check_offsets(what, offsets, n_chunks, pad, &total, &bound)) return rc;
  SHDR_REQUIRE((reinterpret_cast<uintptr_t>(offsets_dev) & 7u) == 0 && (reinterpret_cast<uintptr_t>(out_offsets) & 7u) == 0, SHDR_E_ALIGN,
               "%s: offsets_dev and out_offsets must be 8-byte aligned", what);
  SHDR_REQUIRE(shdr::aligned16(workspace), SHDR_E_ALIGN, "%s: workspace must be 16-byte aligned", what);
  SHDR_REQUIRE(out_capacity >= bound, SHDR_E_SHAPE, "%s: output buffer too small (%lld < %lld)", what, (long long)out_capacity, (long long)bound);
  const Workspace w = carve(workspace, n_chunks, total);
  hipStream_t st = S(stream);
  hipEvent_t ev[SHDR_DEFLATE_STAGES + 1] = {};
  if (stage_ms)
    for (auto& e : ev) SHDR_REQUIRE(hipEventCreate(&e) == hipSuccess, SHDR_E_LAUNCH, "%s: hipEventCreate failed", what);
  auto mark = [&](int i) { if (stage_ms) (void)hipEventRecord(ev[i], st); };
  mark(0);
  hipLaunchKernelGGL(deflate_lz_parse_kernel, dim3((unsigned)n_chunks), dim3(kGroup), 0, st, data, offsets_dev, total, pad, w.tokens, w.lens,
                     w.bits, w.sizes, w.adler, coded);
  mark(1);
  hipLaunchKernelGGL(deflate_scan_kernel, dim3(1), dim3(1024), 0, st, w.sizes, (int64_t)n_chunks, out_offsets);
  mark(2);
  hipLaunchKernelGGL(deflate_lz_write_kernel, dim3((unsigned)n_chunks), dim3(kThreads), 0, st, raw ? raw : data, offsets_dev, total, pad,
                     w.tokens, w.lens, w.bits, w.adler, coded, out_offsets, out, out_capacity);
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

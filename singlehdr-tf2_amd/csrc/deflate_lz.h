// zlib streams with LZ77 matches (RFC 1950 / 1951): the parts that the host routine shdr_deflate_lz_host and the device kernels
// (csrc/deflate_lz.hip) share, so that the device bytes are the host bytes.  Plain C++: also compiled without HIP.
//
// A stream is  78 01 | ONE final dynamic-Huffman block of literals, lengths and distances | Adler-32 of the chunk, big-endian.
//
// THE PARSE is a pure function of the chunk's bytes that 64 lanes can evaluate side by side:
//   * positions are handled in aligned groups of 64 (group g holds positions 64 g .. 64 g + 63);
//   * a table of 2^12 slots holds one position each, no chains.  The slot of position q is hash3 of the bytes q, q + 1, q + 2
//     (so q + 2 must lie in the chunk); the positions of a group are inserted AFTER the group's lookups and the highest position
//     wins a slot.  Candidate A of position p is therefore the most recent position before the start of p's group with p's slot;
//     it is refused when it lies more than 32768 back;
//   * candidate B is p - 1, a run: without it a 64-wide snapshot misses the zero runs that the delta predictor produces;
//   * a match is the common prefix of the bytes at p and at the candidate, at most 258 bytes and never past the chunk's end; less
//     than 3 bytes are no match, and a 3-byte match further than 4096 back is refused (it costs more than three literals);
//   * the longer candidate wins, B on a tie (the smaller distance);
//   * the parse is greedy from position 0: a token starts where the previous one ended, a position without a match is a literal.
// No hash chains, no lazy matching: where zlib finds an older, longer match or defers a match by one byte, this parse does not.
//
// THE CODE: build_lengths_n of deflate_huffman.h over the 286 literal/length counts (end-of-block counts once) and over the 30
// distance counts.  No match in the chunk: all 30 distance lengths are 0.  One distance code in use: its length is 1, the one
// incomplete set that zlib's inflate accepts.  Two or more: a Huffman tree, Kraft sum exactly 1.  Length 258 is symbol 285.
// The block header has a fixed length: HLIT = 29 (286 codes), HDIST = 29 (30 codes), HCLEN = 15, the 19 code-length-code lengths
// are 4 for symbols 0..15 and 0 for 16..18, and the 316 code lengths follow as 4 bits each, never run-length coded:
// 17 + 57 + 1264 = 1338 bits, the symbols start at bit 1354.
//
// TOKENS: one uint32 per position of the chunk -- 0 where an earlier match covers the position, kLiteral | byte for a literal,
// length << 16 | distance for a match (length 3..258, distance 1..32768).
#pragma once
#include "deflate_huffman.h"

#include <new>

namespace shdr_deflate_lz {

using shdr_deflate::BitPut;
using shdr_deflate::HuffWorkT;
using shdr_deflate::kAdlerMod;
using shdr_deflate::kMaxBits;
using shdr_deflate::kMaxChunk;
using shdr_deflate::stream_bytes;

constexpr int kLitSyms = 286;                 // literals 0..255, end-of-block, length codes 257..285
constexpr int kDistSyms = 30;
constexpr int kAllSyms = kLitSyms + kDistSyms;  // the order of the stored lengths: literal/length, then distance
constexpr int kSymbolsAtBit = 1354;           // 16 + 17 + 57 + 4 * 316
constexpr int kHeaderBytes = 170;             // bytes that hold bits 0..1353; the last one holds 2 of them
constexpr int kGroup = 64;
constexpr int kHashBits = 12;
constexpr int kHashSlots = 1 << kHashBits;
constexpr int kMinMatch = 3, kMaxMatch = 258;
constexpr int kMaxDist = 32768;
constexpr int kShortMatchDist = 4096;         // a 3-byte match further back is refused
constexpr int kMaxTokenBits = 15 + 5 + 15 + 13;
constexpr uint32_t kLiteral = 0x80000000u;
constexpr uint32_t kEndOfBlock = kLiteral | 256u;   // the writer's token behind the last position

union LzWork {                                // scratch of the two build_lengths_n calls, one after the other
  HuffWorkT<kLitSyms> lit;
  HuffWorkT<kDistSyms> dist;
};

// ---- the parse --------------------------------------------------------------------------------------------------------------
SHDR_HD inline uint32_t hash3(uint32_t b0, uint32_t b1, uint32_t b2) {
  return ((b0 | (b1 << 8) | (b2 << 16)) * 2654435761u) >> (32 - kHashBits);
}

// length of the common prefix of a[0 .. maxlen) and b[0 .. maxlen), 8 bytes at a time (both little-endian machines)
SHDR_HD inline int match_length(const uint8_t* a, const uint8_t* b, int maxlen, int i = 0) {   // i: bytes known to be equal
  while (i + 8 <= maxlen) {
    uint64_t x, y;
    __builtin_memcpy(&x, a + i, 8);
    __builtin_memcpy(&y, b + i, 8);
    if (x != y) return i + (__builtin_ctzll(x ^ y) >> 3);
    i += 8;
  }
  while (i < maxlen && a[i] == b[i]) ++i;
  return i;
}

// What position p knows after ONE round of loads.  slot: what the table holds for p's hash (a position + 1, or 0 for none) BEFORE p's
// group is inserted.  maxlen: the longest match the chunk's end allows; da: candidate A's distance, 0 for none within reach; la, lb:
// bytes that p has in common with candidates A and B (p - 1) -- all of them when maxlen <= 8, else of the first 8 (kProbe) only,
// and a candidate that reaches 8 goes on (extend_match)
constexpr int kProbe = 8;
SHDR_HD inline void probe_at(const uint8_t* src, int64_t n, int64_t p, uint32_t slot, int& maxlen, int& da, int& la, int& lb) {
  const int64_t rest = n - p;
  maxlen = rest < kMaxMatch ? (int)rest : kMaxMatch;
  const int64_t d = slot ? p - ((int64_t)slot - 1) : 0;
  da = d >= 1 && d <= kMaxDist ? (int)d : 0;
  la = lb = 0;
  if (maxlen >= kProbe) {
    uint64_t x, ya, yb;
    __builtin_memcpy(&x, src + p, 8);
    ya = yb = ~x;                                                // no candidate: not one byte in common
    if (da) __builtin_memcpy(&ya, src + p - da, 8);
    if (p >= 1) __builtin_memcpy(&yb, src + p - 1, 8);
    la = x == ya ? kProbe : __builtin_ctzll(x ^ ya) >> 3;
    lb = x == yb ? kProbe : __builtin_ctzll(x ^ yb) >> 3;
  } else if (maxlen >= kMinMatch) {
    if (da) la = match_length(src + p, src + p - da, maxlen);
    if (p >= 1) lb = match_length(src + p, src + p - 1, maxlen);
  }
}
SHDR_HD inline bool probe_is_open(int maxlen, int la, int lb) { return maxlen > kProbe && (la == kProbe || lb == kProbe); }

// the token of a position with byte `byte` from the full lengths of its candidates: the longer wins, B on a tie
SHDR_HD inline uint32_t choose_token(uint32_t byte, int la, int da, int lb) {
  if (la < kMinMatch || (la == kMinMatch && da > kShortMatchDist)) la = 0;
  if (lb < kMinMatch) lb = 0;
  if (lb >= la) return lb ? ((uint32_t)lb << 16) | 1u : kLiteral | byte;
  return ((uint32_t)la << 16) | (uint32_t)da;
}

// The token that starts at position p
SHDR_HD inline uint32_t token_at(const uint8_t* src, int64_t n, int64_t p, uint32_t slot) {
  int maxlen, da, la, lb;
  probe_at(src, n, p, slot, maxlen, da, la, lb);
  if (probe_is_open(maxlen, la, lb)) {
    if (la == kProbe) la = match_length(src + p, src + p - da, maxlen, kProbe);
    if (lb == kProbe) lb = match_length(src + p, src + p - 1, maxlen, kProbe);
  }
  return choose_token(src[p], la, da, lb);
}

SHDR_HD inline bool token_is_literal(uint32_t t) { return (t & kLiteral) != 0; }
SHDR_HD inline int token_length(uint32_t t) { return (int)(t >> 16); }             // of a match
SHDR_HD inline int token_distance(uint32_t t) { return (int)(t & 0xFFFFu); }

// ---- symbols ----------------------------------------------------------------------------------------------------------------
// length 3..258 -> its code 257..285, the number of extra bits and their value (RFC 1951 section 3.2.5)
SHDR_HD inline void length_symbol(int length, int& sym, int& extra_bits, uint32_t& extra) {
  const uint32_t m = (uint32_t)(length - kMinMatch);
  if (length == kMaxMatch) { sym = 285; extra_bits = 0; extra = 0; return; }
  if (m < 8) { sym = 257 + (int)m; extra_bits = 0; extra = 0; return; }
  const int e = 31 - __builtin_clz(m) - 2;
  sym = 257 + 4 * (e + 1) + (int)((m >> e) & 3u);
  extra_bits = e;
  extra = m & ((1u << e) - 1u);
}
// distance 1..32768 -> its code 0..29
SHDR_HD inline void distance_symbol(int distance, int& sym, int& extra_bits, uint32_t& extra) {
  const uint32_t m = (uint32_t)(distance - 1);
  if (m < 4) { sym = (int)m; extra_bits = 0; extra = 0; return; }
  const int hb = 31 - __builtin_clz(m), e = hb - 1;
  sym = 2 * hb + (int)((m >> e) & 1u);
  extra_bits = e;
  extra = m & ((1u << e) - 1u);
}
SHDR_HD inline int length_extra_bits(int sym) { return sym < 265 || sym == 285 ? 0 : (sym - 261) >> 2; }
SHDR_HD inline int distance_extra_bits(int sym) { return sym < 4 ? 0 : (sym - 2) >> 1; }

// the bits of one token, first bit at bit 0; returns their number (at most kMaxTokenBits).  len/code: literal/length symbols at
// 0..285, distance symbols at kLitSyms..kLitSyms + 29
SHDR_HD inline int token_bits(uint32_t t, const uint8_t* len, const uint16_t* code, uint64_t& v) {
  if (token_is_literal(t)) {
    const int s = (int)(t & 0x1FFu);
    v = code[s];
    return len[s];
  }
  int ls, le, ds, de;
  uint32_t lx, dx;
  length_symbol(token_length(t), ls, le, lx);
  distance_symbol(token_distance(t), ds, de, dx);
  ds += kLitSyms;
  int nb = 0;
  v = code[ls];
  nb += len[ls];
  v |= (uint64_t)lx << nb;
  nb += le;
  v |= (uint64_t)code[ds] << nb;
  nb += len[ds];
  v |= (uint64_t)dx << nb;
  nb += de;
  return nb;
}

// freq[0 .. 316) of a token that starts a symbol
SHDR_HD inline void token_symbols(uint32_t t, int& lit_sym, int& dist_sym) {
  if (token_is_literal(t)) {
    lit_sym = (int)(t & 0x1FFu);
    dist_sym = -1;
    return;
  }
  int e;
  uint32_t x;
  length_symbol(token_length(t), lit_sym, e, x);
  distance_symbol(token_distance(t), dist_sym, e, x);
}

// ---- the code and the header --------------------------------------------------------------------------------------------------
// len[0 .. 316) from freq[0 .. 316)
SHDR_HD inline void build_all_lengths(const uint32_t* freq, uint8_t* len, LzWork& work) {
  shdr_deflate::build_lengths_n<kLitSyms>(freq, len, work.lit);
  shdr_deflate::build_lengths_n<kDistSyms>(freq + kLitSyms, len + kLitSyms, work.dist);
}
SHDR_HD inline void build_all_codes(const uint8_t* len, uint16_t* code) {
  shdr_deflate::build_codes_n<kLitSyms>(len, code);
  shdr_deflate::build_codes_n<kDistSyms>(len + kLitSyms, code + kLitSyms);
}

// bits 0..1353 of the stream into hdr[0..169]; hdr[169] holds bits 1352 and 1353 in its low bits, the rest of it is zero
SHDR_HD inline void write_header(const uint8_t* len, uint8_t* hdr) {
  const uint8_t order[19] = {16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15};
  const uint8_t rev4[16] = {0, 8, 4, 12, 2, 10, 6, 14, 1, 9, 5, 13, 3, 11, 7, 15};
  BitPut b{hdr, 0, 0, 0};
  b.put(0x78, 8);
  b.put(0x01, 8);
  b.put(1, 1);                                                   // BFINAL
  b.put(2, 2);                                                   // BTYPE: dynamic Huffman
  b.put(kLitSyms - 257, 5);                                      // HLIT:  286 codes
  b.put(kDistSyms - 1, 5);                                       // HDIST: 30 codes
  b.put(15, 4);                                                  // HCLEN: 19 lengths
  for (int i = 0; i < 19; ++i) b.put(order[i] <= 15 ? 4 : 0, 3);
  for (int s = 0; s < kAllSyms; ++s) b.put(rev4[len[s]], 4);
  hdr[b.at] = (uint8_t)b.acc;                                    // b.at == 169, b.cnt == 2
}

// bits of the whole block, header and end-of-block included, counted from the first byte of the stream
SHDR_HD inline int64_t stream_bits(const uint32_t* freq, const uint8_t* len) {
  int64_t bits = kSymbolsAtBit;
  for (int s = 0; s < kLitSyms; ++s) bits += (int64_t)freq[s] * (len[s] + (s > 256 ? length_extra_bits(s) : 0));
  for (int s = 0; s < kDistSyms; ++s) bits += (int64_t)freq[kLitSyms + s] * (len[kLitSyms + s] + distance_extra_bits(s));
  return bits;
}

// ---- host side ----------------------------------------------------------------------------------------------------------------
// tokens[0 .. n) of src[0 .. n); `table` is scratch of kHashSlots words
inline void parse_host(const uint8_t* src, int64_t n, uint32_t* tokens, uint32_t* table) {
  for (int i = 0; i < kHashSlots; ++i) table[i] = 0;
  int64_t pos = 0;
  for (int64_t base = 0; base < n; base += kGroup) {
    const int64_t end = base + kGroup < n ? base + kGroup : n;
    for (int64_t p = base; p < end; ++p) tokens[p] = 0;
    while (pos < end) {
      const uint32_t slot = pos + 2 < n ? table[hash3(src[pos], src[pos + 1], src[pos + 2])] : 0u;
      const uint32_t t = token_at(src, n, pos, slot);
      tokens[pos] = t;
      pos += token_is_literal(t) ? 1 : token_length(t);
    }
    for (int64_t p = base; p < end && p + 2 < n; ++p) table[hash3(src[p], src[p + 1], src[p + 2])] = (uint32_t)(p + 1);
  }
}

// The stream of src[0..n) into dst; returns its length, -1 for bad arguments, -2 when `capacity` is less than that length (then
// *need, if given, receives it and nothing is written), -3 when the token scratch (4 n bytes) cannot be allocated.
// *stream_bits_out: as in deflate_huffman.h.
inline int64_t encode_host(const uint8_t* src, int64_t n, uint8_t* dst, int64_t capacity, int64_t* need, int64_t* stream_bits_out = nullptr) {
  if (!src || !dst || n < 1 || n > kMaxChunk) return -1;
  uint32_t* tokens = new (std::nothrow) uint32_t[(size_t)n + kHashSlots];
  if (!tokens) return -3;
  parse_host(src, n, tokens, tokens + n);
  uint32_t freq[kAllSyms];
  uint8_t len[kAllSyms];
  uint16_t code[kAllSyms];
  LzWork work;
  for (int s = 0; s < kAllSyms; ++s) freq[s] = 0;
  freq[256] = 1;
  for (int64_t i = 0; i < n; ++i) {
    if (!tokens[i]) continue;
    int ls, ds;
    token_symbols(tokens[i], ls, ds);
    ++freq[ls];
    if (ds >= 0) ++freq[kLitSyms + ds];
  }
  build_all_lengths(freq, len, work);
  build_all_codes(len, code);
  const int64_t bits = stream_bits(freq, len), total = stream_bytes(bits);
  if (need) *need = total;
  if (stream_bits_out) *stream_bits_out = bits;
  if (capacity < total) {
    delete[] tokens;
    return -2;
  }
  write_header(len, dst);
  BitPut b{dst, kHeaderBytes - 1, dst[kHeaderBytes - 1], kSymbolsAtBit & 7};
  for (int64_t i = 0; i <= n; ++i) {
    const uint32_t t = i < n ? tokens[i] : kEndOfBlock;
    if (!t) continue;
    uint64_t v;
    const int nb = token_bits(t, len, code, v);
    b.put((uint32_t)(v & 0xFFFFFFu), nb < 24 ? nb : 24);          // BitPut holds 7 + 32 bits at the most
    if (nb > 24) b.put((uint32_t)(v >> 24), nb - 24);
  }
  delete[] tokens;
  if (b.cnt) dst[b.at++] = (uint8_t)b.acc;
  const uint32_t a = shdr_deflate::adler32_host(src, n);
  dst[b.at++] = (uint8_t)(a >> 24);
  dst[b.at++] = (uint8_t)(a >> 16);
  dst[b.at++] = (uint8_t)(a >> 8);
  dst[b.at++] = (uint8_t)a;
  return b.at;                                                   // == total
}

}  // namespace shdr_deflate_lz

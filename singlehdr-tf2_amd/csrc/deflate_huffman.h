// Huffman-only zlib streams (RFC 1950 / 1951): the parts that the host routine shdr_deflate_huffman_host and the device kernels
// (csrc/deflate.hip) share, so that the device bytes are the host bytes.  Plain C++: also compiled without HIP.
//
// A stream is  78 01 | ONE final dynamic-Huffman block, literals only | Adler-32 of the chunk, big-endian.  The block header has a
// fixed length: HLIT = 0 (257 literal/length codes), HDIST = 0 (one distance code, of length 0: "no distances"), HCLEN = 15, the 19
// code-length-code lengths are 4 for symbols 0..15 and 0 for 16..18 -- a complete code in which length L is the 4-bit code L -- and
// the 258 code lengths follow as 4 bits each, never run-length coded: 17 + 57 + 1032 = 1106 bits, the symbols start at bit 1122.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define SHDR_HD __host__ __device__
#else
#define SHDR_HD
#endif

namespace shdr_deflate {

constexpr int kSyms = 257;                    // literals 0..255 and end-of-block
constexpr int kMaxBits = 15;
constexpr int kSymbolsAtBit = 1122;           // 16 + 1106
constexpr int kHeaderBytes = 141;             // bytes that hold bits 0..1121; the last one holds 2 of them
constexpr int64_t kMaxChunk = (int64_t)1 << 30;
constexpr uint32_t kAdlerMod = 65521;

template <int N>
struct HuffWorkT {                            // scratch of build_lengths over N symbols: LDS on the device, the stack on the host
  uint32_t w[2 * N];                          // weights: sorted leaves 0..n-1, then the internal nodes in the order they are made
  uint16_t sym[N];
  uint16_t parent[2 * N];
  uint16_t depth[2 * N];
};
using HuffWork = HuffWorkT<kSyms>;

// Code lengths of the symbols with freq != 0 (0 for the others): Huffman's algorithm on the used symbols, ties broken by
// (weight, symbol) and leaves before internal nodes; while the deepest leaf lies below 15 the weights are halved (rounded up, so
// none reaches 0) and the tree is rebuilt.  A Huffman tree is full, so the lengths are complete (Kraft sum 1) whenever two or more
// symbols occur; equal weights end at depth <= 9, so the loop ends.  One symbol alone gets length 1.  The alphabet's size is a
// template argument (deflate_lz.h codes 286 literal/length and 30 distance symbols by the same rule); the sort's result does not
// depend on its gaps, since (weight, symbol) is a total order.
template <int N>
SHDR_HD inline void build_lengths_n(const uint32_t* freq, uint8_t* len, HuffWorkT<N>& k) {
  int n = 0;
  for (int s = 0; s < N; ++s) {
    len[s] = 0;
    if (freq[s]) {
      k.sym[n] = (uint16_t)s;
      k.w[n] = freq[s];
      ++n;
    }
  }
  if (n == 0) return;
  if (n == 1) {
    len[k.sym[0]] = 1;
    return;
  }
  // Shell sort by weight; symbols arrive in increasing order and equal weights keep it only per gap pass, so compare (weight, symbol)
  const int gaps[6] = {132, 57, 23, 10, 4, 1};
  for (int g = 0; g < 6; ++g) {
    const int gap = gaps[g];
    for (int i = gap; i < n; ++i) {
      const uint32_t wi = k.w[i];
      const uint16_t si = k.sym[i];
      int j = i;
      while (j >= gap && (k.w[j - gap] > wi || (k.w[j - gap] == wi && k.sym[j - gap] > si))) {
        k.w[j] = k.w[j - gap];
        k.sym[j] = k.sym[j - gap];
        j -= gap;
      }
      k.w[j] = wi;
      k.sym[j] = si;
    }
  }
  for (;;) {
    int leaf = 0, node = n;                                      // heads of the two queues; both are in non-decreasing order
    for (int m = n; m < 2 * n - 1; ++m) {
      uint32_t sum = 0;
      for (int t = 0; t < 2; ++t) {
        int a;
        if (leaf < n && (node >= m || k.w[leaf] <= k.w[node])) a = leaf++;
        else a = node++;
        sum += k.w[a];
        k.parent[a] = (uint16_t)m;
      }
      k.w[m] = sum;
    }
    k.depth[2 * n - 2] = 0;
    int deepest = 0;
    for (int i = 2 * n - 3; i >= 0; --i) {                       // a parent is made after its children: its index is larger
      k.depth[i] = (uint16_t)(k.depth[k.parent[i]] + 1);
      if (i < n && k.depth[i] > deepest) deepest = k.depth[i];
    }
    if (deepest <= kMaxBits) break;
    for (int i = 0; i < n; ++i) k.w[i] = (k.w[i] + 1) >> 1;      // monotone: the leaves stay sorted
  }
  for (int i = 0; i < n; ++i) len[k.sym[i]] = (uint8_t)k.depth[i];
}
SHDR_HD inline void build_lengths(const uint32_t* freq, uint8_t* len, HuffWork& k) { build_lengths_n<kSyms>(freq, len, k); }

// Canonical codes of RFC 1951 section 3.2.2, bit-reversed: a stream takes Huffman codes from their most significant bit, and the
// writers put bit 0 of a value first.
template <int N>
SHDR_HD inline void build_codes_n(const uint8_t* len, uint16_t* code) {
  uint16_t count[kMaxBits + 1], next[kMaxBits + 1];
  for (int b = 0; b <= kMaxBits; ++b) count[b] = 0;
  for (int s = 0; s < N; ++s) ++count[len[s]];
  count[0] = 0;
  uint32_t c = 0;
  next[0] = 0;
  for (int b = 1; b <= kMaxBits; ++b) {
    c = (c + count[b - 1]) << 1;
    next[b] = (uint16_t)c;
  }
  for (int s = 0; s < N; ++s) {
    const int l = len[s];
    uint32_t v = 0;
    if (l) {
      const uint32_t x = next[l]++;
      for (int b = 0; b < l; ++b) v |= ((x >> b) & 1u) << (l - 1 - b);
    }
    code[s] = (uint16_t)v;
  }
}
SHDR_HD inline void build_codes(const uint8_t* len, uint16_t* code) { build_codes_n<kSyms>(len, code); }

// values go into the stream from their bit 0, bytes fill from their bit 0
struct BitPut {
  uint8_t* p;
  int64_t at;
  uint64_t acc;
  int cnt;
  SHDR_HD inline void put(uint32_t v, int bits) {
    acc |= (uint64_t)v << cnt;
    cnt += bits;
    while (cnt >= 8) {
      p[at++] = (uint8_t)(acc & 255u);
      acc >>= 8;
      cnt -= 8;
    }
  }
};

// bits 0..1121 of the stream into hdr[0..140]; hdr[140] holds bits 1120 and 1121 in its low bits, the rest of it is zero
SHDR_HD inline void write_header(const uint8_t* len, uint8_t* hdr) {
  const uint8_t order[19] = {16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15};
  const uint8_t rev4[16] = {0, 8, 4, 12, 2, 10, 6, 14, 1, 9, 5, 13, 3, 11, 7, 15};
  BitPut b{hdr, 0, 0, 0};
  b.put(0x78, 8);
  b.put(0x01, 8);
  b.put(1, 1);                                                   // BFINAL
  b.put(2, 2);                                                   // BTYPE: dynamic Huffman
  b.put(0, 5);                                                   // HLIT:  257 codes
  b.put(0, 5);                                                   // HDIST: 1 code
  b.put(15, 4);                                                  // HCLEN: 19 lengths
  for (int i = 0; i < 19; ++i) b.put(order[i] <= 15 ? 4 : 0, 3);
  for (int s = 0; s < kSyms; ++s) b.put(rev4[len[s]], 4);
  b.put(rev4[0], 4);                                             // the distance code: length 0
  hdr[b.at] = (uint8_t)b.acc;                                    // b.at == 140, b.cnt == 2
}

// bits of the whole block, header and end-of-block included, counted from the first byte of the stream
SHDR_HD inline int64_t stream_bits(const uint32_t* freq, const uint8_t* len) {
  int64_t bits = kSymbolsAtBit;
  for (int s = 0; s < kSyms; ++s) bits += (int64_t)freq[s] * len[s];
  return bits;
}
SHDR_HD inline int64_t stream_bytes(int64_t bits) { return (bits + 7) / 8 + 4; }

// ---- host side ------------------------------------------------------------------------------------------------------------
inline void histogram_host(const uint8_t* src, int64_t n, uint32_t* freq) {
  for (int s = 0; s < kSyms; ++s) freq[s] = 0;
  for (int64_t i = 0; i < n; ++i) ++freq[src[i]];
  freq[256] = 1;
}

inline uint32_t adler32_host(const uint8_t* src, int64_t n) {
  uint64_t s1 = 1, s2 = 0;
  for (int64_t i = 0; i < n;) {
    const int64_t end = i + 4096 < n ? i + 4096 : n;
    for (; i < end; ++i) {
      s1 += src[i];
      s2 += s1;
    }
    s1 %= kAdlerMod;
    s2 %= kAdlerMod;
  }
  return (uint32_t)((s2 << 16) | s1);
}

// The stream of src[0..n) into dst; returns its length, -1 for bad arguments, -2 when `capacity` is less than that length (then
// *need, if given, receives it and nothing is written).  *stream_bits_out, if given: the bits in front of the padding and the
// Adler-32 (png.h cuts its segments there).
inline int64_t encode_host(const uint8_t* src, int64_t n, uint8_t* dst, int64_t capacity, int64_t* need, int64_t* stream_bits_out = nullptr) {
  if (!src || !dst || n < 1 || n > kMaxChunk) return -1;
  uint32_t freq[kSyms];
  uint8_t len[kSyms];
  uint16_t code[kSyms];
  HuffWork work;
  histogram_host(src, n, freq);
  build_lengths(freq, len, work);
  build_codes(len, code);
  const int64_t bits = stream_bits(freq, len), total = stream_bytes(bits);
  if (need) *need = total;
  if (stream_bits_out) *stream_bits_out = bits;
  if (capacity < total) return -2;
  write_header(len, dst);
  BitPut b{dst, kHeaderBytes - 1, dst[kHeaderBytes - 1], kSymbolsAtBit & 7};
  for (int64_t i = 0; i < n; ++i) b.put(code[src[i]], len[src[i]]);
  b.put(code[256], len[256]);
  if (b.cnt) dst[b.at++] = (uint8_t)b.acc;
  const uint32_t a = adler32_host(src, n);
  dst[b.at++] = (uint8_t)(a >> 24);
  dst[b.at++] = (uint8_t)(a >> 16);
  dst[b.at++] = (uint8_t)(a >> 8);
  dst[b.at++] = (uint8_t)a;
  return b.at;                                                   // == total
}

}  // namespace shdr_deflate

// PNG files (ISO/IEC 15948) of 8-bit grey, RGB and RGBA images: the rules that the host twin shdr_png_encode_host and the device
// kernels (csrc/png_enc.hip, and the segment framing of csrc/deflate_batch.h) share, so that the device bytes are the host bytes.
// Plain C++: also compiled without HIP (tools/png_enc_sweep.cpp).
//
// COLOUR TYPES: bit depth 8, no interlace; C = 1 grey (type 0), C = 3 RGB (type 2), C = 4 RGBA (type 6).  H >= 1, W >= 1 and
// H (W C + 1) < 2^31.  No 16-bit samples, no palettes, no ancillary chunks.
//
// FILTERING: a scanline is one filter-type byte and W C filtered bytes, bpp = C.  x is the byte, a the one bpp to its left, b the one
// above, c the one above a; bytes left of the row and the row above row 0 are zero.  None x, Sub x - a, Up x - b, Average
// x - floor((a + b) / 2) on the 9-bit sum, Paeth x - (the one of a, b, c nearest to a + b - c, ties in that order), all mod 256.
// Adaptive: per row the type whose filtered bytes, read as signed 8-bit, have the smallest sum of absolute values; the lowest type
// number on a tie.  The predictors read RAW bytes, so every row is independent of every other.
//
// SEGMENTS: an image's filtered stream is cut every kPngSegment = 65520 bytes (a multiple of 16 that fits the 16-bit LEN of a stored
// block), whatever the rows; the last segment is shorter.  The stream is ONE zlib stream of independent segments, as Z_SYNC_FLUSH
// writes it: 78 01 in front; a coded segment is the dynamic-Huffman block of the chosen deflate encoder, BFINAL = 1 only in the image's
// last segment, which is zero-padded to a byte, every other one followed by an empty stored block (bits 0 00, zero bits to the byte
// boundary, 00 00 FF FF); a stored segment is one aligned stored block (00 or 01, LEN, NLEN, the bytes).  A segment is coded only if
// its coded bytes, the sync marker included, are strictly fewer than n + 5.  The big-endian Adler-32 of the whole filtered stream
// follows the last segment.
//
// CHUNKS: signature, IHDR, one IDAT per segment (the first carries the two zlib bytes, the last the Adler-32), IEND.  Every chunk ends
// in the CRC-32 of its tag and data (IEEE, reflected, 0xEDB88320).
#pragma once
#include <stdint.h>
#include <string.h>

#include <new>

#include "deflate_huffman.h"
#include "deflate_lz.h"

namespace shdr_png {

using shdr_deflate::kAdlerMod;

constexpr int kPngSegment = 65520;
constexpr int kNone = 0, kSub = 1, kUp = 2, kAverage = 3, kPaeth = 4, kAdaptive = 5;   // shdr.h: SHDR_PNG_FILTER_*
constexpr int kHuffman = 0, kLz = 1;                                                   // shdr.h: SHDR_PNG_DEFLATE_*
constexpr int kFirst = 1, kLast = 2;          // a segment's flags: the image's first, the image's last
constexpr int kHead = 8 + 25;                 // signature and IHDR
constexpr int kIend = 12;
constexpr uint32_t kCrcPoly = 0xEDB88320u;

SHDR_HD inline int colour_type(int c) { return c == 1 ? 0 : c == 3 ? 2 : c == 4 ? 6 : -1; }
SHDR_HD inline int64_t stream_bytes(int64_t h, int64_t w, int64_t c) { return h * (w * c + 1); }
SHDR_HD inline int64_t segments(int64_t stream) { return (stream + kPngSegment - 1) / kPngSegment; }
SHDR_HD inline bool shape_ok(int64_t h, int64_t w, int64_t c) {
  return colour_type((int)c) >= 0 && h >= 1 && w >= 1 && h < ((int64_t)1 << 31) && w < ((int64_t)1 << 31) &&
         stream_bytes(h, w, c) < ((int64_t)1 << 31);
}
// no file is larger: every segment stored
SHDR_HD inline int64_t file_bound(int64_t stream) { return kHead + kIend + 6 + stream + (5 + 12) * segments(stream); }

// ---- filtering ----------------------------------------------------------------------------------------------------------------
SHDR_HD inline int paeth(int a, int b, int c) {
  const int p = a + b - c;
  const int pa = p > a ? p - a : a - p, pb = p > b ? p - b : b - p, pc = p > c ? p - c : c - p;
  return pa <= pb && pa <= pc ? a : pb <= pc ? b : c;
}
SHDR_HD inline uint8_t filtered(int type, int x, int a, int b, int c) {
  const int pred = type == kSub ? a : type == kUp ? b : type == kAverage ? (a + b) >> 1 : type == kPaeth ? paeth(a, b, c) : 0;
  return (uint8_t)(x - pred);
}
SHDR_HD inline uint32_t cost(uint8_t f) { return f < 128 ? f : 256u - f; }      // |f| of f read as signed 8-bit
// the type of the smallest cost, the lowest number on a tie
SHDR_HD inline int cheapest(const uint64_t* costs) {
  int best = 0;
  for (int t = 1; t < 5; ++t)
    if (costs[t] < costs[best]) best = t;
  return best;
}

// ---- what a segment takes in the file (csrc/deflate_batch.h writes the bodies, csrc/png_enc.hip what stands around them) ---------
SHDR_HD inline int seg_front(int flags) { return ((flags & kFirst) ? kHead + 2 : 0) + 8; }           // [head] length tag [78 01]
SHDR_HD inline int seg_back(int flags) { return ((flags & kLast) ? 4 + kIend : 0) + 4; }             // [Adler-32] CRC [IEND]
// bytes of a coded segment whose block has block_bits bits (the zlib bytes of the encoders' own count taken off)
SHDR_HD inline int64_t coded_bytes(int64_t block_bits, bool last) { return last ? (block_bits + 7) / 8 : (block_bits + 3 + 7) / 8 + 4; }
SHDR_HD inline bool use_coded(int64_t coded, int64_t n) { return coded < n + 5; }
SHDR_HD inline void put_stored_header(uint8_t* p, int64_t n, bool last) {
  p[0] = last ? 1 : 0;
  p[1] = (uint8_t)n;
  p[2] = (uint8_t)(n >> 8);
  p[3] = (uint8_t)~n;
  p[4] = (uint8_t)(~n >> 8);
}
SHDR_HD inline void put_be32(uint8_t* p, uint32_t v) {
  p[0] = (uint8_t)(v >> 24);
  p[1] = (uint8_t)(v >> 16);
  p[2] = (uint8_t)(v >> 8);
  p[3] = (uint8_t)v;
}

// Adler-32 of A B from those of A and B and B's length: a = a1 + a2 - 1, b = b1 + b2 + len2 (a1 - 1), mod 65521
SHDR_HD inline uint32_t adler_combine(uint32_t x, uint32_t y, int64_t len2) {
  const uint64_t a1 = x & 0xFFFFu, b1 = x >> 16, a2 = y & 0xFFFFu, b2 = y >> 16, m = kAdlerMod;
  const uint64_t a = (a1 + a2 + m - 1) % m;
  const uint64_t b = (b1 + b2 + (uint64_t)(len2 % (int64_t)m) * ((a1 + m - 1) % m)) % m;
  return (uint32_t)(b << 16 | a);
}

// ---- CRC-32.  A register is the reflected remainder: bit 31 is x^0.  crc_bytes runs the plain register (no inversions) over bytes;
// the CRC of a chunk is ~crc_bytes(0xFFFFFFFF, ...).  For a message A B: reg(init, A B) = reg(init, A) x^(8 |B|) + reg(0, B) mod P, which
// is how the lanes of a block combine their slices (crc_shift).
SHDR_HD inline uint32_t crc_entry(uint32_t i) {
  for (int k = 0; k < 8; ++k) i = (i & 1u) ? (i >> 1) ^ kCrcPoly : i >> 1;
  return i;
}
SHDR_HD inline uint32_t crc_bytes(uint32_t reg, const uint8_t* p, int64_t n, const uint32_t* table) {
  for (int64_t i = 0; i < n; ++i) reg = table[(reg ^ p[i]) & 255u] ^ (reg >> 8);
  return reg;
}
SHDR_HD inline uint32_t crc_mul(uint32_t a, uint32_t b) {                          // a b mod P
  uint32_t p = 0;
  for (uint32_t m = 1u << 31; m; m >>= 1) {
    if (a & m) p ^= b;
    b = (b & 1u) ? (b >> 1) ^ kCrcPoly : b >> 1;
  }
  return p;
}
SHDR_HD inline uint32_t crc_shift(uint32_t reg, int64_t bytes) {                   // reg x^(8 bytes) mod P
  uint32_t sq = 1u << 23;                                                        // x^8
  for (; bytes > 0; bytes >>= 1) {
    if (bytes & 1) reg = crc_mul(reg, sq);
    sq = crc_mul(sq, sq);
  }
  return reg;
}

// the 33 bytes in front of the first IDAT; table: crc_entry(0 .. 255)
SHDR_HD inline void put_head(uint8_t* p, int64_t h, int64_t w, int c, const uint32_t* table) {
  const uint8_t sig[16] = {0x89, 'P', 'N', 'G', 13, 10, 26, 10, 0, 0, 0, 13, 'I', 'H', 'D', 'R'};
  for (int i = 0; i < 16; ++i) p[i] = sig[i];
  put_be32(p + 16, (uint32_t)w);
  put_be32(p + 20, (uint32_t)h);
  p[24] = 8;
  p[25] = (uint8_t)colour_type(c);
  p[26] = p[27] = p[28] = 0;                                                     // deflate, adaptive filtering, no interlace
  put_be32(p + 29, ~crc_bytes(0xFFFFFFFFu, p + 12, 17, table));
}
SHDR_HD inline void put_iend(uint8_t* p) {
  const uint8_t iend[kIend] = {0, 0, 0, 0, 'I', 'E', 'N', 'D', 0xAE, 0x42, 0x60, 0x82};
  for (int i = 0; i < kIend; ++i) p[i] = iend[i];
}

// ---- host side ----------------------------------------------------------------------------------------------------------------
struct CrcTable {
  uint32_t t[256];
  CrcTable() {
    for (uint32_t i = 0; i < 256; ++i) t[i] = crc_entry(i);
  }
};
inline const uint32_t* crc_table_host() {
  static const CrcTable tab;
  return tab.t;
}
inline uint32_t crc32_host(const uint8_t* p, int64_t n, uint32_t crc) { return ~crc_bytes(~crc, p, n, crc_table_host()); }

// row y of pixels [H][W][C] -> its 1 + W C bytes of the filtered stream; filter: a type, or kAdaptive
inline void filter_row_host(const uint8_t* pixels, int64_t y, int64_t w, int c, int filter, uint8_t* out) {
  const int64_t n = w * c;
  const uint8_t *row = pixels + y * n, *above = y ? row - n : nullptr;
  int type = filter;
  if (filter == kAdaptive) {
    uint64_t costs[5] = {0, 0, 0, 0, 0};
    for (int64_t i = 0; i < n; ++i) {
      const int a = i >= c ? row[i - c] : 0, b = above ? above[i] : 0, cc = above && i >= c ? above[i - c] : 0;
      for (int t = 0; t < 5; ++t) costs[t] += cost(filtered(t, row[i], a, b, cc));
    }
    type = cheapest(costs);
  }
  out[0] = (uint8_t)type;
  for (int64_t i = 0; i < n; ++i) {
    const int a = i >= c ? row[i - c] : 0, b = above ? above[i] : 0, cc = above && i >= c ? above[i - c] : 0;
    out[1 + i] = filtered(type, row[i], a, b, cc);
  }
}

// One segment's body into dst (room for n + 5 bytes): returns its length.  scratch: n + 12 bytes.  -3: no memory (the LZ parse).
inline int64_t segment_host(const uint8_t* src, int64_t n, bool last, int deflate, uint8_t* dst, uint8_t* scratch) {
  int64_t need = 0, bits = 0;
  const int64_t r = deflate == kLz ? shdr_deflate_lz::encode_host(src, n, scratch, n + 12, &need, &bits)
                                   : shdr_deflate::encode_host(src, n, scratch, n + 12, &need, &bits);
  if (r == -3) return -3;
  const int64_t coded = r > 0 ? coded_bytes(bits - 16, last) : 0;                // r == -2: need > n + 12, so coded >= need - 6 > n + 5
  if (r > 0 && use_coded(coded, n)) {
    const int64_t block = (bits - 16 + 7) / 8;                                   // the block's bytes, zero bits behind its last one
    memcpy(dst, scratch + 2, (size_t)block);
    if (!last) {
      dst[0] &= 0xFEu;                                                           // BFINAL
      for (int64_t i = block; i < coded - 4; ++i) dst[i] = 0;                    // the three bits may open one more byte
      dst[coded - 4] = dst[coded - 3] = 0;
      dst[coded - 2] = dst[coded - 1] = 0xFF;
    }
    return coded;
  }
  put_stored_header(dst, n, last);
  memcpy(dst + 5, src, (size_t)n);
  return n + 5;
}

// The file of pixels [H][W][C] into out.  Returns its length; -1 bad arguments, -2 capacity is less than that length (*need, if
// given, receives it; nothing is written), -3 no memory.
inline int64_t encode_host(const uint8_t* pixels, int64_t h, int64_t w, int c, int filter, int deflate, uint8_t* out, int64_t capacity,
                           int64_t* need) {
  if (!pixels || !out || !shape_ok(h, w, c) || filter < 0 || filter > kAdaptive || (deflate != kHuffman && deflate != kLz)) return -1;
  const int64_t stream = stream_bytes(h, w, c), bound = file_bound(stream);
  uint8_t* work = new (std::nothrow) uint8_t[(size_t)(stream + bound + kPngSegment + 12)];
  if (!work) return -3;
  uint8_t *flt = work, *file = work + stream, *scratch = file + bound;
  for (int64_t y = 0; y < h; ++y) filter_row_host(pixels, y, w, c, filter, flt + y * (w * c + 1));
  const uint32_t* table = crc_table_host();
  put_head(file, h, w, c, table);
  int64_t at = kHead;
  const int64_t n_seg = segments(stream);
  for (int64_t s = 0; s < n_seg; ++s) {
    const int64_t lo = s * kPngSegment, n = stream - lo < kPngSegment ? stream - lo : kPngSegment;
    const bool first = s == 0, last = s + 1 == n_seg;
    uint8_t* data = file + at + 8;
    int64_t len = 0;
    if (first) {
      data[0] = 0x78;
      data[1] = 0x01;
      len = 2;
    }
    const int64_t body = segment_host(flt + lo, n, last, deflate, data + len, scratch);
    if (body < 0) {
      delete[] work;
      return -3;
    }
    len += body;
    if (last) {
      put_be32(data + len, shdr_deflate::adler32_host(flt, stream));
      len += 4;
    }
    put_be32(file + at, (uint32_t)len);
    memcpy(file + at + 4, "IDAT", 4);
    put_be32(data + len, ~crc_bytes(0xFFFFFFFFu, file + at + 4, len + 4, table));
    at += 12 + len;
  }
  put_iend(file + at);
  at += kIend;
  if (need) *need = at;
  const bool fits = at <= capacity;
  if (fits) memcpy(out, file, (size_t)at);
  delete[] work;
  return fits ? at : -2;
}

}  // namespace shdr_png

// OpenEXR PIZ chunks decoded and, further down, encoded: the rules of the format, shared by the host routines shdr_piz_decode_host /
// shdr_piz_encode_host and the device kernels (csrc/piz.hip, csrc/piz_enc.hip), so that both sides run the same checks, end in the same
// status and write the same bytes.  Plain C++: also compiled without HIP.
//
// Restated from memory of OpenEXR 2.x; UNPINNED, reader and writer: no OpenEXR-written file has been read and no OpenEXR-built reader
// has opened a file written by these rules (there is no OpenEXR library to compare with).
//
// A chunk (little-endian): u16 minNonZero, u16 maxNonZero, bitmap[min .. max] of an 8192-byte bitmap (if min <= max), i32 length, then
// `length` bytes of Huffman block: u32 im, iM, tableLength (ignored), nBits, reserved; the packed code-length table of symbols im .. iM
// (6 bits each; 63: 8 more bits + 6 zero lengths; 59 .. 62: 2 .. 5 zero lengths); from the next byte on nBits bits of code words, both
// read most-significant bit first.  Symbol iM is the run code: 8 raw bits follow, the previous value is repeated that often.  The values
// are the wavelet coefficients of every channel plane (channel after channel, rows x width x words, the two 16-bit words of a FLOAT / UINT
// sample interleaved per pixel); after the inverse wavelet every value goes through the reverse LUT of the bitmap and the rows are
// written scanline by scanline, channel by channel within a row, as little-endian u16: the planar layout exr_load_resize reads.
//
// Canonical codes (OpenEXR's hufCanonicalCodeTable): c = 0; for l = 58 .. 1: first[l] = c, c = (c + n[l]) >> 1; symbols in increasing
// order take first[len]++.  An over-subscribed length set is refused.  An incomplete one is accepted; there the shift can make a short
// code a prefix of a longer one, and the decoder's rule is then: the SHORTEST length whose code range holds the bits wins (the first-level
// table is filled by that very walk).  Bits that no code owns are kBadCode.
//
// Work is bounded: every token consumes at least one bit, every read is clamped to the chunk, every write is checked against the number
// of values the chunk must hold; a chunk ends in a Status whatever its bytes are.
#pragma once
#include <assert.h>
#include <stdint.h>

#include <algorithm>

#ifndef SHDR_HD
#if defined(__HIPCC__)
#define SHDR_HD __host__ __device__
#else
#define SHDR_HD
#endif
#endif

namespace shdr_piz {

enum Status : int {                           // include/shdr.h lists them as SHDR_PIZ_*; _ops.PIZ_REASONS names them
  kOk = 0,
  kTruncated = 1,                             // the chunk ends inside minNonZero / maxNonZero or the length field
  kBitmap = 2,                                // maxNonZero >= 8192, or the bitmap runs past the chunk
  kLength = 3,                                // the Huffman block's length is negative or runs past the chunk
  kNoData = 4,                                // length == 0 or nBits == 0 (the output is never empty)
  kHuffHeader = 5,                            // fewer than 20 bytes of block, im or iM >= 65537, im > iM
  kTableTruncated = 6,                        // the code-length table runs past the block
  kTableRun = 7,                              // a zero run past iM + 1
  kOverSubscribed = 8,                        // Kraft sum of the code lengths > 1
  kNBits = 9,                                 // nBits beyond the bytes that follow the table
  kBadCode = 10,                              // bits that no code owns
  kDataTruncated = 11,                        // a code word or a run count runs past nBits
  kRunNoPrev = 12,                            // a run with no previous value
  kTooMany = 13,                              // more values than the chunk holds
  kTooFew = 14,                               // nBits consumed and fewer values than the chunk holds
  kRawSize = 15,                              // (batch) a stored-raw chunk whose size is not the slot's
  kMode = 16,                                 // (batch) a mode byte other than 0 / 1
  kStatusCount = 17
};

constexpr int kMaxLen = 58;                                      // bits of the longest code word
constexpr int kFastBits = 12;                                    // index bits of the first-level table
constexpr int kSymbols = 65537;                                  // 0 .. 65536
constexpr int kBitmapBytes = 8192;
constexpr int kLutSize = 65536;
constexpr int kMaxRows = 32;                                     // scanlines of a chunk
constexpr int kMaxChannels = 64;
constexpr int64_t kMaxChunk = (int64_t)1 << 28;                  // stored bytes, and decoded bytes, of one chunk
constexpr uint32_t kNone = 0xFFFFFFFFu;                          // "no previous value"
constexpr int kMinSubBits = 128;                                 // a token has at most 58 + 8 bits: no token spans a whole subsequence

struct Head {                                 // where things are in a chunk; offsets from the chunk's first byte
  uint32_t bm_min, bm_max;                    // bitmap[bm_min .. bm_max] is stored (none if bm_min > bm_max) ...
  int64_t bm_at;                              // ... from this byte on
  int64_t block_at, block_len;                // the Huffman block
  uint32_t im, iM, n_bits;
  int64_t data_at, data_len;                  // bytes of code words (set by unpack_lengths)
};

struct Canon {                                // LDS on the device
  uint64_t first[kMaxLen + 1];                // first code of each length
  uint32_t count[kMaxLen + 1], start[kMaxLen + 1];               // symbols of that length; index of the first in `sorted`
  uint32_t run_index;                         // index in `sorted` of symbol iM, or kNone
  int32_t max_len;
};

SHDR_HD inline uint32_t rd16(const uint8_t* p) { return (uint32_t)p[0] | ((uint32_t)p[1] << 8); }
SHDR_HD inline uint32_t rd32(const uint8_t* p) { return rd16(p) | (rd16(p + 2) << 16); }

// the fixed fields of the chunk src[0 .. n): everything but the code-length table
SHDR_HD inline int parse_head(const uint8_t* src, int64_t n, Head& h) {
  if (n < 4) return kTruncated;
  h.bm_min = rd16(src);
  h.bm_max = rd16(src + 2);
  h.bm_at = 4;
  if (h.bm_max >= (uint32_t)kBitmapBytes) return kBitmap;
  int64_t p = 4;
  if (h.bm_min <= h.bm_max) {
    p += (int64_t)(h.bm_max - h.bm_min + 1);
    if (p > n) return kBitmap;
  }
  if (p + 4 > n) return kTruncated;
  const int32_t length = (int32_t)rd32(src + p);
  p += 4;
  if (length < 0 || (int64_t)length > n - p) return kLength;
  if (length == 0) return kNoData;
  h.block_at = p;
  h.block_len = length;
  if (length < 20) return kHuffHeader;
  h.im = rd32(src + p);
  h.iM = rd32(src + p + 4);
  h.n_bits = rd32(src + p + 12);
  if (h.im >= (uint32_t)kSymbols || h.iM >= (uint32_t)kSymbols || h.im > h.iM) return kHuffHeader;
  h.data_at = h.data_len = 0;
  return kOk;
}

// 64 bits of p[0 .. nbytes) from bit position `bit` on (most significant first), zero beyond the end
SHDR_HD inline uint64_t window(const uint8_t* p, int64_t nbytes, uint64_t bit) {
  const int64_t i = (int64_t)(bit >> 3);
  const int s = (int)(bit & 7);
  uint64_t w = 0;
  uint32_t tail = 0;
  if (i + 9 <= nbytes) {
    __builtin_memcpy(&w, p + i, 8);
    w = __builtin_bswap64(w);
    tail = p[i + 8];
  } else {
    for (int k = 0; k < 8; ++k) w = (w << 8) | (i + k < nbytes ? p[i + k] : 0u);
  }
  return s ? (w << s) | (uint64_t)(tail >> (8 - s)) : w;
}

// the code-length table of the block: lens[s] for the symbols with a code (lens is all zero before the call; zero runs are skipped).
// Sets h.data_at / h.data_len and checks nBits.
SHDR_HD inline int unpack_lengths(const uint8_t* src, Head& h, uint8_t* lens) {
  const uint8_t* t = src + h.block_at + 20;
  const int64_t tbytes = h.block_len - 20;
  const uint64_t tbits = 8 * (uint64_t)tbytes;
  uint64_t bit = 0;
  uint32_t s = h.im;
  while (s <= h.iM) {
    if (bit + 6 > tbits) return kTableTruncated;
    const uint32_t l = (uint32_t)(window(t, tbytes, bit) >> 58);
    bit += 6;
    if (l >= 59) {
      uint32_t z = l - 59 + 2;
      if (l == 63) {
        if (bit + 8 > tbits) return kTableTruncated;
        z = (uint32_t)(window(t, tbytes, bit) >> 56) + 6;
        bit += 8;
      }
      if (s + z > h.iM + 1) return kTableRun;
      s += z;
    } else {
      if (l) lens[s] = (uint8_t)l;
      ++s;
    }
  }
  const int64_t used = (int64_t)((bit + 7) >> 3);
  h.data_at = h.block_at + 20 + used;
  h.data_len = tbytes - used;
  if (h.n_bits == 0) return kNoData;
  if ((uint64_t)h.n_bits > 8 * (uint64_t)h.data_len) return kNBits;
  return kOk;
}

// count[1 .. 58] -> first / start / max_len; kOverSubscribed when the Kraft sum exceeds 1
SHDR_HD inline int make_canon(Canon& c) {
  int64_t left = 1;                                              // free code points at this length (capped: 2^30 can never run out again)
  uint32_t at = 0;
  c.max_len = 0;
  c.count[0] = 0;
  c.start[0] = 0;
  c.first[0] = 0;
  for (int l = 1; l <= kMaxLen; ++l) {
    left = 2 * left - (int64_t)c.count[l];
    if (left < 0) return kOverSubscribed;
    if (left > ((int64_t)1 << 30)) left = (int64_t)1 << 30;
    c.start[l] = at;
    at += c.count[l];
    if (c.count[l]) c.max_len = l;
  }
  uint64_t code = 0;
  for (int l = kMaxLen; l >= 1; --l) {
    c.first[l] = code;
    code = (code + c.count[l]) >> 1;
  }
  return kOk;
}

// a table entry: symbol & 0xFFFF | length << 16 | (1 << 22 for the run code); 0: no code
SHDR_HD inline uint32_t walk(const Canon& c, const uint16_t* sorted, uint64_t w, int lo, int hi) {
  for (int l = lo; l <= hi; ++l) {
    const uint64_t d = (w >> (64 - l)) - c.first[l];
    if (d < (uint64_t)c.count[l]) {
      const uint32_t idx = c.start[l] + (uint32_t)d;
      return (uint32_t)sorted[idx] | ((uint32_t)l << 16) | (idx == c.run_index ? 1u << 22 : 0u);
    }
  }
  return 0;
}
SHDR_HD inline uint32_t fast_entry(const Canon& c, const uint16_t* sorted, uint32_t index) {
  const int hi = c.max_len < kFastBits ? c.max_len : kFastBits;
  return walk(c, sorted, (uint64_t)index << (64 - kFastBits), 1, hi);
}
SHDR_HD inline uint32_t lookup(const Canon& c, const uint32_t* fast, const uint16_t* sorted, uint64_t w) {
  const uint32_t e = fast[w >> (64 - kFastBits)];
  return e ? e : walk(c, sorted, w, kFastBits + 1, c.max_len);
}

struct Code {                                 // what the tokens of a chunk are read with
  const uint8_t* data;                        // the code words
  int64_t data_len;
  uint64_t n_bits;
  const Canon* canon;
  const uint32_t* fast;
  const uint16_t* sorted;
};

// the token at bit `pos` < n_bits: kOk (adv bits; a value, or run with its count in val), kBadCode or kDataTruncated
SHDR_HD inline int token(const Code& k, uint64_t pos, uint32_t& adv, uint32_t& val, bool& run) {
  const uint64_t w = window(k.data, k.data_len, pos);
  const uint32_t e = lookup(*k.canon, k.fast, k.sorted, w);
  if (!e) return kBadCode;
  const uint32_t len = (e >> 16) & 63u;
  const uint64_t left = k.n_bits - pos;
  if (len > left) return kDataTruncated;
  run = (e >> 22) != 0;
  if (run) {
    if (len + 8 > left) return kDataTruncated;
    val = (uint32_t)(len <= 56 ? (w << len) >> 56 : window(k.data, k.data_len, pos + len) >> 56);
    adv = len + 8;
  } else {
    val = e & 0xFFFFu;
    adv = len;
  }
  return kOk;
}

// Speculative pass over the tokens that start in [pos, stop): where the next one starts, how many values they hold, the last value
// that is no run (kNone: none).  Bits that no code owns are skipped one at a time; nothing is judged here.
SHDR_HD inline void span_scan(const Code& k, uint64_t pos, uint64_t stop, uint32_t& end, uint32_t& count, uint32_t& last) {
  uint32_t n = 0, lv = kNone;
  while (pos < stop) {
    uint32_t adv = 0, val = 0;
    bool run = false;
    const int st = token(k, pos, adv, val, run);
    if (st == kDataTruncated) {
      pos = k.n_bits;
      break;
    }
    if (st != kOk) {
      ++pos;
      continue;
    }
    if (run) {
      n += val;
    } else {
      ++n;
      lv = val;
    }
    pos += adv;
  }
  end = (uint32_t)pos;
  count = n;
  last = lv;
}

// The true pass over the tokens that start in [pos, stop): values out[at ..], `at` <= expected being the values before pos (after the
// call: before the first token that was not taken) and prev the last of them (kNone: none).  Returns the first error, in stream
// order, or kOk.
SHDR_HD inline int span_write(const Code& k, uint64_t pos, uint64_t stop, uint16_t* out, uint64_t& at, uint64_t expected, uint32_t prev) {
  while (pos < stop) {
    uint32_t adv = 0, val = 0;
    bool run = false;
    const int st = token(k, pos, adv, val, run);
    if (st != kOk) return st;
    if (run) {
      if (prev == kNone) return kRunNoPrev;
      if (at + val > expected) return kTooMany;
      for (uint32_t i = 0; i < val; ++i) out[at + i] = (uint16_t)prev;
      at += val;
    } else {
      if (at + 1 > expected) return kTooMany;
      out[at++] = (uint16_t)val;
      prev = val;
    }
    pos += adv;
  }
  return kOk;
}

// ---- the wavelet ------------------------------------------------------------------------------------------------------------
SHDR_HD inline void dec14(uint16_t l, uint16_t h, uint16_t& a, uint16_t& b) {
  const int16_t ls = (int16_t)l, hs = (int16_t)h;
  const int hi = hs;
  const int ai = ls + (hi & 1) + (hi >> 1);
  const int16_t as = (int16_t)ai;
  a = (uint16_t)as;
  b = (uint16_t)(int16_t)(as - hs);
}
SHDR_HD inline void dec16(uint16_t l, uint16_t h, uint16_t& a, uint16_t& b) {
  const int bb = ((int)l - ((int)h >> 1)) & 0xFFFF;
  const int aa = ((int)h + bb - 0x8000) & 0xFFFF;
  a = (uint16_t)aa;
  b = (uint16_t)bb;
}
template <bool W14>
SHDR_HD inline void dec(uint16_t l, uint16_t h, uint16_t& a, uint16_t& b) {
  if (W14) dec14(l, h, a, b);
  else dec16(l, h, a, b);
}
template <bool W14>
SHDR_HD inline void dec_quad(uint16_t& A, uint16_t& B, uint16_t& C, uint16_t& D) {
  uint16_t i00, i10, i01, i11;
  dec<W14>(A, C, i00, i10);
  dec<W14>(B, D, i01, i11);
  dec<W14>(i00, i01, A, B);
  dec<W14>(i10, i11, C, D);
}
SHDR_HD inline int top_power(int n) {                            // the largest power of two <= n (n >= 1)
  int p = 1;
  while (2 * p <= n) p *= 2;
  return p;
}

// the whole plane in place, OpenEXR's loop: nx by ny values at strides sx / sy
template <bool W14>
inline void wav_decode(uint16_t* in, int nx, int64_t sx, int ny, int64_t sy) {
  const int n = nx < ny ? nx : ny;
  int p = top_power(n), p2 = p;
  p >>= 1;
  while (p >= 1) {
    int y = 0, x = 0;
    for (; y <= ny - p2; y += p2) {
      for (x = 0; x <= nx - p2; x += p2) {
        uint16_t* q = in + y * sy + x * sx;
        dec_quad<W14>(q[0], q[p * sx], q[p * sy], q[p * sy + p * sx]);
      }
      if (nx & p) {
        uint16_t* q = in + y * sy + x * sx;
        dec<W14>(q[0], q[p * sy], q[0], q[p * sy]);
      }
    }
    if (ny & p) {
      for (x = 0; x <= nx - p2; x += p2) {
        uint16_t* q = in + y * sy + x * sx;
        dec<W14>(q[0], q[p * sx], q[0], q[p * sx]);
      }
    }
    p2 = p;
    p >>= 1;
  }
}

// values of a chunk; 0 when the shape is out of range
SHDR_HD inline int64_t chunk_values(int width, int rows, const int32_t* chan_words, int n_chan) {
  if (width < 1 || rows < 1 || rows > kMaxRows || n_chan < 1 || n_chan > kMaxChannels || !chan_words) return 0;
  int64_t words = 0;
  for (int c = 0; c < n_chan; ++c) {
    if (chan_words[c] != 1 && chan_words[c] != 2) return 0;
    words += chan_words[c];
  }
  const int64_t v = (int64_t)width * rows * words;
  return 2 * v <= kMaxChunk ? v : 0;
}

// ---- the host decoder: the twin that judges the kernels -------------------------------------------------------------------------
struct HostWork {                             // the caller's scratch
  uint8_t* lens;                              // [kSymbols]
  uint16_t* sorted;                           // [kSymbols]
  uint32_t* fast;                             // [1 << kFastBits]
  uint16_t* lut;                              // [kLutSize]
  uint16_t* values;                           // [the chunk's values]
};

// src[0 .. n) -> dst[0 .. 2 * values): the status; dst is written only when the chunk is good
inline int decode_host(const uint8_t* src, int64_t n, int width, int rows, const int32_t* chan_words, int n_chan, uint8_t* dst,
                       HostWork& w) {
  const uint64_t expected = (uint64_t)chunk_values(width, rows, chan_words, n_chan);
  Head h;
  if (int st = parse_head(src, n, h)) return st;
  for (int s = 0; s < kSymbols; ++s) w.lens[s] = 0;
  if (int st = unpack_lengths(src, h, w.lens)) return st;
  Canon c;
  for (int l = 0; l <= kMaxLen; ++l) c.count[l] = 0;
  for (uint32_t s = h.im; s <= h.iM; ++s) ++c.count[w.lens[s]];
  c.count[0] = 0;
  if (int st = make_canon(c)) return st;
  uint32_t next[kMaxLen + 1];
  for (int l = 0; l <= kMaxLen; ++l) next[l] = c.start[l];
  c.run_index = kNone;
  for (uint32_t s = h.im; s <= h.iM; ++s) {
    const int l = w.lens[s];
    if (!l) continue;
    if (s == h.iM) c.run_index = next[l];
    w.sorted[next[l]++] = (uint16_t)s;
  }
  for (uint32_t i = 0; i < (1u << kFastBits); ++i) w.fast[i] = fast_entry(c, w.sorted, i);
  const Code k{src + h.data_at, h.data_len, h.n_bits, &c, w.fast, w.sorted};
  uint64_t at = 0;                                               // one span: the whole stream
  if (int st = span_write(k, 0, h.n_bits, w.values, at, expected, kNone)) return st;
  if (at < expected) return kTooFew;
  // reverse LUT
  uint32_t kk = 0;
  for (uint32_t v = 0; v < (uint32_t)kLutSize; ++v) {
    const uint32_t byte = v >> 3;
    const bool in = byte >= h.bm_min && byte <= h.bm_max && ((src[h.bm_at + (byte - h.bm_min)] >> (v & 7)) & 1);
    if (v == 0 || in) w.lut[kk++] = (uint16_t)v;
  }
  const uint32_t max_value = kk - 1;
  for (; kk < (uint32_t)kLutSize; ++kk) w.lut[kk] = 0;
  // wavelet, per channel and word plane
  uint16_t* base = w.values;
  int64_t row_words = 0;
  for (int ch = 0; ch < n_chan; ++ch) row_words += (int64_t)width * chan_words[ch];
  int64_t chan_off = 0;
  for (int ch = 0; ch < n_chan; ++ch) {
    const int words = chan_words[ch];
    for (int j = 0; j < words; ++j) {
      if (max_value < 16384u) wav_decode<true>(base + j, width, words, rows, (int64_t)width * words);
      else wav_decode<false>(base + j, width, words, rows, (int64_t)width * words);
    }
    for (int y = 0; y < rows; ++y) {
      uint8_t* row = dst + 2 * (y * row_words + chan_off);
      const uint16_t* v = base + (int64_t)y * width * words;
      for (int64_t i = 0; i < (int64_t)width * words; ++i) {
        const uint16_t o = w.lut[v[i]];
        row[2 * i] = (uint8_t)(o & 0xFF);
        row[2 * i + 1] = (uint8_t)(o >> 8);
      }
    }
    base += (int64_t)width * rows * words;
    chan_off += (int64_t)width * words;
  }
  return kOk;
}

// ---- the encoder: the forward rules, shared by shdr_piz_encode_host and the kernels of csrc/piz_enc.hip ---------------------------------
// UNPINNED like the decoder: no OpenEXR-built reader has opened what this writes.  The reference is tests/piz_ref.py, byte for byte.
//
// bitmap of the 16-bit values present (value 0 implied: its bit is not stored) -> forward LUT = rank among the present values ->
// forward wavelet per word plane -> the chunk's value sequence (channel after channel) -> tokens: a stretch of L equal values is the
// value once and, if L - 1 >= 3, run codes of at most 255 each, else the value L times -> optimal code of the tokens' frequencies
// (the run code iM = max value + 1 counts 1 + run tokens), two-queue method -> canonical codes -> packed table -> bit stream.
constexpr int kMinRun = 3;                                       // repeats from which a stretch is written with run codes
constexpr int kMaxRun = 255;                                     // repeats per run code
constexpr int kTableZeros = 261;                                 // zero lengths per long table token (63, z - 6)
constexpr int kBitmapWords = kBitmapBytes / 4;
constexpr int64_t kEncodeFixed = 4 + kBitmapBytes + 4 + 20 + (6 * (int64_t)kSymbols + 7) / 8;   // everything but the code words

SHDR_HD inline void enc14(uint16_t a, uint16_t b, uint16_t& l, uint16_t& h) {
  const int as = (int16_t)a, bs = (int16_t)b;
  const int16_t hs = (int16_t)(as - bs);
  const int hi = hs;
  l = (uint16_t)(int16_t)(as - (hi & 1) - (hi >> 1));
  h = (uint16_t)hs;
}
SHDR_HD inline void enc16(uint16_t a, uint16_t b, uint16_t& l, uint16_t& h) {
  const int hh = ((int)a - (int)b + 0x8000) & 0xFFFF;
  l = (uint16_t)(((int)b + (hh >> 1)) & 0xFFFF);
  h = (uint16_t)hh;
}
template <bool W14>
SHDR_HD inline void enc(uint16_t a, uint16_t b, uint16_t& l, uint16_t& h) {
  if (W14) enc14(a, b, l, h);
  else enc16(a, b, l, h);
}
template <bool W14>
SHDR_HD inline void enc_quad(uint16_t& A, uint16_t& B, uint16_t& C, uint16_t& D) {
  uint16_t i00, i01, i10, i11;
  enc<W14>(A, B, i00, i01);
  enc<W14>(C, D, i10, i11);
  enc<W14>(i00, i10, A, C);
  enc<W14>(i01, i11, B, D);
}

// the whole plane in place: the decoder's level schedule walked from the finest level to the coarsest
template <bool W14>
inline void wav_encode(uint16_t* in, int nx, int64_t sx, int ny, int64_t sy) {
  const int n = nx < ny ? nx : ny;
  for (int p = 1, p2 = 2; p2 <= n; p = p2, p2 <<= 1) {
    int y = 0, x = 0;
    for (; y <= ny - p2; y += p2) {
      for (x = 0; x <= nx - p2; x += p2) {
        uint16_t* q = in + y * sy + x * sx;
        enc_quad<W14>(q[0], q[p * sx], q[p * sy], q[p * sy + p * sx]);
      }
      if (nx & p) {
        uint16_t* q = in + y * sy + x * sx;
        enc<W14>(q[0], q[p * sy], q[0], q[p * sy]);
      }
    }
    if (ny & p) {
      for (x = 0; x <= nx - p2; x += p2) {
        uint16_t* q = in + y * sy + x * sx;
        enc<W14>(q[0], q[p * sx], q[0], q[p * sx]);
      }
    }
  }
}

// the forward LUT: words[2048] is the bitmap with bit 0 set, before[i] the bits set in words[0 .. i)
SHDR_HD inline uint32_t lut_rank(const uint32_t* words, const uint32_t* before, uint32_t v) {
  return before[v >> 5] + (uint32_t)__builtin_popcount(words[v >> 5] & ((1u << (v & 31)) - 1u));
}

// a stretch of L >= 1 equal values: how often the value itself is written, and how many run codes follow
SHDR_HD inline void stretch_tokens(uint32_t L, uint32_t& literals, uint32_t& runs) {
  const uint32_t rep = L - 1;
  if (rep >= (uint32_t)kMinRun) {
    literals = 1;
    runs = (rep + kMaxRun - 1) / kMaxRun;
  } else {
    literals = L;
    runs = 0;
  }
}
SHDR_HD inline uint64_t stretch_bits(uint32_t L, uint32_t len, uint32_t run_len) {
  uint32_t lit, runs;
  stretch_tokens(L, lit, runs);
  return (uint64_t)lit * len + (uint64_t)runs * (run_len + 8);
}
// Sink: put(value < 2^bits, bits <= 58)
template <class Sink>
SHDR_HD inline void put_stretch(Sink& s, uint32_t L, uint64_t code, uint32_t len, uint64_t run_code, uint32_t run_len) {
  uint32_t lit, runs;
  stretch_tokens(L, lit, runs);
  for (uint32_t i = 0; i < lit; ++i) s.put(code, (int)len);
  for (uint32_t rep = L - 1; runs; --runs) {
    const uint32_t k = rep < (uint32_t)kMaxRun ? rep : (uint32_t)kMaxRun;
    s.put(run_code, (int)run_len);
    s.put(k, 8);
    rep -= k;
  }
}

// the code-length table: a maximal stretch of Z zero lengths is cut greedily -- 261 at a time as (63, z - 6), a rest of 6 or more the
// same way, a rest of 2 .. 5 as 59 + z - 2, a rest of 1 as a literal 0; a stretch of L equal non-zero lengths is L literals
SHDR_HD inline uint32_t table_stretch_bits(uint32_t l, uint32_t L) {
  if (l) return 6 * L;
  const uint32_t r = L % (uint32_t)kTableZeros;
  return 14 * (L / (uint32_t)kTableZeros) + (r >= 6 ? 14u : r >= 1 ? 6u : 0u);
}
template <class Sink>
SHDR_HD inline void put_table_stretch(Sink& s, uint32_t l, uint32_t L) {
  if (l) {
    for (uint32_t i = 0; i < L; ++i) s.put(l, 6);
    return;
  }
  while (L >= 6) {
    const uint32_t z = L < (uint32_t)kTableZeros ? L : (uint32_t)kTableZeros;
    s.put((63u << 8) | (z - 6), 14);
    L -= z;
  }
  if (L >= 2) s.put(59 + L - 2, 6);
  else if (L == 1) s.put(0, 6);
}

// An MSB-first bit stream gathered into 32-bit words; Out::word(i, w): OR the big-endian word w into bytes 4 i .. 4 i + 3 of a cleared
// stream (the first and the last word of a writer are shared with its neighbours).  Starts at any bit.
template <class Out>
struct BitSink {
  Out out;
  uint64_t acc;
  int64_t index;
  int cnt;                                                       // bits of acc that are the word's so far: < 32 between calls
  SHDR_HD BitSink(Out o, uint64_t bit) : out(o), acc(0), index((int64_t)(bit >> 5)), cnt((int)(bit & 31)) {}
  SHDR_HD void put32(uint32_t v, int n) {
    acc = (acc << n) | v;
    cnt += n;
    if (cnt >= 32) {
      cnt -= 32;
      out.word(index++, (uint32_t)(acc >> cnt));
      acc &= ((uint64_t)1 << cnt) - 1;
    }
  }
  SHDR_HD void put(uint64_t v, int n) {
    if (n > 32) {
      put32((uint32_t)(v >> 32), n - 32);
      put32((uint32_t)v, 32);
    } else if (n > 0) {
      put32((uint32_t)v, n);
    }
  }
  SHDR_HD void flush() {
    if (cnt) out.word(index, (uint32_t)(acc << (32 - cnt)));
    cnt = 0;
  }
};

// The optimal code by the two-queue method.  weight[0 .. n): the leaves' counts in (count, symbol) order, n >= 2; internal nodes
// queue up in creation order (their weights never decrease); on equal weight the leaf is taken first.  Node i < n is leaf i, node
// n + k the k-th internal node, node 2 n - 2 the root.  made[n - 1] and parent[2 n - 1] are scratch / result.
SHDR_HD inline void huff_merge(const uint32_t* weight, uint32_t n, uint32_t* made, uint32_t* parent) {
  uint32_t leaf = 0, head = 0;
  for (uint32_t k = 0; k + 1 < n; ++k) {
    uint32_t sum = 0;
    for (int pick = 0; pick < 2; ++pick) {
      if (leaf < n && (head >= k || weight[leaf] <= made[head])) {
        sum += weight[leaf];
        parent[leaf++] = n + k;
      } else {
        sum += made[head];
        parent[n + head++] = n + k;
      }
    }
    made[k] = sum;
  }
}
SHDR_HD inline uint32_t huff_depth(const uint32_t* parent, uint32_t n, uint32_t node) {
  uint32_t d = 0;
  for (; node != 2 * n - 2; node = parent[node]) ++d;
  return d;
}

// bytes that hold any chunk of `values` values: the fixed parts at their largest, and at most 17 + 8 bits per value (an optimal code
// of at most 65537 symbols spends no more than 17 bits per token on average, and a run code's count covers at least 3 values)
SHDR_HD inline int64_t encode_bound(int64_t values) { return kEncodeFixed + 4 * values; }

// ---- the host encoder: the twin that judges the kernels ---------------------------------------------------------------------------
struct HostOut {
  uint8_t* p;
  void word(int64_t i, uint32_t w) {
    for (int k = 0; k < 4; ++k)
      if (const uint8_t b = (uint8_t)(w >> (24 - 8 * k))) p[4 * i + k] |= b;
  }
};

struct EncWork {                              // the caller's scratch
  uint32_t* words;                            // [kBitmapWords]
  uint32_t* before;                           // [kBitmapWords]
  uint16_t* values;                           // [the chunk's values]
  uint32_t* freq;                             // [kSymbols]
  uint64_t* keys;                             // [kSymbols]
  uint32_t* weight;                           // [kSymbols]
  uint32_t* made;                             // [kSymbols]
  uint32_t* parent;                           // [2 * kSymbols]
  uint8_t* lens;                              // [kSymbols]
  uint64_t* code;                             // [kSymbols]
};

// raw[0 .. 2 * values): the planar scanlines of the chunk -> dst: the PIZ bytes, whatever their size.  Returns their number, or -2 when
// capacity is less than that (nothing is written then).
inline int64_t encode_host(const uint8_t* raw, int width, int rows, const int32_t* chan_words, int n_chan, uint8_t* dst, int64_t capacity,
                           EncWork& w) {
  const int64_t nv = chunk_values(width, rows, chan_words, n_chan);
  // bitmap, LUT
  for (int i = 0; i < kBitmapWords; ++i) w.words[i] = 0;
  for (int64_t i = 0; i < nv; ++i) {
    const uint32_t v = rd16(raw + 2 * i);
    w.words[v >> 5] |= 1u << (v & 31);
  }
  w.words[0] &= ~1u;                                             // value 0 is implied
  uint32_t lo = kBitmapBytes - 1, hi = 0;
  for (int i = kBitmapBytes - 1; i >= 0; --i)
    if ((w.words[i >> 2] >> (8 * (i & 3))) & 255u) lo = (uint32_t)i;
  for (int i = 0; i < kBitmapBytes; ++i)
    if ((w.words[i >> 2] >> (8 * (i & 3))) & 255u) hi = (uint32_t)i;
  const int64_t bm = lo <= hi ? (int64_t)(hi - lo + 1) : 0;
  const int64_t size = 4 + bm;
  w.words[0] |= 1u;
  uint32_t present = 0;
  for (int i = 0; i < kBitmapWords; ++i) {
    w.before[i] = present;
    present += (uint32_t)__builtin_popcount(w.words[i]);
  }
  const uint32_t max_value = present - 1;
  // values: LUT, then the wavelet per channel and word plane
  int64_t row_words = 0;
  for (int ch = 0; ch < n_chan; ++ch) row_words += (int64_t)width * chan_words[ch];
  uint16_t* base = w.values;
  int64_t chan_off = 0;
  for (int ch = 0; ch < n_chan; ++ch) {
    const int words = chan_words[ch];
    for (int y = 0; y < rows; ++y)
      for (int64_t i = 0; i < (int64_t)width * words; ++i)
        base[(int64_t)y * width * words + i] = (uint16_t)lut_rank(w.words, w.before, rd16(raw + 2 * (y * row_words + chan_off + i)));
    for (int j = 0; j < words; ++j) {
      if (max_value < 16384u) wav_encode<true>(base + j, width, words, rows, (int64_t)width * words);
      else wav_encode<false>(base + j, width, words, rows, (int64_t)width * words);
    }
    base += (int64_t)width * rows * words;
    chan_off += (int64_t)width * words;
  }
  // frequencies of the tokens
  for (int s = 0; s < kSymbols; ++s) w.freq[s] = 0;
  uint32_t im = 65535, top = 0, run_tokens = 0;
  for (int64_t i = 0; i < nv;) {
    const uint16_t v = w.values[i];
    int64_t j = i + 1;
    while (j < nv && w.values[j] == v) ++j;
    uint32_t lit, runs;
    stretch_tokens((uint32_t)(j - i), lit, runs);
    w.freq[v] += lit;
    run_tokens += runs;
    if (v < im) im = v;
    if (v > top) top = v;
    i = j;
  }
  const uint32_t iM = top + 1;
  w.freq[iM] = 1 + run_tokens;
  // code lengths
  uint32_t n = 0;
  for (uint32_t s = im; s <= iM; ++s)
    if (w.freq[s]) w.keys[n++] = ((uint64_t)w.freq[s] << 17) | s;
  std::sort(w.keys, w.keys + n);                                 // (count, symbol)
  for (uint32_t i = 0; i < n; ++i) w.weight[i] = (uint32_t)(w.keys[i] >> 17);
  huff_merge(w.weight, n, w.made, w.parent);
  Canon c;
  for (int l = 0; l <= kMaxLen; ++l) c.count[l] = 0;
  for (int s = 0; s < kSymbols; ++s) w.lens[s] = 0;
  uint64_t n_bits = 8 * (uint64_t)run_tokens;
  for (uint32_t i = 0; i < n; ++i) {
    const uint32_t d = huff_depth(w.parent, n, i);
    assert(d >= 1 && d <= (uint32_t)kMaxLen);                    // fewer than 2^27 values: a depth of 41 already needs more weight
    w.lens[w.keys[i] & 0x1FFFFu] = (uint8_t)d;
    ++c.count[d];
    n_bits += (uint64_t)d * w.weight[i];
  }
  n_bits -= w.lens[iM];                                          // the run code counts one more than it is written
  make_canon(c);
  for (uint32_t s = im; s <= iM; ++s)
    if (const int l = w.lens[s]) w.code[s] = c.first[l]++;
  // the table's size, then everything is known
  uint32_t table_bits = 0;
  for (uint32_t s = im; s <= iM;) {
    uint32_t e = s + 1;
    while (e <= iM && w.lens[e] == w.lens[s]) ++e;
    table_bits += table_stretch_bits(w.lens[s], e - s);
    s = e;
  }
  const int64_t table_bytes = (table_bits + 7) >> 3, data_bytes = (int64_t)((n_bits + 7) >> 3);
  const int64_t block = 20 + table_bytes + data_bytes;
  if (size + 4 + block > capacity) return -2;
  dst[0] = (uint8_t)lo; dst[1] = (uint8_t)(lo >> 8); dst[2] = (uint8_t)hi; dst[3] = (uint8_t)(hi >> 8);
  for (int64_t i = 0; i < bm; ++i) {
    const uint32_t k = lo + (uint32_t)i;
    dst[4 + i] = (uint8_t)((w.words[k >> 2] >> (8 * (k & 3))) & (k ? 0xFFu : 0xFEu));
  }
  uint8_t* p = dst + size;
  const uint32_t head[6] = {(uint32_t)block, im, iM, (uint32_t)table_bytes, (uint32_t)n_bits, 0u};
  for (int k = 0; k < 6; ++k)
    for (int b = 0; b < 4; ++b) *p++ = (uint8_t)(head[k] >> (8 * b));
  for (int64_t i = 0; i < table_bytes + data_bytes; ++i) p[i] = 0;
  BitSink<HostOut> table(HostOut{p}, 0);
  for (uint32_t s = im; s <= iM;) {
    uint32_t e = s + 1;
    while (e <= iM && w.lens[e] == w.lens[s]) ++e;
    put_table_stretch(table, w.lens[s], e - s);
    s = e;
  }
  table.flush();
  BitSink<HostOut> data(HostOut{p + table_bytes}, 0);
  for (int64_t i = 0; i < nv;) {
    const uint16_t v = w.values[i];
    int64_t j = i + 1;
    while (j < nv && w.values[j] == v) ++j;
    put_stretch(data, (uint32_t)(j - i), w.code[v], w.lens[v], w.code[iM], w.lens[iM]);
    i = j;
  }
  data.flush();
  return size + 4 + block;
}

}  // namespace shdr_piz

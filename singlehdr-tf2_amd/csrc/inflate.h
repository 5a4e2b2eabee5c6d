// zlib streams (RFC 1950 / 1951) decoded: everything whose correctness is about bytes and bounds, shared by the host routine
// shdr_inflate_host and the device kernel (csrc/inflate.hip), so that both run the same checks.  Plain C++: also compiled without HIP.
//
// inflate_zlib<Io> is the whole decoder.  Decoding is serial, so every value of its state (bit buffer, positions, table entries) is the
// same in every lane of the wave that runs it; what differs between host and device is behind `Io`:
//      word(pos)            the four stream bytes at pos, little-endian, zero beyond the end (pos <= n)
//      uniform(v)           v, known to be the same in every lane (host: v)
//      leader(), lane(), lanes(), sync()   the one lane that runs serial table work, the lanes that share parallel table work, and the
//                           barrier between the two (host: true, 0, 1, nothing)
//      room(out, len)       called before `len` <= 258 bytes are emitted at output position `out` (the device flushes its ring)
//      put / copy / raw     emit one literal, a match (length, distance), bytes of the stream itself (a stored block)
//      finish(out)          everything emitted is in the destination;  adler(out): the Adler-32 of the `out` bytes emitted
// The decoder checks every bound before it calls them: out + len <= capacity, distance <= out, pos + len <= n.
//
// Acceptance is zlib's (inflate.c, inftrees.c, without INFLATE_STRICT and without PKZIP_BUG_WORKAROUND): an over-subscribed code set is
// refused; an incomplete one too, except a literal/length or distance set that is one single 1-bit code (the code-length code never);
// a distance set with no code at all is accepted (a block of literals); the end-of-block symbol must have a code; HLIT > 286 and
// HDIST > 30 are refused, and so is any use of literal/length symbols 286 / 287, of distance symbols 30 / 31 (the fixed codes have them)
// and of a code no symbol owns.  The CINFO window claim is checked for <= 7 only.  Bytes after the Adler-32 are ignored.
//
// Work is bounded: every iteration of every loop consumes at least one stream bit or ends the chunk, and an emitting iteration is
// bounded by the capacity; a chunk ends in a Status and a byte count, whatever its bytes are.
#pragma once
#include <stdint.h>

#ifndef SHDR_HD
#if defined(__HIPCC__)
#define SHDR_HD __host__ __device__
#else
#define SHDR_HD
#endif
#endif

namespace shdr_inflate {

enum Status : int {                           // include/shdr.h lists them as SHDR_INFLATE_*; _ops.INFLATE_REASONS names them
  kOk = 0,
  kTruncated = 1,                             // the stream ends inside the header, a block or the Adler-32
  kHeader = 2,                                // CM != 8, CINFO > 7 or the header check (mod 31)
  kDictionary = 3,                            // FDICT
  kBlockType = 4,                             // BTYPE 3
  kStoredLength = 5,                          // LEN != ~NLEN
  kCounts = 6,                                // HLIT > 286 or HDIST > 30
  kCodeLengthSet = 7,                         // the code-length code is over-subscribed or incomplete
  kRepeat = 8,                                // repeat-16 with no previous length
  kRun = 9,                                   // a run overflows HLIT + HDIST
  kNoEndOfBlock = 10,                         // length of symbol 256 is 0
  kLiteralSet = 11,                           // literal/length code set over-subscribed or incomplete
  kDistanceSet = 12,                          // distance code set over-subscribed or incomplete
  kLiteralCode = 13,                          // an unassigned literal/length code, or symbol 286 / 287
  kDistanceCode = 14,                         // an unassigned distance code, or symbol 30 / 31
  kDistanceFar = 15,                          // a distance beyond the bytes produced so far
  kOverflow = 16,                             // the output is longer than the slot
  kShort = 17,                                // the stream is complete and its output shorter than the slot
  kChecksum = 18,                             // Adler-32
  kRawSize = 19,                              // (batch) a stored-raw chunk whose size is not the slot's
  kMode = 20,                                 // (batch) a mode byte other than 0 / 1
  kStatusCount = 21
};

constexpr int kMaxBits = 15;
constexpr int kWindow = 32768;
constexpr int kLitSyms = 288, kDistSyms = 32, kClSyms = 19;
constexpr int kLitBits = 10, kDistBits = 8, kClBits = 7;         // index bits of the one-lookup tables; longer codes walk the counts
constexpr int kMaxMatch = 258;
constexpr int64_t kMaxChunk = (int64_t)1 << 30;
constexpr uint32_t kAdlerMod = 65521;

// A canonical Huffman code: `fast` answers codes of up to P bits in one lookup (symbol << 4 | length; 0: longer, or nobody's), the
// rest is RFC 1951's canonical order: sym sorted by (length, symbol), count / first code / first index per length.
template <int P, int N>
struct Huff {
  uint16_t fast[1 << P];
  uint16_t sym[N];
  uint16_t count[kMaxBits + 1], first[kMaxBits + 1], start[kMaxBits + 1];
  int32_t bad;                                // 0, 1 over-subscribed, 2 incomplete
  int32_t total;
};

struct Tables {                               // LDS on the device (about 4.5 KiB), the stack on the host
  Huff<kLitBits, kLitSyms> lit;
  Huff<kDistBits, kDistSyms> dist;
  Huff<kClBits, kClSyms> cl;
  uint8_t lens[kLitSyms + kDistSyms];
};

// lens[0 .. n) -> h.  codes: the code-length code (no incomplete set at all).  Returns 0, 1 (over-subscribed) or 2 (incomplete).
template <class Io, int P, int N>
SHDR_HD inline int build(Io& io, Huff<P, N>& h, const uint8_t* lens, int n, bool codes) {
  if (io.leader()) {
    for (int b = 0; b <= kMaxBits; ++b) h.count[b] = 0;
    for (int s = 0; s < n; ++s) ++h.count[lens[s]];
    h.count[0] = 0;
    int left = 1, max = 0, bad = 0;
    for (int b = 1; b <= kMaxBits; ++b) {
      left = (left << 1) - (int)h.count[b];
      if (left < 0) {
        bad = 1;
        break;
      }
      if (h.count[b]) max = b;
    }
    if (!bad && left > 0 && (codes ? true : max > 1)) bad = 2;   // max == 0: no code at all (a block of literals); 1: one 1-bit code
    uint32_t code = 0, at = 0;
    for (int b = 1; b <= kMaxBits; ++b) {
      h.first[b] = (uint16_t)code;
      h.start[b] = (uint16_t)at;
      code = (code + h.count[b]) << 1;
      at += h.count[b];
    }
    if (!bad) {
      for (int s = 0; s < n; ++s)
        if (lens[s]) h.sym[h.start[lens[s]]++] = (uint16_t)s;    // start[] runs ahead while it sorts, and is put back
      for (int b = 1; b <= kMaxBits; ++b) h.start[b] = (uint16_t)(h.start[b] - h.count[b]);
    }
    h.total = bad ? 0 : (int32_t)at;
    h.bad = bad;
  }
  for (int e = io.lane(); e < (1 << P); e += io.lanes()) h.fast[e] = 0;
  io.sync();
  const int total = (int)io.uniform((uint32_t)h.total);
  for (int i = io.lane(); i < total; i += io.lanes()) {
    const int s = h.sym[i], l = lens[s];
    if (l <= P) {
      const uint32_t c = (uint32_t)h.first[l] + (uint32_t)(i - h.start[l]);
      uint32_t r = 0;
      for (int b = 0; b < l; ++b) r |= ((c >> b) & 1u) << (l - 1 - b);       // the stream holds codes from their top bit
      for (uint32_t e = r; e < (1u << P); e += 1u << l) h.fast[e] = (uint16_t)(s << 4 | l);
    }
  }
  io.sync();
  return (int)io.uniform((uint32_t)h.bad);
}

// bits come out of the stream from bit 0 of every byte
template <class Io>
struct Bits {
  uint64_t acc;
  int cnt;                                    // bits of acc that are stream bits (the rest is zero)
  int64_t pos, n;                             // next byte to fetch, bytes of the stream
  SHDR_HD inline void fill(Io& io) {          // afterwards cnt >= 33, unless the stream is exhausted
    if (cnt <= 32 && pos < n) {
      const int64_t left = n - pos;
      const int take = left >= 4 ? 4 : (int)left;
      acc |= (uint64_t)io.word(pos) << cnt;
      cnt += 8 * take;
      pos += take;
    }
  }
  SHDR_HD inline uint32_t peek(int k) const { return (uint32_t)acc & ((1u << k) - 1u); }
  SHDR_HD inline void drop(int k) {
    acc >>= k;
    cnt -= k;
  }
};

// One symbol of `h`: >= 0, or -kTruncated / -bad_code.  At most 15 bits are consumed; call fill() first.
template <class Io, int P, int N>
SHDR_HD inline int decode(Io& io, Bits<Io>& b, const Huff<P, N>& h, int bad_code) {
  const uint32_t e = io.uniform(h.fast[b.peek(P)]);
  const int l = (int)(e & 15u);
  if (l) {
    if (l > b.cnt) return -kTruncated;
    b.drop(l);
    return (int)(e >> 4);
  }
  uint32_t code = 0, first = 0, index = 0;
  for (int len = 1; len <= kMaxBits; ++len) {
    if (len > b.cnt) return -kTruncated;
    code |= (uint32_t)(b.acc >> (len - 1)) & 1u;
    const uint32_t count = io.uniform(h.count[len]);
    if (code < first + count) {
      b.drop(len);
      return (int)io.uniform(h.sym[index + (code - first)]);
    }
    index += count;
    first = (first + count) << 1;
    code <<= 1;
  }
  return -bad_code;
}

template <class Io>
SHDR_HD inline int inflate_body(Io& io, Tables& t, int64_t n, int64_t cap, int64_t& out) {
  Bits<Io> b{0, 0, 0, n};
  out = 0;
  b.fill(io);
  if (b.cnt < 16) return kTruncated;
  const uint32_t cmf = b.peek(8), flg = b.peek(16) >> 8;
  b.drop(16);
  if ((cmf & 15u) != 8u || (cmf >> 4) > 7u || ((cmf << 8) | flg) % 31u) return kHeader;
  if (flg & 0x20u) return kDictionary;
  for (;;) {
    b.fill(io);
    if (b.cnt < 3) return kTruncated;
    const uint32_t final_block = b.peek(1), type = b.peek(3) >> 1;
    b.drop(3);
    if (type == 3) return kBlockType;
    if (type == 0) {
      b.drop(b.cnt & 7);
      b.fill(io);
      if (b.cnt < 32) return kTruncated;
      int64_t len = b.peek(16);
      const uint32_t nlen = (uint32_t)(b.acc >> 16) & 0xffffu;
      if (((uint32_t)len ^ 0xffffu) != nlen) return kStoredLength;
      b.drop(32);
      if (len > cap - out) return kOverflow;
      while (len && b.cnt >= 8) {                                // whole bytes that are in the bit buffer already
        io.room(out, 1);
        io.put(out, (uint8_t)b.peek(8));
        b.drop(8);
        ++out;
        --len;
      }
      if (len) {                                                 // the buffer is empty: b.pos is the next byte of the block
        if (len > n - b.pos) return kTruncated;
        while (len) {
          const int piece = len > 256 ? 256 : (int)len;
          io.room(out, piece);
          io.raw(out, b.pos, piece);
          out += piece;
          b.pos += piece;
          len -= piece;
        }
      }
    } else {
      int hlit = kLitSyms, hdist = kDistSyms;
      if (type == 1) {
        if (io.leader()) {
          for (int s = 0; s < kLitSyms; ++s) t.lens[s] = (uint8_t)(s < 144 ? 8 : s < 256 ? 9 : s < 280 ? 7 : 8);
          for (int s = 0; s < kDistSyms; ++s) t.lens[kLitSyms + s] = 5;
        }
      } else {
        const uint8_t order[kClSyms] = {16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15};
        if (b.cnt < 14) return kTruncated;
        hlit = (int)b.peek(5) + 257;
        hdist = (int)(b.peek(10) >> 5) + 1;
        const int hclen = (int)(b.peek(14) >> 10) + 4;
        b.drop(14);
        if (hlit > 286 || hdist > 30) return kCounts;
        for (int i = 0; i < kClSyms; ++i) {
          uint32_t v = 0;
          if (i < hclen) {
            b.fill(io);
            if (b.cnt < 3) return kTruncated;
            v = b.peek(3);
            b.drop(3);
          }
          if (io.leader()) t.lens[order[i]] = (uint8_t)v;
        }
        if (build(io, t.cl, t.lens, kClSyms, true)) return kCodeLengthSet;
        int prev = 0, eob = 0;
        for (int idx = 0; idx < hlit + hdist;) {
          b.fill(io);
          const int s = decode(io, b, t.cl, kCodeLengthSet);     // a complete code: nobody's codes do not exist
          if (s < 0) return -s;
          int rep = 1, val = s;
          if (s == 16) {
            if (idx == 0) return kRepeat;
            if (b.cnt < 2) return kTruncated;
            rep = 3 + (int)b.peek(2);
            val = prev;
            b.drop(2);
          } else if (s == 17) {
            if (b.cnt < 3) return kTruncated;
            rep = 3 + (int)b.peek(3);
            val = 0;
            b.drop(3);
          } else if (s == 18) {
            if (b.cnt < 7) return kTruncated;
            rep = 11 + (int)b.peek(7);
            val = 0;
            b.drop(7);
          }
          if (idx + rep > hlit + hdist) return kRun;
          if (io.leader())
            for (int r = 0; r < rep; ++r) t.lens[idx + r] = (uint8_t)val;
          if (idx <= 256 && 256 < idx + rep) eob = val;
          idx += rep;
          prev = val;
        }
        if (eob == 0) return kNoEndOfBlock;
      }
      if (build(io, t.lit, t.lens, hlit, false)) return kLiteralSet;
      if (build(io, t.dist, t.lens + hlit, hdist, false)) return kDistanceSet;
      for (;;) {
        b.fill(io);
        const int s = decode(io, b, t.lit, kLiteralCode);
        if (s < 0) return -s;
        if (s < 256) {
          if (out >= cap) return kOverflow;
          io.room(out, 1);
          io.put(out, (uint8_t)s);
          ++out;
          continue;
        }
        if (s == 256) break;
        if (s >= 286) return kLiteralCode;
        const int li = s - 257;                                   // lengths 3..10 one per symbol, then four symbols per extra bit
        int len = 258;
        if (li < 8) {
          len = 3 + li;
        } else if (li < 28) {
          const int x = (li >> 2) - 1;
          if (b.cnt < x) return kTruncated;
          len = 3 + ((4 + (li & 3)) << x) + (int)b.peek(x);
          b.drop(x);
        }
        b.fill(io);
        const int d = decode(io, b, t.dist, kDistanceCode);
        if (d < 0) return -d;
        if (d >= 30) return kDistanceCode;
        int dist = 1 + d;                                         // distances 1..4 one per symbol, then two symbols per extra bit
        if (d >= 4) {
          const int x = (d >> 1) - 1;
          if (b.cnt < x) return kTruncated;
          dist = 1 + ((2 + (d & 1)) << x) + (int)b.peek(x);
          b.drop(x);
        }
        if (dist > out) return kDistanceFar;
        if (len > cap - out) return kOverflow;
        io.room(out, len);
        io.copy(out, len, dist);
        out += len;
      }
    }
    if (final_block) break;
  }
  b.drop(b.cnt & 7);
  b.fill(io);
  if (b.cnt < 32) return kTruncated;
  const uint32_t w = (uint32_t)b.acc;
  const uint32_t stored = (w << 24) | ((w & 0xff00u) << 8) | ((w >> 8) & 0xff00u) | (w >> 24);   // big-endian
  io.finish(out);
  if (io.adler(out) != stored) return kChecksum;
  return out == cap ? kOk : kShort;
}

// The zlib stream of n bytes behind `io` into a slot of `cap` bytes: the Status; *written: the bytes emitted (<= cap), all of them in
// the destination.
template <class Io>
SHDR_HD inline int inflate_zlib(Io& io, Tables& t, int64_t n, int64_t cap, int64_t* written) {
  int64_t out = 0;
  const int st = inflate_body(io, t, n, cap, out);
  io.finish(out);
  *written = out;
  return st;
}

// ---- host side ------------------------------------------------------------------------------------------------------------
struct HostIo {
  const uint8_t* src;
  int64_t n;
  uint8_t* dst;
  inline uint32_t word(int64_t pos) const {
    uint32_t w = 0;
    for (int k = 0; k < 4; ++k)
      if (pos + k < n) w |= (uint32_t)src[pos + k] << (8 * k);
    return w;
  }
  static inline uint32_t uniform(uint32_t v) { return v; }
  static inline bool leader() { return true; }
  static inline int lane() { return 0; }
  static inline int lanes() { return 1; }
  static inline void sync() {}
  static inline void room(int64_t, int) {}
  inline void put(int64_t out, uint8_t v) { dst[out] = v; }
  inline void copy(int64_t out, int len, int dist) {
    for (int i = 0; i < len; ++i) dst[out + i] = dst[out - dist + i];
  }
  inline void raw(int64_t out, int64_t pos, int len) {
    for (int i = 0; i < len; ++i) dst[out + i] = src[pos + i];
  }
  static inline void finish(int64_t) {}
  inline uint32_t adler(int64_t out) const {
    uint32_t s1 = 1, s2 = 0;
    for (int64_t i = 0; i < out;) {
      const int64_t end = i + 4096 < out ? i + 4096 : out;       // 4096 * 255 * 4096 / 2 stays below 2^32
      for (; i < end; ++i) {
        s1 += dst[i];
        s2 += s1;
      }
      s1 %= kAdlerMod;
      s2 %= kAdlerMod;
    }
    return (s2 << 16) | s1;
  }
};

// src[0 .. n) into dst[0 .. capacity): the bytes written; *status receives the Status.  -1 for bad arguments.
inline int64_t inflate_host(const uint8_t* src, int64_t n, uint8_t* dst, int64_t capacity, int* status) {
  if (!status || n < 0 || capacity < 0 || capacity > kMaxChunk || (n && !src) || (capacity && !dst)) return -1;
  Tables t;
  HostIo io{src, n, dst};
  int64_t written = 0;
  *status = inflate_zlib(io, t, n, capacity, &written);
  return written;
}

}  // namespace shdr_inflate

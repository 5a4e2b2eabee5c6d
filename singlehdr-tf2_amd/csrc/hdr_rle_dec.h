// The rules of the Radiance scanline reader, once: the candidate test, the packet step, the parse of one coded line and the status
// codes, shared by the host twin shdr_rgbe_rle_decode_status and the device decoder (csrc/hdr_rle_dec.hip), so that both run the
// same checks.  Plain C++: also compiled without HIP (tools/hdr_rle_dec_sweep.cpp).
//
// The law is shdr_rgbe_rle_decode (csrc/api.cpp).  With rle_ok = 8 <= W <= 32767, a line that starts at byte p is CODED when rle_ok,
// p + 4 <= size and the four bytes are 02 02 W>>8 W&255 (p is then a CANDIDATE); otherwise it is FLAT, 4 W bytes copied.  A coded
// line is four components in turn, each a chain of packets until x == W: a count byte n > 128 is a run of n - 128 copies of the next
// byte, any other n is n literal bytes (n == 0 consumes the count byte alone).  Every read is checked against the file's size, every
// write against the line; the first failure in file order wins, and `stop` is where the reader stood when it failed: the offset of
// the count byte of the failing packet (size, when the data ended in front of a count byte) or the start of a flat line cut short.
//
// What makes the grammar parallel: whether p is a candidate and what a parse from p gives depends on the bytes alone, not on the lines
// before.  The line starts of a file are then the orbit of offset 0 under "at a candidate jump to the end of its parse, anywhere else
// step 4 W"; the device parses every candidate at once and follows the orbit afterwards (hdr_rle_dec.hip).
#pragma once
#include <stdint.h>

#ifndef SHDR_HD
#if defined(__HIPCC__)
#define SHDR_HD __host__ __device__
#else
#define SHDR_HD
#endif
#endif

namespace shdr_rle_dec {

// SHDR_RGBE_DEC_* of include/shdr.h (csrc/hdr_rle_dec.hip asserts that they agree)
enum Status { kOk = 0, kTruncated = 1, kCorruptRun = 2, kCorruptLiteral = 3, kTruncatedFlat = 4, kFallback = 5, kStatusCount = 6 };

SHDR_HD inline bool rle_width(int w) { return w >= 8 && w <= 32767; }

// the four bytes at p are the line marker of this width (b0 .. b3: the bytes, read by the caller after the size check)
SHDR_HD inline bool marker_bytes(int b0, int b1, int b2, int b3, int w) { return b0 == 2 && b1 == 2 && ((b2 << 8) | b3) == w; }

SHDR_HD inline bool is_candidate(const uint8_t* data, int64_t size, int64_t p, int w) {
  return rle_width(w) && p >= 0 && size - p >= 4 && marker_bytes(data[p], data[p + 1], data[p + 2], data[p + 3], w);
}

// One packet: the count byte n stands at pos < size, x bytes of the component are done.  kOk: the packet yields *len bytes (a run of
// the byte at pos + 1 when *run, else the bytes pos + 1 .. pos + *len) and the next count byte stands at *next.
SHDR_HD inline int packet_step(int n, int64_t pos, int64_t size, int x, int w, int* len, bool* run, int64_t* next) {
  if (n > 128) {
    const int r = n - 128;
    if (pos + 1 >= size) return kTruncated;
    if (x + r > w) return kCorruptRun;
    *len = r; *run = true; *next = pos + 2;
  } else {
    if (pos + 1 + n > size) return kTruncated;
    if (x + n > w) return kCorruptLiteral;
    *len = n; *run = false; *next = pos + 1 + n;
  }
  return kOk;
}

struct Line {
  int status;            // kOk or the failure
  int64_t end;           // kOk: the first byte after the line
  int64_t stop;          // failure: where the reader stood
  int64_t comp[4];       // the first count byte of every component reached
};

// The coded line whose marker stands at `at` (a candidate).  read(p) returns the byte at p, asked for 0 <= p < size only, in
// ascending order of p.  Every packet consumes at least one byte, so the walk ends.
template <class Read>
SHDR_HD inline void parse_line(Read& read, int64_t size, int64_t at, int w, Line* out) {
  int64_t pos = at + 4;
  out->end = out->stop = -1;
  for (int c = 0; c < 4; ++c) out->comp[c] = -1;
  for (int c = 0; c < 4; ++c) {
    out->comp[c] = pos;
    int x = 0;
    while (x < w) {
      int st = kTruncated, len = 0;
      bool run = false;
      int64_t next = pos;
      if (pos < size) st = packet_step(read(pos), pos, size, x, w, &len, &run, &next);
      if (st != kOk) {
        out->status = st;
        out->stop = pos;
        return;
      }
      x += len;
      pos = next;
    }
  }
  out->status = kOk;
  out->end = pos;
}

struct HostRead {
  const uint8_t* data;
  SHDR_HD int operator()(int64_t p) const { return data[p]; }
};

// The pixels of a line that parse_line accepted: component c from its first count byte.  Every write is checked against the line again.
inline void expand_line_host(const uint8_t* data, int64_t size, const Line& l, int w, uint8_t* line) {
  for (int c = 0; c < 4; ++c) {
    int64_t pos = l.comp[c];
    int x = 0;
    while (x < w) {
      int len = 0;
      bool run = false;
      int64_t next = pos;
      if (pos >= size || packet_step(data[pos], pos, size, x, w, &len, &run, &next) != kOk) return;
      for (int i = 0; i < len; ++i) line[4 * (x + i) + c] = data[pos + 1 + (run ? 0 : i)];
      x += len;
      pos = next;
    }
  }
}

// The serial reader written from the rules above: `size` bytes of scanline data -> rgbe [height][width][4].  Returns the bytes consumed
// and kOk in *status, or -1 with the failure, the failing scanline and the stop offset.  data may be NULL when size is 0.
inline int64_t decode_serial(const uint8_t* data, int64_t size, int width, int height, uint8_t* rgbe, int* status, int* line,
                             int64_t* stop) {
  int64_t pos = 0;
  const HostRead read{data};
  for (int y = 0; y < height; ++y) {
    uint8_t* dst = rgbe + (int64_t)y * width * 4;
    if (is_candidate(data, size, pos, width)) {
      Line l;
      parse_line(read, size, pos, width, &l);
      if (l.status != kOk) {
        *status = l.status; *line = y; *stop = l.stop;
        return -1;
      }
      expand_line_host(data, size, l, width, dst);
      pos = l.end;
    } else {
      if (size - pos < 4 * (int64_t)width) {
        *status = kTruncatedFlat; *line = y; *stop = pos;
        return -1;
      }
      for (int64_t i = 0; i < 4 * (int64_t)width; ++i) dst[i] = data[pos + i];
      pos += 4 * (int64_t)width;
    }
  }
  *status = kOk; *line = -1; *stop = pos;
  return pos;
}

}  // namespace shdr_rle_dec

// The entropy-coded scan of a baseline JPEG file prepared for the decoder (csrc/jpeg.hip): where the scan ends, which bytes are kept
// (FF 00 stuffing and RSTn markers removed), where the restart segments begin, and where every kept byte lies in the dword-aligned
// segment arena.  Everything whose correctness is about bytes and bounds, shared by the kernels (csrc/jpeg_scan.hip) and the host twin
// shdr_jpeg_scan_host, so that both apply the same rules.  Plain C++: also compiled without HIP (tools/jpeg_scan_sweep.cpp).
//
// A scan region is b[0 .. n): the file from the first byte after the SOS header to its end.  The rules are those of jpeg.parse and
// jpeg.unstuff (jpeg.py), each a function of a byte, its two neighbours and `end` alone:
//      marker at p     p + 1 < n, b[p] == FF, b[p + 1] not 00, not FF, not D0 .. D7 (a final lone FF is no marker)
//      end             the smallest marker position, or none; the end marker is b[end + 1]; nothing at or after `end` counts
//      restart at p    p < end, b[p] == FF, b[p + 1] in D0 .. D7: neither byte is kept, a new segment starts after them
//      stuffing        a 00 whose preceding raw byte is FF is dropped
//      fill            FF FF at p < end sets the fill flag (both bytes are kept: the file is refused on the flag)
// Restart marker k (from 0) of an image has a boundary: the number of kept bytes before it.  An image stores at most seg_cap - 1 of
// them, seg_cap being the segment count its header implies; further markers are counted and never stored (bound_slot).  Segment s
// holds the kept bytes between boundary s - 1 (0 for the first) and boundary s; kept byte number j of the image goes to
// arena[seg_dword[s] * 4 + (j - boundary of s)], and nowhere if that is outside the arena (arena_index).
#pragma once
#include <stdint.h>

#ifndef SHDR_HD
#if defined(__HIPCC__)
#define SHDR_HD __host__ __device__
#else
#define SHDR_HD
#endif
#endif

namespace jpegscan {

constexpr int kTile = 4096;                   // raw bytes per workgroup tile: 256 lanes x 16 bytes (SHDR_JPEG_SCAN_TILE, jpeg.SCAN_TILE)
constexpr int kScanChunk = 256;               // tiles per workgroup of the cross-tile prefix sum: one region of more than
                                              // kTile * kScanChunk = 1 MiB spans two of them
constexpr int64_t kNone = -1;                 // Report::end of a region without an end marker; an unwritten boundary slot
constexpr int64_t kMaxBytes = (int64_t)1 << 33;       // raw bytes of a batch, as shdr_jpeg_batch.data_bytes
constexpr int kMaxImages = 65535;

struct Image {                                // mirror of shdr_jpeg_scan_image (include/shdr.h)
  int64_t offset;                             // first byte of the region in the source buffer, a multiple of 16
  int64_t length;                             // n
  int64_t first_tile;                         // tiles of the images before it; it has ceil(n / kTile)
  int32_t seg_cap;                            // >= 1
  int32_t first_bound;                        // its first boundary slot: the sum of seg_cap - 1 over the images before it
  int32_t first_seg;                          // its first segment: the sum of seg_cap over the images before it
  int32_t reserved;
};

struct Report {                               // mirror of shdr_jpeg_scan_report
  int64_t end;                                // position of the end marker's FF in the region, kNone if there is none
  int64_t kept;                               // kept bytes before `end` (before n without an end)
  int32_t n_rst;                              // restart markers before `end`, however many slots there are
  int32_t fill;                               // 1: FF FF before `end`
  int32_t end_marker;                         // b[end + 1], -1 without an end
  int32_t reserved;
};

enum : uint32_t { kMarker = 1, kRestart = 2, kFill = 4, kDropped = 8 };

// the class of byte `cur`; prev / next: its neighbours in the region, -1 where the region ends.  kMarker, kRestart and kFill speak of
// the pair that begins at this byte, kDropped of this byte.  Only meaningful before `end`, except kMarker, which defines it.
SHDR_HD inline uint32_t byte_class(int prev, int cur, int next) {
  uint32_t c = 0;
  if (cur == 0xFF && next >= 0) {
    if (next >= 0xD0 && next <= 0xD7) c |= kRestart | kDropped;
    else if (next == 0xFF) c |= kFill;
    else if (next != 0x00) c |= kMarker;
  }
  if (prev == 0xFF && (cur == 0x00 || (cur >= 0xD0 && cur <= 0xD7))) c |= kDropped;
  return c;
}

// the slot of restart marker k of `im`, or -1: the markers beyond the seg_cap - 1 that the header implies have none
SHDR_HD inline int64_t bound_slot(const Image& im, int64_t k) {
  return k >= 0 && k < (int64_t)im.seg_cap - 1 ? (int64_t)im.first_bound + k : -1;
}

// the segment of a byte with `rst_before` restart markers before it: what lies beyond the last segment stays in the last
SHDR_HD inline int64_t segment_of(const Image& im, int64_t rst_before) {
  const int64_t s = rst_before < (int64_t)im.seg_cap - 1 ? rst_before : (int64_t)im.seg_cap - 1;
  return (int64_t)im.first_seg + (s < 0 ? 0 : s);
}

// the boundary at which segment `seg` (segment_of) begins; bounds: the batch's slots
SHDR_HD inline int64_t segment_start(const Image& im, int64_t seg, const int64_t* bounds) {
  return seg == im.first_seg ? 0 : bounds[(int64_t)im.first_bound + (seg - im.first_seg) - 1];
}

// the arena position of kept byte number `kept_before` of its image, -1 if it has none inside [0, arena_bytes)
SHDR_HD inline int64_t arena_index(int64_t seg_dword, int64_t seg_start, int64_t kept_before, int64_t arena_bytes) {
  if (seg_start < 0 || kept_before < seg_start || seg_dword < 0 || seg_dword > (arena_bytes >> 2)) return -1;
  const int64_t i = seg_dword * 4 + (kept_before - seg_start);
  return i < arena_bytes ? i : -1;
}

enum Check : int { kOk = 0, kBadCount, kBadRegion, kBadTiles, kBadSlots, kCheckCount };
inline const char* check_text(int c) {
  static const char* const text[kCheckCount] = {
      "ok", "the number of images must be 1 .. 65535 and the source at most 2^33 bytes",
      "a region must start on a multiple of 16, have a length >= 0 and lie inside the source buffer",
      "first_tile must be the number of tiles of the images before it", "seg_cap must be >= 1, first_bound and first_seg the sums over "
      "the images before it, and the boundary and segment arrays must hold them all"};
  return c >= 0 && c < kCheckCount ? text[c] : "?";
}

// the descriptors as kernels and host twin trust them; *bad: the first image that fails; n_segs < 0: no segment array yet (the scan)
inline int check_images(const Image* im, int n_images, int64_t src_bytes, int64_t n_bounds, int64_t n_segs, int64_t* n_tiles, int* bad) {
  *bad = -1;
  if (n_images < 1 || n_images > kMaxImages || src_bytes < 0 || src_bytes >= kMaxBytes) return kBadCount;
  int64_t tiles = 0, slots = 0, segs = 0;
  for (int i = 0; i < n_images; ++i) {
    *bad = i;
    if (im[i].offset < 0 || (im[i].offset & 15) || im[i].length < 0 || im[i].offset > src_bytes || im[i].length > src_bytes - im[i].offset)
      return kBadRegion;
    if (im[i].first_tile != tiles) return kBadTiles;
    if (im[i].seg_cap < 1 || im[i].first_bound != slots || im[i].first_seg != segs) return kBadSlots;
    tiles += (im[i].length + kTile - 1) / kTile;
    slots += im[i].seg_cap - 1;
    segs += im[i].seg_cap;
    if (slots > n_bounds || segs > (int64_t)INT32_MAX || (n_segs >= 0 && segs > n_segs)) return kBadSlots;
  }
  *bad = -1;
  *n_tiles = tiles;
  return kOk;
}

// ---------------------------------------------------------------- the host twin: one region, byte by byte
inline int at(const uint8_t* b, int64_t n, int64_t p) { return p >= 0 && p < n ? (int)b[p] : -1; }

// report and boundaries of image `im`; src: the batch's source buffer; the slots of `im` are all written (kNone where no marker fills them)
inline void scan_host(const uint8_t* src, const Image& im, Report* rep, int64_t* bounds) {
  const uint8_t* b = src + im.offset;
  const int64_t n = im.length;
  for (int64_t k = 0; k < (int64_t)im.seg_cap - 1; ++k) bounds[im.first_bound + k] = kNone;
  int64_t end = kNone;
  for (int64_t p = 0; p < n; ++p)
    if (byte_class(at(b, n, p - 1), b[p], at(b, n, p + 1)) & kMarker) {
      end = p;
      break;
    }
  const int64_t stop = end == kNone ? n : end;
  int64_t kept = 0, rst = 0;
  int fill = 0;
  for (int64_t p = 0; p < stop; ++p) {
    const uint32_t c = byte_class(at(b, n, p - 1), b[p], at(b, n, p + 1));
    if (c & kRestart) {
      const int64_t slot = bound_slot(im, rst);
      if (slot >= 0) bounds[slot] = kept;
      ++rst;
    }
    if (c & kFill) fill = 1;
    if (!(c & kDropped)) ++kept;
  }
  rep->end = end;
  rep->kept = kept;
  rep->n_rst = (int32_t)rst;
  rep->fill = fill;
  rep->end_marker = end == kNone ? -1 : (int)b[end + 1];
  rep->reserved = 0;
}

// the kept bytes of image `im` into the arena (which the caller has filled with FF); end: Report::end of scan_host
inline void compact_host(const uint8_t* src, const Image& im, int64_t end, const int64_t* bounds, const int32_t* seg_dword, int seg_stride,
                         uint8_t* arena, int64_t arena_bytes) {
  const uint8_t* b = src + im.offset;
  const int64_t n = im.length;
  const int64_t stop = end == kNone || end > n ? n : end;
  int64_t kept = 0, rst = 0;
  for (int64_t p = 0; p < stop; ++p) {
    const uint32_t c = byte_class(at(b, n, p - 1), b[p], at(b, n, p + 1));
    if (!(c & kDropped)) {
      const int64_t seg = segment_of(im, rst);
      const int64_t i = arena_index(seg_dword[seg * seg_stride], segment_start(im, seg, bounds), kept, arena_bytes);
      if (i >= 0) arena[i] = b[p];
      ++kept;
    }
    if (c & kRestart) ++rst;
  }
}

}  // namespace jpegscan

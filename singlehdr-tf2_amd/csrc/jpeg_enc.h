// Baseline-JPEG writer: everything the kernels (csrc/jpeg_enc.hip) and the host twin (shdr_jpeg_encode_host and its two stages,
// csrc/api.cpp) must agree on, so that both write the file libjpeg writes for the same pixels, quality, subsampling and restart
// interval -- byte for byte what PIL's Image.save(..., "JPEG", quality=, subsampling=, restart_marker_blocks=) gives.  Plain C++: also
// compiled without HIP (tools/jpeg_enc_sweep.cpp).  The integer colour conversion, box filters and forward DCT are jpeg_int.h.
//
// Grid and scan order.  Layout 0 / 1 / 2 = 4:4:4 / 4:2:2 / 4:2:0: Y is sampled h x v = 1x1 / 2x1 / 2x2, Cb and Cr 1x1.  An MCU covers
// 8h x 8v pixels and holds h*v Y blocks (row-major inside the MCU), then the Cb block, then the Cr block; the scan walks the MCUs row by
// row.  A coefficient arena is int16 [blocks][64] in exactly that order, every block in zig-zag order, dummy blocks included.
//
// Edges (jcprepct.c, jcsample.c, jccoefct.c):
//   bottom   the image is replicated downwards at full resolution only up to a multiple of v; the DOWNSAMPLED rows are then replicated:
//            chroma row j reads the full-resolution rows v * jj + dy, jj = min(j, ceil(H / v) - 1), each clamped to H - 1
//   right    every component is replicated at full resolution, then downsampled: chroma column i reads columns h * i + dx clamped to
//            W - 1; the box filter's bias alternates along the whole row (jpeg_int.h)
//   dummies  a Y block of an MCU beyond ceil(W / 8) block columns or ceil(H / 8) block rows has no AC and the DC of the block before it
//            in the MCU (so a dummy row starts from the last block of the row above).  Chroma blocks are never dummies.
//
// Entropy coding (T.81 F.1.2): the Annex-K tables; a DC is coded as the difference to the previous block of its component in scan order,
// 0 at the start of a restart segment.  A segment is `restart` MCUs (all of them if restart is 0); its last byte is padded with 1-bits,
// every FF byte of it is followed by a 00, and segment k (from 0) of an image is followed by the marker FF D0 + (k mod 8) unless it
// is the last.  Baseline range: an AC of category > 10 or a DC difference of category > 11 cannot be coded.
#pragma once
#include <stdint.h>

#include "jpeg_int.h"

#ifndef SHDR_HD
#if defined(__HIPCC__)
#define SHDR_HD __host__ __device__
#else
#define SHDR_HD
#endif
#endif

namespace jpegenc {

constexpr int kHeaderMax = 640;               // SHDR_JPEG_ENC_HEADER_MAX: 623 bytes from SOI to the end of SOS, 629 with a DRI segment
constexpr int kMaxDim = 65535;
constexpr int kMaxImages = 65535;
constexpr int kBlockBits = 1664;              // a block takes at most 11 + 11 + 63 * (16 + 10) = 1660 bits
constexpr int kBlockWords = kBlockBits / 32;
constexpr int64_t kMaxBlocks = (int64_t)1 << 25;      // blocks of a call: 32 bits of arena position and of stuffed size hold them all
enum Status : int32_t { kOk = 0, kOutOfRange = 1 };   // SHDR_JPEG_ENC_*: the per-image status word

struct Image {                                // mirror of shdr_jpeg_enc_image (include/shdr.h)
  int32_t height, width;
  int32_t layout;                             // 0: 4:4:4, 1: 4:2:2, 2: 4:2:0
  int32_t quality;                            // 1 .. 100
  int32_t restart;                            // MCUs per restart segment, 0: one segment
  int32_t reserved;
};

struct Geometry {
  int h, v, hv, nbm;                          // Y sampling, Y blocks per MCU, blocks per MCU
  int mcus_x, mcus_y;
  int ywib, yhib;                             // Y blocks across and down that hold image samples
  int crows;                                  // downsampled chroma rows made from image rows: ceil(H / v)
  int64_t mcus, blocks, segments;
};

SHDR_HD inline bool image_ok(const Image& im) {
  return im.height >= 1 && im.height <= kMaxDim && im.width >= 1 && im.width <= kMaxDim && im.layout >= 0 && im.layout <= 2 &&
         im.quality >= 1 && im.quality <= 100 && im.restart >= 0 && im.restart <= 65535;
}

SHDR_HD inline Geometry geometry(const Image& im) {
  Geometry g;
  g.h = im.layout == 0 ? 1 : 2;
  g.v = im.layout == 2 ? 2 : 1;
  g.hv = g.h * g.v;
  g.nbm = g.hv + 2;
  g.mcus_x = (im.width + 8 * g.h - 1) / (8 * g.h);
  g.mcus_y = (im.height + 8 * g.v - 1) / (8 * g.v);
  g.ywib = (im.width + 7) / 8;
  g.yhib = (im.height + 7) / 8;
  g.crows = (im.height + g.v - 1) / g.v;
  g.mcus = (int64_t)g.mcus_x * g.mcus_y;
  g.blocks = g.mcus * g.nbm;
  g.segments = im.restart > 0 ? (g.mcus + im.restart - 1) / im.restart : 1;
  return g;
}

// ---------------------------------------------------------------- the edge rules
SHDR_HD inline int imin(int a, int b) { return a < b ? a : b; }
// the full-resolution row / column that sample (dy, dx) of downsampled chroma sample (j, i) reads
SHDR_HD inline int chroma_src_row(const Geometry& g, int height, int j, int dy) { return imin(g.v * imin(j, g.crows - 1) + dy, height - 1); }
SHDR_HD inline int chroma_src_col(const Geometry& g, int width, int i, int dx) { return imin(g.h * i + dx, width - 1); }
// Y block r of MCU (my, mx) holds no image sample
SHDR_HD inline bool y_block_dummy(const Geometry& g, int my, int mx, int r) { return mx * g.h + r % g.h >= g.ywib || my * g.v + r / g.h >= g.yhib; }

// ---------------------------------------------------------------- quantiser and zig-zag
// entry `natural` (row * 8 + column) of the IJG-scaled Annex-K table, clamped to 1 .. 255 (jcparam.c, force_baseline)
SHDR_HD inline int quant_value(int natural, bool chroma, int quality) {
  constexpr uint8_t luma[64] = {16, 11, 10, 16, 24, 40, 51, 61, 12, 12, 14, 19, 26, 58, 60, 55, 14, 13, 16, 24, 40, 57, 69, 56,
                                14, 17, 22, 29, 51, 87, 80, 62, 18, 22, 37, 56, 68, 109, 103, 77, 24, 35, 55, 64, 81, 104, 113, 92,
                                49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112, 100, 103, 99};
  constexpr uint8_t chro[64] = {17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99, 99, 99,
                                47, 66, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99,
                                99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99};
  const int q = quality < 1 ? 1 : (quality > 100 ? 100 : quality);
  const int scale = q < 50 ? 5000 / q : 200 - 2 * q;
  const int t = ((chroma ? chro[natural] : luma[natural]) * scale + 50) / 100;
  return t < 1 ? 1 : (t > 255 ? 255 : t);
}
// jcdctmgr.c: the DCT output is scaled by 8; round half up on the magnitude, the sign restored
SHDR_HD inline int quantise(int c, int tq) {
  const int a = ((c < 0 ? -c : c) + 4 * tq) / (8 * tq);
  return c < 0 ? -a : a;
}
// the natural index of zig-zag position k, and the zig-zag position of a natural index
SHDR_HD inline int zigzag_natural(int k) {
  constexpr uint8_t t[64] = {0,  1,  8,  16, 9,  2,  3,  10, 17, 24, 32, 25, 18, 11, 4,  5,  12, 19, 26, 33, 40, 48,
                             41, 34, 27, 20, 13, 6,  7,  14, 21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23,
                             30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};
  return t[k];
}
SHDR_HD inline int zigzag_position(int natural) {
  constexpr uint8_t t[64] = {0,  1,  5,  6,  14, 15, 27, 28, 2,  4,  7,  13, 16, 26, 29, 42, 3,  8,  12, 17, 25, 30,
                             41, 43, 9,  11, 18, 24, 31, 40, 44, 53, 10, 19, 23, 32, 39, 45, 52, 54, 20, 22, 33, 38,
                             46, 51, 55, 60, 21, 34, 37, 47, 50, 56, 59, 61, 35, 36, 48, 49, 57, 58, 62, 63};
  return t[natural];
}

// ---------------------------------------------------------------- the four standard Huffman tables (T.81 K.3 - K.6)
struct HuffSpec {
  uint8_t counts[16];
  int nsym;
  uint8_t symbols[162];
};
constexpr HuffSpec kDcLuma = {{0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0}, 12, {0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11}};
constexpr HuffSpec kDcChroma = {{0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0}, 12, {0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11}};
constexpr HuffSpec kAcLuma = {
    {0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 0x7d},
    162,
    {0x01, 0x02, 0x03, 0x00, 0x04, 0x11, 0x05, 0x12, 0x21, 0x31, 0x41, 0x06, 0x13, 0x51, 0x61, 0x07, 0x22, 0x71, 0x14, 0x32, 0x81,
     0x91, 0xa1, 0x08, 0x23, 0x42, 0xb1, 0xc1, 0x15, 0x52, 0xd1, 0xf0, 0x24, 0x33, 0x62, 0x72, 0x82, 0x09, 0x0a, 0x16, 0x17, 0x18,
     0x19, 0x1a, 0x25, 0x26, 0x27, 0x28, 0x29, 0x2a, 0x34, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48,
     0x49, 0x4a, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58, 0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a, 0x73, 0x74, 0x75,
     0x76, 0x77, 0x78, 0x79, 0x7a, 0x83, 0x84, 0x85, 0x86, 0x87, 0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99,
     0x9a, 0xa2, 0xa3, 0xa4, 0xa5, 0xa6, 0xa7, 0xa8, 0xa9, 0xaa, 0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3,
     0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4, 0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda, 0xe1, 0xe2, 0xe3, 0xe4, 0xe5,
     0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf1, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9, 0xfa}};
constexpr HuffSpec kAcChroma = {
    {0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 0x77},
    162,
    {0x00, 0x01, 0x02, 0x03, 0x11, 0x04, 0x05, 0x21, 0x31, 0x06, 0x12, 0x41, 0x51, 0x07, 0x61, 0x71, 0x13, 0x22, 0x32, 0x81, 0x08,
     0x14, 0x42, 0x91, 0xa1, 0xb1, 0xc1, 0x09, 0x23, 0x33, 0x52, 0xf0, 0x15, 0x62, 0x72, 0xd1, 0x0a, 0x16, 0x24, 0x34, 0xe1, 0x25,
     0xf1, 0x17, 0x18, 0x19, 0x1a, 0x26, 0x27, 0x28, 0x29, 0x2a, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47,
     0x48, 0x49, 0x4a, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58, 0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a, 0x73, 0x74,
     0x75, 0x76, 0x77, 0x78, 0x79, 0x7a, 0x82, 0x83, 0x84, 0x85, 0x86, 0x87, 0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97,
     0x98, 0x99, 0x9a, 0xa2, 0xa3, 0xa4, 0xa5, 0xa6, 0xa7, 0xa8, 0xa9, 0xaa, 0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba,
     0xc2, 0xc3, 0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4, 0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda, 0xe2, 0xe3, 0xe4,
     0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9, 0xfa}};

// code / length arrays: entry[symbol] = length << 16 | code, 0 for a symbol the table does not hold (canonical codes, T.81 Annex C)
struct CodeTable {
  uint32_t entry[256];
};
constexpr CodeTable make_codes(const HuffSpec& s) {
  CodeTable t = {};
  uint32_t code = 0;
  int k = 0;
  for (int length = 1; length <= 16; ++length) {
    for (int i = 0; i < s.counts[length - 1]; ++i) t.entry[s.symbols[k++]] = (uint32_t)length << 16 | code++;
    code <<= 1;
  }
  return t;
}
struct CodeTables {
  CodeTable t[4];                             // slot = 2 * (component is chroma) + (AC)
};
constexpr CodeTables kCodes = {{make_codes(kDcLuma), make_codes(kAcLuma), make_codes(kDcChroma), make_codes(kAcChroma)}};

// ---------------------------------------------------------------- the bits of a block
// category (size) of a value and the category's extra bits
SHDR_HD inline int category(int v) {
  int a = v < 0 ? -v : v, s = 0;
  while (a) {
    ++s;
    a >>= 1;
  }
  return s;
}
SHDR_HD inline uint32_t extra_bits(int v, int s) { return (uint32_t)(v >= 0 ? v : v + (1 << s) - 1); }

// The codes of one block, in order, given to put(code, length) (length <= 27: a code and its extra bits together); zz(k): coefficient
// k of the zig-zag order; pred: the DC the difference is taken to.  Returns false, having put nothing more, at a coefficient outside
// the baseline range.  tables: kCodes or a copy of it.
template <class Z, class Put>
SHDR_HD inline bool code_block(const CodeTables& tables, const Z& zz, int pred, bool chroma, Put&& put) {
  const CodeTable& dc = tables.t[chroma ? 2 : 0];
  const CodeTable& ac = tables.t[chroma ? 3 : 1];
  const int diff = zz(0) - pred;
  int s = category(diff);
  if (s > 11) return false;
  uint32_t e = dc.entry[s];
  put((e & 0xffffu) << s | extra_bits(diff, s), (int)(e >> 16) + s);
  int run = 0;
#if defined(__HIPCC__)
#pragma unroll                                // (the kernels keep the block in registers)
#endif
  for (int k = 1; k < 64; ++k) {
    const int v = zz(k);
    if (v == 0) {
      ++run;
      continue;
    }
    s = category(v);
    if (s > 10) return false;
    for (; run > 15; run -= 16) {
      e = ac.entry[0xF0];
      put(e & 0xffffu, (int)(e >> 16));
    }
    e = ac.entry[run << 4 | s];
    put((e & 0xffffu) << s | extra_bits(v, s), (int)(e >> 16) + s);
    run = 0;
  }
  if (run) {
    e = ac.entry[0x00];
    put(e & 0xffffu, (int)(e >> 16));
  }
  return true;
}

// the block (of the image's arena) whose DC block b is predicted from, -1: predicted from 0 (the start of a restart segment)
SHDR_HD inline int64_t pred_block(const Geometry& g, int restart, int64_t b) {
  const int64_t m = b / g.nbm;
  const int k = (int)(b % g.nbm);
  if (k > 0 && k < g.hv) return b - 1;                          // a Y block after another of the same MCU
  if (m == 0 || (restart > 0 && m % restart == 0)) return -1;
  return k == 0 ? (m - 1) * g.nbm + g.hv - 1 : b - g.nbm;      // the last Y block, or the same chroma block, of the MCU before
}
SHDR_HD inline bool block_is_chroma(const Geometry& g, int64_t b) { return (int)(b % g.nbm) >= g.hv; }
// the restart segment of block b, and the first block of segment s
SHDR_HD inline int64_t segment_of_block(const Geometry& g, int restart, int64_t b) { return restart > 0 ? b / g.nbm / restart : 0; }
SHDR_HD inline int64_t segment_first_block(const Geometry& g, int restart, int64_t s) {
  if (restart <= 0) return s <= 0 ? 0 : g.blocks;
  const int64_t b = s * restart * g.nbm;
  return b < g.blocks ? b : g.blocks;
}
SHDR_HD inline int rst_marker(int64_t k) { return 0xD0 + (int)(k & 7); }

// what a caller has to provide: bytes of a file at the very most, and 32-bit words of the unstuffed scan
SHDR_HD inline int64_t out_bound(const Geometry& g) { return kHeaderMax + g.blocks * (2 * kBlockBits / 8) + g.segments * 4 + 2; }
SHDR_HD inline int64_t arena_words_bound(const Geometry& g) { return g.blocks * kBlockWords + 2 * g.segments + 2; }

// ---------------------------------------------------------------- the transform of one MCU (the host twin's; the kernel does the same per lane)
// pixel(y, x, rgb[3]): the 8-bit pixel of the image.  out: g.nbm blocks of 64 int16, zig-zag order.
template <class Pixel>
inline void transform_mcu(const Image& im, const Geometry& g, int my, int mx, const Pixel& pixel, int16_t* out) {
  using namespace shdr::jpegint;
  int blk[6][64];
  const int mw = 8 * g.h, mh = 8 * g.v;
  auto ycc_at = [&](int y, int x, int* ycc) {
    int rgb[3];
    pixel(y, x, rgb);
    rgb_to_ycc(rgb[0], rgb[1], rgb[2], ycc[0], ycc[1], ycc[2]);
  };
  for (int py = 0; py < mh; ++py)
    for (int px = 0; px < mw; ++px) {
      int ycc[3];
      ycc_at(imin(my * mh + py, im.height - 1), imin(mx * mw + px, im.width - 1), ycc);
      blk[(py >> 3) * g.h + (px >> 3)][(py & 7) * 8 + (px & 7)] = ycc[0] - 128;
    }
  for (int cy = 0; cy < 8; ++cy)
    for (int cx = 0; cx < 8; ++cx) {
      const int j = my * 8 + cy, i = mx * 8 + cx;
      int s[2][2][3];
      for (int dy = 0; dy < g.v; ++dy)
        for (int dx = 0; dx < g.h; ++dx) ycc_at(chroma_src_row(g, im.height, j, dy), chroma_src_col(g, im.width, i, dx), s[dy][dx]);
      for (int c = 1; c < 3; ++c) {
        const int val = g.hv == 4 ? box_h2v2(s[0][0][c], s[0][1][c], s[1][0][c], s[1][1][c], i)
                      : g.hv == 2 ? box_h2v1(s[0][0][c], s[0][1][c], i) : s[0][0][c];
        blk[g.hv + c - 1][cy * 8 + cx] = val - 128;
      }
    }
  for (int b = 0; b < g.nbm; ++b) {
    for (int r = 0; r < 8; ++r) fdct_1d(&blk[b][r * 8], 1, true);
    for (int c = 0; c < 8; ++c) fdct_1d(&blk[b][c], 8, false);
    int16_t* o = out + b * 64;
    const bool dummy = b < g.hv && y_block_dummy(g, my, mx, b);
    for (int n = 0; n < 64; ++n)
      o[zigzag_position(n)] = dummy ? (int16_t)0 : (int16_t)quantise(blk[b][n], quant_value(n, b >= g.hv, im.quality));
    if (dummy) o[0] = o[-64];
  }
}

// pixels uint8 [H][W][3] -> coef int16 [g.blocks][64]
inline void transform_host(const uint8_t* rgb, const Image& im, int16_t* coef) {
  const Geometry g = geometry(im);
  auto pixel = [&](int y, int x, int* out) {
    const uint8_t* p = rgb + ((int64_t)y * im.width + x) * 3;
    out[0] = p[0]; out[1] = p[1]; out[2] = p[2];
  };
  for (int my = 0; my < g.mcus_y; ++my)
    for (int mx = 0; mx < g.mcus_x; ++mx) transform_mcu(im, g, my, mx, pixel, coef + ((int64_t)my * g.mcus_x + mx) * g.nbm * 64);
}

// ---------------------------------------------------------------- header
// SOI, APP0 (JFIF 1.01, no density unit, 1:1), DQT 0, DQT 1, SOF0, DHT DC0, AC0, DC1, AC1, DRI if restart > 0, SOS: the bytes up to
// the first byte of the scan.  out: kHeaderMax bytes; returns the length.
SHDR_HD inline int header_length(const Image& im) { return im.restart > 0 ? 629 : 623; }
inline int compose_header(const Image& im, uint8_t* out) {
  const Geometry g = geometry(im);
  int n = 0;
  auto put = [&](int b) { out[n++] = (uint8_t)b; };
  auto put16 = [&](int v) { put(v >> 8); put(v & 255); };
  put(0xFF); put(0xD8);
  put(0xFF); put(0xE0); put16(16);
  for (const char* s = "JFIF"; *s; ++s) put(*s);
  put(0); put(1); put(1); put(0); put16(1); put16(1); put(0); put(0);
  for (int t = 0; t < 2; ++t) {
    put(0xFF); put(0xDB); put16(67); put(t);
    for (int k = 0; k < 64; ++k) put(quant_value(zigzag_natural(k), t == 1, im.quality));
  }
  put(0xFF); put(0xC0); put16(17); put(8); put16(im.height); put16(im.width); put(3);
  put(1); put(g.h << 4 | g.v); put(0);
  put(2); put(0x11); put(1);
  put(3); put(0x11); put(1);
  const HuffSpec* specs[4] = {&kDcLuma, &kAcLuma, &kDcChroma, &kAcChroma};
  for (int t = 0; t < 4; ++t) {
    put(0xFF); put(0xC4); put16(19 + specs[t]->nsym); put((t & 1) << 4 | t >> 1);
    for (int k = 0; k < 16; ++k) put(specs[t]->counts[k]);
    for (int k = 0; k < specs[t]->nsym; ++k) put(specs[t]->symbols[k]);
  }
  if (im.restart > 0) {
    put(0xFF); put(0xDD); put16(4); put16(im.restart);
  }
  put(0xFF); put(0xDA); put16(12); put(3);
  put(1); put(0x00); put(2); put(0x11); put(3); put(0x11);
  put(0); put(63); put(0);
  return n;
}

// ---------------------------------------------------------------- the entropy stage on the host
// coef int16 [g.blocks][64] -> the scan: the stuffed segments with the RSTn markers between them.  Returns the byte count, or
// kRangeError with *bad_block set, or kCapacityError; nothing is written at or past out + capacity.
constexpr int64_t kRangeError = -2, kCapacityError = -3;
inline int64_t entropy_host(const int16_t* coef, const Image& im, uint8_t* out, int64_t capacity, int64_t* bad_block) {
  const Geometry g = geometry(im);
  int64_t n = 0;
  bool fits = true;
  uint64_t acc = 0;                           // the low `nbits` bits are pending
  int nbits = 0;
  auto byte_out = [&](uint32_t b) {
    for (int rep = 0; rep < (b == 0xFF ? 2 : 1); ++rep) {
      if (n < capacity) out[n] = rep ? (uint8_t)0 : (uint8_t)b;
      else fits = false;
      ++n;
    }
  };
  auto put = [&](uint32_t code, int len) {
    acc = acc << len | code;
    nbits += len;
    while (nbits >= 8) {
      nbits -= 8;
      byte_out((uint32_t)(acc >> nbits) & 255u);
    }
  };
  auto raw_out = [&](int b) {
    if (n < capacity) out[n] = (uint8_t)b;
    else fits = false;
    ++n;
  };
  for (int64_t b = 0; b < g.blocks; ++b) {
    const int64_t seg = segment_of_block(g, im.restart, b);
    if (b > 0 && b == segment_first_block(g, im.restart, seg)) {
      if (nbits) put((1u << (8 - nbits)) - 1, 8 - nbits);
      raw_out(0xFF);
      raw_out(rst_marker(seg - 1));
    }
    const int64_t pb = pred_block(g, im.restart, b);
    const int16_t* zz = coef + b * 64;
    if (!code_block(kCodes, [&](int k) { return (int)zz[k]; }, pb < 0 ? 0 : (int)coef[pb * 64], block_is_chroma(g, b), put)) {
      if (bad_block) *bad_block = b;
      return kRangeError;
    }
  }
  if (nbits) put((1u << (8 - nbits)) - 1, 8 - nbits);
  return fits ? n : kCapacityError;
}

// the whole file: header, scan, EOI
inline int64_t encode_host(const uint8_t* rgb, const Image& im, int16_t* coef_scratch, uint8_t* out, int64_t capacity, int64_t* bad_block) {
  uint8_t header[kHeaderMax];
  const int hn = compose_header(im, header);
  transform_host(rgb, im, coef_scratch);
  for (int i = 0; i < hn && i < capacity; ++i) out[i] = header[i];
  const int64_t room = capacity > hn ? capacity - hn : 0;
  const int64_t sn = entropy_host(coef_scratch, im, out + (capacity > hn ? hn : capacity), room, bad_block);
  if (sn < 0) return sn;
  if (capacity < hn || room - sn < 2) return kCapacityError;
  out[hn + sn] = 0xFF;
  out[hn + sn + 1] = 0xD9;
  return hn + sn + 2;
}

}  // namespace jpegenc

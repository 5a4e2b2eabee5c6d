// Gain maps of SDR / HDR image pairs (Ultra HDR v1, Adobe hdrgm metadata): every rule that the kernels of csrc/gainmap.hip and the
// host twins shdr_gainmap_encode_host / shdr_gainmap_apply_host share, so that the device bits are the host bits (DESIGN.md "Gain
// maps").  Plain C++, fp32 unless a line says otherwise: also compiled without HIP (tools/gainmap_sweep.cpp).  Compile every user
// with -ffp-contract=off: each product and each sum below is rounded on its own.
//
//  1 SDR  lin = kSrgbToLinear[byte]: the sRGB EOTF in float64, rounded to fp32 once; the 256 literals below are the table of both sides.
//  2 HDR  NaN and negatives -> 0, +inf -> FLT_MAX (sanitise); with reverse_channels the image's channel 2 is red.
//  3 s    fixed, or exp2((float)a) with a = mean log2(Y_sdr) - mean log2(max(Y_hdr, 2^-20)) over the pixels whose three SDR bytes are all in
//         [16, 239]; Y = 0.2126 r + 0.7152 g + 0.0722 b, left to right.  The logs are summed in float64 in a FIXED tree: the image's
//         pixels are cut into parts of stat_chunk(pixels) pixels; lane t of 256 adds pixels part * chunk + t, + 256, ... in ascending
//         order; the 256 lanes meet in a halving tree (lane t += lane t + 128, + 64, ...); the parts (at most 256) meet the same
//         way.  No pixel qualifies: s = 1.
//  4 cell per channel the sum of lin over the cell's pixels, row by row, left to right, divided by the pixel count (edge cells are
//         clipped to the image); the same for sanitise(hdr) * s; g = log2((hdr + 1/64) / (sdr + 1/64)).  Sums, products, means and
//         the quotient are float64 and the quotient is rounded to fp32 ONCE (at most FLT_MAX): with fp32 sums the 64 roundings of an
//         8 x 8 cell moved g by more than log2_poly's own error.
//  5 g is clamped to [lo, hi]; min and max over the image's cells and channels (as ordered integers: the same bits in any order);
//         max - min < 2^-10 -> max = min + 2^-10.
//  6 code = rint(255 (g - min) / (max - min)) clamped to 0 .. 255, the product first.
//  7 log2_poly / exp2_poly: exponent bits and a polynomial of plain products and sums; their measured errors are in DESIGN.md.
//  8 apply: r = code / 255 at the four map texels around u = (x + 0.5) / f - 0.5 (clamped to the map), mixed along x then y;
//         gamma != 1: r = exp2(log2(r) / gamma), 0 stays 0; L = min (1 - r) + max r; out = max((lin + offset_sdr) exp2(L w) - offset_hdr, 0).
#pragma once
#include <float.h>
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <new>

#include "shdr.h"

#ifndef SHDR_HD
#if defined(__HIPCC__)
#define SHDR_HD __host__ __device__
#else
#define SHDR_HD
#endif
#endif

namespace shdr_gainmap {

constexpr int kLanes = 256;                    // lanes of every tree below: the block size of the kernels
constexpr int kCellsPerBlock = 1024;           // shdr.h: SHDR_GAINMAP_CELLS_PER_BLOCK
constexpr int kPixelsPerBlock = 1024;          // shdr.h: SHDR_GAINMAP_PIXELS_PER_BLOCK (apply)
constexpr int kMinStatChunk = 4096;
constexpr int kMaxSide = 65535;                // what a JPEG file holds
constexpr float kOffset = 0.015625f;           // OffsetSDR = OffsetHDR = 1/64
constexpr float kMinSpan = 0.0009765625f;      // 2^-10
constexpr float kMinLuma = 9.5367431640625e-07f;   // 2^-20

constexpr float kSrgbToLinear[256] = {
    0x0p+0f, 0x1.3e4568p-12f, 0x1.3e4568p-11f, 0x1.dd681cp-11f, 0x1.3e4568p-10f, 0x1.8dd6c2p-10f, 0x1.dd681cp-10f, 0x1.167cbap-9f,
    0x1.3e4568p-9f, 0x1.660e14p-9f, 0x1.8dd6c2p-9f, 0x1.b6a31cp-9f, 0x1.e1e31ep-9f, 0x1.07c38cp-8f, 0x1.1fcc2cp-8f, 0x1.390ffap-8f,
    0x1.53936cp-8f, 0x1.6f5adep-8f, 0x1.8c6a94p-8f, 0x1.aac6cp-8f, 0x1.ca7382p-8f, 0x1.eb74e2p-8f, 0x1.06e76cp-7f, 0x1.18c2a6p-7f,
    0x1.2b4e0ap-7f, 0x1.3e8b7cp-7f, 0x1.527cd6p-7f, 0x1.6723eep-7f, 0x1.7c8292p-7f, 0x1.929a88p-7f, 0x1.a96d92p-7f, 0x1.c0fd68p-7f,
    0x1.d94bbep-7f, 0x1.f25a44p-7f, 0x1.061552p-6f, 0x1.135f3ep-6f, 0x1.210bb8p-6f, 0x1.2f1b8cp-6f, 0x1.3d8f84p-6f, 0x1.4c6866p-6f,
    0x1.5ba6fap-6f, 0x1.6b4c04p-6f, 0x1.7b5842p-6f, 0x1.8bcc74p-6f, 0x1.9ca958p-6f, 0x1.adefaap-6f, 0x1.bfa02p-6f, 0x1.d1bb74p-6f,
    0x1.e4425ap-6f, 0x1.f73586p-6f, 0x1.054ad4p-5f, 0x1.0f31bap-5f, 0x1.194fccp-5f, 0x1.23a55ep-5f, 0x1.2e32c8p-5f, 0x1.38f86p-5f,
    0x1.43f678p-5f, 0x1.4f2d64p-5f, 0x1.5a9d76p-5f, 0x1.664702p-5f, 0x1.722a56p-5f, 0x1.7e47c8p-5f, 0x1.8a9fa4p-5f, 0x1.97323ap-5f,
    0x1.a3ffd8p-5f, 0x1.b108dp-5f, 0x1.be4d6cp-5f, 0x1.cbcdfap-5f, 0x1.d98ac6p-5f, 0x1.e7841cp-5f, 0x1.f5ba48p-5f, 0x1.0216cap-4f,
    0x1.096f26p-4f, 0x1.10e65cp-4f, 0x1.187c9p-4f, 0x1.2031e8p-4f, 0x1.280688p-4f, 0x1.2ffa92p-4f, 0x1.380e2ap-4f, 0x1.404174p-4f,
    0x1.489494p-4f, 0x1.5107acp-4f, 0x1.599adep-4f, 0x1.624e4ep-4f, 0x1.6b221ep-4f, 0x1.74167p-4f, 0x1.7d2b66p-4f, 0x1.86612p-4f,
    0x1.8fb7cp-4f, 0x1.992f68p-4f, 0x1.a2c83ap-4f, 0x1.ac8256p-4f, 0x1.b65ddcp-4f, 0x1.c05aecp-4f, 0x1.ca79a8p-4f, 0x1.d4ba3p-4f,
    0x1.df1ca2p-4f, 0x1.e9a12p-4f, 0x1.f447cap-4f, 0x1.ff10bcp-4f, 0x1.04fe0cp-3f, 0x1.0a84fep-3f, 0x1.101d44p-3f, 0x1.15c6eep-3f,
    0x1.1b8208p-3f, 0x1.214ea6p-3f, 0x1.272cd4p-3f, 0x1.2d1ca2p-3f, 0x1.331e1ep-3f, 0x1.393158p-3f, 0x1.3f566p-3f, 0x1.458d42p-3f,
    0x1.4bd60ep-3f, 0x1.5230d4p-3f, 0x1.589dap-3f, 0x1.5f1c84p-3f, 0x1.65ad8ap-3f, 0x1.6c50c4p-3f, 0x1.73063ep-3f, 0x1.79ce06p-3f,
    0x1.80a82ep-3f, 0x1.8794cp-3f, 0x1.8e93ccp-3f, 0x1.95a55ep-3f, 0x1.9cc986p-3f, 0x1.a40052p-3f, 0x1.ab49cep-3f, 0x1.b2a60ap-3f,
    0x1.ba1512p-3f, 0x1.c196f4p-3f, 0x1.c92bbep-3f, 0x1.d0d37cp-3f, 0x1.d88e3ep-3f, 0x1.e05c0ep-3f, 0x1.e83cfcp-3f, 0x1.f03116p-3f,
    0x1.f83866p-3f, 0x1.00297ep-2f, 0x1.044072p-2f, 0x1.086116p-2f, 0x1.0c8b7p-2f, 0x1.10bf86p-2f, 0x1.14fd6p-2f, 0x1.194502p-2f,
    0x1.1d9676p-2f, 0x1.21f1bep-2f, 0x1.2656e4p-2f, 0x1.2ac5ecp-2f, 0x1.2f3edep-2f, 0x1.33c1cp-2f, 0x1.384e98p-2f, 0x1.3ce56cp-2f,
    0x1.418642p-2f, 0x1.46312p-2f, 0x1.4ae60ep-2f, 0x1.4fa51p-2f, 0x1.546e2cp-2f, 0x1.59416cp-2f, 0x1.5e1edp-2f, 0x1.630664p-2f,
    0x1.67f82ap-2f, 0x1.6cf428p-2f, 0x1.71fa68p-2f, 0x1.770aecp-2f, 0x1.7c25bcp-2f, 0x1.814adcp-2f, 0x1.867a54p-2f, 0x1.8bb428p-2f,
    0x1.90f86p-2f, 0x1.9647p-2f, 0x1.9ba01p-2f, 0x1.a10394p-2f, 0x1.a67192p-2f, 0x1.abea1p-2f, 0x1.b16d14p-2f, 0x1.b6faa4p-2f,
    0x1.bc92c6p-2f, 0x1.c2357ep-2f, 0x1.c7e2d2p-2f, 0x1.cd9acap-2f, 0x1.d35d6ap-2f, 0x1.d92ab6p-2f, 0x1.df02b8p-2f, 0x1.e4e57p-2f,
    0x1.ead2e8p-2f, 0x1.f0cb26p-2f, 0x1.f6ce2cp-2f, 0x1.fcdcp-2f, 0x1.017a56p-1f, 0x1.048c18p-1f, 0x1.07a34ap-1f, 0x1.0abfeep-1f,
    0x1.0de208p-1f, 0x1.11099ap-1f, 0x1.1436a8p-1f, 0x1.176932p-1f, 0x1.1aa13ep-1f, 0x1.1ddecap-1f, 0x1.2121dep-1f, 0x1.246a7ap-1f,
    0x1.27b8ap-1f, 0x1.2b0c54p-1f, 0x1.2e6598p-1f, 0x1.31c46ep-1f, 0x1.3528dcp-1f, 0x1.3892ep-1f, 0x1.3c028p-1f, 0x1.3f77bcp-1f,
    0x1.42f29ap-1f, 0x1.467318p-1f, 0x1.49f93ep-1f, 0x1.4d850ap-1f, 0x1.511682p-1f, 0x1.54ada4p-1f, 0x1.584a78p-1f, 0x1.5becfep-1f,
    0x1.5f9538p-1f, 0x1.634328p-1f, 0x1.66f6d4p-1f, 0x1.6ab03ap-1f, 0x1.6e6f6p-1f, 0x1.723448p-1f, 0x1.75fef4p-1f, 0x1.79cf64p-1f,
    0x1.7da59ep-1f, 0x1.8181a4p-1f, 0x1.856378p-1f, 0x1.894b1cp-1f, 0x1.8d3892p-1f, 0x1.912bdep-1f, 0x1.9525p-1f, 0x1.9923fep-1f,
    0x1.9d28d8p-1f, 0x1.a13392p-1f, 0x1.a5442cp-1f, 0x1.a95aacp-1f, 0x1.ad771p-1f, 0x1.b1995ep-1f, 0x1.b5c198p-1f, 0x1.b9efbep-1f,
    0x1.be23d4p-1f, 0x1.c25ddep-1f, 0x1.c69ddcp-1f, 0x1.cae3d2p-1f, 0x1.cf2fcp-1f, 0x1.d381aap-1f, 0x1.d7d994p-1f, 0x1.dc377ep-1f,
    0x1.e09b6ap-1f, 0x1.e5055cp-1f, 0x1.e97556p-1f, 0x1.edeb5cp-1f, 0x1.f2676cp-1f, 0x1.f6e98cp-1f, 0x1.fb71bcp-1f, 0x1p+0f,
};

SHDR_HD inline uint32_t float_bits(float v) {
  uint32_t u;
  memcpy(&u, &v, 4);
  return u;
}
SHDR_HD inline float bits_float(uint32_t u) {
  float v;
  memcpy(&v, &u, 4);
  return v;
}

// ---- rule 7 ------------------------------------------------------------------------------------------------------------------
// log2 of a positive normal number (+inf gives 128; the callers never pass zero, a denormal or a negative).  x = m 2^e with m in
// [sqrt(1/2), sqrt(2)); z = (m - 1) / (m + 1), |z| <= 0.1716; log2(m) = (2 / ln 2) (z + z^3 / 3 + z^5 / 5 + z^7 / 7 + z^9 / 9), the next term
// is below 2e-10.
SHDR_HD inline float log2_poly(float x) {
  const uint32_t u = float_bits(x);
  int e = (int)(u >> 23 & 255u) - 127;
  float m = bits_float((u & 0x007FFFFFu) | 0x3F800000u);
  if (m > 1.41421356f) {
    m = m * 0.5f;
    e += 1;
  }
  const float z = (m - 1.0f) / (m + 1.0f);
  const float z2 = z * z;
  float p = 0.320598997f;                      // 2 / (9 ln 2)
  p = p * z2 + 0.412198710f;                   // 2 / (7 ln 2)
  p = p * z2 + 0.577078016f;                   // 2 / (5 ln 2)
  p = p * z2 + 0.961796694f;                   // 2 / (3 ln 2)
  p = p * z2 + 2.88539008f;                    // 2 / ln 2
  return (float)e + z * p;
}

// 2^x, x clamped to [-125, 127] (no denormal results, no overflow; a NaN counts as -125).  n = x rounded to the nearest integer (halves
// away from zero), r = x - n exactly, 2^r = exp(r ln 2) by its series to the 7th power (|r ln 2| <= 0.3466: the next term is below 6e-9).
SHDR_HD inline float exp2_poly(float x) {
  x = x > -125.0f ? x : -125.0f;
  x = x < 127.0f ? x : 127.0f;
  const int n = (int)(x + (x < 0.0f ? -0.5f : 0.5f));
  const float y = (x - (float)n) * 0.693147181f;
  float p = 1.98412698e-4f;                    // 1 / 5040
  p = p * y + 1.38888889e-3f;                  // 1 / 720
  p = p * y + 8.33333333e-3f;                  // 1 / 120
  p = p * y + 4.16666667e-2f;                  // 1 / 24
  p = p * y + 0.166666667f;                    // 1 / 6
  p = p * y + 0.5f;
  p = p * y + 1.0f;
  p = p * y + 1.0f;
  return p * bits_float((uint32_t)(n + 127) << 23);
}

// ---- rules 2, 3 --------------------------------------------------------------------------------------------------------------
SHDR_HD inline float sanitise(float x) {
  x = x > 0.0f ? x : 0.0f;                     // NaN compares false
  return x > FLT_MAX ? FLT_MAX : x;
}
SHDR_HD inline float luma(float r, float g, float b) { return 0.2126f * r + 0.7152f * g + 0.0722f * b; }

// pixels per part of the statistics: a multiple of 256, at most 256 parts
SHDR_HD inline int64_t stat_chunk(int64_t pixels) {
  int64_t c = (pixels + kLanes - 1) / kLanes;
  c = (c + kLanes - 1) / kLanes * kLanes;
  return c < kMinStatChunk ? kMinStatChunk : c;
}
SHDR_HD inline int64_t stat_parts(int64_t pixels) { return (pixels + stat_chunk(pixels) - 1) / stat_chunk(pixels); }

struct Stat {
  double sdr, hdr;                             // sums of log2(Y)
  int64_t n;                                   // pixels that qualify
};
SHDR_HD inline void stat_add(Stat& a, const Stat& b) {
  a.sdr += b.sdr;
  a.hdr += b.hdr;
  a.n += b.n;
}

// one pixel's share; px: index of the pixel in both arenas
SHDR_HD inline void stat_pixel(Stat& a, const uint8_t* sdr, const float* hdr, int64_t px, int reverse, const float* tab) {
  const int r8 = sdr[3 * px], g8 = sdr[3 * px + 1], b8 = sdr[3 * px + 2];
  if (r8 < 16 || r8 > 239 || g8 < 16 || g8 > 239 || b8 < 16 || b8 > 239) return;
  const float hr = sanitise(hdr[3 * px + (reverse ? 2 : 0)]), hg = sanitise(hdr[3 * px + 1]), hb = sanitise(hdr[3 * px + (reverse ? 0 : 2)]);
  const float ys = luma(tab[r8], tab[g8], tab[b8]);
  float yh = luma(hr, hg, hb);
  yh = yh > kMinLuma ? yh : kMinLuma;
  a.sdr += (double)log2_poly(ys);
  a.hdr += (double)log2_poly(yh);
  a.n += 1;
}

// what lane t of part `part` adds up
SHDR_HD inline Stat stat_lane(const uint8_t* sdr, const float* hdr, int64_t pix_off, int64_t pixels, int64_t part, int t, int reverse,
                              const float* tab) {
  Stat a = {0.0, 0.0, 0};
  const int64_t chunk = stat_chunk(pixels), lo = part * chunk, hi = lo + chunk < pixels ? lo + chunk : pixels;
  for (int64_t e = lo + t; e < hi; e += kLanes) stat_pixel(a, sdr, hdr, pix_off + e, reverse, tab);
  return a;
}

SHDR_HD inline float scale_of(const Stat& all) {
  if (all.n == 0) return 1.0f;
  const double a = all.sdr / (double)all.n - all.hdr / (double)all.n;
  return exp2_poly((float)a);
}

// ---- rules 4 .. 6 ------------------------------------------------------------------------------------------------------------
SHDR_HD inline int map_side(int side, int f) { return (side + f - 1) / f; }

// g of the three channels of cell (cy, cx), clamped to [lo, hi]; out[0] is red
SHDR_HD inline void cell_gain(const uint8_t* sdr, const float* hdr, int64_t pix_off, int h, int w, int f, int cy, int cx, float s, float lo,
                              float hi, int reverse, const float* tab, float out[3]) {
  const int y0 = cy * f, x0 = cx * f, y1 = y0 + f < h ? y0 + f : h, x1 = x0 + f < w ? x0 + f : w;
  double as[3] = {0.0, 0.0, 0.0}, ah[3] = {0.0, 0.0, 0.0};
  for (int y = y0; y < y1; ++y) {
    for (int x = x0; x < x1; ++x) {
      const int64_t px = 3 * (pix_off + (int64_t)y * w + x);
      for (int c = 0; c < 3; ++c) {
        as[c] += (double)tab[sdr[px + c]];
        ah[c] += (double)sanitise(hdr[px + (reverse ? 2 - c : c)]) * (double)s;
      }
    }
  }
  const double count = (double)((y1 - y0) * (x1 - x0));
  for (int c = 0; c < 3; ++c) {
    const double ratio = (ah[c] / count + 0.015625) / (as[c] / count + 0.015625);
    const float g = log2_poly(ratio < (double)FLT_MAX ? (float)ratio : FLT_MAX);
    out[c] = g < lo ? lo : g > hi ? hi : g;
  }
}

// floats as integers of the same order (-0 below +0)
SHDR_HD inline uint32_t ordered_key(float v) {
  const uint32_t u = float_bits(v);
  return (u & 0x80000000u) ? ~u : u | 0x80000000u;
}
SHDR_HD inline float ordered_value(uint32_t k) { return bits_float((k & 0x80000000u) ? k & 0x7FFFFFFFu : ~k); }
constexpr uint32_t kKeyMinInit = 0xFFFFFFFFu, kKeyMaxInit = 0u;

SHDR_HD inline float widened_max(float mn, float mx) { return mx - mn < kMinSpan ? mn + kMinSpan : mx; }

SHDR_HD inline uint8_t quantise(float g, float mn, float mx) {
  const float v = rintf(255.0f * (g - mn) / (mx - mn));
  return (uint8_t)(v < 0.0f ? 0.0f : v > 255.0f ? 255.0f : v);
}

// ---- rule 8 ------------------------------------------------------------------------------------------------------------------
struct ApplyParams {                           // of one image
  int h, w, mh, mw, f, mc;                     // mc: channels of the map, 1 or 3
  float mn, mx, gamma, offset_sdr, offset_hdr, weight;
};

// the three channels of output pixel (y, x); sdr: the pixel's three bytes; map: the image's map [mh][mw][mc]
SHDR_HD inline void apply_pixel(const uint8_t* sdr, const uint8_t* map, const ApplyParams& p, int y, int x, const float* tab, float out[3]) {
  const float ff = (float)p.f;
  float u = ((float)x + 0.5f) / ff - 0.5f, v = ((float)y + 0.5f) / ff - 0.5f;
  const float umax = (float)(p.mw - 1), vmax = (float)(p.mh - 1);
  u = u > 0.0f ? u : 0.0f;
  u = u < umax ? u : umax;
  v = v > 0.0f ? v : 0.0f;
  v = v < vmax ? v : vmax;
  const int xa = (int)u, ya = (int)v, xb = xa + 1 < p.mw ? xa + 1 : xa, yb = ya + 1 < p.mh ? ya + 1 : ya;
  const float fx = u - (float)xa, fy = v - (float)ya;
  for (int c = 0; c < 3; ++c) {
    const int mc = p.mc == 3 ? c : 0;
    const float r00 = (float)map[((int64_t)ya * p.mw + xa) * p.mc + mc] / 255.0f, r01 = (float)map[((int64_t)ya * p.mw + xb) * p.mc + mc] / 255.0f;
    const float r10 = (float)map[((int64_t)yb * p.mw + xa) * p.mc + mc] / 255.0f, r11 = (float)map[((int64_t)yb * p.mw + xb) * p.mc + mc] / 255.0f;
    const float top = r00 + (r01 - r00) * fx, bottom = r10 + (r11 - r10) * fx;
    float r = top + (bottom - top) * fy;
    if (p.gamma != 1.0f) r = r > 0.0f ? exp2_poly(log2_poly(r) / p.gamma) : 0.0f;
    const float l = p.mn * (1.0f - r) + p.mx * r;
    const float o = (tab[sdr[c]] + p.offset_sdr) * exp2_poly(l * p.weight) - p.offset_hdr;
    out[c] = o > 0.0f ? o : 0.0f;
  }
}

// ---- host: the descriptors' derived fields, the checks in front of every launch, the twins ------------------------------------------
// Every check returns SHDR_OK or a negative SHDR_E_* code with its reason in `why`; nothing is written before all of them pass.
constexpr int kWhy = 256;

inline bool finite_f(float v) { return (float_bits(v) & 0x7F800000u) != 0x7F800000u; }

SHDR_HD inline int64_t cells_of(const shdr_gainmap_image& im) { return (int64_t)map_side(im.height, im.factor) * map_side(im.width, im.factor); }

struct EncodeTotals {
  int64_t cells, stat_blocks, cell_blocks;
};

// the shape of image i alone
inline int check_encode_shape(const shdr_gainmap_image* images, int i, char* why) {
  const shdr_gainmap_image& im = images[i];
  if (im.height < 1 || im.width < 1 || im.height > kMaxSide || im.width > kMaxSide) {
    snprintf(why, kWhy, "image %d is %d x %d: H and W must be 1 .. %d", i, im.height, im.width, kMaxSide);
    return SHDR_E_SHAPE;
  }
  if (im.factor != 1 && im.factor != 2 && im.factor != 4 && im.factor != 8) {
    snprintf(why, kWhy, "image %d has factor %d (1, 2, 4 or 8)", i, im.factor);
    return SHDR_E_SHAPE;
  }
  return SHDR_OK;
}

// what the derived fields of image i must hold, given the totals of the images before it; adds the image to the totals
inline shdr_gainmap_image derived_of(const shdr_gainmap_image& im, EncodeTotals& t) {
  shdr_gainmap_image d = im;
  d.cell_off = t.cells;
  d.stat_block0 = (int32_t)t.stat_blocks;
  d.cell_block0 = (int32_t)t.cell_blocks;
  d.reserved = 0;
  const int64_t cells = cells_of(im);
  t.cells += cells;
  t.stat_blocks += stat_parts((int64_t)im.height * im.width);
  t.cell_blocks += (cells + kCellsPerBlock - 1) / kCellsPerBlock;
  return d;
}

inline int fill_encode(shdr_gainmap_image* images, int n, EncodeTotals* tot, char* why) {
  if (!images) return snprintf(why, kWhy, "null images"), SHDR_E_NULL;
  if (n < 1) return snprintf(why, kWhy, "the number of images must be positive, got %d", n), SHDR_E_SHAPE;
  EncodeTotals t = {0, 0, 0};
  for (int i = 0; i < n; ++i) {
    if (int rc = check_encode_shape(images, i, why)) return rc;
    images[i] = derived_of(images[i], t);
    if (t.stat_blocks >= ((int64_t)1 << 31) || t.cell_blocks >= ((int64_t)1 << 31))
      return snprintf(why, kWhy, "%d images are more than one launch takes", i + 1), SHDR_E_SHAPE;
  }
  *tot = t;
  return SHDR_OK;
}

inline int check_encode(const shdr_gainmap_image* images, int n, int64_t arena_pixels, const float* scales, float lo, float hi,
                        EncodeTotals* tot, char* why) {
  if (!images) return snprintf(why, kWhy, "null images"), SHDR_E_NULL;
  if (n < 1) return snprintf(why, kWhy, "the number of images must be positive, got %d", n), SHDR_E_SHAPE;
  if (!(finite_f(lo) && finite_f(hi) && lo < hi)) return snprintf(why, kWhy, "the range [%g, %g] must be finite and not empty", lo, hi), SHDR_E_SHAPE;
  EncodeTotals t = {0, 0, 0};
  for (int i = 0; i < n; ++i) {
    if (int rc = check_encode_shape(images, i, why)) return rc;
    const shdr_gainmap_image& im = images[i];
    const int64_t pixels = (int64_t)im.height * im.width;
    if (im.pix_off < 0 || im.pix_off > arena_pixels || pixels > arena_pixels - im.pix_off)
      return snprintf(why, kWhy, "image %d (%d x %d at pixel %lld) leaves the arenas of %lld pixels", i, im.height, im.width, (long long)im.pix_off,
                      (long long)arena_pixels), SHDR_E_SHAPE;
    const shdr_gainmap_image d = derived_of(im, t);
    if (t.stat_blocks >= ((int64_t)1 << 31) || t.cell_blocks >= ((int64_t)1 << 31))
      return snprintf(why, kWhy, "%d images are more than one launch takes", i + 1), SHDR_E_SHAPE;
    if (d.cell_off != im.cell_off || d.stat_block0 != im.stat_block0 || d.cell_block0 != im.cell_block0)
      return snprintf(why, kWhy, "image %d: the derived fields are not those of shdr_gainmap_encode_sizes", i), SHDR_E_SHAPE;
    if (scales && !(finite_f(scales[i]) && scales[i] > 0.0f))
      return snprintf(why, kWhy, "image %d: the scale must be finite and positive, got %g", i, scales[i]), SHDR_E_SHAPE;
  }
  *tot = t;
  return SHDR_OK;
}

template <class T>
inline void tree256(T* lanes, void (*add)(T&, const T&)) {
  for (int s = kLanes / 2; s > 0; s >>= 1)
    for (int t = 0; t < s; ++t) add(lanes[t], lanes[t + s]);
}

// rule 3 of one image, as the statistics launch and the first lines of the cell launch compute it
inline Stat image_stat_host(const uint8_t* sdr, const float* hdr, const shdr_gainmap_image& im, int reverse) {
  const int64_t pixels = (int64_t)im.height * im.width, parts = stat_parts(pixels);
  Stat part[kLanes], lanes[kLanes];
  for (int p = 0; p < kLanes; ++p) {
    if (p < parts) {
      for (int t = 0; t < kLanes; ++t) lanes[t] = stat_lane(sdr, hdr, im.pix_off, pixels, p, t, reverse, kSrgbToLinear);
      tree256(lanes, stat_add);
      part[p] = lanes[0];
    } else {
      part[p] = Stat{0.0, 0.0, 0};
    }
  }
  tree256(part, stat_add);
  return part[0];
}

inline int encode_host(const uint8_t* sdr, const float* hdr, int64_t arena_pixels, const shdr_gainmap_image* images, int n, const float* scales,
                       float lo, float hi, int reverse, uint8_t* maps, int64_t map_capacity, shdr_gainmap_meta* meta, int64_t meta_capacity,
                       char* why) {
  if (!sdr || !hdr || !maps || !meta) return snprintf(why, kWhy, "null pointer"), SHDR_E_NULL;
  EncodeTotals tot;
  if (int rc = check_encode(images, n, arena_pixels, scales, lo, hi, &tot, why)) return rc;
  if (map_capacity < 3 * tot.cells)
    return snprintf(why, kWhy, "the maps need %lld bytes, the destination has %lld", (long long)(3 * tot.cells), (long long)map_capacity), SHDR_E_SHAPE;
  if (meta_capacity < n) return snprintf(why, kWhy, "%d meta records are needed, the destination has %lld", n, (long long)meta_capacity), SHDR_E_SHAPE;
  int64_t most = 0;
  for (int i = 0; i < n; ++i) most = cells_of(images[i]) > most ? cells_of(images[i]) : most;
  float* g = new (std::nothrow) float[3 * most];
  if (!g) return snprintf(why, kWhy, "no memory for %lld cells", (long long)most), SHDR_E_SHAPE;
  for (int i = 0; i < n; ++i) {
    const shdr_gainmap_image& im = images[i];
    Stat all = {0.0, 0.0, 0};
    float s;
    if (scales) {
      s = scales[i];
    } else {
      all = image_stat_host(sdr, hdr, im, reverse);
      s = scale_of(all);
    }
    const int mh = map_side(im.height, im.factor), mw = map_side(im.width, im.factor);
    uint32_t kmin = kKeyMinInit, kmax = kKeyMaxInit;
    for (int cy = 0; cy < mh; ++cy) {
      for (int cx = 0; cx < mw; ++cx) {
        float* o = g + 3 * ((int64_t)cy * mw + cx);
        cell_gain(sdr, hdr, im.pix_off, im.height, im.width, im.factor, cy, cx, s, lo, hi, reverse, kSrgbToLinear, o);
        for (int c = 0; c < 3; ++c) {
          const uint32_t k = ordered_key(o[c]);
          kmin = k < kmin ? k : kmin;
          kmax = k > kmax ? k : kmax;
        }
      }
    }
    const float mn = ordered_value(kmin), mx = widened_max(mn, ordered_value(kmax));
    uint8_t* map = maps + 3 * im.cell_off;
    for (int64_t e = 0; e < 3 * (int64_t)mh * mw; ++e) map[e] = quantise(g[e], mn, mx);
    meta[i].gain_min = mn;
    meta[i].gain_max = mx;
    meta[i].scale = s;
    meta[i].reserved = 0;
    meta[i].count = all.n;
  }
  delete[] g;
  return SHDR_OK;
}

SHDR_HD inline ApplyParams params_of(const shdr_gainmap_apply_image& im) {
  return ApplyParams{im.height, im.width, im.map_height, im.map_width, im.factor, im.map_channels,
                     im.gain_min, im.gain_max, im.gamma, im.offset_sdr, im.offset_hdr, im.weight};
}

// fill: write block0 instead of comparing it
inline int check_apply(shdr_gainmap_apply_image* images, int n, bool fill, int64_t arena_pixels, int64_t map_bytes, int64_t out_capacity,
                       int64_t* n_blocks, char* why) {
  if (!images) return snprintf(why, kWhy, "null images"), SHDR_E_NULL;
  if (n < 1) return snprintf(why, kWhy, "the number of images must be positive, got %d", n), SHDR_E_SHAPE;
  int64_t blocks = 0, next_pixel = 0;
  for (int i = 0; i < n; ++i) {
    shdr_gainmap_apply_image& im = images[i];
    if (im.height < 1 || im.width < 1 || im.height > kMaxSide || im.width > kMaxSide)
      return snprintf(why, kWhy, "image %d is %d x %d: H and W must be 1 .. %d", i, im.height, im.width, kMaxSide), SHDR_E_SHAPE;
    if (im.factor < 1 || im.factor > 64) return snprintf(why, kWhy, "image %d has factor %d (1 .. 64)", i, im.factor), SHDR_E_SHAPE;
    if (im.map_height != map_side(im.height, im.factor) || im.map_width != map_side(im.width, im.factor))
      return snprintf(why, kWhy, "image %d: a %d x %d map is not that of a %d x %d image at factor %d", i, im.map_height, im.map_width, im.height,
                      im.width, im.factor), SHDR_E_SHAPE;
    if (im.map_channels != 1 && im.map_channels != 3) return snprintf(why, kWhy, "image %d: a map has 1 or 3 channels, got %d", i, im.map_channels), SHDR_E_SHAPE;
    if (!(finite_f(im.gain_min) && finite_f(im.gain_max) && finite_f(im.gamma) && im.gamma > 0.0f && finite_f(im.offset_sdr) &&
          finite_f(im.offset_hdr) && im.weight >= 0.0f && im.weight <= 1.0f))
      return snprintf(why, kWhy, "image %d: the metadata must be finite, gamma positive and the weight in [0, 1]", i), SHDR_E_SHAPE;
    if (fill) {
      im.block0 = (int32_t)blocks;
      im.reserved = 0;
    } else {
      const int64_t pixels = (int64_t)im.height * im.width, room = arena_pixels < out_capacity ? arena_pixels : out_capacity;
      const int64_t cells = (int64_t)im.map_height * im.map_width * im.map_channels;
      if (im.pix_off < next_pixel || im.pix_off > room || pixels > room - im.pix_off)
        return snprintf(why, kWhy, "image %d (%d x %d at pixel %lld) overlaps the image before it or leaves the arena of %lld or the destination of %lld pixels",
                        i, im.height, im.width, (long long)im.pix_off, (long long)arena_pixels, (long long)out_capacity), SHDR_E_SHAPE;
      if (im.map_off < 0 || im.map_off > map_bytes || cells > map_bytes - im.map_off)
        return snprintf(why, kWhy, "image %d: a map of %lld bytes at byte %lld leaves the %lld map bytes", i, (long long)cells, (long long)im.map_off,
                        (long long)map_bytes), SHDR_E_SHAPE;
      if (im.block0 != blocks) return snprintf(why, kWhy, "image %d: block0 is not that of shdr_gainmap_apply_sizes", i), SHDR_E_SHAPE;
      next_pixel = im.pix_off + pixels;
    }
    blocks += ((int64_t)im.height * im.width + kPixelsPerBlock - 1) / kPixelsPerBlock;
    if (blocks >= ((int64_t)1 << 31)) return snprintf(why, kWhy, "%d images are more than one launch takes", i + 1), SHDR_E_SHAPE;
  }
  if (n_blocks) *n_blocks = blocks;
  return SHDR_OK;
}

inline int apply_host(const uint8_t* sdr, int64_t arena_pixels, const uint8_t* maps, int64_t map_bytes, const shdr_gainmap_apply_image* images,
                      int n, float* out, int64_t out_capacity, char* why) {
  if (!sdr || !maps || !out) return snprintf(why, kWhy, "null pointer"), SHDR_E_NULL;
  if (int rc = check_apply(const_cast<shdr_gainmap_apply_image*>(images), n, false, arena_pixels, map_bytes, out_capacity, nullptr, why)) return rc;
  for (int i = 0; i < n; ++i) {
    const shdr_gainmap_apply_image& im = images[i];
    const ApplyParams p = params_of(im);
    for (int y = 0; y < im.height; ++y)
      for (int x = 0; x < im.width; ++x) {
        const int64_t px = im.pix_off + (int64_t)y * im.width + x;
        apply_pixel(sdr + 3 * px, maps + im.map_off, p, y, x, kSrgbToLinear, out + 3 * px);
      }
  }
  return SHDR_OK;
}

}  // namespace shdr_gainmap

// Sanitizer sweep of the gain-map host twins (csrc/gainmap.h) and the measurement of the header's two polynomials.  The kernels of
// csrc/gainmap.hip compute every pixel, cell and map byte with the functions of this header, so what holds here is what stands behind
// the device's reads of an image.  Stand-alone, no HIP, not part of the library or of the test suite:
//
//     c++ -std=c++17 -O1 -g -ffp-contract=off -fsanitize=address,undefined -fno-sanitize-recover=all -I include -I singlehdr-tf2_amd/csrc \
//         tools/gainmap_sweep.cpp -o /tmp/gainmap_sweep
//     /tmp/gainmap_sweep
//
// 1. log2_poly against float64 over EVERY fp32 mantissa, at exponent 0 and at the exponents -8 .. 8 that the clamped range of a gain
//    can reach; exp2_poly against float64 on the grid k 2^-16 of [-16, 16].  The largest errors are printed: DESIGN.md quotes them and
//    tests/test_gainmap_host.py derives its tolerance from them.
// 2. 4000 random batches of 1 .. 3 images -- widths and heights 1 .. 70, all four factors, five kinds of content with NaN, infinities,
//    negatives and 1e30 among the HDR values, both channel orders, fixed and automatic scale -- are encoded from heap blocks of exactly
//    the arenas' sizes into heap blocks of exactly the maps' and records' sizes, then into blocks of one byte and of one record less,
//    which must be refused with nothing written.  Every map is applied again (one- and three-channel maps, gamma 1 and 2.2) into a
//    block of exactly the pixels, and into one of a pixel less and from a map of a byte less, which must be refused.  A read or a write
//    one byte outside any block is an AddressSanitizer report.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "gainmap.h"

namespace {

using namespace shdr_gainmap;

long long g_runs = 0, g_pixels = 0, g_refused = 0;
uint32_t g_state = 2025;
uint32_t rnd() { return g_state = g_state * 1664525u + 1013904223u, g_state >> 8; }
float unit() { return (float)(rnd() & 0xFFFF) / 65536.0f; }

#define CHECK(cond)                                                        \
  do {                                                                     \
    if (!(cond)) {                                                         \
      fprintf(stderr, "line %d: %s fails (run %lld)\n", __LINE__, #cond, g_runs); \
      abort();                                                             \
    }                                                                      \
  } while (0)

void measure() {
  double worst0 = 0.0, worst = 0.0;
  for (int e = -8; e <= 8; ++e) {
    for (uint32_t m = 0; m < (1u << 23); ++m) {
      const float x = bits_float((uint32_t)(e + 127) << 23 | m);
      const double err = fabs((double)log2_poly(x) - log2((double)x));
      if (e == 0 && err > worst0) worst0 = err;
      if (err > worst) worst = err;
    }
  }
  printf("log2_poly: largest |error| over every mantissa at exponent 0: %.4g; at exponents -8 .. 8: %.4g\n", worst0, worst);
  double rel = 0.0;
  for (int k = -(16 << 16); k <= (16 << 16); ++k) {
    const float x = (float)k / 65536.0f;
    const double err = fabs((double)exp2_poly(x) / exp2((double)x) - 1.0);
    if (err > rel) rel = err;
  }
  printf("exp2_poly: largest relative error on k 2^-16 in [-16, 16]: %.4g\n", rel);
}

float hdr_value(int kind) {
  switch (kind) {
    case 0: return unit() * 8.0f;
    case 1: return 0.25f;
    case 2: return expf((unit() - 0.5f) * 30.0f);
    case 3: {
      const uint32_t r = rnd() % 8;
      return r == 0 ? NAN : r == 1 ? INFINITY : r == 2 ? -INFINITY : r == 3 ? -1.5f : r == 4 ? 1e30f : r == 5 ? 0.0f : unit();
    }
    default: return unit() < 0.5f ? 0.0f : 1e-30f;
  }
}

void one_batch() {
  const int n = 1 + (int)(rnd() % 3), kind = (int)(rnd() % 5), reverse = (int)(rnd() & 1);
  const bool fixed = (rnd() & 3) == 0;
  std::vector<shdr_gainmap_image> images(n);
  int64_t pixels = 0;
  for (int i = 0; i < n; ++i) {
    memset(&images[i], 0, sizeof(images[i]));
    images[i].pix_off = pixels;
    images[i].height = 1 + (int)(rnd() % 70);
    images[i].width = 1 + (int)(rnd() % 70);
    images[i].factor = 1 << (rnd() % 4);
    pixels += (int64_t)images[i].height * images[i].width;
  }
  char why[kWhy];
  EncodeTotals tot;
  CHECK(fill_encode(images.data(), n, &tot, why) == SHDR_OK);
  uint8_t* sdr = new uint8_t[3 * pixels];
  float* hdr = new float[3 * pixels];
  for (int64_t e = 0; e < 3 * pixels; ++e) {
    sdr[e] = kind == 4 ? (rnd() & 1 ? 255 : 0) : (uint8_t)(rnd() & 255);
    hdr[e] = hdr_value(kind);
  }
  std::vector<float> scales(n);
  for (int i = 0; i < n; ++i) scales[i] = 0.125f + unit() * 4.0f;
  const float* sc = fixed ? scales.data() : nullptr;
  const float lo = -4.0f, hi = 8.0f;
  const int64_t map_bytes = 3 * tot.cells;
  uint8_t* maps = new uint8_t[map_bytes];
  shdr_gainmap_meta* meta = new shdr_gainmap_meta[n];
  CHECK(encode_host(sdr, hdr, pixels, images.data(), n, sc, lo, hi, reverse, maps, map_bytes, meta, n, why) == SHDR_OK);
  for (int i = 0; i < n; ++i) {
    CHECK(meta[i].gain_min >= lo && meta[i].gain_max <= hi + kMinSpan && meta[i].gain_max - meta[i].gain_min >= kMinSpan * 0.99f);
    CHECK(meta[i].scale > 0.0f && finite_f(meta[i].scale) && meta[i].count >= 0 && meta[i].count <= (int64_t)images[i].height * images[i].width);
    if (fixed) CHECK(meta[i].scale == scales[i] && meta[i].count == 0);
  }
  {                                            // one byte, one record less: refused, and the smaller blocks are not touched
    uint8_t* small = new uint8_t[map_bytes - 1 > 0 ? map_bytes - 1 : 1];
    memset(small, 0x5A, map_bytes - 1 > 0 ? map_bytes - 1 : 1);
    CHECK(encode_host(sdr, hdr, pixels, images.data(), n, sc, lo, hi, reverse, small, map_bytes - 1, meta, n, why) == SHDR_E_SHAPE);
    for (int64_t e = 0; e < map_bytes - 1; ++e) CHECK(small[e] == 0x5A);
    delete[] small;
    shdr_gainmap_meta* fewer = new shdr_gainmap_meta[n > 1 ? n - 1 : 1];
    memset(fewer, 0x5A, sizeof(shdr_gainmap_meta) * (n > 1 ? n - 1 : 1));
    CHECK(encode_host(sdr, hdr, pixels, images.data(), n, sc, lo, hi, reverse, maps, map_bytes, fewer, n - 1, why) == SHDR_E_SHAPE);
    for (size_t e = 0; e < sizeof(shdr_gainmap_meta) * (n > 1 ? n - 1 : 0); ++e) CHECK(reinterpret_cast<uint8_t*>(fewer)[e] == 0x5A);
    delete[] fewer;
    CHECK(encode_host(sdr, hdr, pixels - 1, images.data(), n, sc, lo, hi, reverse, maps, map_bytes, meta, n, why) == SHDR_E_SHAPE);   // an arena a pixel short
    g_refused += 3;
  }
  // apply: the three-channel maps as written, then one-channel maps cut from them, gamma 1 and 2.2
  for (int pass = 0; pass < 2; ++pass) {
    const int mc = pass == 0 ? 3 : 1;
    std::vector<shdr_gainmap_apply_image> ap(n);
    int64_t off = 0;
    for (int i = 0; i < n; ++i) {
      memset(&ap[i], 0, sizeof(ap[i]));
      ap[i].pix_off = images[i].pix_off;
      ap[i].map_off = off;
      ap[i].height = images[i].height;
      ap[i].width = images[i].width;
      ap[i].factor = images[i].factor;
      ap[i].map_height = map_side(images[i].height, images[i].factor);
      ap[i].map_width = map_side(images[i].width, images[i].factor);
      ap[i].map_channels = mc;
      ap[i].gain_min = meta[i].gain_min;
      ap[i].gain_max = meta[i].gain_max;
      ap[i].gamma = pass == 0 ? 1.0f : 2.2f;
      ap[i].offset_sdr = ap[i].offset_hdr = kOffset;
      ap[i].weight = pass == 0 ? 1.0f : unit();
      off += (int64_t)ap[i].map_height * ap[i].map_width * mc;
    }
    uint8_t* m = new uint8_t[off];
    if (mc == 3) memcpy(m, maps, off); else for (int64_t e = 0; e < off; ++e) m[e] = maps[3 * e + 1];
    int64_t blocks = 0;
    CHECK(check_apply(ap.data(), n, true, 0, 0, 0, &blocks, why) == SHDR_OK && blocks >= n);
    float* out = new float[3 * pixels];
    CHECK(apply_host(sdr, pixels, m, off, ap.data(), n, out, pixels, why) == SHDR_OK);
    for (int64_t e = 0; e < 3 * pixels; ++e) CHECK(out[e] >= 0.0f && finite_f(out[e]));
    delete[] out;
    float* small = new float[3 * (pixels - 1) > 0 ? 3 * (pixels - 1) : 1];
    CHECK(apply_host(sdr, pixels, m, off, ap.data(), n, small, pixels - 1, why) == SHDR_E_SHAPE);
    delete[] small;
    uint8_t* short_map = new uint8_t[off - 1 > 0 ? off - 1 : 1];
    memcpy(short_map, m, off - 1);
    out = new float[3 * pixels];
    CHECK(apply_host(sdr, pixels, short_map, off - 1, ap.data(), n, out, pixels, why) == SHDR_E_SHAPE);
    delete[] out;
    delete[] short_map;
    delete[] m;
    g_refused += 2;
  }
  delete[] meta;
  delete[] maps;
  delete[] hdr;
  delete[] sdr;
  g_pixels += pixels;
  ++g_runs;
}

void bad_descriptors() {
  char why[kWhy];
  EncodeTotals tot;
  shdr_gainmap_image im;
  memset(&im, 0, sizeof(im));
  im.height = im.width = 8;
  im.factor = 3;
  CHECK(fill_encode(&im, 1, &tot, why) == SHDR_E_SHAPE);
  im.factor = 4;
  im.height = 0;
  CHECK(fill_encode(&im, 1, &tot, why) == SHDR_E_SHAPE);
  im.height = 8;
  CHECK(fill_encode(&im, 1, &tot, why) == SHDR_OK);
  im.pix_off = 1;                              // 64 pixels at pixel 1 of an arena of 64
  CHECK(check_encode(&im, 1, 64, nullptr, -4.0f, 8.0f, &tot, why) == SHDR_E_SHAPE);
  im.pix_off = 0;
  im.cell_block0 = 1;
  CHECK(check_encode(&im, 1, 64, nullptr, -4.0f, 8.0f, &tot, why) == SHDR_E_SHAPE);
  im.cell_block0 = 0;
  CHECK(check_encode(&im, 1, 64, nullptr, 8.0f, -4.0f, &tot, why) == SHDR_E_SHAPE);
  const float zero = 0.0f;
  CHECK(check_encode(&im, 1, 64, &zero, -4.0f, 8.0f, &tot, why) == SHDR_E_SHAPE);
  CHECK(check_encode(&im, 1, 64, nullptr, -4.0f, 8.0f, &tot, why) == SHDR_OK);
}

}  // namespace

int main(int argc, char** argv) {
  if (argc < 2 || strcmp(argv[1], "--no-measure") != 0) measure();
  bad_descriptors();
  for (int i = 0; i < 4000; ++i) one_batch();
  printf("gainmap_sweep: %lld batches, %lld pixels encoded and applied twice, %lld short destinations refused: clean\n", g_runs, g_pixels, g_refused);
  return 0;
}

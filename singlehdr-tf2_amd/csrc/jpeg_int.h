// libjpeg's integer arithmetic, restated bit for bit: the "islow" Loeffler-Ligtenberg-Moschytz DCT pair (jfdctint.c,
// jidctint.c), the fancy (triangle) chroma upsamplers (jdsample.c), YCbCr -> RGB (jdcolor.c), and the forward side: RGB -> YCbCr
// (jccolor.c) and the chroma box filters (jcsample.c).  Shared by the training simulator's JPEG round trip (camera.hip), the file
// decoder (jpeg.hip) and the file encoder (jpeg_enc.h: jpeg_enc.hip and its host twin); the kernels are compiled with
// -ffp-contract=off, and nothing in here is floating point.  Plain C++: also compiled without HIP (tools/jpeg_enc_sweep.cpp).
#pragma once
#include <stdint.h>
#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define SHDR_JPEGINT_FN __host__ __device__ __forceinline__
#else
#define SHDR_JPEGINT_FN inline
#endif

namespace shdr {
namespace jpegint {

constexpr int CONST_BITS = 13, PASS1_BITS = 2;
constexpr int F_0_298631336 = 2446, F_0_390180644 = 3196, F_0_541196100 = 4433, F_0_765366865 = 6270;
constexpr int F_0_899976223 = 7373, F_1_175875602 = 9633, F_1_501321110 = 12299, F_1_847759065 = 15137;
constexpr int F_1_961570560 = 16069, F_2_053119869 = 16819, F_2_562915447 = 20995, F_3_072711026 = 25172;

SHDR_JPEGINT_FN int descale(int x, int n) { return (x + (1 << (n - 1))) >> n; }

// 1-D forward pass over d[0..7*stride]
SHDR_JPEGINT_FN void fdct_1d(int* d, int stride, bool first) {
  const int a0 = d[0], a1 = d[stride], a2 = d[2 * stride], a3 = d[3 * stride], a4 = d[4 * stride], a5 = d[5 * stride],
            a6 = d[6 * stride], a7 = d[7 * stride];
  int t0 = a0 + a7, t7 = a0 - a7, t1 = a1 + a6, t6 = a1 - a6, t2 = a2 + a5, t5 = a2 - a5, t3 = a3 + a4, t4 = a3 - a4;
  const int t10 = t0 + t3, t13 = t0 - t3, t11 = t1 + t2, t12 = t1 - t2;
  const int sh = first ? CONST_BITS - PASS1_BITS : CONST_BITS + PASS1_BITS;
  d[0] = first ? (t10 + t11) * (1 << PASS1_BITS) : descale(t10 + t11, PASS1_BITS);            // (a product: the sums may be negative)
  d[4 * stride] = first ? (t10 - t11) * (1 << PASS1_BITS) : descale(t10 - t11, PASS1_BITS);
  int z1 = (t12 + t13) * F_0_541196100;
  d[2 * stride] = descale(z1 + t13 * F_0_765366865, sh);
  d[6 * stride] = descale(z1 - t12 * F_1_847759065, sh);
  z1 = t4 + t7;
  int z2 = t5 + t6, z3 = t4 + t6, z4 = t5 + t7;
  const int z5 = (z3 + z4) * F_1_175875602;
  t4 *= F_0_298631336; t5 *= F_2_053119869; t6 *= F_3_072711026; t7 *= F_1_501321110;
  z1 *= -F_0_899976223; z2 *= -F_2_562915447;
  z3 = z3 * -F_1_961570560 + z5;
  z4 = z4 * -F_0_390180644 + z5;
  d[7 * stride] = descale(t4 + z1 + z3, sh);
  d[5 * stride] = descale(t5 + z2 + z4, sh);
  d[3 * stride] = descale(t6 + z2 + z3, sh);
  d[stride] = descale(t7 + z1 + z4, sh);
}

// 1-D inverse pass: columns first (jidctint.c pass 1), then rows
SHDR_JPEGINT_FN void idct_1d(int* d, int stride, bool first) {
  int z2 = d[2 * stride], z3 = d[6 * stride];
  int z1 = (z2 + z3) * F_0_541196100;
  int t2 = z1 - z3 * F_1_847759065, t3 = z1 + z2 * F_0_765366865;
  int t0 = (d[0] + d[4 * stride]) << CONST_BITS, t1 = (d[0] - d[4 * stride]) << CONST_BITS;
  const int t10 = t0 + t3, t13 = t0 - t3, t11 = t1 + t2, t12 = t1 - t2;
  t0 = d[7 * stride]; t1 = d[5 * stride]; t2 = d[3 * stride]; t3 = d[stride];
  z1 = t0 + t3; z2 = t1 + t2; z3 = t0 + t2;
  int z4 = t1 + t3;
  const int z5 = (z3 + z4) * F_1_175875602;
  t0 *= F_0_298631336; t1 *= F_2_053119869; t2 *= F_3_072711026; t3 *= F_1_501321110;
  z1 *= -F_0_899976223; z2 *= -F_2_562915447;
  z3 = z3 * -F_1_961570560 + z5;
  z4 = z4 * -F_0_390180644 + z5;
  t0 += z1 + z3; t1 += z2 + z4; t2 += z2 + z3; t3 += z1 + z4;
  const int sh = first ? CONST_BITS - PASS1_BITS : CONST_BITS + PASS1_BITS + 3;
  d[0] = descale(t10 + t3, sh); d[7 * stride] = descale(t10 - t3, sh);
  d[stride] = descale(t11 + t2, sh); d[6 * stride] = descale(t11 - t2, sh);
  d[2 * stride] = descale(t12 + t1, sh); d[5 * stride] = descale(t12 - t1, sh);
  d[3 * stride] = descale(t13 + t0, sh); d[4 * stride] = descale(t13 - t0, sh);
}

SHDR_JPEGINT_FN uint8_t clamp_u8(int v) { return (uint8_t)(v < 0 ? 0 : (v > 255 ? 255 : v)); }
SHDR_JPEGINT_FN int clamp_to(int v, int hi) { return v < 0 ? 0 : (v > hi ? hi : v); }               // into [0, hi]

// h2v2_fancy_upsample: output sample (y, x) of the 2x upsampled plane from a ch x cw plane with row pitch `stride`: near row /
// far row, near column / far column, weights 9:3:3:1.  The first / last row and column have no far neighbour: libjpeg
// replicates the near one, which the clamps restate.
SHDR_JPEGINT_FN int fancy_up_h2v2(const uint8_t* __restrict__ p, int stride, int ch, int cw, int y, int x) {
  const int cy = y >> 1, cx = x >> 1;
  const int fy = clamp_to(cy + ((y & 1) ? 1 : -1), ch - 1);
  const int fx = clamp_to(cx + ((x & 1) ? 1 : -1), cw - 1);
  const int this_col = 3 * p[cy * stride + cx] + p[fy * stride + cx];
  const int far_col = 3 * p[cy * stride + fx] + p[fy * stride + fx];
  return (3 * this_col + far_col + ((x & 1) ? 7 : 8)) >> 4;
}

// h2v1_fancy_upsample: output sample x of a row of cw samples, weights 3:1, bias 1 (even x) / 2 (odd x); the clamped far
// sample gives the first and last output their unfiltered value, as libjpeg's special cases do
SHDR_JPEGINT_FN int fancy_up_h2v1(const uint8_t* __restrict__ row, int cw, int x) {
  const int cx = x >> 1;
  const int fx = clamp_to(cx + ((x & 1) ? 1 : -1), cw - 1);
  return (3 * row[cx] + row[fx] + ((x & 1) ? 2 : 1)) >> 2;
}

// jdcolor.c: u = Cb - 128, v = Cr - 128; 16-bit fixed point, the green term shares one rounding
SHDR_JPEGINT_FN void ycc_to_rgb(int yy, int u, int v, int& r, int& g, int& b) {
  const int half = 1 << 15;
  r = yy + ((91881 * v + half) >> 16);                       // FIX(1.40200)
  g = yy + ((-22554 * u + half - 46802 * v) >> 16);          // FIX(0.34414), FIX(0.71414)
  b = yy + ((116130 * u + half) >> 16);                      // FIX(1.77200)
  r = r < 0 ? 0 : (r > 255 ? 255 : r);
  g = g < 0 ? 0 : (g > 255 ? 255 : g);
  b = b < 0 ? 0 : (b > 255 ? 255 : b);
}

// jccolor.c rgb_ycc_convert: 16-bit fixed point, FIX(x) = (int)(x * 65536 + 0.5); Cb and Cr carry the 128 offset and round with
// ONE_HALF - 1
constexpr int FIX_0_29900 = 19595, FIX_0_58700 = 38470, FIX_0_11400 = 7471, FIX_0_16874 = 11059, FIX_0_33126 = 21709,
              FIX_0_50000 = 32768, FIX_0_41869 = 27439, FIX_0_08131 = 5329;
SHDR_JPEGINT_FN void rgb_to_ycc(int r, int g, int b, int& y, int& cb, int& cr) {
  const int half = 1 << 15, off = 128 << 16;
  y = (FIX_0_29900 * r + FIX_0_58700 * g + FIX_0_11400 * b + half) >> 16;
  cb = (-FIX_0_16874 * r - FIX_0_33126 * g + FIX_0_50000 * b + off + half - 1) >> 16;
  cr = (FIX_0_50000 * r - FIX_0_41869 * g - FIX_0_08131 * b + off + half - 1) >> 16;
}

// jcsample.c: output sample number `col` of a row of the WHOLE plane; the bias alternates along it, 1, 2, 1, 2 ... for h2v2
// (a, b: the upper pair, c, d: the lower) and 0, 1, 0, 1 ... for h2v1
SHDR_JPEGINT_FN int box_h2v2(int a, int b, int c, int d, int col) { return (a + b + c + d + 1 + (col & 1)) >> 2; }
SHDR_JPEGINT_FN int box_h2v1(int a, int b, int col) { return (a + b + (col & 1)) >> 1; }

}  // namespace jpegint
}  // namespace shdr

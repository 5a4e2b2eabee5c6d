// cv2's INTER_LINEAR map for float32 (restated from OpenCV's resize.cpp, see the top of dataset.hip), shared by the Radiance
// (dataset.hip) and OpenEXR (exr.hip) loaders so that both resize with the same arithmetic in the same order.  Include it only
// from translation units compiled with -ffp-contract=off.
#pragma once
#include <hip/hip_runtime.h>

namespace shdr {
namespace linear {

// one axis of cv2's bilinear map: taps s0, s1 (inside [0, n)) and the weight of s1
struct Taps {
  int s0, s1;
  float f;
};

__device__ __forceinline__ Taps linear_taps(int d, double scale, int n, bool clamp_weight) {
  float f = (float)(((double)d + 0.5) * scale - 0.5);
  int s = (int)floorf(f);
  f -= (float)s;
  if (clamp_weight) {                              // horizontal rule: the edge tap takes the whole weight
    if (s < 0) { s = 0; f = 0.0f; }
    if (s >= n - 1) { s = n - 1; f = 0.0f; }
  }
  Taps t;
  t.s0 = min(max(s, 0), n - 1);                    // vertical rule: clamp the rows, keep the weights
  t.s1 = min(max(s + 1, 0), n - 1);
  t.f = f;
  return t;
}

__device__ __forceinline__ float3 lerp3(float3 a, float3 b, float f) {
  const float g = 1.0f - f;
  return make_float3(a.x * g + b.x * f, a.y * g + b.y * f, a.z * g + b.z * f);
}

// output pixel (oy, ox) of an (H0, W0) -> (H, W) resize; fetch(row, col) returns one source pixel.  Horizontal pass first,
// then vertical, as OpenCV does.
template <typename Fetch>
__device__ __forceinline__ float3 bilinear3(int oy, int ox, int H0, int W0, double sy, double sx, Fetch fetch) {
  const Taps ty = linear_taps(oy, sy, H0, false), tx = linear_taps(ox, sx, W0, true);
  const float3 h0 = lerp3(fetch(ty.s0, tx.s0), fetch(ty.s0, tx.s1), tx.f);
  const float3 h1 = lerp3(fetch(ty.s1, tx.s0), fetch(ty.s1, tx.s1), tx.f);
  return lerp3(h0, h1, ty.f);
}

}  // namespace linear
}  // namespace shdr

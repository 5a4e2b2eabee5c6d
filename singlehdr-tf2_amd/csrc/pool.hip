// Pooling, bilinear 2x resize and global average pooling, forward (NHWC fp32, gfx950): the fp32 instantiations of the channel-vector
// kernels of nhwc_vec.h, one thread per 16-byte channel quad.
#include "nhwc_vec.h"

using shdr::check_nhwc;
using shdr::launch_vec;

extern "C" int shdr_avgpool2_fwd_f32(const float* x, float* y, int N, int H, int W, int C, void* stream) {
  if (int rc = check_nhwc<4>("avgpool2", x, y, N, H, W, C)) return rc;
  SHDR_REQUIRE(H >= 2 && W >= 2, SHDR_E_SHAPE, "avgpool2: H, W must be >= 2");
  return launch_vec("avgpool2", shdr::pool2_kernel<float, false>, (long)N * (H / 2) * (W / 2) * (C / 4), stream, x, y, N, H, W, C);
}

extern "C" int shdr_maxpool2_fwd_f32(const float* x, float* y, int N, int H, int W, int C, void* stream) {
  if (int rc = check_nhwc<4>("maxpool2", x, y, N, H, W, C)) return rc;
  SHDR_REQUIRE((H & 1) == 0 && (W & 1) == 0, SHDR_E_SHAPE, "maxpool2: H=%d, W=%d must be even", H, W);
  return launch_vec("maxpool2", shdr::pool2_kernel<float, true>, (long)N * (H / 2) * (W / 2) * (C / 4), stream, x, y, N, H, W, C);
}

extern "C" int shdr_maxpool3s2_fwd_f32(const float* x, float* y, int N, int H, int W, int C, void* stream) {
  if (int rc = check_nhwc<4>("maxpool3s2", x, y, N, H, W, C)) return rc;
  int Ho, Wo, pt, pl;
  shdr_same_pad(H, 3, 2, &Ho, &pt);
  shdr_same_pad(W, 3, 2, &Wo, &pl);
  return launch_vec("maxpool3s2", shdr::maxpool3s2_kernel<float>, (long)N * Ho * Wo * (C / 4), stream, x, y, N, H, W, C, Ho, Wo, pt, pl);
}

extern "C" int shdr_resize2x_fwd_f32(const float* x, float* y, int N, int H, int W, int C, void* stream) {
  if (int rc = check_nhwc<4>("resize2x", x, y, N, H, W, C)) return rc;
  return launch_vec("resize2x", shdr::resize2x_kernel<float>, (long)N * H * W * (C / 4), stream, x, y, N, H, W, C);
}

extern "C" int shdr_gap_fwd_f32(const float* x, float* y, int N, int HW, int C, void* stream) {
  if (int rc = check_nhwc<4>("gap", x, y, N, HW, 1, C)) return rc;
  hipLaunchKernelGGL(shdr::gap_kernel<float>, dim3((C + 63) / 64, N), dim3(256), 0, shdr::stream_of(stream), x, y, HW, C);
  return shdr::check_launch("gap");
}

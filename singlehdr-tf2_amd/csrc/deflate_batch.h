// What the batched device encoders (csrc/deflate.hip, csrc/deflate_lz.hip) share beside the codec headers: the chunk bounds, the
// scan of the stored sizes and the checks of the host arguments.  Included by both; every translation unit gets its own copy.
#pragma once
#include "shdr_internal.h"
#include "deflate_huffman.h"

namespace shdr_deflate_batch {
namespace {                                   // internal linkage: the kernel and its host stub exist once per translation unit

using shdr_deflate::kMaxChunk;

inline hipStream_t S(void* s) { return reinterpret_cast<hipStream_t>(s); }
inline int64_t align16(int64_t v) { return (v + 15) & ~(int64_t)15; }

// chunk c of the batch, clamped into the data: [lo, lo + n)
__device__ __forceinline__ void chunk_range(const int64_t* __restrict__ offsets, int64_t c, int64_t total, int64_t& lo, int64_t& n) {
  int64_t a = offsets[c], b = offsets[c + 1];
  a = a < 0 ? 0 : a > total ? total : a;
  b = b < a ? a : b > total ? total : b;
  if (b - a > kMaxChunk) b = a + kMaxChunk;
  lo = a;
  n = b - a;
}

// out_offsets[c] = sum of the sizes before c, out_offsets[C] = the total.  One block.
__global__ __launch_bounds__(1024) void deflate_scan_kernel(const int64_t* __restrict__ sizes, int64_t count, int64_t* __restrict__ out_offsets) {
  __shared__ int64_t part[16];
  __shared__ int64_t carry_s;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  if (threadIdx.x == 0) carry_s = 0;
  __syncthreads();
  for (int64_t base = 0; base < count; base += 1024) {
    const int64_t r = base + threadIdx.x;
    const int64_t v = r < count ? sizes[r] : 0;
    int64_t incl = v;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
      const int64_t t = __shfl_up(incl, off, 64);
      if (lane >= off) incl += t;
    }
    if (lane == 63) part[wave] = incl;
    __syncthreads();
    int64_t before = carry_s;
    for (int w = 0; w < wave; ++w) before += part[w];
    if (r < count) out_offsets[r] = before + incl - v;
    __syncthreads();
    if (threadIdx.x == 1023) carry_s = before + incl;
    __syncthreads();
  }
  if (threadIdx.x == 0) out_offsets[count] = carry_s;
}

int check_offsets(const char* what, const int64_t* offsets, int n_chunks, int pad, int64_t* total, int64_t* bound) {
  SHDR_REQUIRE(offsets, SHDR_E_NULL, "%s: null offsets", what);
  SHDR_REQUIRE(n_chunks > 0, SHDR_E_SHAPE, "%s: the number of chunks must be positive, got %d", what, n_chunks);
  SHDR_REQUIRE(pad >= 0 && pad <= 4096, SHDR_E_SHAPE, "%s: pad must be in [0, 4096], got %d", what, pad);
  SHDR_REQUIRE(offsets[0] == 0, SHDR_E_SHAPE, "%s: offsets[0] must be 0", what);
  for (int c = 0; c < n_chunks; ++c) {
    const int64_t n = offsets[c + 1] - offsets[c];
    SHDR_REQUIRE(n >= 1 && n <= kMaxChunk, SHDR_E_SHAPE, "%s: chunk %d has %lld bytes (1 .. 2^30 are supported)", what, c, (long long)n);
  }
  *total = offsets[n_chunks];
  *bound = offsets[n_chunks] + (int64_t)pad * n_chunks;          // a stored chunk is never larger than the chunk
  return SHDR_OK;
}

}  // namespace
}  // namespace shdr_deflate_batch

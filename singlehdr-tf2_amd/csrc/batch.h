// What the batched byte coders (deflate, inflate, Radiance RLE, JPEG, PIZ, the EXR packers) share on the device and on the host
// (DESIGN.md "What the byte coders share").  Integer helpers only; every one is pinned by the coders' byte-for-byte tests.
//   wave_scan     inclusive scan over the 64 lanes of a wave
//   block_scan    exclusive prefix over the lanes of a block (+ the block's total)
//   scan_array    exclusive prefix sum of an array of any length by ONE block: the carry loop
//   clamped_span  chunk c of an offset table, clamped into its buffer whatever the device copy of the table holds
//   last_le       the last i with a[i] <= v
//   Carver        a workspace cut into 16-byte aligned parts (host)
#pragma once
#include "shdr_internal.h"

namespace shdr {

inline constexpr int64_t align16(int64_t v) { return (v + 15) & ~(int64_t)15; }

struct plus {
  template <class T>
  __device__ __forceinline__ T operator()(T a, T b) const { return a + b; }
};
struct maximum {
  template <class T>
  __device__ __forceinline__ T operator()(T a, T b) const { return a < b ? b : a; }
};

// Inclusive scan of v over the lanes of this wave (blocks are one-dimensional: lane = threadIdx.x & 63).  Unsigned sums wrap.
template <class T, class Op = plus>
__device__ __forceinline__ T wave_scan(T v, Op op = Op()) {
  const int lane = threadIdx.x & 63;
#pragma unroll
  for (int off = 1; off < 64; off <<= 1) {
    const T t = __shfl_up(v, off, 64);
    if (lane >= off) v = op(v, t);
  }
  return v;
}

// Exclusive prefix sum of v over the THREADS lanes of the block; the inclusive one is the result + v.  Every lane calls it.
// part: LDS [THREADS / 64].  One barrier after the waves' sums are written, one before it returns: part may be written again.
template <int THREADS, class T>
__device__ __forceinline__ T block_scan(T v, T* part) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const T incl = wave_scan(v);
  if (lane == 63) part[wave] = incl;
  __syncthreads();
  T before = 0;
  for (int w = 0; w < wave; ++w) before += part[w];
  __syncthreads();
  return before + incl - v;
}
// ... and the sum over the whole block, the same in every lane
template <int THREADS, class T>
__device__ __forceinline__ T block_scan(T v, T* part, T& total) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const T incl = wave_scan(v);
  if (lane == 63) part[wave] = incl;
  __syncthreads();
  T before = 0, all = 0;
  for (int w = 0; w < THREADS / 64; ++w) {
    if (w < wave) before += part[w];
    all += part[w];
  }
  __syncthreads();
  total = all;
  return before + incl - v;
}

// store(i, load(0) + ... + load(i - 1)) for every i < n, by the ONE block of THREADS lanes that calls it (all of them), PER
// consecutive items per lane and step; returns the sum of all n, the same in every lane.  The sums have the type load returns.
// load(i) is called before store(i, .) by the same lane, so the scan may run in place.
// A step is bound by the latency of its loads, and the first of them also waits for whatever stores are still in flight: the stores are
// issued TWO barriers in front of the next step's loads (with block_scan and the stores right in front of the loads, the 4-item scans
// of jpeg_enc.hip took 16 % longer).
template <int THREADS, int PER, class Load, class Store>
__device__ __forceinline__ auto scan_array(int64_t n, Load load, Store store) -> decltype(load((int64_t)0)) {
  using T = decltype(load((int64_t)0));
  __shared__ T part[THREADS / 64];
  __shared__ T carry_s;                                          // the sum of the steps before this one
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  if (threadIdx.x == 0) carry_s = 0;
  __syncthreads();
  for (int64_t base = 0; base < n; base += (int64_t)THREADS * PER) {
    const int64_t i0 = base + (int64_t)PER * threadIdx.x;
    T v[PER], mine = 0;
#pragma unroll
    for (int k = 0; k < PER; ++k) {
      v[k] = i0 + k < n ? load(i0 + k) : (T)0;
      mine += v[k];
    }
    const T incl = wave_scan(mine);
    if (lane == 63) part[wave] = incl;
    __syncthreads();
    T before = carry_s;
    for (int w = 0; w < wave; ++w) before += part[w];
    T run = before + incl - mine;
#pragma unroll
    for (int k = 0; k < PER; ++k) {
      if (i0 + k < n) store(i0 + k, run);
      run += v[k];
    }
    __syncthreads();
    if (threadIdx.x == THREADS - 1) carry_s = before + incl;
    __syncthreads();
  }
  return carry_s;
}

// [off[c], off[c + 1]) clamped into [0, total] and to max_len bytes: nothing a kernel derives from it leaves the buffer
struct Span {
  int64_t lo, n;
};
__device__ __forceinline__ Span clamped_span(const int64_t* __restrict__ off, int64_t c, int64_t total, int64_t max_len = INT64_MAX) {
  int64_t a = off[c], b = off[c + 1];
  a = a < 0 ? 0 : a > total ? total : a;
  b = b < a ? a : b > total ? total : b;
  if (b - a > max_len) b = a + max_len;
  return Span{a, b - a};
}

// the last i in [0, n) with a[i] <= v (a is sorted and a[0] <= v is given)
template <class T>
__device__ __forceinline__ int64_t last_le(const T* __restrict__ a, int64_t n, T v) {
  int64_t lo = 0, hi = n;
  while (hi - lo > 1) {
    const int64_t mid = (lo + hi) >> 1;
    if (a[mid] <= v) lo = mid; else hi = mid;
  }
  return lo;
}

// A caller's workspace cut into parts, each on a multiple of 16 bytes: Carver c(base); w.bits = c.take<int64_t>(n); ...
// w.bytes = c.bytes().  With base NULL only the sizes mean anything (the *_sizes entry points).
class Carver {
 public:
  explicit Carver(void* base) : p_(static_cast<char*>(base)) {}
  template <class T>
  T* take(int64_t count) {
    T* r = reinterpret_cast<T*>(p_ + o_);
    o_ += align16((int64_t)sizeof(T) * count);
    return r;
  }
  int64_t bytes() const { return o_; }

 private:
  char* p_;
  int64_t o_ = 0;
};

}  // namespace shdr

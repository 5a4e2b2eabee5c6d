// zlib streams of a BATCH of chunks inflated on the device, one launch: the decoder is inflate_zlib of inflate.h, the very code of the
// host routine shdr_inflate_host, so the checks (and the per-chunk status codes) are the same on both sides.
//
// One 64-lane workgroup -- one wave -- per chunk.  Decoding a stream is serial: the bit buffer, the positions and every table entry are
// the same in all 64 lanes (values that come out of memory pass through readfirstlane, so the compiler may keep the whole decode state
// on the scalar side), and every branch of the decoder is taken by all lanes together.  What the lanes share out is
//   * the stream: a 2 KiB window of it is staged in LDS by all lanes (aligned dwords, bytes at the ends of the stream: nothing outside
//     [src, src + n) is read), and the bit buffer is refilled from there, 32 bits at a time;
//   * table construction: one lane counts and sorts the code lengths, all lanes fill the one-lookup tables;
//   * emission: the last 32 KiB of output live in an LDS ring, which is the DEFLATE window.  A match of length L at distance D is
//     ring[pos + i] = ring[pos - D + (i mod D)], lane i (and i + 64, ...): only bytes from before the match are read, so an overlapping
//     match needs no order inside the copy.  In a ring of exactly 32 KiB the slot that lane i writes can be the slot that lane
//     i - (32768 - D) reads, a lower lane or an earlier pass of the same wave: a wave runs its LDS reads and writes in program order,
//     the read comes first;
//   * the flush of the ring to global memory, before unflushed bytes could be overwritten (every 32 KiB or so) and at the end: bytes up
//     to a 4-byte boundary of the destination, aligned dwords (each put together from two LDS dwords), the bytes that are left.  The
//     Adler-32 is summed in the same pass: A = sum b[i], B = sum i b[i] per lane in 64 bits (i < 2^30: no overflow), so that
//     s1 = 1 + A and s2 = N + N A - B (mod 65521) once N is known.  Matches never read global memory.
// LDS: ring 32 KiB + window 2 KiB + tables 4.5 KiB: four workgroups per CU.  Deterministic, no atomics, no host wait, no allocation.
#include "shdr_internal.h"
#include "batch.h"
#include "inflate.h"

namespace {

using namespace shdr_inflate;

constexpr int kLanes = 64;
constexpr int kRing = kWindow;                                   // bytes; a power of two
constexpr int kInWords = 512;                                    // dwords of the staged stream window

__device__ __forceinline__ uint32_t rfl(uint32_t v) { return (uint32_t)__builtin_amdgcn_readfirstlane((int)v); }
__device__ __forceinline__ int64_t rfl64(int64_t v) {
  return (int64_t)(((uint64_t)rfl((uint32_t)((uint64_t)v >> 32)) << 32) | rfl((uint32_t)v));
}
// LDS accesses of one wave complete in program order; this only keeps the compiler from moving them across
__device__ __forceinline__ void wave_order() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

struct DeviceIo {
  const uint8_t* src;
  int64_t n;
  uint8_t* dst;
  uint8_t* ring;                                                 // LDS [kRing]
  uint32_t* inw;                                                 // LDS [kInWords]
  int64_t wbase;                                                 // stream position of inw[0]; the window is valid where it overlaps [0, n)
  bool wvalid;
  int64_t flushed;
  uint64_t sumA, sumB;                                           // this lane's share of the checksum
  int ln;

  __device__ __forceinline__ void refill(int64_t pos) {
    const int64_t base = pos - (int64_t)((reinterpret_cast<uintptr_t>(src) + (uint64_t)pos) & 3u);   // an aligned address; >= -3
    wave_order();
    for (int j = ln; j < kInWords; j += kLanes) {
      const int64_t o = base + 4 * (int64_t)j;
      uint32_t w = 0;
      if (o >= 0 && o + 4 <= n) {
        w = *reinterpret_cast<const uint32_t*>(src + o);
      } else {
        for (int k = 0; k < 4; ++k)
          if (o + k >= 0 && o + k < n) w |= (uint32_t)src[o + k] << (8 * k);
      }
      inw[j] = w;
    }
    wbase = rfl64(base);
    wvalid = true;
    wave_order();
  }
  __device__ __forceinline__ uint32_t word(int64_t pos) {
    if (!wvalid || pos < wbase || pos - wbase > 4 * kInWords - 8) refill(pos);
    const int r = (int)(pos - wbase);                            // 0 .. 4 kInWords - 8
    const uint32_t w0 = inw[r >> 2], w1 = inw[(r >> 2) + 1];
    return rfl((uint32_t)((((uint64_t)w1 << 32) | w0) >> (8 * (r & 3))));
  }
  static __device__ __forceinline__ uint32_t uniform(uint32_t v) { return rfl(v); }
  __device__ __forceinline__ bool leader() const { return ln == 0; }
  __device__ __forceinline__ int lane() const { return ln; }
  static __device__ __forceinline__ int lanes() { return kLanes; }
  static __device__ __forceinline__ void sync() { __syncthreads(); }

  __device__ __forceinline__ void sum(int64_t i, uint32_t b) {
    sumA += b;
    sumB += (uint64_t)i * b;
  }
  // ring bytes [flushed, upto) -> dst; upto - flushed <= kRing
  __device__ __forceinline__ void flush(int64_t upto) {
    wave_order();
    int64_t a = flushed;
    int64_t head = (int64_t)((4u - (uint32_t)(reinterpret_cast<uintptr_t>(dst + a) & 3u)) & 3u);
    if (head > upto - a) head = upto - a;
    if (ln < head) {
      const uint8_t v = ring[(a + ln) & (kRing - 1)];
      dst[a + ln] = v;
      sum(a + ln, v);
    }
    a += head;
    const int64_t words = (upto - a) >> 2;
    const uint32_t* ring32 = reinterpret_cast<const uint32_t*>(ring);
    for (int64_t w = ln; w < words; w += kLanes) {
      const int64_t p = a + 4 * w;
      const int r = (int)(p & (kRing - 1));
      const uint32_t w0 = ring32[r >> 2], w1 = ring32[((r >> 2) + 1) & (kRing / 4 - 1)];
      const uint32_t v = (uint32_t)((((uint64_t)w1 << 32) | w0) >> (8 * (r & 3)));
      *reinterpret_cast<uint32_t*>(dst + p) = v;
      const uint32_t b0 = v & 255u, b1 = (v >> 8) & 255u, b2 = (v >> 16) & 255u, b3 = v >> 24;
      sumA += b0 + b1 + b2 + b3;
      sumB += (uint64_t)p * (b0 + b1 + b2 + b3) + (b1 + 2 * b2 + 3 * b3);
    }
    a += 4 * words;
    if (ln < upto - a) {
      const uint8_t v = ring[(a + ln) & (kRing - 1)];
      dst[a + ln] = v;
      sum(a + ln, v);
    }
    flushed = upto;
    wave_order();
  }
  __device__ __forceinline__ void room(int64_t out, int len) {
    if (out + len - flushed > kRing) flush(out);
  }
  __device__ __forceinline__ void put(int64_t out, uint8_t v) {
    if (ln == 0) ring[out & (kRing - 1)] = v;
    wave_order();
  }
  __device__ __forceinline__ void copy(int64_t out, int len, int dist) {
    const uint32_t o = (uint32_t)out, D = (uint32_t)dist;        // ring indices need the low 15 bits only
    if (dist >= len) {
      for (uint32_t i = ln; i < (uint32_t)len; i += kLanes) ring[(o + i) & (kRing - 1)] = ring[(o - D + i) & (kRing - 1)];
    } else if (dist == 1) {
      const uint8_t v = ring[(o - 1u) & (kRing - 1)];
      for (uint32_t i = ln; i < (uint32_t)len; i += kLanes) ring[(o + i) & (kRing - 1)] = v;
    } else {
      for (uint32_t i = ln; i < (uint32_t)len; i += kLanes) ring[(o + i) & (kRing - 1)] = ring[(o - D + i % D) & (kRing - 1)];
    }
    wave_order();
  }
  __device__ __forceinline__ void raw(int64_t out, int64_t pos, int len) {
    const uint32_t o = (uint32_t)out;
    for (int i = ln; i < len; i += kLanes) ring[(o + (uint32_t)i) & (kRing - 1)] = src[pos + i];
    wave_order();
  }
  __device__ __forceinline__ void finish(int64_t out) {
    if (out > flushed) flush(out);
  }
  __device__ __forceinline__ uint32_t adler(int64_t out) const {
    uint64_t a = sumA % kAdlerMod, b = sumB % kAdlerMod;
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
      a += __shfl_xor(a, off, kLanes);
      b += __shfl_xor(b, off, kLanes);
    }
    a %= kAdlerMod;
    b %= kAdlerMod;
    const uint64_t nm = (uint64_t)out % kAdlerMod;
    const uint64_t s1 = (1 + a) % kAdlerMod, s2 = (nm + nm * a + kAdlerMod - b) % kAdlerMod;
    return rfl((uint32_t)((s2 << 16) | s1));
  }
};

__global__ __launch_bounds__(kLanes) void inflate_kernel(const uint8_t* __restrict__ src, int64_t src_bytes, const int64_t* __restrict__ src_off,
                                                         uint8_t* __restrict__ dst, int64_t dst_bytes, const int64_t* __restrict__ dst_off,
                                                         const uint8_t* __restrict__ mode, int32_t* __restrict__ status,
                                                         int64_t* __restrict__ written) {
  __shared__ __attribute__((aligned(16))) uint8_t ring[kRing];
  __shared__ uint32_t inw[kInWords];
  __shared__ Tables tables;
  const int64_t c = blockIdx.x;
  const int ln = threadIdx.x;
  const shdr::Span from = shdr::clamped_span(src_off, c, src_bytes, kMaxChunk), slot = shdr::clamped_span(dst_off, c, dst_bytes, kMaxChunk);
  const int64_t slo = rfl64(from.lo), n = rfl64(from.n), dlo = rfl64(slot.lo), cap = rfl64(slot.n);
  const uint32_t m = mode ? rfl(mode[c]) : 1u;
  int st;
  int64_t wrote = 0;
  if (m == 0) {                                                  // stored raw: the slot's bytes as they are
    if (n == cap) {
      for (int64_t i = ln; i < n; i += kLanes) dst[dlo + i] = src[slo + i];
      wrote = n;
      st = kOk;
    } else {
      st = kRawSize;
    }
  } else if (m == 1) {
    DeviceIo io{src + slo, n, dst + dlo, ring, inw, 0, false, 0, 0, 0, ln};
    st = inflate_zlib(io, tables, n, cap, &wrote);
  } else {
    st = kMode;
  }
  if (ln == 0) {
    status[c] = st;
    written[c] = wrote;
  }
}

// offsets of one side of a batch: non-decreasing, inside [0, *total]
int check_table(const char* what, const char* name, const int64_t* off, int n_chunks, int64_t limit, int64_t total) {
  SHDR_REQUIRE(off[0] >= 0, SHDR_E_SHAPE, "%s: %s[0] is negative", what, name);
  for (int c = 0; c < n_chunks; ++c) {
    const int64_t n = off[c + 1] - off[c];
    SHDR_REQUIRE(n >= 0 && n <= limit, SHDR_E_SHAPE, "%s: chunk %d has %lld bytes in %s (0 .. 2^30 are supported)", what, c, (long long)n, name);
  }
  SHDR_REQUIRE(total < 0 || off[n_chunks] <= total, SHDR_E_SHAPE, "%s: %s ends at %lld, the buffer holds %lld bytes", what, name,
               (long long)off[n_chunks], (long long)total);
  return SHDR_OK;
}

int check_tables(const char* what, const int64_t* src_off, const int64_t* dst_off, int n_chunks, int64_t src_bytes, int64_t dst_bytes) {
  SHDR_REQUIRE(src_off && dst_off, SHDR_E_NULL, "%s: null offsets", what);
  SHDR_REQUIRE(n_chunks > 0, SHDR_E_SHAPE, "%s: the number of chunks must be positive, got %d", what, n_chunks);
  if (int rc = check_table(what, "src_off", src_off, n_chunks, kMaxChunk, src_bytes)) return rc;
  return check_table(what, "dst_off", dst_off, n_chunks, kMaxChunk, dst_bytes);
}

}  // namespace

extern "C" int64_t shdr_inflate_host(const uint8_t* src, int64_t n, uint8_t* dst, int64_t capacity, int* status) {
  const int64_t r = inflate_host(src, n, dst, capacity, status);
  if (r < 0) shdr::set_error("inflate_host: bad arguments (null pointer, a negative size, or a capacity beyond 2^30 bytes)");
  return r;
}

extern "C" int shdr_inflate_batch_sizes(const int64_t* src_off, const int64_t* dst_off, int n_chunks, int64_t* src_bytes, int64_t* dst_bytes) {
  if (int rc = check_tables("inflate_batch_sizes", src_off, dst_off, n_chunks, -1, -1)) return rc;
  if (src_bytes) *src_bytes = src_off[n_chunks];
  if (dst_bytes) *dst_bytes = dst_off[n_chunks];
  return SHDR_OK;
}

extern "C" int shdr_inflate_batch(const uint8_t* src, int64_t src_bytes, const int64_t* src_off, const int64_t* src_off_dev, uint8_t* dst,
                                  int64_t dst_bytes, const int64_t* dst_off, const int64_t* dst_off_dev, const uint8_t* mode, int n_chunks,
                                  int32_t* status, int64_t* written, void* stream, float* stage_ms) {
  const char* what = "inflate_batch";
  SHDR_REQUIRE(src_off_dev && dst_off_dev && status && written, SHDR_E_NULL, "%s: null pointer", what);
  SHDR_REQUIRE(src_bytes >= 0 && dst_bytes >= 0 && (src || !src_bytes) && (dst || !dst_bytes), SHDR_E_NULL, "%s: null buffer", what);
  if (int rc = check_tables(what, src_off, dst_off, n_chunks, src_bytes, dst_bytes)) return rc;
  SHDR_REQUIRE((reinterpret_cast<uintptr_t>(src_off_dev) & 7u) == 0 && (reinterpret_cast<uintptr_t>(dst_off_dev) & 7u) == 0 &&
                   (reinterpret_cast<uintptr_t>(written) & 7u) == 0 && (reinterpret_cast<uintptr_t>(status) & 3u) == 0,
               SHDR_E_ALIGN, "%s: the offset tables and `written` must be 8-byte aligned, `status` 4-byte aligned", what);
  hipStream_t st = shdr::stream_of(stream);
  shdr::StageTimer<SHDR_INFLATE_STAGES> timer(stage_ms, st);
  hipLaunchKernelGGL(inflate_kernel, dim3((unsigned)n_chunks), dim3(kLanes), 0, st, src, src_bytes, src_off_dev, dst, dst_bytes, dst_off_dev,
                     mode, status, written);
  timer.mark();
  return shdr::check_launch(what);
}

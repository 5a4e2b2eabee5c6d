// Internal helpers shared by the libshdr translation units (gfx950 only).
#pragma once
#include <hip/hip_runtime.h>
#include <stdlib.h>
#include <stdarg.h>
#include <stdint.h>
#include <stdio.h>

#include "shdr.h"

// ---- MFMA / LDS-DMA vocabulary of the matrix-pipe kernels: the vector operands and the address spaces of global_load_lds ----------------
using f32x4 = __attribute__((ext_vector_type(4))) float;
using f16x8 = __attribute__((ext_vector_type(8))) _Float16;
using f16x4 = __attribute__((ext_vector_type(4))) _Float16;
typedef __attribute__((__vector_size__(4 * sizeof(short)))) short sv4;      // one ds_read_b64_tr_b16
typedef __attribute__((address_space(1))) const void* gptr_t;
typedef __attribute__((address_space(3))) void* lptr_t;
typedef __attribute__((address_space(3))) sv4* lsv4_t;
// Images with 64-byte rows (32 halves: one MFMA k-chunk of a pixel or of a cout): physical 16-byte slot = k-group ^ row_swz(row),
// conflict-free for the four 16-lane groups of a ds_read_b128; applied on the SOURCE address of the LDS-DMA.
__host__ __device__ inline int row_swz(int row) { return (-(row >> 2)) & 3; }

namespace shdr {

// thread-local last-error message, returned by shdr_last_error()
void set_error(const char* fmt, ...);

inline int fail(int code, const char* fmt, ...) __attribute__((format(printf, 2, 3)));
inline int fail(int code, const char* fmt, ...) {
  char buf[512];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof(buf), fmt, ap);
  va_end(ap);
  set_error("%s", buf);
  return code;
}

inline int check_launch(const char* what) {
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return fail(SHDR_E_LAUNCH, "%s: %s", what, hipGetErrorString(e));
  return SHDR_OK;
}

// Launch-time state that HIP keeps per device (hipFuncSetAttribute, occupancy) is cached per device, not per process: a host
// that drives several GPUs from one process (the reference's tf.distribute.MirroredStrategy layout) gets it right as well.
constexpr int kMaxDevices = 16;
inline int device_slot() {
  int d = 0;
  if (hipGetDevice(&d) != hipSuccess) d = 0;
  return d & (kMaxDevices - 1);
}

// The 16 zero bytes that an out-of-image LDS-DMA piece reads instead of the tensor.  Internal linkage: the library is built without
// relocatable device code, so every translation unit that stages with LDS-DMA carries its own instance (and the others none).
static __device__ __attribute__((aligned(16))) unsigned zero_page[4] = {0u, 0u, 0u, 0u};

inline bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }

// the `void* stream` of the C ABI (include/shdr.h) as HIP's handle
inline hipStream_t stream_of(void* s) { return reinterpret_cast<hipStream_t>(s); }

// SHDR_* environment switches (kernel-family opt-outs, tile experiments, thresholds) are read ONCE per call site and process, not on
// every launch -- a conv launch used to walk the environment up to ten times.  shdr_config_reload() (include/shdr.h) invalidates every
// cached value: call it after changing a switch inside a running process (the tests do).
extern int g_env_epoch;
struct EnvSlot {
  int epoch = -1;
  const char* value = nullptr;
};
inline const char* env_cached(EnvSlot& slot, const char* name) {
  const int e = __atomic_load_n(&g_env_epoch, __ATOMIC_ACQUIRE);
  if (slot.epoch != e) {                         // (two threads racing here store the same two words)
    slot.value = getenv(name);
    slot.epoch = e;
  }
  return slot.value;
}
#define SHDR_ENV(name) ([]() -> const char* { static ::shdr::EnvSlot slot; return ::shdr::env_cached(slot, name); }())

// shdr_order_dependent_launches(): bumped on the host by every launch whose RESULT depends on the order in which floating-point atomics
// reach memory (more than one atomic add per address).  Nothing on the device.
extern int64_t g_order_dependent_launches;
inline void count_order_dependent() { __atomic_add_fetch(&g_order_dependent_launches, 1, __ATOMIC_RELAXED); }

#define SHDR_REQUIRE(cond, code, ...) \
  do {                                \
    if (!(cond)) return ::shdr::fail((code), __VA_ARGS__); \
  } while (0)

// The optional device-event times of a call's N stages (the stage_ms arguments of shdr.h): an event in front of the first stage, mark()
// behind every stage; the destructor waits for the last event recorded and fills out[0 .. N).  Measurement never fails the call it
// measures: a time that an event call kept from being read is -1, a stage that the call never reached (no mark()) is 0.  Nothing is
// created, recorded or waited for when out is NULL, nothing is allocated, and every event created is destroyed.
template <int N>
class StageTimer {
 public:
  StageTimer(float* out, hipStream_t st) : out_(out), st_(st) {
    if (!out_) return;
    while (made_ <= N && hipEventCreate(&ev_[made_]) == hipSuccess) ++made_;
    mark();
  }
  StageTimer(const StageTimer&) = delete;
  StageTimer& operator=(const StageTimer&) = delete;
  void mark() {
    if (marks_ == recorded_ && recorded_ < made_ && hipEventRecord(ev_[recorded_], st_) == hipSuccess) ++recorded_;
    ++marks_;
  }
  ~StageTimer() {
    if (!out_) return;
    const bool ok = recorded_ > 0 && hipEventSynchronize(ev_[recorded_ - 1]) == hipSuccess;
    for (int i = 0; i < N; ++i) {
      if (i + 1 >= marks_) out_[i] = 0.0f;
      else if (!ok || i + 1 >= recorded_ || hipEventElapsedTime(&out_[i], ev_[i], ev_[i + 1]) != hipSuccess) out_[i] = -1.0f;
    }
    for (int i = 0; i < made_; ++i) (void)hipEventDestroy(ev_[i]);
  }

 private:
  float* out_;
  hipStream_t st_;
  hipEvent_t ev_[N + 1];
  int made_ = 0, marks_ = 0, recorded_ = 0;      // events created; mark() calls; events recorded (the first `recorded_` marks)
};

// Grid size for HBM-bound grid-stride kernels: ~8 blocks of 256 threads per CU.
inline int stream_grid(int64_t work_items, int block = 256) {
  int64_t g = (work_items + block - 1) / block;
  if (g < 1) g = 1;
  if (g > 256 * 8) g = 256 * 8;
  return static_cast<int>(g);
}

// Block slots of the chip for one kernel: CUs x the kernel's occupancy at this block size and dynamic LDS (0 on failure).
// The split-K weight-gradient kernels cut their grids to ONE round of these slots: every block pays a prologue and a tile of
// atomics, and a grid a few blocks over a whole round spends that round on a handful of CUs (wgrad_f16.hip has the measurements).
template <typename KernelT>
inline long block_slots(KernelT kernel, int threads, size_t lds) {
  int dev = 0, cus = 0, occ = 0;
  if (hipGetDevice(&dev) != hipSuccess || hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess ||
      hipOccupancyMaxActiveBlocksPerMultiprocessor(&occ, kernel, threads, lds) != hipSuccess || cus < 1 || occ < 1)
    return 0;
  return (long)cus * occ;
}
// The launch set-up that HIP keeps per (kernel, device), done once per pair: the kernel is the template argument, so every instantiation
// has its own memo and a launch site is one call.  Each returns SHDR_OK or SHDR_E_ARCH with the runtime's message; none makes a HIP call
// beyond hipGetDevice once the pair is set up.
// The dynamic-LDS limit: one hipFuncSetAttribute per size needed -- a kernel launched with one size sets it once, one whose size depends
// on the layer raises it whenever a larger size arrives.
template <auto Kernel>
inline int dynamic_lds(int lds) {
  static int set_dev[kMaxDevices] = {};
  int& set = set_dev[device_slot()];
  if (lds > set) {
    hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(Kernel), hipFuncAttributeMaxDynamicSharedMemorySize, lds);
    if (e != hipSuccess) return fail(SHDR_E_ARCH, "hipFuncSetAttribute: %s", hipGetErrorString(e));
    set = lds;
  }
  return SHDR_OK;
}
// ... and the kernel's block slots (the split-K weight gradients); a failed query is an error named after `who`
template <auto Kernel>
inline int dynamic_lds_slots(int threads, int lds, const char* who, long& slots) {
  static long slots_dev[kMaxDevices] = {};
  long& s = slots_dev[device_slot()];
  if (s == 0) {
    if (int e = dynamic_lds<Kernel>(lds)) return e;
    s = block_slots(Kernel, threads, lds);
    if (s == 0) return fail(SHDR_E_ARCH, "%s: occupancy query failed", who);
  }
  slots = s;
  return SHDR_OK;
}
// ... and the kernel's blocks per CU at that size, 1 .. cap (the persistent grids), asked again when the size changes; a failed query
// counts as 1
template <auto Kernel>
inline int dynamic_lds_occupancy(int threads, int lds, int cap, int& occ) {
  static int occ_dev[kMaxDevices] = {}, lds_dev[kMaxDevices] = {};     // (LDS bytes are never 0 here: 0 = not queried yet)
  const int slot = device_slot();
  if (lds != lds_dev[slot]) {
    if (int e = dynamic_lds<Kernel>(lds)) return e;
    int nb = 0;
    const hipError_t e = hipOccupancyMaxActiveBlocksPerMultiprocessor(&nb, reinterpret_cast<const void*>(Kernel), threads, lds);
    occ_dev[slot] = (e != hipSuccess || nb < 1) ? 1 : (nb > cap ? cap : nb);
    lds_dev[slot] = lds;
  }
  occ = occ_dev[slot];
  return SHDR_OK;
}
// slices (of `units` work items, at least `min_slice` each) per tile so that tiles x slices fills `rounds` rounds of the slots
inline long slice_for_rounds(long slots, long tiles, long units, long min_slice) {
  long rounds = 1;
  if (const char* e = SHDR_ENV("SHDR_WGRAD_ROUNDS")) rounds = atol(e) > 0 ? atol(e) : 1;
  long ns = slots * rounds / tiles;
  if (ns < 1) ns = 1;
  long slice = (units + ns - 1) / ns;
  return slice < min_slice ? min_slice : slice;
}

// out[c] += sum over the g partial rows ws[b * C + c] (written by reduction kernels that give every block its own row instead
// of ending in atomics on the same C addresses).  Block = 16 columns x 16 row lanes, four independent loads in flight per thread
// (64 columns x 4 row lanes with one dependent load chain per thread took 43 us on 2048 rows: latency-bound), blockIdx.y = row slice.
__global__ __launch_bounds__(256) static void col_fold_kernel(const float* __restrict__ ws, float* __restrict__ out, int g, int C) {
  __shared__ double part[16][17];                      // the fold adds in double: its result carries ONE rounding, at the atomic
  const int cl = threadIdx.x & 15, rl = threadIdx.x >> 4;
  const int c = blockIdx.x * 16 + cl;
  const int r0 = blockIdx.y * 256, r1 = r0 + 256 < g ? r0 + 256 : g;
  double t0 = 0.0, t1 = 0.0, t2 = 0.0, t3 = 0.0;
  if (c < C) {
    int r = r0 + rl;
    for (; r + 48 < r1; r += 64) {
      t0 += ws[(size_t)r * C + c]; t1 += ws[(size_t)(r + 16) * C + c]; t2 += ws[(size_t)(r + 32) * C + c]; t3 += ws[(size_t)(r + 48) * C + c];
    }
    for (; r < r1; r += 16) t0 += ws[(size_t)r * C + c];
  }
  part[rl][cl] = (t0 + t1) + (t2 + t3);
  __syncthreads();
  if (rl == 0 && c < C) {
    double t = 0.0;
#pragma unroll
    for (int k = 0; k < 16; ++k) t += part[k][cl];
    atomicAdd(out + c, (float)t);
  }
}
inline void launch_col_fold(const float* ws, float* out, int g, int C, hipStream_t st) {
  if (g > 256) count_order_dependent();                // more than one row slice: several atomics per address
  hipLaunchKernelGGL(col_fold_kernel, dim3((C + 15) / 16, (g + 255) / 256), dim3(256), 0, st, ws, out, g, C);
}
// The deterministic forms (shdr.h "Deterministic mode"): a fold that adds in a FIXED order and touches `out` once per address without an
// atomic, so the caller must order it against every other writer of `out`.
//   out[c] = out[c] + (float)(sum over the g rows of ws[r * rstride + c])     (accumulate = 0: out[c] = the sum)
// col_fold_kernel's block (16 columns x 16 row lanes, double sums) over ALL rows: lane rl adds rows rl, rl + 16, ... in that order, thread
// (0, cl) adds the 16 lane sums in lane order -- the order is a function of g alone.
__global__ __launch_bounds__(256) static void col_fold_det_kernel(const float* __restrict__ ws, float* __restrict__ out, int g, int C,
                                                                  size_t rstride, size_t ystride, int accumulate) {
  __shared__ double part[16][17];
  ws += blockIdx.y * ystride;                          // blockIdx.y: independent column ranges at the same offset of ws and out
  out += blockIdx.y * ystride;
  const int cl = threadIdx.x & 15, rl = threadIdx.x >> 4;
  const int c = blockIdx.x * 16 + cl;
  double t0 = 0.0, t1 = 0.0, t2 = 0.0, t3 = 0.0;
  if (c < C) {
    int r = rl;
    for (; r + 48 < g; r += 64) {
      t0 += ws[(size_t)r * rstride + c]; t1 += ws[(size_t)(r + 16) * rstride + c];
      t2 += ws[(size_t)(r + 32) * rstride + c]; t3 += ws[(size_t)(r + 48) * rstride + c];
    }
    for (; r < g; r += 16) t0 += ws[(size_t)r * rstride + c];
  }
  part[rl][cl] = (t0 + t1) + (t2 + t3);
  __syncthreads();
  if (rl == 0 && c < C) {
    double t = 0.0;
#pragma unroll
    for (int k = 0; k < 16; ++k) t += part[k][cl];
    out[c] = accumulate ? out[c] + (float)t : (float)t;
  }
}
inline void launch_col_fold_det(const float* ws, float* out, int g, int C, hipStream_t st, size_t rstride = 0, int accumulate = 1,
                                int ny = 1, size_t ystride = 0) {
  hipLaunchKernelGGL(col_fold_det_kernel, dim3((C + 15) / 16, ny), dim3(256), 0, st, ws, out, g, C, rstride ? rstride : (size_t)C, ystride,
                     accumulate);
}
// Bijective XCD-aware remap of a 1-D grid: hardware block ids go round-robin over the 8 XCDs, so consecutive LOGICAL ids -- neighbouring
// tiles, the cout slices of one tile, the taps of one slice -- share an XCD and its L2.
__device__ __forceinline__ int xcd_remap(int bid, int nwg) {
  const int q = nwg >> 3, r = nwg & 7, xcd = bid & 7, idx = bid >> 3;
  return (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + idx;
}

// grids of the reductions that have a deterministic form: ONE definition for the launch and for shdr_det_workspace_bytes()
inline int bias_grad_grid(int64_t npix, int C) {
  int CL = 1;
  while (CL < C && CL < 256) CL <<= 1;
  const long PL = 256 / CL;
  long g = (npix + PL * 64 - 1) / (PL * 64);
  return (int)(g < 1 ? 1 : (g > 1024 ? 1024 : g));
}
inline int row_sum_grid(int64_t n, int cap) {             // blocks per sample of diff_loss / sample_dot (cap 128), of tv_loss (cap 512)
  const int g = stream_grid(n);
  return g > cap ? cap : g;
}
constexpr long kDetSlots = 512;              // block slots the slices of a deterministic weight gradient aim at: a constant, not the device's
// bytes of the deterministic weight gradients' workspaces (-1: the family does not take the layer); shdr_det_workspace_bytes()
int64_t wgrad_det_bytes(const shdr_conv2d_desc* d, int which);
int64_t wgrad_winograd_det_bytes(const shdr_conv2d_desc* d, int which);
int64_t wgrad_x3_det_bytes(const shdr_conv2d_desc* d, int which);
constexpr int kApplyRfMaxBlocks = 256;       // blocks per sample of apply_rf_bwd (one slab each in the deterministic form)
constexpr int kBiasMaxBlocks = 2048;         // rows of the act_bwd_bias workspace (shdr_workspace_bytes(SHDR_OP_ACT_BWD_BIAS))

__device__ __forceinline__ float act_apply(float v, int act) {
  switch (act) {
    case SHDR_ACT_RELU: return fmaxf(v, 0.0f);
    case SHDR_ACT_LRELU: return v >= 0.0f ? v : v * 0.1f;
    case SHDR_ACT_TANH: return tanhf(v);
    default: return v;
  }
}

// max |y| of a 256-thread block -> a range slot (conv_x3.hip "Range"): the waves' maxima meet in LDS and ONE thread issues the atomicMax,
// only when the block's maximum exceeds what the slot already holds (same-address atomics execute one after the other at the memory
// side).  Every thread of the block must call it.
__device__ __forceinline__ void range_out_block256(unsigned* slot, float m) {
  __shared__ float range_part[4];
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) m = fmaxf(m, __shfl_xor(m, off, 64));
  if ((threadIdx.x & 63) == 0) range_part[threadIdx.x >> 6] = m;
  __syncthreads();
  if (threadIdx.x == 0) {
    const unsigned b = __float_as_uint(fmaxf(fmaxf(range_part[0], range_part[1]), fmaxf(range_part[2], range_part[3])));
    if (b > __hip_atomic_load(slot, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMax(slot, b);
  }
}

// The activation of four values at once: ONE uniform dispatch per vector instead of one per element, and tanhf -- an inlined libm
// routine of ~45 instructions -- only in kernels instantiated with TANH.  The epilogues of the convolution kernels apply two
// activations to 64 accumulators per lane: with act_apply() per element the epilogue alone was 40 - 70 KB of code (256 copies of
// tanhf), more than the 64 KB instruction cache, and it sits inside the tile loop of the persistent kernels.
// tanh for the heads of the fp32 split-operand kernel: 1 - 2 / (e^{2|x|} + 1) with the hardware exponential and reciprocal (relative error
// < 1e-6 for |x| >= 0.1), the odd polynomial x (1 - x^2/3 + 2 x^4/15 - 17 x^6/315) below it (truncation 1.4e-9 at 0.1) -- the accuracy
// class of the split-operand products themselves (3 * 2^-22 each).  Few registers: the libm routine cost the 16 -> 3 head kernel a wave
// per SIMD (conv_x3n.hip: launch bounds of the 3x3 tanh instantiations; tools/head_cost.py)
__device__ __forceinline__ float tanh_fast(float x) {
  const float ax = fabsf(x), x2 = x * x;
  const float e = __expf(2.0f * ax);                          // inf for large |x|: 2 / inf = 0 -> 1
  const float big = 1.0f - 2.0f * __frcp_rn(e + 1.0f);
  const float small = ax * (1.0f + x2 * (-0.33333334f + x2 * (0.13333334f - 0.05396825f * x2)));
  return copysignf(ax < 0.1f ? small : big, x);
}

// TANH: 0 = not compiled in, 1 = libm's tanhf, 2 = tanh_fast
template <int TANH, class V4>
__device__ __forceinline__ void act_apply4(V4& v, int act) {
  switch (act) {
    case SHDR_ACT_RELU:
#pragma unroll
      for (int e = 0; e < 4; ++e) v[e] = fmaxf(v[e], 0.0f);
      break;
    case SHDR_ACT_LRELU:
#pragma unroll
      for (int e = 0; e < 4; ++e) v[e] = v[e] >= 0.0f ? v[e] : v[e] * 0.1f;
      break;
    case SHDR_ACT_TANH:
      if constexpr (TANH != 0) {
#pragma unroll
        for (int e = 0; e < 4; ++e) v[e] = TANH == 2 ? tanh_fast(v[e]) : tanhf(v[e]);
      }
      break;
    default:
      break;
  }
}

// The fused inference epilogue of the fp16 forward kernels (shdr_conv2d_fwd_fused_f16), applied after bias + act1:
//   v = act2(v * scale[co] + shift[co] + residual[pix * res_cstride + co])    (scale / shift / residual NULL -> skipped)
// Compiled only into the FUSED instantiations of conv_f16.hip, conv_f16_patch.hip and conv_f16_w3.hip: the training instantiations
// never see it.  Four consecutive couts co .. co + 3 of one output pixel; only the first nvalid of them exist (the 3-channel heads),
// and the residual is read only where res_ok (a pixel inside the output).
struct FusedEpiF16 {
  const float* scale;
  const float* shift;
  const void* res;         // fp32 or fp16 [N, Ho, Wo, res_cstride]
  int res_f32, res_cstride, act2;
};

template <int TANH, class V4>
__device__ __forceinline__ void fused_epi4_f16(V4& v, int co, size_t pix, int nvalid, bool res_ok, const FusedEpiF16& f) {
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    if (e >= nvalid) break;
    if (f.scale) v[e] *= f.scale[co + e];
    if (f.shift) v[e] += f.shift[co + e];
    if (f.res && res_ok) {
      const size_t i = pix * (size_t)f.res_cstride + (size_t)(co + e);
      v[e] += f.res_f32 ? static_cast<const float*>(f.res)[i] : (float)static_cast<const _Float16*>(f.res)[i];
    }
  }
  act_apply4<TANH>(v, f.act2);
}

}  // namespace shdr

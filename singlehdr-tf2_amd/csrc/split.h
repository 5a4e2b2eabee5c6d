// The contract of the split-operand ("x3") arithmetic, stated once for every kernel that keeps it (conv_x3.hip, conv_x3n.hip, up2_fused.hip,
// up2_lowres.hip, wgrad_x3.hip and the planner in conv_plan.hip; the tests' model is tests/conv_ref.py):
//   - a RANGE SLOT is a device word holding the bit pattern of an upper bound of max |x| of a tensor.  The input of a launch is multiplied
//     by 2^T, T = range_exponent(slot), and split into two fp16 planes (split4); the epilogue multiplies by 2^-T and writes max |y| into
//     the slot of the output (range_out);
//   - the filter is multiplied by 2^S (weight_scale) and split the same way; 2^-S lives in the packed filter's header.
// Every function here is force-inlined into its callers: a kernel's instruction stream does not depend on which file states the rule.
#pragma once
#include "shdr_internal.h"

// the prepare entries with `premax`: header slot kHdrMaxW already holds max |w| (written by the kernel that produced w: the input gradient's
// filter transform) -- no memset, no absmax launch
extern "C" int shdr_conv2d_x3_prepare_filter_premax_f32(const shdr_conv2d_desc* d, const float* w, float* prepared, int premax, void* stream);
extern "C" int shdr_conv2d_x3n_prepare_filter_premax_f32(const shdr_conv2d_desc* d, const float* w, float* prepared, int premax, void* stream);

namespace shdr {

// ---- the packed filter's header: 16 floats in front of the fp16 images (64 bytes keep the images 16-byte aligned) -------------------------
constexpr int kSplitHeaderFloats = 16;
constexpr int kHdrMaxW = 0;          // max |w| (bits)
constexpr int kHdrInvScale = 1;      // 2^-S
constexpr int kHdrInputRange = 2;    // the input's range slot of desc.prologue = SHDR_PROLOGUE_RANGE_SCALE (shdr_conv2d_x3_input_absmax_f32)

// ---- workspaces of the planned entry points ---------------------------------------------------------------------------------------------
inline size_t up256(size_t b) { return (b + 255) & ~(size_t)255; }
constexpr size_t kRangeScratch = 256;      // tail of a workspace: the slots of sources that arrive without a range

// ---- the input side ---------------------------------------------------------------------------------------------------------------------
// A bound, given by its bit pattern, is usable unless the slot is empty or zero, non-finite, or a word with the sign bit set (non-negative
// floats order like their bit patterns); without one the tensor is split as it stands.  T of a usable bound: 2^T brings it into
// [2^10, 2^11), clamped to +-126.
__device__ __forceinline__ bool range_bound_ok(unsigned b) { return b != 0u && b < 0x7f800000u; }
__device__ __forceinline__ int range_exponent_of(unsigned b) {
  int ex;
  frexpf(__uint_as_float(b), &ex);                             // bound in [2^(ex-1), 2^ex)
  const int T = 11 - ex;
  return T < -126 ? -126 : (T > 126 ? 126 : T);
}
// T of a slot; 0 for a null slot or one without a usable bound
__device__ __forceinline__ int range_exponent(const unsigned* slot) {
  const unsigned b = slot ? *slot : 0u;
  if (!range_bound_ok(b)) return 0;
  return range_exponent_of(b);
}
// 2^T and 2^-T for the larger of the two bounds (r2, or both, may be null); 1 without a usable bound
__device__ __forceinline__ void range_scale(const unsigned* r1, const unsigned* r2, float& xs, float& ixs) {
  xs = 1.0f;
  ixs = 1.0f;
  unsigned b = r1 ? *r1 : 0u;
  if (r2) {
    const unsigned b2 = *r2;
    b = b2 > b ? b2 : b;
  }
  if (range_bound_ok(b)) {
    const int T = range_exponent_of(b);
    xs = ldexpf(1.0f, T);
    ixs = ldexpf(1.0f, -T);
  }
}
// one float4 -> (fp16(v xs), fp16((v xs - fp16(v xs)) 2^11)) as two packed register pairs: v_fma_mixlo/hi_f16 multiply, round and pack in
// one instruction, v_fma_mix_f32 forms v xs - (float)h exactly (the product is exact, the difference representable): 12 vector
// instructions per float4 (the compiler's cast / convert / subtract / multiply / pack sequence: 19)
__device__ __forceinline__ void split4(const f32x4 v, float xs, unsigned (&h)[2], unsigned (&l)[2]) {
  const float k2048 = 2048.0f;
#pragma unroll
  for (int p = 0; p < 2; ++p) {
    float t0, t1;
    asm("v_fma_mixlo_f16 %0, %1, %2, 0" : "=v"(h[p]) : "v"(v[2 * p]), "s"(xs));
    asm("v_fma_mixhi_f16 %0, %1, %2, 0" : "+v"(h[p]) : "v"(v[2 * p + 1]), "s"(xs));
    asm("v_fma_mix_f32 %0, %1, %2, -%3 op_sel_hi:[0,0,1]" : "=v"(t0) : "v"(v[2 * p]), "s"(xs), "v"(h[p]));
    asm("v_fma_mix_f32 %0, %1, %2, -%3 op_sel:[0,0,1] op_sel_hi:[0,0,1]" : "=v"(t1) : "v"(v[2 * p + 1]), "s"(xs), "v"(h[p]));
    asm("v_fma_mixlo_f16 %0, %1, %2, 0" : "=v"(l[p]) : "v"(t0), "s"(k2048));
    asm("v_fma_mixhi_f16 %0, %1, %2, 0" : "+v"(l[p]) : "v"(t1), "s"(k2048));
  }
}

// ---- the output side --------------------------------------------------------------------------------------------------------------------
// max |y| of a block of NW waves (4 or 8) -> the range slot: the waves' maxima meet in NW LDS words of their own and ONE thread issues a
// no-return atomicMax, and only when the block's maximum exceeds what the slot already holds.  Atomics execute at the memory side, one
// after the other per address (measured ~4 ns each): one per WAVE cost the small layers of the U-Nets 15 - 35 us per launch, all of it
// in the first round of blocks, which finish together and all still see the slot empty.
// When the slot's old value is read is the caller's choice:
//   LATE = false  `seen` = the value loaded at the START of the epilogue: the load's round trip to the memory side runs under the output
//                 stores (the tiled kernels, one tile per block)
//   LATE = true   thread 0 loads it behind the barrier and `seen` is ignored (the persistent blocks, which all finish together)
template <int NW = 4, bool LATE = false>
__device__ __forceinline__ void range_out(unsigned* slot, float m, int lane, int wave, unsigned seen, unsigned* lds) {
  static_assert(NW == 4 || NW == 8, "blocks of four or eight waves");
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) m = fmaxf(m, __shfl_xor(m, off, 64));
  if (lane == 0) lds[wave] = __float_as_uint(m);
  asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");      // (not __syncthreads(): that would also sit out the output stores)
  if (threadIdx.x == 0) {
    const unsigned b01 = lds[0] > lds[1] ? lds[0] : lds[1], b23 = lds[2] > lds[3] ? lds[2] : lds[3];
    unsigned b = b01 > b23 ? b01 : b23;                        // non-negative floats order like their bit patterns
    if (NW == 8) {
      const unsigned b45 = lds[4] > lds[5] ? lds[4] : lds[5], b67 = lds[6] > lds[7] ? lds[6] : lds[7];
      const unsigned b47 = b45 > b67 ? b45 : b67;
      b = b47 > b ? b47 : b;
    }
#ifndef SHDR_ABL_NO_RANGE_ATOMIC
    if (LATE) seen = __hip_atomic_load(slot, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (b > seen) atomicMax(slot, b);
#endif
  }
}

// ---- the filter side --------------------------------------------------------------------------------------------------------------------
// 2^S of a pack kernel: S = 14 - ex brings max |w| max(1, |x2_scale|) (max |w| from the header, a zero filter counted as 1e-30) into
// [2^13, 2^14), clamped to +-100; inv = 2^-S, which thread 0 of the caller's block 0 writes to hdr[kHdrInvScale]
__device__ __forceinline__ float weight_scale(const float* hdr, float x2_scale, float& inv) {
  const float mx = fmaxf(__uint_as_float(reinterpret_cast<const unsigned*>(hdr)[kHdrMaxW]) * fmaxf(1.0f, fabsf(x2_scale)), 1e-30f);
  int ex;
  frexpf(mx, &ex);                                             // mx = f * 2^ex, f in [0.5, 1)
  int S = 14 - ex;
  S = S < -100 ? -100 : (S > 100 ? 100 : S);
  const float s = ldexpf(1.0f, S);
  inv = ldexpf(1.0f, -S);
  return s;
}
// max |w| of n floats -> *out (bits, atomicMax; the caller zeroes it): split_absmax_kernel of conv_x3.hip, for filters and the unaligned
// tail of shdr_absmax_f32
void launch_split_absmax(const float* w, long n, unsigned* out, hipStream_t st);

// ---- the stencil of the low-res up-sampling forms ---------------------------------------------------------------------------------------
// every product and sum of the stencil is one of these: explicit multiplies and fused multiply-adds, so the roundings of a pixel do not
// depend on how the compiler contracts or unrolls (the row walk of up2_lowres_stencil_kernel is unrolled by three and its copies must agree
// to the bit; up2_fused_kernel must agree with it)
__device__ __forceinline__ f32x4 mul4(f32x4 a, float s) {
  f32x4 r;
#pragma unroll
  for (int e = 0; e < 4; ++e) r[e] = __fmul_rn(a[e], s);
  return r;
}
__device__ __forceinline__ f32x4 fma4(f32x4 a, float s, f32x4 c) {
  f32x4 r;
#pragma unroll
  for (int e = 0; e < 4; ++e) r[e] = __builtin_fmaf(a[e], s, c[e]);
  return r;
}
__device__ __forceinline__ f32x4 fma4v(f32x4 a, f32x4 s, f32x4 c) {
  f32x4 r;
#pragma unroll
  for (int e = 0; e < 4; ++e) r[e] = __builtin_fmaf(a[e], s[e], c[e]);
  return r;
}

}  // namespace shdr

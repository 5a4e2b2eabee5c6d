// float32 bits -> IEEE half bits, round to nearest even, in integer arithmetic (the same on the host and on the device): subnormal
// halves, overflow to +-inf, NaN stays NaN with the top mantissa bits and the sign kept -- numpy's astype(float16), bit for bit.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define SHDR_HALF_HD __host__ __device__
#else
#define SHDR_HALF_HD
#endif

SHDR_HALF_HD inline uint16_t shdr_half_bits(uint32_t f) {
  const uint32_t sign = (f & 0x80000000u) >> 16;
  const uint32_t fexp = f & 0x7f800000u;
  if (fexp >= 0x47800000u) {                                     // 2^16 and above, inf, NaN
    if (fexp == 0x7f800000u && (f & 0x007fffffu) != 0) {
      uint32_t m = 0x7c00u + ((f & 0x007fffffu) >> 13);
      if (m == 0x7c00u) ++m;                                     // a NaN whose payload lies in the dropped bits stays a NaN
      return (uint16_t)(sign + m);
    }
    return (uint16_t)(sign + 0x7c00u);
  }
  if (fexp <= 0x38000000u) {                                     // below 2^-14: a subnormal half, or zero
    if (fexp < 0x33000000u) return (uint16_t)sign;               // below 2^-25: zero (2^-25 itself ties to even, zero, below)
    const uint32_t e = fexp >> 23;
    uint32_t sig = (0x00800000u + (f & 0x007fffffu)) >> (113 - e);
    // half-way and an even result: no increment, unless the shift dropped set bits (then it was above half-way)
    if ((sig & 0x00003fffu) != 0x00001000u || (f & 0x000007ffu)) sig += 0x00001000u;
    return (uint16_t)(sign + (sig >> 13));
  }
  uint32_t sig = f & 0x007fffffu;
  if ((sig & 0x00003fffu) != 0x00001000u) sig += 0x00001000u;
  return (uint16_t)(sign + ((fexp - 0x38000000u) >> 13) + (sig >> 13));   // a mantissa carry moves into the exponent, up to inf
}

// finite values beyond +-65504 -> +-65504 (inf and NaN pass)
SHDR_HALF_HD inline uint32_t shdr_half_saturate(uint32_t f) {
  const uint32_t mag = f & 0x7fffffffu;
  return (mag > 0x477fe000u && mag < 0x7f800000u) ? (f & 0x80000000u) | 0x477fe000u : f;
}

// OCP e4m3fn under one power-of-two scale: the scale rule (host and device, from the float's bits so
// that both agree exactly), the device conversion and the host's software encoder that defines it.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>

#include "mfma.h"

namespace rs {

constexpr int kE4m3MaxExp = 40;  // the clamp of a scale exponent: 2^-(e_u + e_i) stays a normal float

// the largest e with absmax 2^e <= 448 = 1.75 2^8, clamped; 0 for absmax = 0. absmax = m 2^x with
// m in [1, 2): e = 8 - x for m <= 1.75, else 7 - x (subnormals clamp to the upper end, inf / NaN to
// the lower)
__host__ __device__ inline int e4m3_exponent_bits(uint32_t bits) {
  bits &= 0x7fffffffu;
  if (bits == 0) return 0;
  const int x = (int)(bits >> 23) - 127;
  const int e = 8 - x - ((bits & 0x7fffffu) > 0x600000u ? 1 : 0);
  return e < -kE4m3MaxExp ? -kE4m3MaxExp : e > kE4m3MaxExp ? kE4m3MaxExp : e;
}

__device__ __forceinline__ int e4m3_exponent(float absmax) { return e4m3_exponent_bits(__float_as_uint(absmax)); }
// 2^e for |e| <= 126
__device__ __forceinline__ float e4m3_pow2(int e) { return __uint_as_float((uint32_t)(127 + e) << 23); }
// four floats (already scaled, |x| <= 448) to four e4m3 bytes, RNE, element 0 in the low byte
__device__ __forceinline__ uint32_t e4m3_pack4(const floatx4& x) {
  int w = __builtin_amdgcn_cvt_pk_fp8_f32(x[0], x[1], 0, false);
  w = __builtin_amdgcn_cvt_pk_fp8_f32(x[2], x[3], w, true);
  return (uint32_t)w;
}

// eight e4m3 bytes to the bf16 operand that holds the same values (exact: 4 significant bits)
// (v_cvt_scalef32_pk_bf16_fp8 at scale 1: two bytes an instruction)
__device__ __forceinline__ bf16x8 e4m3_to_bf16x8(long v) {
  typedef __bf16 bf16x2 __attribute__((ext_vector_type(2)));
  const uint32_t lo = (uint32_t)(unsigned long long)v, hi = (uint32_t)((unsigned long long)v >> 32);
  const bf16x2 a = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(lo, 1.0f, false);
  const bf16x2 b = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(lo, 1.0f, true);
  const bf16x2 c = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(hi, 1.0f, false);
  const bf16x2 d = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(hi, 1.0f, true);
  return bf16x8{a[0], a[1], b[0], b[1], c[0], c[1], d[0], d[1]};
}

// One float to its e4m3fn byte: sign, 4 exponent bits (bias 7), 3 mantissa bits; subnormals in
// steps of 2^-9 below 2^-6; round to nearest, ties to the even code; +-0 keep their sign; NaN, inf
// and everything that rounds past 448 give the NaN code 0x7f under the sign.
inline uint8_t e4m3_encode_one(float v) {
  uint32_t b;
  memcpy(&b, &v, 4);
  const uint8_t sign = (uint8_t)((b >> 24) & 0x80u);
  b &= 0x7fffffffu;
  if (b >= 0x43f00000u) return sign | 0x7f;  // |v| >= 480 (the first value past the 448 | 480 midpoint's reach), inf, NaN
  const int x = (int)(b >> 23) - 127;
  uint32_t code;
  if (x >= -6) {
    // normal: drop 20 mantissa bits with RNE; a carry runs into the exponent field as it should
    const uint32_t m = (b & 0x7fffffu) | ((uint32_t)(x + 7) << 23);  // biased for e4m3
    const uint32_t keep = m >> 20, rest = m & 0xfffffu;
    code = keep + ((rest > 0x80000u || (rest == 0x80000u && (keep & 1u))) ? 1u : 0u);
  } else if (x >= -10) {
    // subnormal: units of 2^-9; |v| = 1.f 2^x, the integer part of |v| 2^9 with RNE
    const uint32_t m = (b & 0x7fffffu) | 0x800000u;  // 24 bits, value m 2^(x - 23)
    const int sh = 23 - (x + 9);                     // |v| 2^9 = m >> sh, sh in 14 .. 24
    const uint32_t keep = m >> sh, rest = m & ((1u << sh) - 1u), half = 1u << (sh - 1);
    code = keep + ((rest > half || (rest == half && (keep & 1u))) ? 1u : 0u);
  } else {
    code = 0;  // below half of the smallest subnormal (2^-10 itself is a tie to the even code 0)
  }
  return sign | (uint8_t)code;
}

}  // namespace rs

// MFMA operand types and the fragment / storage helpers shared by the matrix kernels (device only).
#pragma once
#include <hip/hip_runtime.h>

namespace rs {

typedef float floatx4 __attribute__((ext_vector_type(4)));
typedef float floatx16 __attribute__((ext_vector_type(16)));
typedef __bf16 bf16x4 __attribute__((ext_vector_type(4)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef short shortx4 __attribute__((ext_vector_type(4)));
typedef short shortx8 __attribute__((ext_vector_type(8)));
typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));

// two fp32 quads rounded to one 8-element bf16 operand
__device__ __forceinline__ bf16x8 cvt8(const floatx4& lo, const floatx4& hi) {
  bf16x8 r;
  r[0] = (__bf16)lo[0]; r[1] = (__bf16)lo[1]; r[2] = (__bf16)lo[2]; r[3] = (__bf16)lo[3];
  r[4] = (__bf16)hi[0]; r[5] = (__bf16)hi[1]; r[6] = (__bf16)hi[2]; r[7] = (__bf16)hi[3];
  return r;
}

// ds_read_b64_tr_b16 from a row-major bf16 LDS image: 4 consecutive rows of one column per lane
// (EXEC must be full)
__device__ __forceinline__ shortx4 tr4(const __bf16* p) {
  typedef __attribute__((address_space(3))) shortx4* lptr;
  return __builtin_amdgcn_ds_read_tr16_b64_v4i16((lptr)(p));
}
// two of them joined into an 8-row operand
__device__ __forceinline__ bf16x8 tr_frag(const __bf16* lo, const __bf16* hi) {
  const shortx4 a = tr4(lo);
  const shortx4 b = tr4(hi);
  return __builtin_bit_cast(bf16x8, __builtin_shufflevector(a, b, 0, 1, 2, 3, 4, 5, 6, 7));
}

// four consecutive elements, fp32 or bf16 storage: one 16- or 8-byte access; fp32 -> bf16 rounds
// to nearest even, bf16 -> fp32 is exact
__device__ __forceinline__ void put4(float* p, const floatx4& v) { *reinterpret_cast<floatx4*>(p) = v; }
__device__ __forceinline__ void put4(__bf16* p, const floatx4& v) {
  bf16x4 h;
  h[0] = (__bf16)v[0]; h[1] = (__bf16)v[1]; h[2] = (__bf16)v[2]; h[3] = (__bf16)v[3];
  *reinterpret_cast<bf16x4*>(p) = h;
}
__device__ __forceinline__ floatx4 ld4(const float* p) { return *reinterpret_cast<const floatx4*>(p); }
__device__ __forceinline__ floatx4 ld4(const __bf16* p) {
  const bf16x4 h = *reinterpret_cast<const bf16x4*>(p);
  return floatx4{(float)h[0], (float)h[1], (float)h[2], (float)h[3]};
}

}  // namespace rs

// The fence-free hand-off of partial results to the workgroup that finishes last (device only).
//
// Producers store their partials and take a ticket; the workgroup whose ticket is the last one
// reads every partial and finishes the job in the same launch. No release / acquire fence is
// issued (an agent release writes back the whole L2, microseconds per workgroup). Instead, as
// MI355X_MICROARCH.md ("Valid forms", consumer conditions 1-4) requires, ALL of these hold:
//   1. every load of the handed-off bytes is an sc1 load (ld_sc1), never a plain one;
//   2. every one of those bytes was stored sc1 (st_sc1: write-through to memory);
//   3. every storing wave waits for its stores (s_waitcnt vmcnt(0)), and the one agent-scope add
//      per workgroup comes behind a workgroup barrier, so after the wait of every wave it signals for;
//   4. the shape is the measured one: a relaxed agent-scope counter add, the last adder consumes.
// A change to one of the four is a change to all users: tower.hip (BatchNorm statistics, weight
// gradient tiles: last_arriver), lookup.hip (segment-sum fix) and optim.hip (gradient norm), the
// last two with the ticket written out in their kernels.
#pragma once
#include <hip/hip_runtime.h>

namespace rs {

__device__ __forceinline__ float ld_sc1(const float* p) {
  return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ double ld_sc1(const double* p) {
  return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ int ld_sc1(const int* p) {
  return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ void st_sc1(float* p, float v) {
  __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ void st_sc1(double* p, double v) {
  __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ void st_sc1(int* p, int v) {
  __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// One ticket per workgroup: every thread's sc1 stores drained, the workgroup's barrier, one
// agent-scope add; returns true (uniformly) in the workgroup whose add came last.
__device__ __forceinline__ bool last_arriver(int* cnt, int last) {
  __shared__ int s_last;
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
  if (threadIdx.x == 0) {
    const int old = __hip_atomic_fetch_add(cnt, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    s_last = old == last;
  }
  __syncthreads();
  return s_last != 0;
}

}  // namespace rs

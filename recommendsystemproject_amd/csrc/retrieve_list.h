// The candidate-list pieces shared by the kernels that keep a user's K best scores while columns
// stream by in ascending order (retrieve.hip fused_topk_kernel, ivf.hip ivf_scan_kernel): the
// (order key, ~column) words, the "never held K" threshold, the rank-sort prune and the two K
// buckets. A list entry is one 64-bit word: the score's order key in the high half, the
// complement of its catalog column in the low half, so that a greater word is a better entry
// (value descending, then the lower column) and words of different columns are never equal.
#pragma once
#include "common.h"

namespace rs {

constexpr int kFtMaxK = 256;
constexpr int kFtSmallK = 32;  // K <= 32: lists of 80 (FtCfg KB = 0), K <= 256: lists of 352 (KB = 1)

// The threshold of a list that has never held K entries: NaN, so every score is admitted
// (!(s <= NaN)), -inf and NaN scores included.
constexpr uint32_t kFtNeverHeldK = 0x7fc00000u;

__device__ __forceinline__ uint32_t ft_order_key(float v) {
  const uint32_t u = __float_as_uint(v);
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);  // ascending uint order == ascending float
}
__device__ __forceinline__ float ft_key_value(uint32_t k) {
  const uint32_t u = (k & 0x80000000u) ? (k & 0x7fffffffu) : ~k;
  return __uint_as_float(u);
}

__device__ __forceinline__ unsigned long long ft_word(float s, int col) {
  return ((unsigned long long)ft_order_key(s) << 32) | (uint32_t)~col;
}
__device__ __forceinline__ int ft_word_col(unsigned long long w) { return (int32_t)~(uint32_t)w; }
__device__ __forceinline__ float ft_word_value(unsigned long long w) { return ft_key_value((uint32_t)(w >> 32)); }

// the best K of list L (n entries) to L[0 .. K), sorted descending; thr = value of the K-th
template <int CAP>
__device__ __forceinline__ void ft_prune_row(unsigned long long* L, int* cnt, float* thr, int K, int lane) {
  constexpr int J = (CAP + 63) / 64;
  const int n = min(__builtin_amdgcn_readfirstlane(*cnt), CAP);
  unsigned long long own[J];
  int rank[J];
#pragma unroll
  for (int j = 0; j < J; ++j) {
    const int i = lane + 64 * j;
    own[j] = i < n ? L[i] : 0ull;
    rank[j] = 0;
  }
  // unrolled: the broadcast reads of a batch are in flight together (one exposed LDS round trip
  // per entry otherwise)
#pragma unroll 8
  for (int q = 0; q < n; ++q) {
    const unsigned long long v = L[q];  // broadcast read
#pragma unroll
    for (int j = 0; j < J; ++j) rank[j] += v > own[j] ? 1 : 0;
  }
  __builtin_amdgcn_wave_barrier();  // every read of the old list before the first write
#pragma unroll
  for (int j = 0; j < J; ++j) {
    const int i = lane + 64 * j;
    if (i < n && rank[j] < K) {
      L[rank[j]] = own[j];
      if (rank[j] == K - 1) *thr = ft_key_value((uint32_t)(own[j] >> 32));
    }
  }
  if (lane == 0) *cnt = min(n, K);
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
}

}  // namespace rs

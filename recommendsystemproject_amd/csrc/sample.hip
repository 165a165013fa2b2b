// Hard negatives mined from the item index (rs_sample_negatives): for every user, n catalog columns
// drawn uniformly without replacement from a window of ranks of the model's own ordering, on the
// device. The ordering is the fused sweep's (retrieve.hip: rs_fused_topk and its e4m3 / filtered
// forms give the first C entries, value descending, ties by the lower column, history and filter
// columns at -inf); this file only turns those C candidates into the sample.
//
// Definition, per user b with candidates (col_j, val_j), j = 0 .. C - 1:
//   eligible   val_j > -inf, 0 <= col_j < N, item_ids[col_j] != pos_ids[b] (the test is on the item
//              id: every column that holds the positive's id is out);
//   e_0 < e_1 < .. < e_{E-1}   the eligible positions, in candidate order;
//   pool       hi = min(skip + window, E), lo = min(skip, max(hi - n, 0)): e_lo .. e_{hi-1}, P = hi - lo
//              members (the window slides towards the top only as far as needed to hold n);
//   draw       a pool member's key is (h << 32) | col, h = fmix32(col ^ k0) ^ k1 with (k0, k1) the
//              halves of mix64(seed ^ mix64(draw * 0x9e3779b97f4a7c15 + b * 0xd1b54a32d192ed03))
//              (rng.h): distinct keys, so a total order; the output is the n members with the
//              smallest keys in ascending key order. A pure function of its arguments.
//   short      0 < P < n: all P in key order, repeated cyclically up to n, count = P; P = 0: ids and
//              columns -1, count = 0; otherwise count = n.
//
// Kernel: one wave per user, four users per 256-thread block. Lane l holds candidate positions
// l, l + 64, l + 128 and l + 192; eligible positions are numbered with a ballot and popcount
// prefixes over the four passes, E / lo / hi are wave-uniform, and the keys (all-ones outside the
// pool) are rank-sorted through 2 KiB of wave-private LDS as ft_prune_row sorts a candidate list:
// every lane counts the keys below each of its own with broadcast reads. A member of rank r writes
// the output slots r, r + P, .. < n. No atomics, no workspace, no block barrier (the waves of a
// block never meet).
#include "common.h"
#include "rng.h"

namespace rs {
namespace {

constexpr int kSnMaxC = 256;   // candidates a user (the sweep's largest K)
constexpr int kSnUsers = 4;    // users (waves) a block
constexpr int kSnPass = kSnMaxC / kWave;

struct SnArgs {
  const int32_t* cand_idx;
  const float* cand_val;
  int64_t ld_cand;
  int B, C;
  const int64_t* item_ids;
  int N;
  const int64_t* pos_ids;  // null: no positive exclusion
  int64_t pos_stride;
  int skip, window, n;
  uint64_t seed, draw;
  int64_t* out_ids;
  int32_t* out_cols;
  int64_t ld_out;
  int32_t* out_count;
};

__global__ __launch_bounds__(kSnUsers * kWave) void sample_negatives_kernel(SnArgs a) {
  __shared__ unsigned long long s_keys[kSnUsers][kSnMaxC];
  const int lane = threadIdx.x & (kWave - 1);
  const int wave = threadIdx.x / kWave;
  const int b = blockIdx.x * kSnUsers + wave;
  if (b >= a.B) return;  // wave-uniform
  unsigned long long* L = s_keys[wave];

  const int64_t pos_id = a.pos_ids ? a.pos_ids[(int64_t)b * a.pos_stride] : 0;
  int col[kSnPass];
  int64_t id[kSnPass];
  bool elig[kSnPass];
#pragma unroll
  for (int j = 0; j < kSnPass; ++j) {
    const int i = lane + kWave * j;
    const bool have = i < a.C;
    col[j] = have ? a.cand_idx[(int64_t)b * a.ld_cand + i] : -1;
    const float v = have ? a.cand_val[(int64_t)b * a.ld_cand + i] : -INFINITY;
    elig[j] = v > -INFINITY && col[j] >= 0 && col[j] < a.N;
    id[j] = elig[j] ? a.item_ids[col[j]] : -1;
    if (a.pos_ids && id[j] == pos_id) elig[j] = false;
  }

  // the eligible candidates' positions among the eligible, in candidate order
  int epos[kSnPass];
  int E = 0;
  const unsigned long long below = (1ull << lane) - 1ull;
#pragma unroll
  for (int j = 0; j < kSnPass; ++j) {
    const unsigned long long m = __ballot(elig[j]);
    epos[j] = E + __popcll(m & below);
    E += __popcll(m);
  }
  const int hi = min(a.skip + a.window, E);
  const int lo = min(a.skip, max(hi - a.n, 0));
  const int P = hi - lo;

  const uint64_t base = mix64(a.seed ^ mix64(a.draw * 0x9e3779b97f4a7c15ULL + (uint64_t)b * 0xd1b54a32d192ed03ULL));
  const uint32_t k0 = (uint32_t)base, k1 = (uint32_t)(base >> 32);
  unsigned long long own[kSnPass];
  int rank[kSnPass];
#pragma unroll
  for (int j = 0; j < kSnPass; ++j) {
    const bool in_pool = elig[j] && epos[j] >= lo && epos[j] < hi;
    const uint32_t h = fmix32((uint32_t)col[j] ^ k0) ^ k1;
    own[j] = in_pool ? ((unsigned long long)h << 32) | (uint32_t)col[j] : ~0ull;  // col < 2^31: never all-ones
    L[lane + kWave * j] = own[j];
    rank[j] = 0;
  }
  __builtin_amdgcn_wave_barrier();  // every key written before the first broadcast read
  __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
#pragma unroll 8
  for (int q = 0; q < a.C; ++q) {
    const unsigned long long v = L[q];  // broadcast read
#pragma unroll
    for (int j = 0; j < kSnPass; ++j) rank[j] += v < own[j] ? 1 : 0;
  }

  int64_t* oid = a.out_ids + (int64_t)b * a.ld_out;
  int32_t* ocol = a.out_cols + (int64_t)b * a.ld_out;
  if (P == 0) {
    for (int t = lane; t < a.n; t += kWave) {
      oid[t] = -1;
      ocol[t] = -1;
    }
  } else {
#pragma unroll
    for (int j = 0; j < kSnPass; ++j) {
      if (own[j] == ~0ull) continue;  // outside the pool
      for (int t = rank[j]; t < a.n; t += P) {  // rank < P; the cyclic fill of a short pool
        oid[t] = id[j];
        ocol[t] = col[j];
      }
    }
  }
  if (lane == 0) a.out_count[b] = min(P, a.n);
}

}  // namespace
}  // namespace rs

using namespace rs;

extern "C" int rs_sample_negatives(const int32_t* cand_idx, const float* cand_val, int64_t ld_cand, int B, int C,
                                   const int64_t* item_ids, int64_t N, const int64_t* pos_ids, int64_t pos_stride,
                                   int skip, int window, int n, uint64_t seed, uint64_t draw, int64_t* out_ids,
                                   int32_t* out_cols, int64_t ld_out, int32_t* out_count, void* stream) {
  RS_CHECK_ARG(cand_idx && cand_val && item_ids && out_ids && out_cols && out_count,
               "rs_sample_negatives: null cand_idx / cand_val / item_ids / out_ids / out_cols / out_count");
  RS_CHECK_ARG(B >= 0 && N >= 1 && N < (int64_t)1 << 31,
               "rs_sample_negatives: bad sizes (B=%d N=%lld; B >= 0, 1 <= N < 2^31)", B, (long long)N);
  RS_CHECK_ARG(C >= 1 && C <= kSnMaxC, "rs_sample_negatives: C = %d outside [1, 256]", C);
  RS_CHECK_ARG(skip >= 0, "rs_sample_negatives: skip = %d < 0", skip);
  RS_CHECK_ARG(n >= 1 && n <= window, "rs_sample_negatives: n = %d outside [1, window = %d]", n, window);
  RS_CHECK_ARG((int64_t)skip + window <= 255, "rs_sample_negatives: skip + window = %lld > 255",
               (long long)skip + window);
  RS_CHECK_ARG(ld_cand >= C, "rs_sample_negatives: ld_cand = %lld < C = %d", (long long)ld_cand, C);
  RS_CHECK_ARG(ld_out >= n, "rs_sample_negatives: ld_out = %lld < n = %d", (long long)ld_out, n);
  if (B == 0) return 0;
  SnArgs a;
  a.cand_idx = cand_idx; a.cand_val = cand_val; a.ld_cand = ld_cand; a.B = B; a.C = C;
  a.item_ids = item_ids; a.N = (int)N; a.pos_ids = pos_ids; a.pos_stride = pos_stride;
  a.skip = skip; a.window = window; a.n = n; a.seed = seed; a.draw = draw;
  a.out_ids = out_ids; a.out_cols = out_cols; a.ld_out = ld_out; a.out_count = out_count;
  sample_negatives_kernel<<<cdiv(B, kSnUsers), kSnUsers * kWave, 0, as_stream(stream)>>>(a);
  RS_CHECK_LAUNCH("rs_sample_negatives");
  return 0;
}

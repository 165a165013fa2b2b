// Fused top-K retrieval over an item index (serving, and validate(retrieval='fused')): the K best
// catalog columns of every user by dot product, with their scores, without the [B, N] score matrix
// of the staged pipeline (rs_gemm_f32 -> rs_mask_history -> rs_topk_rows per column chunk,
// retrieval.hip). Same result: value descending, ties by the lower column, history columns -inf.
//
// Grid: row tiles x column splits, the row tiles of one split adjacent in dispatch order so that
// their item reads meet in L2. A wave owns 32 users as the B operands of 32 x 32 MFMA tiles
// (registers) and streams the split's columns in ascending order through a double-buffered LDS
// tile shared by the workgroup, with up to two more tiles in flight in registers; a lane then
// holds 16 scores of ONE user (column = lane & 31 of the accumulator tile), so the user's running
// threshold is a register.
//
// Candidate lists (LDS, one per user, wave-private): a score is admitted while the list has never
// held K entries, afterwards only if it is strictly greater than the threshold (the K-th best at
// the last prune). The threshold moves between 32-column blocks only, and columns arrive in
// ascending order, so a later equal score always has the higher column and is rightly dropped.
// A list that could overflow in the next block (more than CAP - 32 entries) is pruned to its best
// K by a rank sort of (order key, ~column) words: distinct words, so the order is total. History
// exclusion is a binary search of the column in the user's sorted CSR slice, on admission only.
// Each split writes its K candidates (sorted) split-major into a workspace; rs_topk_rows merges
// them (ties by candidate position = column order). K <= 32: 4 waves x 32 users per workgroup,
// lists of 80; K <= 256: one wave of 32 users, lists of 352 (rows x capacity x 8 B beside the item
// tiles in 160 KiB).
#include <type_traits>

#include "common.h"
#include "mfma.h"

namespace rs {
namespace {

constexpr int kFtMaxK = 256;
constexpr int kFtSmallK = 32;

__device__ __forceinline__ uint32_t ft_order_key(float v) {
  const uint32_t u = __float_as_uint(v);
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);  // ascending uint order == ascending float
}
__device__ __forceinline__ float ft_key_value(uint32_t k) {
  const uint32_t u = (k & 0x80000000u) ? (k & 0x7fffffffu) : ~k;
  return __uint_as_float(u);
}

// DP: the embedding width the registers and LDS are sized for (D <= DP); KB: the K bucket
template <int DP, bool F32, int KB>
struct FtCfg {
  static constexpr int NW = KB == 0 ? 4 : 1;        // waves per workgroup
  static constexpr int NT = 64 * NW;
  static constexpr int ROWS = 32 * NW;              // users per workgroup
  static constexpr int CAP = KB == 0 ? 80 : 352;    // list capacity: K + 32 <= CAP - 16
  static constexpr int ESZ = F32 ? 4 : 2;
  static constexpr int PTMAX = F32 ? DP + 4 : DP + 8;  // LDS row pitch (elements) at D = DP
  // items per tile: two LDS buffers within 72 KB (one wave stages at most 64 rows)
  static constexpr int TI = (KB == 0 && 2 * 128 * PTMAX * ESZ <= 72 * 1024) ? 128
                            : (2 * 64 * PTMAX * ESZ <= 72 * 1024) ? 64 : 32;
  static constexpr int NB = TI / 32;                // 32-item blocks per tile
  static constexpr int CPR = DP * ESZ / 16;         // 16-byte chunks per item row at D = DP
  static constexpr int SL = TI * CPR / NT;          // staged chunks per thread and tile
  // tiles in flight in registers beyond the one in LDS (up to 64 staging VGPRs): with one, a
  // workgroup per CU kept 16-32 KB in flight and the kernel ran at the load latency
  static constexpr int DEPTH = SL <= 8 ? 2 : 1;
  static_assert(TI * CPR % NT == 0, "whole chunks per thread");
};

struct FtArgs {
  const float* U;
  int64_t ldu;
  int B;
  const void* items;
  int64_t ldi;
  int N, D, K;
  const int64_t* user_ids;
  int64_t uid_stride;
  const int64_t* hist_off;
  const int32_t* hist_idx;
  int64_t num_users;
  int splits, split_cols, nrt;
  int32_t* out_idx;  // [B][ld_out], this split's candidates at split * K
  float* out_val;    // nullable
  int64_t ld_out;
};

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

template <int DP, bool F32, int KB>
__global__ __launch_bounds__((FtCfg<DP, F32, KB>::NT)) void fused_topk_kernel(FtArgs a) {
  using Cfg = FtCfg<DP, F32, KB>;
  using E = std::conditional_t<F32, float, __bf16>;
  constexpr int NT = Cfg::NT, ROWS = Cfg::ROWS, CAP = Cfg::CAP, TI = Cfg::TI, NB = Cfg::NB;
  constexpr int CPR = Cfg::CPR, SL = Cfg::SL, ESZ = Cfg::ESZ;
  __shared__ __attribute__((aligned(16))) E tiles[2][TI * Cfg::PTMAX];
  __shared__ unsigned long long lists[ROWS * CAP];
  __shared__ int s_cnt[ROWS];
  __shared__ float s_thr[ROWS];

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int c = lane & 31, h = lane >> 5;
  const int rt = blockIdx.x % a.nrt, split = blockIdx.x / a.nrt;
  const int D = a.D, K = a.K;
  const int PT = F32 ? D + 4 : D + 8;
  const int lrow = wave * 32 + c;  // this lane's user: list row and, + rt * ROWS, batch row
  const int o = rt * ROWS + lrow;
  const bool o_ok = o < a.B;
  const int c_begin = split * a.split_cols;
  const int c_end = split == a.splits - 1 ? a.N : c_begin + a.split_cols;
  const int ntiles = (c_end - c_begin + TI - 1) / TI;

  // NaN threshold: "never held K entries", every score is admitted (!(s <= NaN)); rows past B
  // admit nothing
  if (h == 0) {
    s_cnt[lrow] = 0;
    s_thr[lrow] = o_ok ? __uint_as_float(0x7fc00000u) : INFINITY;
  }
  float thr = o_ok ? __uint_as_float(0x7fc00000u) : INFINITY;

  int64_t h_lo = 0, h_hi = 0;  // the user's CSR slice (sorted ascending)
  if (o_ok && a.user_ids && a.hist_off && a.hist_idx) {
    const int64_t uid = a.user_ids[(int64_t)o * a.uid_stride];
    if (uid >= 0 && uid < a.num_users) {
      h_lo = a.hist_off[uid];
      h_hi = a.hist_off[uid + 1];
    }
  }

  // user fragments (B operand). bf16: lane (c, h) holds U[o][16 s + 8 h .. + 7] of k-step s;
  // fp32: U[o][h D/2 + s] (k-step s pairs embedding columns s and D/2 + s)
  bf16x8 ub[F32 ? 1 : DP / 16];
  float uf[F32 ? DP / 2 : 1];
  if constexpr (F32) {
#pragma unroll
    for (int s4 = 0; s4 < DP / 8; ++s4) {
      floatx4 x = {0.f, 0.f, 0.f, 0.f};
      if (o_ok && 8 * s4 < D) x = ld4(a.U + (int64_t)o * a.ldu + h * (D / 2) + 4 * s4);
#pragma unroll
      for (int j = 0; j < 4; ++j) uf[4 * s4 + j] = x[j];
    }
  } else {
#pragma unroll
    for (int s = 0; s < DP / 16; ++s) {
      floatx4 x0 = {0.f, 0.f, 0.f, 0.f}, x1 = x0;
      if (o_ok && 16 * s < D) {
        const float* p = a.U + (int64_t)o * a.ldu + 16 * s + 8 * h;
        x0 = ld4(p);
        x1 = ld4(p + 4);
      }
      ub[s] = cvt8(x0, x1);
    }
  }

  // staging: chunk `slot` = 16 bytes `ch` of tile row `row` (the mapping of D = DP; a chunk past
  // the row's end repeats its last one: same bytes to the same LDS address). Loads are
  // unconditional, rows clamped to N - 1 (columns past c_end are masked where consumed).
  constexpr int DEPTH = Cfg::DEPTH;
  u32x4 st[DEPTH][SL];
  const int cpr = D * ESZ / 16;
  auto load_tile = [&](u32x4 (&r)[SL], int t) {
    const int64_t c0 = (int64_t)c_begin + (int64_t)t * TI;
#pragma unroll
    for (int i = 0; i < SL; ++i) {
      const int slot = tid + NT * i;
      const int row = slot / CPR, ch = min(slot % CPR, cpr - 1);
      const int64_t g = min(c0 + row, (int64_t)a.N - 1);
      r[i] = *reinterpret_cast<const u32x4*>(reinterpret_cast<const char*>(a.items) + g * a.ldi * ESZ + ch * 16);
    }
  };
  auto store_tile = [&](const u32x4 (&r)[SL], int buf) {
#pragma unroll
    for (int i = 0; i < SL; ++i) {
      const int slot = tid + NT * i;
      const int row = slot / CPR, ch = min(slot % CPR, cpr - 1);
      *reinterpret_cast<u32x4*>(reinterpret_cast<char*>(tiles[buf]) + row * PT * ESZ + ch * 16) = r[i];
    }
  };

  // one 32-item block's scores: element e = column colbase + 8 (e >> 2) + 4 h + (e & 3), user c
  auto admit_block = [&](const floatx16& acc, int colbase) {
#pragma unroll
    for (int e = 0; e < 16; ++e) {
      const int col = colbase + 8 * (e >> 2) + 4 * h + (e & 3);
      float s = acc[e];
      const bool cand = col < c_end && !(s <= thr);
      if (__any(cand)) {
        if (cand) {
          int64_t lo = h_lo, hi = h_hi;
          while (lo < hi) {
            const int64_t mid = (lo + hi) >> 1;
            if (a.hist_idx[mid] < col) lo = mid + 1; else hi = mid;
          }
          if (lo < h_hi && a.hist_idx[lo] == col) s = -INFINITY;
          if (!(s <= thr)) {
            const int slot = atomicAdd(&s_cnt[lrow], 1);
            if (slot < CAP)
              lists[lrow * CAP + slot] = ((unsigned long long)ft_order_key(s) << 32) | (uint32_t)~col;
          }
        }
      }
    }
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    const int n = s_cnt[lrow];
    unsigned long long need = __ballot(h == 0 && n > CAP - 32);
    while (need) {
      const int r = wave * 32 + __ffsll((long long)need) - 1;
      ft_prune_row<CAP>(&lists[r * CAP], &s_cnt[r], &s_thr[r], K, lane);
      need &= need - 1;
    }
    thr = s_thr[lrow];
  };

  auto compute_tile = [&](int t) {
    const E* T = tiles[t & 1];
    floatx16 acc[NB];
#pragma unroll
    for (int ib = 0; ib < NB; ++ib)
#pragma unroll
      for (int e = 0; e < 16; ++e) acc[ib][e] = 0.f;
    if constexpr (F32) {
#pragma unroll
      for (int s4 = 0; s4 < DP / 8; ++s4) {
        if (8 * s4 < D) {
#pragma unroll
          for (int ib = 0; ib < NB; ++ib) {
            const floatx4 a4 = ld4(reinterpret_cast<const float*>(T) + (ib * 32 + c) * PT + h * (D / 2) + 4 * s4);
#pragma unroll
            for (int j = 0; j < 4; ++j)
              acc[ib] = __builtin_amdgcn_mfma_f32_32x32x2f32(a4[j], uf[4 * s4 + j], acc[ib], 0, 0, 0);
          }
        }
      }
    } else {
#pragma unroll
      for (int s = 0; s < DP / 16; ++s) {
        if (16 * s < D) {
#pragma unroll
          for (int ib = 0; ib < NB; ++ib) {
            const bf16x8 af = *reinterpret_cast<const bf16x8*>(reinterpret_cast<const __bf16*>(T) +
                                                               (ib * 32 + c) * PT + 16 * s + 8 * h);
            acc[ib] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(af, ub[s], acc[ib], 0, 0, 0);
          }
        }
      }
    }
#pragma unroll
    for (int ib = 0; ib < NB; ++ib) {
      float m = acc[ib][0];
#pragma unroll
      for (int e = 1; e < 16; ++e) m = fmaxf(m, acc[ib][e]);
      if (__any(!(m <= thr))) admit_block(acc[ib], c_begin + t * TI + ib * 32);
    }
  };

  // tile t is consumed from LDS buffer t & 1 while stage t % DEPTH holds tile t + 1 (stored to the
  // other buffer after the compute) and the other stages the tiles after it; tiles past the
  // split's end are clamped reads that nobody consumes
  load_tile(st[0], 0);
  store_tile(st[0], 0);
#pragma unroll
  for (int d = 0; d < DEPTH; ++d) load_tile(st[d], 1 + d);
  __syncthreads();
  for (int t0 = 0; t0 < ntiles; t0 += DEPTH) {
#pragma unroll
    for (int d = 0; d < DEPTH; ++d) {
      const int t = t0 + d;
      if (t < ntiles) {
        compute_tile(t);
        store_tile(st[d], (t + 1) & 1);
        load_tile(st[d], t + 1 + DEPTH);
        __syncthreads();
      }
    }
  }

  // this split's K candidates per user, sorted (value descending, column ascending)
  for (int r = 0; r < 32; ++r) {
    const int lr = wave * 32 + r;
    const int64_t orow = (int64_t)rt * ROWS + lr;
    if (orow >= a.B) break;
    ft_prune_row<CAP>(&lists[lr * CAP], &s_cnt[lr], &s_thr[lr], K, lane);
    for (int i = lane; i < K; i += 64) {
      const unsigned long long v = lists[lr * CAP + i];
      const int64_t p = orow * a.ld_out + (int64_t)split * K + i;
      a.out_idx[p] = (int32_t)~(uint32_t)v;
      if (a.out_val) a.out_val[p] = ft_key_value((uint32_t)(v >> 32));
    }
  }
}

// one wave per candidate: out[b, j] = U[b] . items[cand[b, j]]
__global__ __launch_bounds__(256) void rescore_kernel(const float* __restrict__ U, int64_t ldu, int B,
                                                      const float* __restrict__ items, int64_t ldi, int64_t N,
                                                      int D, const int32_t* __restrict__ cand,
                                                      const float* __restrict__ cand_val, int C, int64_t ld_cand,
                                                      float* __restrict__ out, int64_t ld_out) {
  const int lane = threadIdx.x & 63;
  const int64_t w = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (w >= (int64_t)B * C) return;
  const int64_t b = w / C;
  const int j = (int)(w % C);
  const int64_t col = cand[b * ld_cand + j];
  float r;
  if (cand_val && cand_val[b * ld_cand + j] == -INFINITY) {
    r = -INFINITY;  // an excluded candidate stays excluded
  } else if (col < 0 || col >= N) {
    r = __uint_as_float(0x7fc00000u);  // bad column: never read, flagged in the value
  } else {
    float s = 0.f;
    for (int d = lane; d < D; d += 64) s += U[b * ldu + d] * items[col * ldi + d];
    r = wave_sum(s);
  }
  if (lane == 0) out[b * ld_out + j] = r;
}

inline int ft_rows(int K) { return K <= kFtSmallK ? 128 : 32; }

template <int DP, bool F32>
int ft_launch_k(const FtArgs& a, int grid, hipStream_t st) {
  if (a.K <= kFtSmallK)
    fused_topk_kernel<DP, F32, 0><<<grid, FtCfg<DP, F32, 0>::NT, 0, st>>>(a);
  else
    fused_topk_kernel<DP, F32, 1><<<grid, FtCfg<DP, F32, 1>::NT, 0, st>>>(a);
  RS_CHECK_LAUNCH("rs_fused_topk");
  return 0;
}

template <bool F32>
int ft_launch(const FtArgs& a, int grid, hipStream_t st) {
  if (a.D <= 64) return ft_launch_k<64, F32>(a, grid, st);
  if (a.D <= 128) return ft_launch_k<128, F32>(a, grid, st);
  return ft_launch_k<256, F32>(a, grid, st);
}

}  // namespace
}  // namespace rs

using namespace rs;

extern "C" int rs_fused_topk_splits(int B, int64_t N, int D, int K) {
  (void)D;
  if (B < 1 || N < 1 || K < 1 || K > N) return 1;
  // one round of workgroups over the 256 CUs (every workgroup has the same work, and each split
  // pays its lists' warm-up: K ln(columns / K) admissions per user); a split keeps at least
  // max(K, 2048) columns and N / splits >= K (no padding candidate)
  const int64_t want = cdiv(256, cdiv(B, ft_rows(K)));
  const int64_t most = N / (K > 2048 ? K : 2048);
  int64_t s = want < most ? want : most;
  if (s > 1024) s = 1024;
  return s < 1 ? 1 : (int)s;
}

extern "C" int64_t rs_fused_topk_ws_bytes(int B, int64_t N, int D, int K, int splits) {
  if (splits <= 0) splits = rs_fused_topk_splits(B, N, D, K);
  if (B < 1 || K < 1) return 16;
  return (int64_t)B * splits * K * 8;  // values fp32 + columns int32, [B][splits * K] each
}

extern "C" int rs_fused_topk(const float* U, int64_t ldu, int B, const void* items, int items_bf16,
                             int64_t ldi, int64_t N, int D, int K, const int64_t* user_ids,
                             int64_t uid_stride, const int64_t* hist_off, const int32_t* hist_idx,
                             int64_t num_users, int splits, void* ws, int64_t ws_bytes, int32_t* out_idx,
                             float* out_val, int64_t ld_out, void* stream) {
  RS_CHECK_ARG(U && items && out_idx && B >= 0, "rs_fused_topk: null U / items / out_idx or B < 0");
  RS_CHECK_ARG(D >= 16 && D <= 256 && D % 16 == 0,
               "rs_fused_topk: D = %d, must be a multiple of 16 in [16, 256]", D);
  RS_CHECK_ARG(K >= 1 && K <= kFtMaxK && N >= 1 && N < (int64_t)1 << 31 && K <= N,
               "rs_fused_topk: bad sizes (N=%lld K=%d; K <= min(N, 256), N < 2^31)", (long long)N, K);
  RS_CHECK_ARG(ldu >= D && ldu % 4 == 0 && ldi >= D && ldi % (items_bf16 ? 8 : 4) == 0 && aligned16(U) &&
                   aligned16(items) && ld_out >= K,
               "rs_fused_topk: rows of U and items must be 16-byte aligned, ld >= D, ld_out >= K");
  if (splits <= 0) splits = rs_fused_topk_splits(B, N, D, K);
  RS_CHECK_ARG(N / splits >= K, "rs_fused_topk: splits = %d leaves a split fewer than K = %d columns", splits,
               K);
  const int64_t need = splits > 1 ? rs_fused_topk_ws_bytes(B, N, D, K, splits) : 0;
  RS_CHECK_ARG(splits == 1 || (ws && ws_bytes >= need),
               "rs_fused_topk: workspace of %lld bytes, needs %lld (rs_fused_topk_ws_bytes)",
               (long long)ws_bytes, (long long)need);
  if (B == 0) return 0;
  FtArgs a;
  a.U = U; a.ldu = ldu; a.B = B;
  a.items = items; a.ldi = ldi; a.N = (int)N; a.D = D; a.K = K;
  a.user_ids = user_ids; a.uid_stride = uid_stride; a.hist_off = hist_off; a.hist_idx = hist_idx;
  a.num_users = num_users;
  a.splits = splits; a.split_cols = (int)(N / splits); a.nrt = cdiv(B, ft_rows(K));
  const int64_t ldw = (int64_t)splits * K;
  float* ws_val = static_cast<float*>(ws);
  int32_t* ws_idx = reinterpret_cast<int32_t*>(ws_val + (int64_t)B * ldw);
  if (splits == 1) {
    a.out_idx = out_idx; a.out_val = out_val; a.ld_out = ld_out;
  } else {
    a.out_idx = ws_idx; a.out_val = ws_val; a.ld_out = ldw;
  }
  const int64_t grid = (int64_t)a.nrt * splits;
  RS_CHECK_ARG(grid < (int64_t)1 << 31, "rs_fused_topk: grid too large");
  RS_RET_IF(items_bf16 ? ft_launch<false>(a, (int)grid, as_stream(stream))
                       : ft_launch<true>(a, (int)grid, as_stream(stream)));
  if (splits == 1) return 0;
  // split-major candidates, sorted within a split: position order == column order among equal values
  return rs_topk_rows(ws_val, ldw, B, (int)ldw, K, ws_idx, ldw, 0, out_idx, out_val, ld_out, stream);
}

extern "C" int rs_rescore_rows(const float* U, int64_t ldu, int B, const float* items, int64_t ldi, int64_t N,
                               int D, const int32_t* cand, const float* cand_val, int C, int64_t ld_cand,
                               float* out_val, int64_t ld_out, void* stream) {
  RS_CHECK_ARG(U && items && cand && out_val && B >= 0 && N >= 1 && D >= 1 && C >= 1 && ldu >= D && ldi >= D &&
                   ld_cand >= C && ld_out >= C,
               "rs_rescore_rows: bad args (B=%d N=%lld D=%d C=%d)", B, (long long)N, D, C);
  if (B == 0) return 0;
  const int64_t blocks = ((int64_t)B * C + 3) / 4;
  RS_CHECK_ARG(blocks < (int64_t)1 << 31, "rs_rescore_rows: too many candidates");
  rescore_kernel<<<(int)blocks, 256, 0, as_stream(stream)>>>(U, ldu, B, items, ldi, N, D, cand, cand_val, C,
                                                             ld_cand, out_val, ld_out);
  RS_CHECK_LAUNCH("rs_rescore_rows");
  return 0;
}

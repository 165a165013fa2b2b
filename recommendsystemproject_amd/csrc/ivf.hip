// Cluster-pruned (IVF) retrieval: the exhaustive search of retrieve.hip restricted, per user, to
// the catalog columns of the lists that user probes.
//
// Definition. A catalog of N columns, an assignment assign[c] in [0, nlist) of every column to a
// list, and for user b the nprobe lists probe[b, :] (distinct; the caller takes them as
// rs_fused_topk of the users against the centroids). The result is the first K entries of
// rs_fused_topk_filtered's order -- masked score descending, ties by the LOWER CATALOG COLUMN, the
// user's history and the columns outside the user's filter at -inf -- taken over the columns c
// with assign[c] in probe[b, :], and only the entries whose masked score is above -inf. If fewer
// than K exist the rest is (column -1, score -inf). Unlike the exhaustive search a masked column
// is never returned. With nprobe == nlist and no filler it is the exhaustive result, bit for bit:
// a score formed through ft_mfma has the same bits for the same (user, item row) whatever else
// shares the tile (retrieve_tile.h), and the order is total.
//
// Storage. The item rows are kept sorted by list (rows_sorted[r] = row perm[r] of the catalog,
// list l at rows [list_off[l], list_off[l + 1]), ascending catalog column inside a list). Columns
// in every argument and result are the catalog's; the sorted order is internal.
//
// Three stages on the caller's stream, no host synchronisation; every grid is an upper bound from
// B, nprobe, nlist, and surplus blocks exit.
//   group  (rs_ivf_group): the (user, probe slot) pairs p = b * nprobe + slot grouped by list
//          (histogram, exclusive scan by one workgroup, scatter by atomics) and each list's pairs
//          cut into work items of at most 32. The order of the pairs inside a list can differ from
//          run to run; the result cannot, as scores do not depend on tile company and the final
//          order is total.
//   scan   (rs_ivf_scan): one wave per work item. Its (up to) 32 users are the B operands
//          (FtUser::load, the row from the work list), the list's rows stream through the tile
//          pipeline of fused_topk_kernel (ft_load_tile clamps to the array's last row: reads past
//          the list's end land in the next list and fail the `row < end` test). Candidate lists
//          as there (retrieve_list.h); the word's column is perm[row], ascending inside a work
//          item, so a later equal score has the higher column. History (binary search) and the
//          filter bit are tested on admission on the catalog column. Each pair gets its K best
//          words, sorted, in the workspace; a list with fewer writes the filler word 0 (column
//          -1 under the smallest order key: below every real word, -inf and NaN included).
//   merge  (rs_ivf_merge): a wave per user folds its nprobe sorted runs into the best K by the
//          64-bit word, so ties across lists break by the lower catalog column; a run whose head
//          is below the current K-th is skipped. -inf entries and fillers leave as (-1, -inf).
#include "retrieve_list.h"
#include "retrieve_tile.h"

namespace rs {
namespace {

constexpr int kIvfMaxLists = 65536;
constexpr int kIvfMaxProbe = 256;
constexpr int kIvfUsers = 32;  // users of a work item: one wave's B operands

// the workspace: byte offsets of its parts (each a multiple of 16) and the work-item bound
struct IvfLayout {
  int64_t work_items;  // the scan's grid: B nprobe / 32 + min(nlist, B nprobe), rounded up
  int64_t words;       // u64 [B nprobe][K]: pair p's K best, sorted descending
  int64_t work;        // int32 [work_items][4]: {list, first pair slot, pairs, 0}; list -1: surplus
  int64_t pairs;       // int32 [B nprobe]: the pair indices grouped by list
  int64_t cursor;      // int32 [nlist]: the histogram, then the scatter's cursors
  int64_t pair_off;    // int32 [nlist + 1]: exclusive scan of the histogram
  int64_t tile_off;    // int32 [nlist + 1]: exclusive scan of the lists' work items
  int64_t bytes;
};

inline int64_t up16(int64_t x) { return (x + 15) & ~(int64_t)15; }

inline IvfLayout ivf_layout(int64_t B, int64_t nprobe, int64_t nlist, int64_t K) {
  IvfLayout w;
  const int64_t P = B * nprobe;
  w.work_items = (P + kIvfUsers - 1) / kIvfUsers + (nlist < P ? nlist : P);
  w.words = 0;
  w.work = w.words + up16(P * K * 8);
  w.pairs = w.work + w.work_items * 16;
  w.cursor = w.pairs + up16(P * 4);
  w.pair_off = w.cursor + up16(nlist * 4);
  w.tile_off = w.pair_off + up16((nlist + 1) * 4);
  w.bytes = w.tile_off + up16((nlist + 1) * 4);
  return w;
}

// ---- group

__global__ __launch_bounds__(256) void ivf_hist_kernel(const int32_t* __restrict__ probe, int64_t ld_probe, int P,
                                                       int nprobe, int nlist, int K, int32_t* __restrict__ cursor,
                                                       unsigned long long* __restrict__ words) {
  const int p = blockIdx.x * 256 + threadIdx.x;
  if (p >= P) return;
  const int l = probe[(int64_t)(p / nprobe) * ld_probe + p % nprobe];
  if ((unsigned)l < (unsigned)nlist) {
    atomicAdd(&cursor[l], 1);
  } else {  // no such list: the pair contributes nothing
    for (int i = 0; i < K; ++i) words[(int64_t)p * K + i] = 0ull;
  }
}

// one workgroup: pair_off = exclusive scan of the histogram, tile_off = of ceil(count / 32);
// cursor[l] = pair_off[l]
__global__ __launch_bounds__(1024) void ivf_offsets_kernel(int nlist, int32_t* __restrict__ cursor,
                                                           int32_t* __restrict__ pair_off,
                                                           int32_t* __restrict__ tile_off) {
  __shared__ int s_p[1024], s_t[1024];
  const int tid = threadIdx.x;
  const int per = (nlist + 1023) / 1024;  // <= 64 consecutive lists a thread
  const int l0 = tid * per, l1 = min(l0 + per, nlist);
  int np = 0, nt = 0;
  for (int l = l0; l < l1; ++l) {
    const int n = cursor[l];
    np += n;
    nt += (n + kIvfUsers - 1) / kIvfUsers;
  }
  s_p[tid] = np;
  s_t[tid] = nt;
  __syncthreads();
  for (int d = 1; d < 1024; d <<= 1) {  // inclusive scan
    const int ap = tid >= d ? s_p[tid - d] : 0, at = tid >= d ? s_t[tid - d] : 0;
    __syncthreads();
    s_p[tid] += ap;
    s_t[tid] += at;
    __syncthreads();
  }
  int bp = s_p[tid] - np, bt = s_t[tid] - nt;
  for (int l = l0; l < l1; ++l) {
    const int n = cursor[l];
    pair_off[l] = bp;
    tile_off[l] = bt;
    cursor[l] = bp;
    bp += n;
    bt += (n + kIvfUsers - 1) / kIvfUsers;
  }
  if (tid == 1023) {
    pair_off[nlist] = s_p[1023];
    tile_off[nlist] = s_t[1023];
  }
}

// thread i < P scatters pair i under its list; thread i < work_items writes work item i
__global__ __launch_bounds__(256) void ivf_scatter_kernel(const int32_t* __restrict__ probe, int64_t ld_probe, int P,
                                                          int nprobe, int nlist, int work_items,
                                                          int32_t* __restrict__ cursor,
                                                          const int32_t* __restrict__ pair_off,
                                                          const int32_t* __restrict__ tile_off,
                                                          int32_t* __restrict__ pairs, int32_t* __restrict__ work) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i < P) {
    const int l = probe[(int64_t)(i / nprobe) * ld_probe + i % nprobe];
    if ((unsigned)l < (unsigned)nlist) pairs[atomicAdd(&cursor[l], 1)] = i;
  }
  if (i < work_items) {
    int l = -1, first = 0, n = 0;
    if (i < tile_off[nlist]) {
      int lo = 0, hi = nlist - 1;  // the last list with tile_off[l] <= i
      while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (tile_off[mid] <= i) lo = mid; else hi = mid - 1;
      }
      l = lo;
      first = pair_off[l] + kIvfUsers * (i - tile_off[l]);
      n = min(kIvfUsers, pair_off[l + 1] - first);
    }
    work[4 * i + 0] = l;
    work[4 * i + 1] = first;
    work[4 * i + 2] = n;
    work[4 * i + 3] = 0;
  }
}

// ---- scan

struct IvfScanArgs {
  const float* U;
  int64_t ldu;
  const void* rows;  // cluster-sorted item rows
  int64_t ldi;
  int N, D, K, nprobe;
  int item_exp;  // e4m3 rows: the index's scale exponent
  const int32_t* perm;      // [N]: the catalog column of sorted row r
  const int32_t* list_off;  // [nlist + 1]
  const int64_t* user_ids;
  int64_t uid_stride;
  const int64_t* hist_off;
  const int32_t* hist_idx;
  int64_t num_users;
  const int32_t* filter_ids;  // null: nobody is filtered
  int64_t fid_stride;
  const uint32_t* filter_bits;
  int64_t filter_ld;
  int num_filters;
  const int32_t* work;
  const int32_t* pairs;
  unsigned long long* words;
};

// KB: the K bucket of the candidate lists (FtCfg::CAP); the tiles are the one-wave sweep's
template <int DP, FtElem EK, int KB>
__global__ __launch_bounds__(64) void ivf_scan_kernel(IvfScanArgs a) {
  // 32-item tiles for the instance whose 64-item tiles fill the register file in the sweep
  using Cfg = FtCfg<DP, EK, 1, DP == 256 && EK == kBF16>;
  using E = FtStore<EK>;
  constexpr int CAP = FtCfg<DP, EK, KB>::CAP, TI = Cfg::TI, NB = Cfg::NB;
  constexpr int SL = Cfg::SL, ESZ = Cfg::ESZ;
  static_assert(Cfg::NT == 64 && Cfg::ROWS == kIvfUsers, "one wave, 32 users");
  __shared__ __attribute__((aligned(16))) E tiles[2][TI * Cfg::PTMAX];
  __shared__ unsigned long long lists[kIvfUsers * CAP];
  __shared__ int s_cnt[kIvfUsers];
  __shared__ float s_thr[kIvfUsers];
  __shared__ int s_pair[kIvfUsers];
  __shared__ int s_frow[kIvfUsers];  // the users' filter rows (first word's index, -1: unfiltered)

  const int list = a.work[4 * blockIdx.x];
  if (list < 0) return;  // a surplus block of the grid's bound
  const int first = a.work[4 * blockIdx.x + 1], nu = a.work[4 * blockIdx.x + 2];

  const int tid = threadIdx.x, lane = tid;
  const int c = lane & 31, h = lane >> 5;
  const int D = a.D, K = a.K;
  const int PT = ft_pitch<EK>(D);
  const bool o_ok = c < nu;  // list row c holds a user
  const int pair = o_ok ? a.pairs[first + c] : 0;
  const int o = pair / a.nprobe;  // this lane's batch row
  const int r_begin = a.list_off[list], r_end = a.list_off[list + 1];
  const int ntiles = (r_end - r_begin + TI - 1) / TI;

  // NaN threshold: "never held K entries", every score is admitted (!(s <= NaN)); rows without a
  // user admit nothing
  if (h == 0) {
    s_cnt[c] = 0;
    s_thr[c] = o_ok ? __uint_as_float(kFtNeverHeldK) : INFINITY;
    s_pair[c] = pair;
    int frow = -1;
    if (o_ok && a.filter_ids) {
      const int id = a.filter_ids[(int64_t)o * a.fid_stride];
      if (id >= 0 && id < a.num_filters) frow = id * (int)a.filter_ld;
    }
    s_frow[c] = frow;
  }
  float thr = o_ok ? __uint_as_float(kFtNeverHeldK) : INFINITY;

  int64_t h_lo = 0, h_hi = 0;  // the user's CSR slice (sorted ascending)
  if (o_ok && a.user_ids && a.hist_off && a.hist_idx) {
    const int64_t uid = a.user_ids[(int64_t)o * a.uid_stride];
    if (uid >= 0 && uid < a.num_users) {
      h_lo = a.hist_off[uid];
      h_hi = a.hist_off[uid + 1];
    }
  }

  FtUser<DP, EK> uf;  // user fragments (B operand)
  uf.load(a.U, a.ldu, o, o_ok, D, h, a.item_exp);

  constexpr int DEPTH = Cfg::DEPTH;
  u32x4 st[DEPTH][SL];
  const int cpr = D * ESZ / 16;
  auto load_tile = [&](u32x4 (&r)[SL], int t) {
    ft_load_tile<Cfg>(r, a.rows, a.ldi, a.N, (int64_t)r_begin + (int64_t)t * TI, tid, cpr);
  };
  auto store_tile = [&](const u32x4 (&r)[SL], int buf) { ft_store_tile<Cfg>(r, tiles[buf], PT, tid, cpr); };
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");

  // one 32-row block's scores: element e = sorted row rowbase + 8 (e >> 2) + 4 h + (e & 3), user c
  auto admit_block = [&](const floatx16& acc, int rowbase) {
#pragma unroll
    for (int e = 0; e < 16; ++e) {
      const int row = rowbase + 8 * (e >> 2) + 4 * h + (e & 3);
      float s = acc[e];
      const bool cand = row < r_end && !(s <= thr);
      if (__any(cand)) {
        if (cand) {
          const int col = a.perm[row];  // the catalog column: history, filters and the word use it
          int64_t lo = h_lo, hi = h_hi;
          while (lo < hi) {
            const int64_t mid = (lo + hi) >> 1;
            if (a.hist_idx[mid] < col) lo = mid + 1; else hi = mid;
          }
          if (lo < h_hi && a.hist_idx[lo] == col) s = -INFINITY;
          const int frow = s_frow[c];
          if (frow >= 0 && !((a.filter_bits[frow + (col >> 5)] >> (col & 31)) & 1u)) s = -INFINITY;
          if (!(s <= thr)) {
            const int slot = atomicAdd(&s_cnt[c], 1);
            if (slot < CAP) lists[c * CAP + slot] = ft_word(s, col);
          }
        }
      }
    }
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    const int n = s_cnt[c];
    unsigned long long need = __ballot(h == 0 && n > CAP - 32);
    while (need) {
      const int r = __ffsll((long long)need) - 1;
      ft_prune_row<CAP>(&lists[r * CAP], &s_cnt[r], &s_thr[r], K, lane);
      need &= need - 1;
    }
    thr = s_thr[c];
  };

  auto compute_tile = [&](int t) {
    floatx16 acc[NB];
    ft_mfma<DP, EK, NB>(tiles[t & 1], PT, D, c, h, uf, acc);
#pragma unroll
    for (int ib = 0; ib < NB; ++ib) {
      float m = acc[ib][0];
#pragma unroll
      for (int e = 1; e < 16; ++e) m = fmaxf(m, acc[ib][e]);
      if (__any(!(m <= thr))) admit_block(acc[ib], r_begin + t * TI + ib * 32);
    }
  };

  // the tile pipeline of fused_topk_kernel; tiles past the list's end are clamped reads that
  // nobody consumes
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

  // every pair's K best, sorted; the filler word 0 where the list held fewer
  for (int r = 0; r < nu; ++r) {
    ft_prune_row<CAP>(&lists[r * CAP], &s_cnt[r], &s_thr[r], K, lane);
    const int n = s_cnt[r];
    unsigned long long* out = a.words + (int64_t)s_pair[r] * K;
    for (int i = lane; i < K; i += 64) out[i] = i < n ? lists[r * CAP + i] : 0ull;
  }
}

template <int DP, FtElem EK>
int ivf_launch_k(const IvfScanArgs& a, int grid, hipStream_t st) {
  if (a.K <= kFtSmallK)
    ivf_scan_kernel<DP, EK, 0><<<grid, 64, 0, st>>>(a);
  else
    ivf_scan_kernel<DP, EK, 1><<<grid, 64, 0, st>>>(a);
  RS_CHECK_LAUNCH("rs_ivf_scan");
  return 0;
}

template <FtElem EK>
int ivf_launch(const IvfScanArgs& a, int grid, hipStream_t st) {
  if (a.D <= 64) return ivf_launch_k<64, EK>(a, grid, st);
  if (a.D <= 128) return ivf_launch_k<128, EK>(a, grid, st);
  return ivf_launch_k<256, EK>(a, grid, st);
}

// ---- merge

// one wave per user: R = the best K so far (sorted descending), folded with one run at a time.
// Words of different pairs differ unless both are fillers; a run's entry goes behind an equal
// entry of R, so the merge is a permutation and every slot below K is written once.
__global__ __launch_bounds__(64) void ivf_merge_kernel(const unsigned long long* __restrict__ words, int nprobe, int K,
                                                       int32_t* __restrict__ out_cols, float* __restrict__ out_val,
                                                       int64_t ld_out) {
  __shared__ unsigned long long R[2][kFtMaxK];
  __shared__ unsigned long long Lr[kFtMaxK];
  constexpr int J = kFtMaxK / 64;
  const int lane = threadIdx.x;
  const int64_t b = blockIdx.x;
  const unsigned long long* W = words + b * nprobe * K;
  for (int i = lane; i < K; i += 64) R[0][i] = W[i];
  unsigned long long nx[J];  // the next run, in flight during the fold of this one
#pragma unroll
  for (int j = 0; j < J; ++j) {
    const int i = lane + 64 * j;
    nx[j] = nprobe > 1 && i < K ? W[K + i] : 0ull;
  }
  int cur = 0;
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
  for (int q = 1; q < nprobe; ++q) {
#pragma unroll
    for (int j = 0; j < J; ++j) {
      const int i = lane + 64 * j;
      if (i < K) Lr[i] = nx[j];
      nx[j] = q + 1 < nprobe && i < K ? W[(int64_t)(q + 1) * K + i] : 0ull;
    }
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    if (Lr[0] > R[cur][K - 1]) {  // uniform; else nothing of this run enters
      for (int i = lane; i < K; i += 64) {
        const unsigned long long x = R[cur][i], y = Lr[i];
        int lo = 0, hi = K;  // the entries of the run above x
        while (lo < hi) {
          const int mid = (lo + hi) >> 1;
          if (Lr[mid] > x) lo = mid + 1; else hi = mid;
        }
        if (i + lo < K) R[cur ^ 1][i + lo] = x;
        lo = 0, hi = K;  // the entries of R at or above y
        while (lo < hi) {
          const int mid = (lo + hi) >> 1;
          if (R[cur][mid] >= y) lo = mid + 1; else hi = mid;
        }
        if (i + lo < K) R[cur ^ 1][i + lo] = y;
      }
      cur ^= 1;
    }
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
  }
  for (int i = lane; i < K; i += 64) {
    const unsigned long long w = R[cur][i];
    const float v = ft_word_value(w);
    const bool real = w != 0ull && v != -INFINITY;
    out_cols[b * ld_out + i] = real ? ft_word_col(w) : -1;
    out_val[b * ld_out + i] = real ? v : -INFINITY;
  }
}

// the sizes every entry shares, checked before any device call
int ivf_sizes(const char* name, int B, int nprobe, int nlist, int K) {
  RS_CHECK_ARG(B >= 0, "%s: B = %d < 0", name, B);
  RS_CHECK_ARG(K >= 1 && K <= kFtMaxK, "%s: K = %d, must be in [1, 256]", name, K);
  RS_CHECK_ARG(nlist >= 1 && nlist <= kIvfMaxLists, "%s: nlist = %d, must be in [1, 65536]", name, nlist);
  RS_CHECK_ARG(nprobe >= 1 && nprobe <= nlist && nprobe <= kIvfMaxProbe,
               "%s: nprobe = %d, must be in [1, min(nlist = %d, 256)]", name, nprobe, nlist);
  RS_CHECK_ARG((int64_t)B * nprobe < (int64_t)1 << 31, "%s: B * nprobe = %lld (user, list) pairs: 2^31 or more", name,
               (long long)B * nprobe);
  return 0;
}

int ivf_workspace(const char* name, int B, int nprobe, int nlist, int K, const void* ws, int64_t ws_bytes,
                  IvfLayout* w) {
  *w = ivf_layout(B, nprobe, nlist, K);
  RS_CHECK_ARG(ws && aligned16(ws) && ws_bytes >= w->bytes,
               "%s: workspace of %lld bytes, needs %lld, 16-byte aligned (rs_ivf_ws_bytes)", name, (long long)ws_bytes,
               (long long)w->bytes);
  return 0;
}

template <class T>
T* ws_at(void* ws, int64_t off) {
  return reinterpret_cast<T*>(static_cast<char*>(ws) + off);
}

}  // namespace
}  // namespace rs

using namespace rs;

extern "C" int64_t rs_ivf_ws_bytes(int B, int nprobe, int nlist, int K, int64_t* layout) {
  if (layout)
    for (int i = 0; i < 8; ++i) layout[i] = 0;
  if (B < 1 || nprobe < 1 || nlist < 1 || K < 1) return 16;
  const IvfLayout w = ivf_layout(B, nprobe, nlist, K);
  if (layout) {
    layout[0] = w.work_items; layout[1] = w.words; layout[2] = w.work; layout[3] = w.pairs;
    layout[4] = w.cursor; layout[5] = w.pair_off; layout[6] = w.tile_off; layout[7] = w.bytes;
  }
  return w.bytes;
}

extern "C" int rs_ivf_group(const int32_t* probe, int64_t ld_probe, int B, int nprobe, int nlist, int K, void* ws,
                            int64_t ws_bytes, void* stream) {
  RS_RET_IF(ivf_sizes("rs_ivf_group", B, nprobe, nlist, K));
  RS_CHECK_ARG(probe && ld_probe >= nprobe, "rs_ivf_group: null probe or ld_probe = %lld < nprobe = %d",
               (long long)ld_probe, nprobe);
  if (B == 0) return 0;
  IvfLayout w;
  RS_RET_IF(ivf_workspace("rs_ivf_group", B, nprobe, nlist, K, ws, ws_bytes, &w));
  const int P = B * nprobe, WI = (int)w.work_items;
  hipStream_t st = as_stream(stream);
  int32_t* cursor = ws_at<int32_t>(ws, w.cursor);
  int32_t* pair_off = ws_at<int32_t>(ws, w.pair_off);
  int32_t* tile_off = ws_at<int32_t>(ws, w.tile_off);
  const hipError_t e = hipMemsetAsync(cursor, 0, (size_t)nlist * 4, st);
  RS_CHECK_ARG(e == hipSuccess, "rs_ivf_group: hipMemsetAsync failed: %s", hipGetErrorString(e));
  ivf_hist_kernel<<<cdiv(P, 256), 256, 0, st>>>(probe, ld_probe, P, nprobe, nlist, K, cursor,
                                                ws_at<unsigned long long>(ws, w.words));
  RS_CHECK_LAUNCH("rs_ivf_group (histogram)");
  ivf_offsets_kernel<<<1, 1024, 0, st>>>(nlist, cursor, pair_off, tile_off);
  RS_CHECK_LAUNCH("rs_ivf_group (offsets)");
  ivf_scatter_kernel<<<cdiv(P > WI ? P : WI, 256), 256, 0, st>>>(probe, ld_probe, P, nprobe, nlist, WI, cursor, pair_off,
                                                                 tile_off, ws_at<int32_t>(ws, w.pairs),
                                                                 ws_at<int32_t>(ws, w.work));
  RS_CHECK_LAUNCH("rs_ivf_group (scatter)");
  return 0;
}

extern "C" int rs_ivf_scan(const float* U, int64_t ldu, int B, const void* rows, int item_kind, int item_exp,
                           int64_t ldi, int64_t N, int D, int K, const int32_t* perm, const int32_t* list_off,
                           int nlist, int nprobe, const int64_t* user_ids, int64_t uid_stride,
                           const int64_t* hist_off, const int32_t* hist_idx, int64_t num_users,
                           const int32_t* filter_ids, int64_t fid_stride, const uint32_t* filter_bits,
                           int64_t filter_ld, int num_filters, void* ws, int64_t ws_bytes, void* stream) {
  RS_CHECK_ARG(item_kind >= 0 && item_kind <= 2, "rs_ivf_scan: item_kind = %d (0 fp32, 1 bf16, 2 e4m3)", item_kind);
  RS_CHECK_ARG(item_kind != 2 || (item_exp >= -kE4m3MaxExp && item_exp <= kE4m3MaxExp),
               "rs_ivf_scan: item_exp = %d outside [-40, 40]", item_exp);
  const int ld_mult = item_kind == 0 ? 4 : item_kind == 1 ? 8 : 16;  // a row stride of whole 16-byte chunks
  RS_CHECK_ARG(U && rows && perm && list_off, "rs_ivf_scan: null U / rows / perm / list_off");
  RS_CHECK_ARG(D >= 16 && D <= 256 && D % 16 == 0, "rs_ivf_scan: D = %d, must be a multiple of 16 in [16, 256]", D);
  RS_CHECK_ARG(N >= 1 && N < (int64_t)1 << 31, "rs_ivf_scan: bad sizes (N=%lld; 1 <= N < 2^31)", (long long)N);
  RS_RET_IF(ivf_sizes("rs_ivf_scan", B, nprobe, nlist, K));
  RS_CHECK_ARG(ldu >= D && ldu % 4 == 0 && ldi >= D && ldi % ld_mult == 0 && aligned16(U) && aligned16(rows),
               "rs_ivf_scan: rows of U and the item rows must be 16-byte aligned, ld >= D");
  RS_CHECK_ARG(num_filters >= 0, "rs_ivf_scan: num_filters = %d < 0", num_filters);
  if (!filter_ids || num_filters == 0) {
    filter_ids = nullptr;
  } else {
    const int64_t fwords = (N + 31) / 32;
    RS_CHECK_ARG(filter_bits, "rs_ivf_scan: null filter_bits with num_filters = %d", num_filters);
    RS_CHECK_ARG(filter_ld >= fwords, "rs_ivf_scan: filter_ld = %lld, a row of N = %lld columns has %lld words (rs_pack_mask)",
                 (long long)filter_ld, (long long)N, (long long)fwords);
    RS_CHECK_ARG(filter_ld * num_filters < (int64_t)1 << 31, "rs_ivf_scan: %d filters of %lld words: 2^31 words or more",
                 num_filters, (long long)filter_ld);
  }
  if (B == 0) return 0;
  IvfLayout w;
  RS_RET_IF(ivf_workspace("rs_ivf_scan", B, nprobe, nlist, K, ws, ws_bytes, &w));
  IvfScanArgs a;
  a.U = U; a.ldu = ldu; a.rows = rows; a.ldi = ldi; a.N = (int)N; a.D = D; a.K = K; a.nprobe = nprobe;
  a.item_exp = item_kind == 2 ? item_exp : 0;
  a.perm = perm; a.list_off = list_off;
  a.user_ids = user_ids; a.uid_stride = uid_stride; a.hist_off = hist_off; a.hist_idx = hist_idx;
  a.num_users = num_users;
  a.filter_ids = filter_ids; a.fid_stride = fid_stride; a.filter_bits = filter_bits; a.filter_ld = filter_ld;
  a.num_filters = num_filters;
  a.work = ws_at<int32_t>(ws, w.work); a.pairs = ws_at<int32_t>(ws, w.pairs);
  a.words = ws_at<unsigned long long>(ws, w.words);
  RS_CHECK_ARG(w.work_items < (int64_t)1 << 31, "rs_ivf_scan: grid too large");
  const int grid = (int)w.work_items;
  return item_kind == 0   ? ivf_launch<kF32>(a, grid, as_stream(stream))
         : item_kind == 1 ? ivf_launch<kBF16>(a, grid, as_stream(stream))
                          : ivf_launch<kE4M3>(a, grid, as_stream(stream));
}

extern "C" int rs_ivf_merge(int B, int nprobe, int nlist, int K, void* ws, int64_t ws_bytes, int32_t* out_cols,
                            float* out_val, int64_t ld_out, void* stream) {
  RS_RET_IF(ivf_sizes("rs_ivf_merge", B, nprobe, nlist, K));
  RS_CHECK_ARG(out_cols && out_val && ld_out >= K, "rs_ivf_merge: null out_cols / out_val or ld_out = %lld < K = %d",
               (long long)ld_out, K);
  if (B == 0) return 0;
  IvfLayout w;
  RS_RET_IF(ivf_workspace("rs_ivf_merge", B, nprobe, nlist, K, ws, ws_bytes, &w));
  ivf_merge_kernel<<<B, 64, 0, as_stream(stream)>>>(ws_at<unsigned long long>(ws, w.words), nprobe, K, out_cols,
                                                    out_val, ld_out);
  RS_CHECK_LAUNCH("rs_ivf_merge");
  return 0;
}

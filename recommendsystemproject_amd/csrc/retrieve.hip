// Fused top-K retrieval over an item index (serving, and validate(retrieval='fused')): the K best
// catalog columns of every user by dot product, with their scores, without the [B, N] score matrix
// of the staged pipeline (rs_gemm_f32 -> rs_mask_history -> rs_topk_rows per column chunk,
// retrieval.hip). Same result: value descending, ties by the lower column, history columns -inf.
// Beside it, on the same tiles (retrieve_tile.h): the full-catalog rank of one target column per
// user in that order (target_rank_kernel below; evaluation).
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
//
// Catalog filters (rs_fused_topk_filtered / rs_target_rank_filtered; the FILT instances, the others
// compile without any of it): a user may name one of F packed allow-lists (rs_pack_mask: bit c & 31
// of word c >> 5 of row f is column c). A column outside the user's list scores -inf exactly as a
// history column does. The host starts the splits of a filtered call on filter words wherever that
// leaves every split its K columns (filter_split_words); a block's 32 columns are then one word of
// the user's row, fetched by the lane, and the masked scores are set to -inf BEFORE the block
// maximum: a block with nothing allowed is skipped like a block below the threshold, and a
// selective filter does not send every finite score down the serial admission path. Splits that
// must start inside a word (few columns a split: small catalogs only) test the column's bit on
// admission instead, as history does. The rank kernel funnel-shifts two words there; it takes
// the sign-trick path only for blocks whose 32 bits are set for every user of the wave.
#include "retrieve_list.h"
#include "retrieve_tile.h"

namespace rs {
namespace {

// Catalog filters: a user's packed row as its first word's index in `bits` (one register; -1:
// unfiltered) and the 32 bits of the block of columns [colbase, colbase + 32), bit i = column
// colbase + i is allowed. Columns at or past N read as 0.
struct FtFilter {
  const int32_t* ids;  // [B] with stride, null: nobody is filtered
  int64_t id_stride;
  const uint32_t* bits;  // [num_filters][ld] words, num_filters * ld < 2^31
  int64_t ld;
  int num_filters;
  int words;        // ceil(N / 32)
  int split_words;  // != 0: split s starts at column 32 * (s * words / splits) (one word a block)
};

__device__ __forceinline__ int ft_filter_row(const FtFilter& f, int o, bool o_ok) {
  if (!o_ok || !f.ids || !f.bits) return -1;
  const int id = f.ids[(int64_t)o * f.id_stride];
  return id >= 0 && id < f.num_filters ? id * (int)f.ld : -1;
}

__device__ __forceinline__ uint32_t ft_filter_word(const FtFilter& f, int row, int colbase) {
  if (row < 0) return 0xffffffffu;
  const int w = colbase >> 5, sh = colbase & 31;
  if (w >= f.words) return 0u;
  const uint32_t lo = f.bits[row + w];
  if (sh == 0) return lo;  // uniform over the workgroup: every block of a word-aligned split
  const uint32_t hi = w + 1 < f.words ? f.bits[row + w + 1] : 0u;
  return __builtin_amdgcn_alignbit(hi, lo, sh);
}

// the 16 bits of a block's word that belong to lane half h, bit e = element e (column colbase +
// 8 (e >> 2) + 4 h + (e & 3)): nibbles 2 q + h of the word
__device__ __forceinline__ uint32_t ft_elem_bits(uint32_t word, int h) {
  const uint32_t v = word >> (4 * h);
  return (v & 0xfu) | ((v >> 4) & 0xf0u) | ((v >> 8) & 0xf00u) | ((v >> 12) & 0xf000u);
}

// the columns [begin, end) of a split
__device__ __forceinline__ void ft_split_range(int split, int splits, int split_cols, int N, int words,
                                               int split_words, int& begin, int& end) {
  if (split_words) {
    begin = 32 * (int)((int64_t)split * words / splits);
    end = split == splits - 1 ? N : 32 * (int)((int64_t)(split + 1) * words / splits);
  } else {
    begin = split * split_cols;
    end = split == splits - 1 ? N : begin + split_cols;
  }
}

struct FtArgs {
  const float* U;
  int64_t ldu;
  int B;
  const void* items;
  int64_t ldi;
  int N, D, K;
  int item_exp;  // e4m3 items: the index's scale exponent
  const int64_t* user_ids;
  int64_t uid_stride;
  const int64_t* hist_off;
  const int32_t* hist_idx;
  int64_t num_users;
  int splits, split_cols, nrt;
  int32_t* out_idx;  // [B][ld_out], this split's candidates at split * K
  float* out_val;    // nullable
  int64_t ld_out;
  FtFilter f;  // the FILT instances only
};

template <int DP, FtElem EK, int KB, bool FILT>
__global__ __launch_bounds__((FtCfg<DP, EK, KB>::NT)) void fused_topk_kernel(FtArgs a) {
  // the one unfiltered instance that fills all 512 registers takes 32-item tiles when filtered
  // (half the staging registers) rather than spill to scratch
  using Cfg = FtCfg<DP, EK, KB, FILT && DP == 256 && EK == kBF16 && KB == 1>;
  using E = FtStore<EK>;
  constexpr int ROWS = Cfg::ROWS, CAP = Cfg::CAP, TI = Cfg::TI, NB = Cfg::NB;
  constexpr int SL = Cfg::SL, ESZ = Cfg::ESZ;
  __shared__ __attribute__((aligned(16))) E tiles[2][TI * Cfg::PTMAX];
  __shared__ unsigned long long lists[ROWS * CAP];
  __shared__ int s_cnt[ROWS];
  __shared__ float s_thr[ROWS];
  __shared__ int s_frow[FILT ? ROWS : 1];  // FILT: the users' filter rows (a register fewer to hold)

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int c = lane & 31, h = lane >> 5;
  const int rt = blockIdx.x % a.nrt, split = blockIdx.x / a.nrt;
  const int D = a.D, K = a.K;
  const int PT = ft_pitch<EK>(D);
  const int lrow = wave * 32 + c;  // this lane's user: list row and, + rt * ROWS, batch row
  const int o = rt * ROWS + lrow;
  const bool o_ok = o < a.B;
  int c_begin = split * a.split_cols;
  int c_end = split == a.splits - 1 ? a.N : c_begin + a.split_cols;
  if constexpr (FILT) {
    ft_split_range(split, a.splits, a.split_cols, a.N, a.f.words, a.f.split_words, c_begin, c_end);
    if (h == 0) s_frow[lrow] = ft_filter_row(a.f, o, o_ok);
  }
  const int ntiles = (c_end - c_begin + TI - 1) / TI;

  // NaN threshold: "never held K entries", every score is admitted (!(s <= NaN)); rows past B
  // admit nothing
  if (h == 0) {
    s_cnt[lrow] = 0;
    s_thr[lrow] = o_ok ? __uint_as_float(kFtNeverHeldK) : INFINITY;
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

  // staging registers of the tiles in flight (retrieve_tile.h)
  constexpr int DEPTH = Cfg::DEPTH;
  u32x4 st[DEPTH][SL];
  const int cpr = D * ESZ / 16;
  auto load_tile = [&](u32x4 (&r)[SL], int t) {
    ft_load_tile<Cfg>(r, a.items, a.ldi, a.N, (int64_t)c_begin + (int64_t)t * TI, tid, cpr);
  };
  auto store_tile = [&](const u32x4 (&r)[SL], int buf) { ft_store_tile<Cfg>(r, tiles[buf], PT, tid, cpr); };

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
          if constexpr (FILT) {  // splits that start inside a filter word: the bit on admission
            const int frow = s_frow[lrow];
            if (!a.f.split_words && frow >= 0 && !((a.f.bits[frow + (col >> 5)] >> (col & 31)) & 1u)) s = -INFINITY;
          }
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
    floatx16 acc[NB];
    ft_mfma<DP, EK, NB>(tiles[t & 1], PT, D, c, h, uf, acc);
#pragma unroll
    for (int ib = 0; ib < NB; ++ib) {
      if constexpr (FILT) {
        // word-aligned splits: the block's filter word before its maximum
        const int frow = s_frow[lrow], fwi = (c_begin + t * TI + ib * 32) >> 5;
        const uint32_t fw = !a.f.split_words || frow < 0 ? 0xffffffffu : fwi < a.f.words ? a.f.bits[frow + fwi] : 0u;
        if (__any(fw != 0xffffffffu)) {
          const uint32_t v = fw >> (4 * h);  // element e: bit 8 (e >> 2) + (e & 3)
#pragma unroll
          for (int e = 0; e < 16; ++e) acc[ib][e] = (v >> (8 * (e >> 2) + (e & 3))) & 1u ? acc[ib][e] : -INFINITY;
        }
      }
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

// Target rank (rs_target_rank): for every user the number of catalog columns that precede its
// target column in rs_fused_topk's order (masked value descending, ties by the lower column); a
// full-catalog rank without candidate lists, prunes or a K. Same grid, staging and MFMA tiles as
// the four-wave fused_topk_kernel; only the two item tiles live in LDS. Item rows are fp32, bf16
// or e4m3 bytes under one scale (retrieve_tile.h FtElem; rs_*_e4m3), one instance each.
//
// The target's score is formed by the same MFMA sequence as every other score, so that exact
// copies of the target row tie with it: before the sweep a wave stages the target rows of its 32
// users as one 32-item block (in the item tiles' LDS, not yet in use) and lane (c, h) takes the
// diagonal element, item row c against user c. A target inside the user's own history scores -inf.
//
// Counting: a lane holds 16 scores of one user per block. A block that lies inside the split, holds
// no lane's target and no history column of the wave's users is counted from the sign of s - thr
// (s >= ts left of the target, s > ts right of it, as s >= the next float above ts). The
// others take the exact test per element; history columns come from a per-lane cursor into the
// user's sorted slice that only moves forward, like the columns, and count only when the target
// itself is masked and they lie left of it. The count is a register; the two half-lanes of a user
// add by one shuffle. One split writes the rank itself (one launch); otherwise each split stores
// its partial count to ws [splits][B] and target_rank_reduce adds them: integer sums, the same
// for every split count (int32 atomics would need the output zeroed first: a launch more for one
// split, none fewer otherwise).
constexpr int kTrNoCol = 0x7fffffff;  // past every column (N < 2^31): a cursor at its slice's end

struct TrArgs {
  const float* U;
  int64_t ldu;
  int B;
  const void* items;
  int64_t ldi;
  int N, D;
  int item_exp;  // e4m3 items: the index's scale exponent
  const int32_t* target_col;
  int64_t tc_stride;
  const int64_t* user_ids;
  int64_t uid_stride;
  const int64_t* hist_off;
  const int32_t* hist_idx;
  int64_t num_users;
  int splits, split_cols, nrt;
  int32_t* out;  // one split: the ranks [B]; else this split's partial counts at split * B
  FtFilter f;    // the FILT instances only
};

template <int DP, FtElem EK, bool FILT>
__global__ __launch_bounds__((FtCfg<DP, EK, 0>::NT)) void target_rank_kernel(TrArgs a) {
  using Cfg = FtCfg<DP, EK, 0>;
  using E = FtStore<EK>;
  constexpr int NW = Cfg::NW, ROWS = Cfg::ROWS, TI = Cfg::TI, NB = Cfg::NB, SL = Cfg::SL, ESZ = Cfg::ESZ;
  __shared__ __attribute__((aligned(16))) E tiles[2][TI * Cfg::PTMAX];

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int c = lane & 31, h = lane >> 5;
  const int rt = blockIdx.x % a.nrt, split = blockIdx.x / a.nrt;
  const int D = a.D;
  const int PT = ft_pitch<EK>(D);
  const int o = rt * ROWS + wave * 32 + c;  // this lane's user
  const bool o_ok = o < a.B;
  int c_begin = split * a.split_cols;
  int c_end = split == a.splits - 1 ? a.N : c_begin + a.split_cols;
  int frow = -1;  // the user's filter row
  if constexpr (FILT) {
    ft_split_range(split, a.splits, a.split_cols, a.N, a.f.words, a.f.split_words, c_begin, c_end);
    frow = ft_filter_row(a.f, o, o_ok);
  }
  const int ntiles = (c_end - c_begin + TI - 1) / TI;

  int tcol = -1;  // the target column, -1: not in the catalog (or a row past B)
  if (o_ok) {
    const int t = a.target_col[(int64_t)o * a.tc_stride];
    if (t >= 0 && t < a.N) tcol = t;
  }
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
    ft_load_tile<Cfg>(r, a.items, a.ldi, a.N, (int64_t)c_begin + (int64_t)t * TI, tid, cpr);
  };
  auto store_tile = [&](const u32x4 (&r)[SL], int buf) { ft_store_tile<Cfg>(r, tiles[buf], PT, tid, cpr); };
  load_tile(st[0], 0);  // in flight during the target pass

  // the target's score: WPR waves at a time stage their 32 target rows (a lane without a target
  // reads row 0 and drops the result) into the 2 * TI rows of the item tiles
  float ts = 0.f;
  {
    constexpr int WPR = 2 * TI / 32 < NW ? 2 * TI / 32 : NW;
    E* blk = &tiles[0][0] + (wave % WPR) * 32 * PT;
    for (int w0 = 0; w0 < NW; w0 += WPR) {
      const bool mine = wave >= w0 && wave < w0 + WPR;
      if (mine) {
        for (int slot = lane; slot < 32 * cpr; slot += 64) {  // rows < 32: always an active source lane
          const int row = slot / cpr, ch = slot % cpr;
          const int64_t g = __shfl(max(tcol, 0), row);
          ft_store_slot<ESZ>(blk, PT, row, ch,
                             *reinterpret_cast<const u32x4*>(reinterpret_cast<const char*>(a.items) +
                                                             g * a.ldi * ESZ + ch * 16));
        }
      }
      __syncthreads();
      if (mine) {
        floatx16 acc[1];
        ft_mfma<DP, EK, 1>(blk, PT, D, c, h, uf, acc);
        // item row c of the block is element 4 (c >> 3) + (c & 3) of the half-lane (c >> 2) & 1
        const int ed = 4 * (c >> 3) + (c & 3);
        float v = 0.f;
#pragma unroll
        for (int e = 0; e < 16; ++e) v = e == ed ? acc[0][e] : v;
        const float w = __shfl_xor(v, 32);
        ts = h == ((c >> 2) & 1) ? v : w;
      }
      __syncthreads();
    }
  }

  // the history cursor: the first slice entry at or after the split's first column
  int64_t hp = h_hi;
  if (h_lo < h_hi) {
    int64_t lo = h_lo, hi = h_hi;
    while (lo < hi) {
      const int64_t mid = (lo + hi) >> 1;
      if (a.hist_idx[mid] < c_begin) lo = mid + 1; else hi = mid;
    }
    hp = lo;
    if (tcol >= 0) {  // the target is masked like any other column
      lo = h_lo, hi = h_hi;
      while (lo < hi) {
        const int64_t mid = (lo + hi) >> 1;
        if (a.hist_idx[mid] < tcol) lo = mid + 1; else hi = mid;
      }
      if (lo < h_hi && a.hist_idx[lo] == tcol) ts = -INFINITY;
    }
  }
  if constexpr (FILT) {  // and by its own filter bit
    if (frow >= 0 && tcol >= 0 && !((a.f.bits[frow + (tcol >> 5)] >> (tcol & 31)) & 1u)) ts = -INFINITY;
  }
  int hnext = hp < h_hi ? a.hist_idx[hp] : kTrNoCol;
  // s > ts  <=>  s >= ts_up, the next float above ts (ts = +-0: the smallest subnormal)
  const uint32_t tb = __float_as_uint(ts);
  const float ts_up = __uint_as_float(ts == 0.f ? 1u : (tb & 0x80000000u) ? tb - 1 : tb + 1);
  int cnt = 0;

  // one 32-item block's scores: element e = column colbase + 8 (e >> 2) + 4 h + (e & 3), user c
  auto count_block = [&](const floatx16& acc, int colbase) {
    if (colbase >= c_end) return;
    const bool t_in = (unsigned)(tcol - colbase) < 32u;
    const bool h_in = hnext - colbase < 32;
    uint32_t fw = 0xffffffffu;  // the block's filter bits: the fast path needs all 32 of every user
    if constexpr (FILT) fw = ft_filter_word(a.f, frow, colbase);
    if (colbase <= c_end - 32 && !__any(t_in || h_in || fw != 0xffffffffu)) {
      // s >= thr <=> the sign of s - thr is clear (f32 subnormals are kept, so the difference of
      // unequal floats is never zero; x - x = +0): the 16 sign bits go through one funnel shift
      // each into w, two VALU operations per score and no compare
      const float thr = colbase < tcol ? ts : ts_up;
      uint32_t w = 0;
#pragma unroll
      for (int e = 0; e < 16; ++e) w = __builtin_amdgcn_alignbit(w, __float_as_uint(acc[e] - thr), 31);
      cnt += 16 - __popc(w);
      return;
    }
    uint32_t hmask = 0;  // bit e: element e is a masked (history or filtered) column of this user
    while (hnext - colbase < 32) {
      const int d = hnext - colbase;  // >= 0: the cursor never lags a block
      if (((d >> 2) & 1) == h) hmask |= 1u << (4 * (d >> 3) + (d & 3));
      ++hp;
      hnext = hp < h_hi ? a.hist_idx[hp] : kTrNoCol;
    }
    if constexpr (FILT) hmask |= ~ft_elem_bits(fw, h) & 0xffffu;  // a filtered column counts as history does
#pragma unroll
    for (int e = 0; e < 16; ++e) {
      const int col = colbase + 8 * (e >> 2) + 4 * h + (e & 3);
      const float s = acc[e];
      const bool left = col < tcol;
      const bool live = (unsigned)col < (unsigned)c_end && col != tcol;
      const bool raw = s > ts || (s == ts && left);
      const bool hist = (hmask >> e) & 1u;
      cnt += live && (hist ? (ts == -INFINITY && left) : raw) ? 1 : 0;
    }
  };

  auto compute_tile = [&](int t) {
    floatx16 acc[NB];
    ft_mfma<DP, EK, NB>(tiles[t & 1], PT, D, c, h, uf, acc);
#pragma unroll
    for (int ib = 0; ib < NB; ++ib) count_block(acc[ib], c_begin + t * TI + ib * 32);
  };

  // the tile pipeline of fused_topk_kernel
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

  cnt += __shfl_xor(cnt, 32);
  if (h == 0 && o_ok) a.out[(int64_t)split * a.B + o] = a.splits == 1 && tcol < 0 ? -1 : cnt;
}

// out[b] = the sum of the splits' partial counts, -1 for a target outside the catalog
__global__ __launch_bounds__(256) void target_rank_reduce(const int32_t* __restrict__ part, int splits, int B,
                                                          const int32_t* __restrict__ target_col,
                                                          int64_t tc_stride, int N, int32_t* __restrict__ out) {
  const int b = blockIdx.x * 256 + threadIdx.x;
  if (b >= B) return;
  const int t = target_col[(int64_t)b * tc_stride];
  int r = 0;
  for (int s = 0; s < splits; ++s) r += part[(int64_t)s * B + b];
  out[b] = t >= 0 && t < N ? r : -1;
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

template <int DP, FtElem EK, bool FILT>
int ft_launch_k(const FtArgs& a, int grid, hipStream_t st) {
  if (a.K <= kFtSmallK)
    fused_topk_kernel<DP, EK, 0, FILT><<<grid, FtCfg<DP, EK, 0>::NT, 0, st>>>(a);
  else
    fused_topk_kernel<DP, EK, 1, FILT><<<grid, FtCfg<DP, EK, 1>::NT, 0, st>>>(a);
  RS_CHECK_LAUNCH("rs_fused_topk");
  return 0;
}

template <FtElem EK, bool FILT>
int ft_launch_d(const FtArgs& a, int grid, hipStream_t st) {
  if (a.D <= 64) return ft_launch_k<64, EK, FILT>(a, grid, st);
  if (a.D <= 128) return ft_launch_k<128, EK, FILT>(a, grid, st);
  return ft_launch_k<256, EK, FILT>(a, grid, st);
}

// the FILT instances only for a call that names filters: every other call runs the kernels it ran
// before filters existed
template <FtElem EK>
int ft_launch(const FtArgs& a, int grid, hipStream_t st) {
  return a.f.ids ? ft_launch_d<EK, true>(a, grid, st) : ft_launch_d<EK, false>(a, grid, st);
}

template <FtElem EK, bool FILT>
int tr_launch_d(const TrArgs& a, int grid, hipStream_t st) {
  if (a.D <= 64)
    target_rank_kernel<64, EK, FILT><<<grid, FtCfg<64, EK, 0>::NT, 0, st>>>(a);
  else if (a.D <= 128)
    target_rank_kernel<128, EK, FILT><<<grid, FtCfg<128, EK, 0>::NT, 0, st>>>(a);
  else
    target_rank_kernel<256, EK, FILT><<<grid, FtCfg<256, EK, 0>::NT, 0, st>>>(a);
  RS_CHECK_LAUNCH("rs_target_rank");
  return 0;
}

template <FtElem EK>
int tr_launch(const TrArgs& a, int grid, hipStream_t st) {
  return a.f.ids ? tr_launch_d<EK, true>(a, grid, st) : tr_launch_d<EK, false>(a, grid, st);
}

// rs_pack_mask: a wave per 64 columns of one filter, one ballot, two words
__global__ __launch_bounds__(256) void pack_mask_kernel(const uint8_t* __restrict__ mask, int64_t ld, int64_t N,
                                                        int64_t blocks_per_row, uint32_t* __restrict__ bits,
                                                        int64_t ld_bits) {
  const int64_t f = blockIdx.x / blocks_per_row;
  const int64_t c = (blockIdx.x % blocks_per_row) * 256 + threadIdx.x;
  const unsigned long long b = __ballot(c < N && mask[f * ld + c] != 0);
  const int lane = threadIdx.x & 63;
  // lanes 0 and 32 hold the first column of a word; columns at or past N contributed 0 bits
  if ((lane & 31) == 0 && c < N) bits[f * ld_bits + (c >> 5)] = (uint32_t)(b >> lane);
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

// The filter arguments of the two _filtered calls, checked (after N) and made the kernels' FtFilter:
// no ids or no filters is the unfiltered call.
static int filter_args(const char* name, const int32_t* filter_ids, int64_t fid_stride, const uint32_t* filter_bits,
                       int64_t filter_ld, int num_filters, int64_t N, FtFilter* f) {
  *f = FtFilter{};
  RS_CHECK_ARG(num_filters >= 0, "%s: num_filters = %d < 0", name, num_filters);
  if (!filter_ids || num_filters == 0) return 0;
  const int64_t words = (N + 31) / 32;
  RS_CHECK_ARG(filter_bits, "%s: null filter_bits with num_filters = %d", name, num_filters);
  RS_CHECK_ARG(filter_ld >= words, "%s: filter_ld = %lld, a row of N = %lld columns has %lld words (rs_pack_mask)",
               name, (long long)filter_ld, (long long)N, (long long)words);
  RS_CHECK_ARG(filter_ld * num_filters < (int64_t)1 << 31, "%s: %d filters of %lld words: 2^31 words or more", name,
               num_filters, (long long)filter_ld);
  f->ids = filter_ids; f->id_stride = fid_stride; f->bits = filter_bits; f->ld = filter_ld;
  f->num_filters = num_filters; f->words = (int)words;
  return 0;
}

// Filtered calls start every split on a filter word (one word per 32-column block) where that
// leaves each split `min_cols` columns: split s covers the words [s W / splits, (s + 1) W / splits),
// the last one the catalog's tail, so a split has at least 32 (W / splits) - 31 columns.
static int filter_split_words(const FtFilter& f, int splits, int min_cols) {
  return f.ids && 32 * (int64_t)(f.words / splits) - 31 >= min_cols ? 1 : 0;
}

// rs_fused_topk, rs_fused_topk_e4m3 and rs_fused_topk_filtered: ek the item element, ldi in
// elements (e4m3: bytes)
static int fused_topk_any(const float* U, int64_t ldu, int B, const void* items, FtElem ek, int item_exp,
                          int64_t ldi, int64_t N, int D, int K, const int64_t* user_ids, int64_t uid_stride,
                          const int64_t* hist_off, const int32_t* hist_idx, int64_t num_users, int splits,
                          void* ws, int64_t ws_bytes, int32_t* out_idx, float* out_val, int64_t ld_out,
                          void* stream, const int32_t* filter_ids = nullptr, int64_t fid_stride = 0,
                          const uint32_t* filter_bits = nullptr, int64_t filter_ld = 0, int num_filters = 0) {
  const int ld_mult = ek == kF32 ? 4 : ek == kBF16 ? 8 : 16;  // a row stride of whole 16-byte chunks
  RS_CHECK_ARG(U && items && out_idx && B >= 0, "rs_fused_topk: null U / items / out_idx or B < 0");
  RS_CHECK_ARG(D >= 16 && D <= 256 && D % 16 == 0,
               "rs_fused_topk: D = %d, must be a multiple of 16 in [16, 256]", D);
  RS_CHECK_ARG(K >= 1 && K <= kFtMaxK && N >= 1 && N < (int64_t)1 << 31 && K <= N,
               "rs_fused_topk: bad sizes (N=%lld K=%d; K <= min(N, 256), N < 2^31)", (long long)N, K);
  RS_CHECK_ARG(ldu >= D && ldu % 4 == 0 && ldi >= D && ldi % ld_mult == 0 && aligned16(U) &&
                   aligned16(items) && ld_out >= K,
               "rs_fused_topk: rows of U and items must be 16-byte aligned, ld >= D, ld_out >= K");
  FtFilter flt;
  RS_RET_IF(filter_args("rs_fused_topk_filtered", filter_ids, fid_stride, filter_bits, filter_ld, num_filters, N,
                        &flt));
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
  a.items = items; a.ldi = ldi; a.N = (int)N; a.D = D; a.K = K; a.item_exp = item_exp;
  a.user_ids = user_ids; a.uid_stride = uid_stride; a.hist_off = hist_off; a.hist_idx = hist_idx;
  a.num_users = num_users;
  a.splits = splits; a.split_cols = (int)(N / splits); a.nrt = cdiv(B, ft_rows(K));
  a.f = flt; a.f.split_words = filter_split_words(flt, splits, K);
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
  RS_RET_IF(ek == kF32    ? ft_launch<kF32>(a, (int)grid, as_stream(stream))
            : ek == kBF16 ? ft_launch<kBF16>(a, (int)grid, as_stream(stream))
                          : ft_launch<kE4M3>(a, (int)grid, as_stream(stream)));
  if (splits == 1) return 0;
  // split-major candidates, sorted within a split: position order == column order among equal values
  return rs_topk_rows(ws_val, ldw, B, (int)ldw, K, ws_idx, ldw, 0, out_idx, out_val, ld_out, stream);
}

extern "C" int rs_fused_topk(const float* U, int64_t ldu, int B, const void* items, int items_bf16,
                             int64_t ldi, int64_t N, int D, int K, const int64_t* user_ids,
                             int64_t uid_stride, const int64_t* hist_off, const int32_t* hist_idx,
                             int64_t num_users, int splits, void* ws, int64_t ws_bytes, int32_t* out_idx,
                             float* out_val, int64_t ld_out, void* stream) {
  return fused_topk_any(U, ldu, B, items, items_bf16 ? kBF16 : kF32, 0, ldi, N, D, K, user_ids, uid_stride,
                        hist_off, hist_idx, num_users, splits, ws, ws_bytes, out_idx, out_val, ld_out, stream);
}

extern "C" int rs_fused_topk_e4m3(const float* U, int64_t ldu, int B, const void* items, int item_exp,
                                  int64_t ldi, int64_t N, int D, int K, const int64_t* user_ids,
                                  int64_t uid_stride, const int64_t* hist_off, const int32_t* hist_idx,
                                  int64_t num_users, int splits, void* ws, int64_t ws_bytes,
                                  int32_t* out_idx, float* out_val, int64_t ld_out, void* stream) {
  RS_CHECK_ARG(item_exp >= -kE4m3MaxExp && item_exp <= kE4m3MaxExp,
               "rs_fused_topk_e4m3: item_exp = %d outside [-40, 40]", item_exp);
  return fused_topk_any(U, ldu, B, items, kE4M3, item_exp, ldi, N, D, K, user_ids, uid_stride, hist_off,
                        hist_idx, num_users, splits, ws, ws_bytes, out_idx, out_val, ld_out, stream);
}

extern "C" int rs_fused_topk_filtered(const float* U, int64_t ldu, int B, const void* items, int item_kind,
                                      int item_exp, int64_t ldi, int64_t N, int D, int K, const int64_t* user_ids,
                                      int64_t uid_stride, const int64_t* hist_off, const int32_t* hist_idx,
                                      int64_t num_users, const int32_t* filter_ids, int64_t fid_stride,
                                      const uint32_t* filter_bits, int64_t filter_ld, int num_filters, int splits,
                                      void* ws, int64_t ws_bytes, int32_t* out_idx, float* out_val, int64_t ld_out,
                                      void* stream) {
  RS_CHECK_ARG(item_kind >= 0 && item_kind <= 2,
               "rs_fused_topk_filtered: item_kind = %d (0 fp32, 1 bf16, 2 e4m3)", item_kind);
  RS_CHECK_ARG(item_kind != 2 || (item_exp >= -kE4m3MaxExp && item_exp <= kE4m3MaxExp),
               "rs_fused_topk_filtered: item_exp = %d outside [-40, 40]", item_exp);
  return fused_topk_any(U, ldu, B, items, item_kind == 0 ? kF32 : item_kind == 1 ? kBF16 : kE4M3,
                        item_kind == 2 ? item_exp : 0, ldi, N, D, K, user_ids, uid_stride, hist_off, hist_idx,
                        num_users, splits, ws, ws_bytes, out_idx, out_val, ld_out, stream, filter_ids, fid_stride,
                        filter_bits, filter_ld, num_filters);
}

extern "C" int rs_pack_mask(const uint8_t* mask, int64_t ld, int F, int64_t N, uint32_t* bits, int64_t ld_bits,
                            void* stream) {
  RS_CHECK_ARG(mask && bits && F >= 1, "rs_pack_mask: null mask / bits or F = %d < 1", F);
  RS_CHECK_ARG(N >= 1 && N < (int64_t)1 << 31, "rs_pack_mask: bad sizes (N=%lld; 1 <= N < 2^31)", (long long)N);
  RS_CHECK_ARG(ld >= N && ld_bits >= (N + 31) / 32,
               "rs_pack_mask: ld = %lld < N = %lld or ld_bits = %lld < %lld words", (long long)ld, (long long)N,
               (long long)ld_bits, (long long)((N + 31) / 32));
  const int64_t blocks_per_row = (N + 255) / 256;
  RS_CHECK_ARG(blocks_per_row * F < (int64_t)1 << 31, "rs_pack_mask: too many filters (F=%d N=%lld)", F, (long long)N);
  pack_mask_kernel<<<(int)(blocks_per_row * F), 256, 0, as_stream(stream)>>>(mask, ld, N, blocks_per_row, bits,
                                                                            ld_bits);
  RS_CHECK_LAUNCH("rs_pack_mask");
  return 0;
}

extern "C" int rs_target_rank_splits(int B, int64_t N, int D) {
  (void)D;
  if (B < 1 || N < 1) return 1;
  // one round of workgroups over the 256 CUs, as rs_fused_topk_splits; no lists to warm up, so
  // the only floor is 2048 columns a split (its tile pipeline's fill against its sweep)
  const int64_t want = cdiv(256, cdiv(B, 128));
  const int64_t most = N / 2048;
  int64_t s = want < most ? want : most;
  if (s > 1024) s = 1024;
  return s < 1 ? 1 : (int)s;
}

extern "C" int64_t rs_target_rank_ws_bytes(int B, int64_t N, int D, int splits) {
  if (splits <= 0) splits = rs_target_rank_splits(B, N, D);
  if (B < 1 || splits == 1) return 16;
  const int64_t n = (int64_t)B * splits * 4;  // int32 partial counts [splits][B]
  return n < 16 ? 16 : n;
}

// rs_target_rank, rs_target_rank_e4m3 and rs_target_rank_filtered: ek the item element, ldi in
// elements (e4m3: bytes)
static int target_rank_any(const float* U, int64_t ldu, int B, const void* items, FtElem ek, int item_exp,
                           int64_t ldi, int64_t N, int D, const int32_t* target_col, int64_t tc_stride,
                           const int64_t* user_ids, int64_t uid_stride, const int64_t* hist_off,
                           const int32_t* hist_idx, int64_t num_users, int splits, void* ws, int64_t ws_bytes,
                           int32_t* out_rank, void* stream, const int32_t* filter_ids = nullptr,
                           int64_t fid_stride = 0, const uint32_t* filter_bits = nullptr, int64_t filter_ld = 0,
                           int num_filters = 0) {
  const int ld_mult = ek == kF32 ? 4 : ek == kBF16 ? 8 : 16;  // a row stride of whole 16-byte chunks
  RS_CHECK_ARG(U && items && target_col && out_rank && B >= 0,
               "rs_target_rank: null U / items / target_col / out_rank or B < 0");
  RS_CHECK_ARG(D >= 16 && D <= 256 && D % 16 == 0,
               "rs_target_rank: D = %d, must be a multiple of 16 in [16, 256]", D);
  RS_CHECK_ARG(N >= 1 && N < (int64_t)1 << 31, "rs_target_rank: bad sizes (N=%lld; 1 <= N < 2^31)", (long long)N);
  RS_CHECK_ARG(ldu >= D && ldu % 4 == 0 && ldi >= D && ldi % ld_mult == 0 && aligned16(U) &&
                   aligned16(items),
               "rs_target_rank: rows of U and items must be 16-byte aligned, ld >= D");
  FtFilter flt;
  RS_RET_IF(filter_args("rs_target_rank_filtered", filter_ids, fid_stride, filter_bits, filter_ld, num_filters, N,
                        &flt));
  if (splits <= 0) splits = rs_target_rank_splits(B, N, D);
  RS_CHECK_ARG(splits <= N, "rs_target_rank: splits = %d leaves a split no column (N=%lld)", splits, (long long)N);
  const int64_t need = splits > 1 ? rs_target_rank_ws_bytes(B, N, D, splits) : 0;
  RS_CHECK_ARG(splits == 1 || (ws && ws_bytes >= need),
               "rs_target_rank: workspace of %lld bytes, needs %lld (rs_target_rank_ws_bytes)",
               (long long)ws_bytes, (long long)need);
  if (B == 0) return 0;
  TrArgs a;
  a.U = U; a.ldu = ldu; a.B = B;
  a.items = items; a.ldi = ldi; a.N = (int)N; a.D = D; a.item_exp = item_exp;
  a.target_col = target_col; a.tc_stride = tc_stride;
  a.user_ids = user_ids; a.uid_stride = uid_stride; a.hist_off = hist_off; a.hist_idx = hist_idx;
  a.num_users = num_users;
  a.splits = splits; a.split_cols = (int)(N / splits); a.nrt = cdiv(B, 128);
  a.f = flt; a.f.split_words = filter_split_words(flt, splits, 1);
  a.out = splits == 1 ? out_rank : static_cast<int32_t*>(ws);
  const int64_t grid = (int64_t)a.nrt * splits;
  RS_CHECK_ARG(grid < (int64_t)1 << 31, "rs_target_rank: grid too large");
  RS_RET_IF(ek == kF32    ? tr_launch<kF32>(a, (int)grid, as_stream(stream))
            : ek == kBF16 ? tr_launch<kBF16>(a, (int)grid, as_stream(stream))
                          : tr_launch<kE4M3>(a, (int)grid, as_stream(stream)));
  if (splits == 1) return 0;
  target_rank_reduce<<<cdiv(B, 256), 256, 0, as_stream(stream)>>>(a.out, splits, B, target_col, tc_stride, (int)N,
                                                                 out_rank);
  RS_CHECK_LAUNCH("rs_target_rank (reduce)");
  return 0;
}

extern "C" int rs_target_rank(const float* U, int64_t ldu, int B, const void* items, int items_bf16,
                              int64_t ldi, int64_t N, int D, const int32_t* target_col, int64_t tc_stride,
                              const int64_t* user_ids, int64_t uid_stride, const int64_t* hist_off,
                              const int32_t* hist_idx, int64_t num_users, int splits, void* ws,
                              int64_t ws_bytes, int32_t* out_rank, void* stream) {
  return target_rank_any(U, ldu, B, items, items_bf16 ? kBF16 : kF32, 0, ldi, N, D, target_col, tc_stride,
                         user_ids, uid_stride, hist_off, hist_idx, num_users, splits, ws, ws_bytes, out_rank,
                         stream);
}

extern "C" int rs_target_rank_e4m3(const float* U, int64_t ldu, int B, const void* items, int item_exp,
                                   int64_t ldi, int64_t N, int D, const int32_t* target_col, int64_t tc_stride,
                                   const int64_t* user_ids, int64_t uid_stride, const int64_t* hist_off,
                                   const int32_t* hist_idx, int64_t num_users, int splits, void* ws,
                                   int64_t ws_bytes, int32_t* out_rank, void* stream) {
  RS_CHECK_ARG(item_exp >= -kE4m3MaxExp && item_exp <= kE4m3MaxExp,
               "rs_target_rank_e4m3: item_exp = %d outside [-40, 40]", item_exp);
  return target_rank_any(U, ldu, B, items, kE4M3, item_exp, ldi, N, D, target_col, tc_stride, user_ids,
                         uid_stride, hist_off, hist_idx, num_users, splits, ws, ws_bytes, out_rank, stream);
}

extern "C" int rs_target_rank_filtered(const float* U, int64_t ldu, int B, const void* items, int item_kind,
                                       int item_exp, int64_t ldi, int64_t N, int D, const int32_t* target_col,
                                       int64_t tc_stride, const int64_t* user_ids, int64_t uid_stride,
                                       const int64_t* hist_off, const int32_t* hist_idx, int64_t num_users,
                                       const int32_t* filter_ids, int64_t fid_stride, const uint32_t* filter_bits,
                                       int64_t filter_ld, int num_filters, int splits, void* ws, int64_t ws_bytes,
                                       int32_t* out_rank, void* stream) {
  RS_CHECK_ARG(item_kind >= 0 && item_kind <= 2,
               "rs_target_rank_filtered: item_kind = %d (0 fp32, 1 bf16, 2 e4m3)", item_kind);
  RS_CHECK_ARG(item_kind != 2 || (item_exp >= -kE4m3MaxExp && item_exp <= kE4m3MaxExp),
               "rs_target_rank_filtered: item_exp = %d outside [-40, 40]", item_exp);
  return target_rank_any(U, ldu, B, items, item_kind == 0 ? kF32 : item_kind == 1 ? kBF16 : kE4M3,
                         item_kind == 2 ? item_exp : 0, ldi, N, D, target_col, tc_stride, user_ids, uid_stride,
                         hist_off, hist_idx, num_users, splits, ws, ws_bytes, out_rank, stream, filter_ids,
                         fid_stride, filter_bits, filter_ld, num_filters);
}

// ---- the e4m3 index format (e4m3.h): scale exponent, host encoder, device quantiser

namespace {
// one 16-byte chunk of a destination row a thread: 16 floats in, one 16-byte store
__global__ __launch_bounds__(256) void quantize_e4m3_kernel(const float* __restrict__ x, int64_t ldx, int64_t N,
                                                            int D, int exp, uint8_t* __restrict__ q,
                                                            int64_t ldq) {
  const int cpr = D / 16;  // 16-byte chunks of a destination row
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= N * cpr) return;
  const int64_t row = i / cpr;
  const int ch = (int)(i % cpr);
  const float sc = e4m3_pow2(exp);
  const float* p = x + row * ldx + 16 * ch;
  u32x4 w;
#pragma unroll
  for (int j = 0; j < 4; ++j) w[j] = e4m3_pack4(ld4(p + 4 * j) * sc);
  *reinterpret_cast<u32x4*>(q + row * ldq + 16 * ch) = w;
}
}  // namespace

extern "C" int rs_e4m3_exponent(float absmax) {
  uint32_t b;
  memcpy(&b, &absmax, 4);
  return e4m3_exponent_bits(b);
}

extern "C" int rs_e4m3_encode_host(const float* x, int64_t n, int exp, uint8_t* out) {
  RS_CHECK_ARG((x && out) || n == 0, "rs_e4m3_encode_host: null x / out");
  RS_CHECK_ARG(n >= 0 && exp >= -kE4m3MaxExp && exp <= kE4m3MaxExp,
               "rs_e4m3_encode_host: n = %lld < 0 or exp = %d outside [-40, 40]", (long long)n, exp);
  for (int64_t i = 0; i < n; ++i) out[i] = e4m3_encode_one(ldexpf(x[i], exp));
  return 0;
}

extern "C" int rs_quantize_e4m3(const float* x, int64_t ldx, int64_t N, int D, int exp, uint8_t* q, int64_t ldq,
                                void* stream) {
  RS_CHECK_ARG(x && q && N >= 0, "rs_quantize_e4m3: null x / q or N < 0");
  RS_CHECK_ARG(D >= 16 && D % 16 == 0, "rs_quantize_e4m3: D = %d, must be a positive multiple of 16", D);
  RS_CHECK_ARG(exp >= -kE4m3MaxExp && exp <= kE4m3MaxExp, "rs_quantize_e4m3: exp = %d outside [-40, 40]", exp);
  RS_CHECK_ARG(ldx >= D && ldx % 4 == 0 && ldq >= D && ldq % 16 == 0 && aligned16(x) && aligned16(q),
               "rs_quantize_e4m3: rows of x and q must be 16-byte aligned, ld >= D");
  if (N == 0) return 0;
  const int64_t blocks = (N * (D / 16) + 255) / 256;
  RS_CHECK_ARG(blocks < (int64_t)1 << 31, "rs_quantize_e4m3: too many rows");
  quantize_e4m3_kernel<<<(int)blocks, 256, 0, as_stream(stream)>>>(x, ldx, N, D, exp, q, ldq);
  RS_CHECK_LAUNCH("rs_quantize_e4m3");
  return 0;
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

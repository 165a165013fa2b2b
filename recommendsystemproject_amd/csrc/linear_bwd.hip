// One-pass backward of the sequence input (bf16 compute mode): SequenceFeatureProcessor's
//   x = drop_b(drop_a(cat W^T + b) + pos[l])
// from ONE stream over the token rows of dx [M, 64] and cat [M, dcat]:
//   y = dx * mask_b * mask_a   db += colsum(y)         (fp32, before rounding)
//   dW[64][dcat] += y^T cat    dcat = y W              (bf16 MFMA, fp32 accumulation)
// It replaces the write-back of seq_input_dropout_bwd_kernel, wgrad_bf16_kernel<64, 64> (a second
// read of dx) and the input-gradient rowgemm (a third): dx is never written. The positional
// gradient (the sum over samples of dx * mask_b) is rs_seq_input_pos_grad's (dropout.hip), a
// read-only pass in seq_input_dropout_bwd_kernel's sample order.
// Every output carries the bits of the kernels it replaces: the row split is wgrad_bf16_launch's
// (the same chunks meet the same MFMAs in the same order, the same number of partials meets the
// same reduce), and dcat uses rowgemm_bf16_kernel's k map and MFMA order.
// The same kernel with ONE mask is the attention out-projection's backward (rs_outproj_bwd_bf16):
// dx = dh1, cat = att, W = Wo; y = dh1 * mask is the dsa the FFN backward no longer stores.
//
// Shared pieces: the weight-gradient side of both kernels here (wave grid, transposed reads, MFMA
// order, partial-tile write, ordered column sum) is WgradTile (wgrad_tile.h), the one
// wgrad_bf16_kernel uses; the row split is wgrad_row_split (gemm_stream.h), the one
// wgrad_bf16_launch uses; the pipeline of both kernels is stream_two_sets below; the launch tail
// is reduce_partials. A kernel here adds its own loads, masks, input-gradient product and stores.
// A workgroup of 4 waves owns a row range; rows are staged 32 at a time through registers into
// row-major bf16 LDS images of y and cat (double buffered, two further chunks in flight in
// registers: one chunk per 4-wave workgroup does not cover the HBM latency). The masks are applied
// to the fp32 registers on the way (keep4 of element row * 64 + col: the draws of rs_dropout_*).
// dcat reads the y image as it lies (rows = MFMA columns, 16x16x32 MFMA with W on the row side, so
// a lane holds 4 consecutive output columns) against W fragments kept in registers for the whole
// kernel. Each workgroup writes one partial row [dW | db]; one fixed-order reduce job with two
// output ranges adds them to the gradients.
#include "common.h"
#include "gemm_stream.h"
#include "mfma.h"
#include "rng.h"
#include "wgrad_tile.h"

#include <type_traits>

namespace rs {

namespace {

constexpr int SB_D = 64;  // encoder width (dx columns)

// The pipeline of a workgroup's row range [r0, r1): chunk j lives in LDS buffer j & 1 and travels
// through register set j & 1, two chunks in flight in registers behind the one in LDS.
//   load_chunk(SET, c0)        requests the chunk at row c0 into register set SET
//   store_chunk(SET, buf, c0)  consumes set SET into LDS buffer buf (past the range: zeros)
//   step(NXT, buf, c0)         computes on buffer buf; then store_chunk(NXT, buf ^ 1, c0 + WB_BK):
//     the next chunk, requested two steps ago, whose loads are consumed BEFORE this chunk's global
//     stores are issued (stores and loads share vmcnt); then those stores; then
//     load_chunk(NXT, c0 + 3 * WB_BK) behind them, and a barrier
// Whole pairs in the loop, an odd last chunk after it: an exit between the two steps would give
// the wait counts a path on which the older register set looks like the newer one (vmcnt(0)).
typedef std::integral_constant<int, 0> set0;
typedef std::integral_constant<int, 1> set1;
template <class Load, class Store, class Step>
__device__ __forceinline__ void stream_two_sets(int r0, int r1, Load&& load_chunk, Store&& store_chunk,
                                                Step&& step) {
  load_chunk(set0{}, r0);
  store_chunk(set0{}, 0, r0);
  load_chunk(set1{}, r0 + WB_BK);
  load_chunk(set0{}, r0 + 2 * WB_BK);
  __syncthreads();
  int c0 = r0;
  for (; c0 + WB_BK < r1; c0 += 2 * WB_BK) {
    step(set1{}, 0, c0);
    step(set0{}, 1, c0 + WB_BK);
  }
  if (c0 < r1) step(set1{}, 0, c0);
}

struct SeqBwdArgs {
  const float* dx;   // [M][64]
  const float* cat;  // [M][ldcat]
  const float* W;    // [64][ldw]
  float* dcat;       // [M][NC]
  float* ws;         // [blocks][64*NC + 64]
  int M, NC, ldcat, ldw;
  float p;
  const int64_t* key;
  int site_a, site_b;
};

// NCP: dcat padded to a multiple of 32. ONE: a single mask (site_a; the out-projection's dropout1).
template <int NCP, bool ONE = false>
__global__ __launch_bounds__(256) void seq_input_bwd_bf16_kernel(SeqBwdArgs a, int rows_per_block) {
  typedef WgradTile<SB_D, NCP> Tile;
  constexpr int PY = Tile::PY, PX = Tile::PX;
  constexpr int NYS = WB_BK * SB_D / 4 / 256;  // dx float4 slots per thread (2)
  constexpr int NXS = WB_BK * NCP / 4 / 256;   // cat float4 slots per thread
  constexpr int NTW = NCP / 32;                // dcat column tiles (16 wide) per wave
  static_assert(NYS * 256 * 4 == WB_BK * SB_D && NXS * 256 * 4 == WB_BK * NCP, "whole slots");
  extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
  __bf16* Ys = reinterpret_cast<__bf16*>(smem_raw);  // [2][WB_BK][PY]
  __bf16* Xs = Ys + 2 * WB_BK * PY;                    // [2][WB_BK][PX]
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int NC = a.NC;
  const int r0 = blockIdx.x * rows_per_block;
  const int r1 = min(a.M, r0 + rows_per_block);
  const bool drop = a.p > 0.f;
  DropKey ka{}, kb{};
  if (drop) {
    ka = make_key(a.key, a.site_a, a.p);
    if constexpr (!ONE) kb = make_key(a.key, a.site_b, a.p);
  }
  typedef const __attribute__((address_space(1))) floatx4* gptr4;

  // W fragments of this wave's dcat tiles: lane (r, q) holds W[16q + 8u + e][16j + r]
  const int r = lane & 15, q = lane >> 4;
  const int rg = wave & 1;  // 16-row group of the chunk
  bf16x8 wf[NTW][2];
#pragma unroll
  for (int t = 0; t < NTW; ++t) {
    // unconditional loads (column clamped, scaled to zero after -- a select is turned back into
    // a guarded load, whose join waits for it)
    const int n = ((wave >> 1) + 2 * t) * 16 + r;
    const float* wp = a.W + min(n, NC - 1);
    const float wz = n < NC ? 1.f : 0.f;
    float w[2][8];
#pragma unroll
    for (int u = 0; u < 2; ++u)
#pragma unroll
      for (int e = 0; e < 8; ++e) w[u][e] = wp[(int64_t)(16 * q + 8 * u + e) * a.ldw];
#pragma unroll
    for (int u = 0; u < 2; ++u)
#pragma unroll
      for (int e = 0; e < 8; ++e) wf[t][u][e] = (__bf16)(w[u][e] * wz);
  }

  floatx4 sy[2][NYS], sx[2][NXS];  // two chunks in flight behind the one in LDS
  float ysum[NYS][4];
#pragma unroll
  for (int i = 0; i < NYS; ++i)
#pragma unroll
    for (int e = 0; e < 4; ++e) ysum[i][e] = 0.f;
  // unconditional loads, row and column clamped (store_chunk zeroes what lies outside): no branch
  // whose join would wait for them
  auto load_chunk = [&](auto SET, int c0) {
    constexpr int S = decltype(SET)::value;
#pragma unroll
    for (int i = 0; i < NYS; ++i) {
      const int s = tid + i * 256;
      const int m = min(c0 + s / (SB_D / 4), r1 - 1), c = (s % (SB_D / 4)) * 4;
      sy[S][i] = *(gptr4)(a.dx + (int64_t)m * SB_D + c);
    }
#pragma unroll
    for (int i = 0; i < NXS; ++i) {
      const int s = tid + i * 256;
      const int m = min(c0 + s / (NCP / 4), r1 - 1), c = min((s % (NCP / 4)) * 4, NC - 4);
      sx[S][i] = *(gptr4)(a.cat + (int64_t)m * a.ldcat + c);
    }
  };
  // masks and bias sums on the fp32 registers, then one rounding to bf16
  auto store_chunk = [&](auto SET, int buf, int c0) {
    constexpr int S = decltype(SET)::value;
#pragma unroll
    for (int i = 0; i < NYS; ++i) {
      const int s = tid + i * 256;
      const int kk = s / (SB_D / 4), c = (s % (SB_D / 4)) * 4, m = c0 + kk;
      floatx4 v = m < r1 ? sy[S][i] : floatx4{0.f, 0.f, 0.f, 0.f};
      float ma[4] = {1.f, 1.f, 1.f, 1.f};
      if (drop) {
        const uint64_t e0 = (uint64_t)m * SB_D + c;
        if constexpr (!ONE) {
          float mb[4];
          keep4(kb, e0, mb);
#pragma unroll
          for (int e = 0; e < 4; ++e) v[e] *= mb[e];
        }
        keep4(ka, e0, ma);
      }
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        v[e] *= ma[e];
        ysum[i][e] += v[e];
      }
      put4(&Ys[(buf * WB_BK + kk) * PY + c], v);
    }
#pragma unroll
    for (int i = 0; i < NXS; ++i) {
      const int s = tid + i * 256;
      const int kk = s / (NCP / 4), c = (s % (NCP / 4)) * 4;
      put4(&Xs[(buf * WB_BK + kk) * PX + c], c0 + kk < r1 && c < NC ? sx[S][i] : floatx4{0.f, 0.f, 0.f, 0.f});
    }
  };
  Tile tile(tid);
  auto step = [&](auto NXT, int buf, int c0) {
    const __bf16* Y = Ys + buf * WB_BK * PY;
    tile.product(Y, Xs + buf * WB_BK * PX);
    // dcat rows 16*rg .. +15 of the chunk, this wave's column tiles
    floatx4 dacc[NTW];
    {
      bf16x8 yf[2];
#pragma unroll
      for (int u = 0; u < 2; ++u) yf[u] = *reinterpret_cast<const bf16x8*>(Y + (16 * rg + r) * PY + 16 * q + 8 * u);
#pragma unroll
      for (int t = 0; t < NTW; ++t) {
        dacc[t] = floatx4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int u = 0; u < 2; ++u)
          dacc[t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wf[t][u], yf[u], dacc[t], 0, 0, 0);
      }
    }
    store_chunk(NXT, buf ^ 1, c0 + WB_BK);  // before this chunk's dcat stores (stream_two_sets)
    {
      const int m = c0 + 16 * rg + r;
#pragma unroll
      for (int t = 0; t < NTW; ++t) {
        const int n0 = ((wave >> 1) + 2 * t) * 16 + 4 * q;
        if (m < r1 && n0 < NC) *reinterpret_cast<floatx4*>(a.dcat + (int64_t)m * NC + n0) = dacc[t];
      }
    }
    load_chunk(NXT, c0 + 3 * WB_BK);
    __syncthreads();
  };
  stream_two_sets(r0, r1, load_chunk, store_chunk, step);
  // partial row of this workgroup: [dW 64 x NC | db 64]; the column partials go through the
  // staging LDS
  float* out = a.ws + (int64_t)blockIdx.x * (SB_D * NC + SB_D);
  tile.write(out, SB_D, NC);
  const float rsum = Tile::column_sum(reinterpret_cast<float*>(smem_raw), ysum, tid, SB_D);
  if (tid < SB_D) out[SB_D * NC + tid] = rsum;
}

int seq_bwd_pad(int NC) { return (NC + 31) / 32 * 32; }

// The launch tail of every entry point here: dW += the sum of the nblk partial rows' [Mo x No]
// parts, db += that of their [Mo] parts, in one fixed-order reduce job with two output ranges.
int reduce_partials(const float* ws, int nblk, int Mo, int No, float* dW, float* db, hipStream_t st) {
  float* outs[2] = {dW, db};
  const int begins[2] = {0, Mo * No};
  const float one[2] = {1.f, 1.f};
  return reduce_job(ws, nblk, Mo * No + Mo, 2, outs, begins, one, one, st);
}

bool seq_bwd_shape_ok(int M, int d, int NC) {
  return M >= 1 && d == SB_D && NC >= 8 && NC <= 96 && NC % 8 == 0;
}


// ------------------------------------------------------------------ in-projection backward
// dW[192][64] += dY^T X, db += colsum(dY), dx = dY W (+ dx_in) from ONE read of dY = dqkv
// [M, 192] (bf16 storage): the pair it replaces (wgrad_bf16_kernel<192, 64, true, false> and the
// input-gradient rowgemm) streamed dqkv twice. The same pipeline as above without the masks: the
// dY image feeds the weight gradient through transposed reads and dx through plain row reads
// against a bf16 image of W staged once ([n][k], K = 192). The residual rows (dx_in, which may be
// dx itself: every element is read and later written by the same lane) travel with the chunk's
// prefetch, so waiting for them never drains newer loads.
constexpr int LB_N = 192, LB_K = 64;  // dY columns (GEMM K of dx), X / dx columns

struct LinBwdArgs {
  const __bf16* dy;    // [M][192]
  const float* x;      // [M][64]
  const float* W;      // [192][ldw]
  const float* dx_in;  // [M][64] or null
  float* dx;           // [M][64]
  float* ws;           // [blocks][192*64 + 192]
  int M, ldw;
};

template <bool RES>
__global__ __launch_bounds__(256) void linear_bwd_bf16_kernel(LinBwdArgs a, int rows_per_block) {
  typedef WgradTile<LB_N, LB_K> Tile;
  constexpr int PY = Tile::PY, PX = Tile::PX, PW = LB_N + 8;
  constexpr int NYS = WB_BK * LB_N / 8 / 256;  // dY 16-byte slots (8 bf16) per thread (3)
  constexpr int NXS = WB_BK * LB_K / 4 / 256;  // X float4 slots per thread (2)
  constexpr int KC = LB_N / 64;                // 64-wide k chunks of the dx product
  static_assert(NYS * 256 * 8 == WB_BK * LB_N && NXS * 256 * 4 == WB_BK * LB_K, "whole slots");
  extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
  __bf16* Ys = reinterpret_cast<__bf16*>(smem_raw);  // [2][WB_BK][PY]
  __bf16* Xs = Ys + 2 * WB_BK * PY;                    // [2][WB_BK][PX]
  __bf16* Wt = Xs + 2 * WB_BK * PX;                    // [64][PW]: Wt[n][k] = W[k][n]
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int r0 = blockIdx.x * rows_per_block;
  const int r1 = min(a.M, r0 + rows_per_block);
  const int r = lane & 15, q = lane >> 4;
  const int rg = wave & 1;  // 16-row group of the chunk; column tiles (wave >> 1) and (wave >> 1) + 2
  typedef const __attribute__((address_space(1))) floatx4* gptr4;
  typedef const __attribute__((address_space(1))) u32x4* gptru4;

  {  // W -> bf16 [n][k] (host: ldw % 4 == 0, 16-byte aligned)
    floatx4 w[LB_N * LB_K / 4 / 256];
#pragma unroll
    for (int i = 0; i < LB_N * LB_K / 4 / 256; ++i) {
      const int s = tid + i * 256;
      w[i] = *(gptr4)(a.W + (int64_t)(s / (LB_K / 4)) * a.ldw + (s % (LB_K / 4)) * 4);
    }
#pragma unroll
    for (int i = 0; i < LB_N * LB_K / 4 / 256; ++i) {
      const int s = tid + i * 256;
      const int k = s / (LB_K / 4), n = (s % (LB_K / 4)) * 4;
#pragma unroll
      for (int e = 0; e < 4; ++e) Wt[(n + e) * PW + k] = (__bf16)w[i][e];
    }
  }

  u32x4 sy[2][NYS];
  floatx4 sx[2][NXS], sr[2][RES ? 2 : 1], res[RES ? 2 : 1];
  float ysum[NYS][8];
#pragma unroll
  for (int i = 0; i < NYS; ++i)
#pragma unroll
    for (int e = 0; e < 8; ++e) ysum[i][e] = 0.f;
  auto load_chunk = [&](auto SET, int c0) {
    constexpr int S = decltype(SET)::value;
#pragma unroll
    for (int i = 0; i < NYS; ++i) {
      const int s = tid + i * 256;
      const int m = min(c0 + s / (LB_N / 8), r1 - 1), c = (s % (LB_N / 8)) * 8;
      sy[S][i] = *(gptru4)(a.dy + (int64_t)m * LB_N + c);
    }
#pragma unroll
    for (int i = 0; i < NXS; ++i) {
      const int s = tid + i * 256;
      const int m = min(c0 + s / (LB_K / 4), r1 - 1), c = (s % (LB_K / 4)) * 4;
      sx[S][i] = *(gptr4)(a.x + (int64_t)m * LB_K + c);
    }
    if constexpr (RES) {
      const int m = min(c0 + 16 * rg + r, r1 - 1);
#pragma unroll
      for (int t = 0; t < 2; ++t)
        sr[S][t] = *(gptr4)(a.dx_in + (int64_t)m * LB_K + ((wave >> 1) + 2 * t) * 16 + 4 * q);
    }
  };
  auto store_chunk = [&](auto SET, int buf, int c0) {
    constexpr int S = decltype(SET)::value;
#pragma unroll
    for (int i = 0; i < NYS; ++i) {
      const int s = tid + i * 256;
      const int kk = s / (LB_N / 8), c = (s % (LB_N / 8)) * 8;
      const u32x4 v = c0 + kk < r1 ? sy[S][i] : u32x4{0u, 0u, 0u, 0u};
      const bf16x8 hv = __builtin_bit_cast(bf16x8, v);
#pragma unroll
      for (int e = 0; e < 8; ++e) ysum[i][e] += (float)hv[e];
      *reinterpret_cast<u32x4*>(&Ys[(buf * WB_BK + kk) * PY + c]) = v;
    }
#pragma unroll
    for (int i = 0; i < NXS; ++i) {
      const int s = tid + i * 256;
      const int kk = s / (LB_K / 4), c = (s % (LB_K / 4)) * 4;
      put4(&Xs[(buf * WB_BK + kk) * PX + c], c0 + kk < r1 ? sx[S][i] : floatx4{0.f, 0.f, 0.f, 0.f});
    }
    if constexpr (RES) {
#pragma unroll
      for (int t = 0; t < 2; ++t) res[t] = sr[S][t];
    }
  };
  Tile tile(tid);
  auto step = [&](auto NXT, int buf, int c0) {
    const __bf16* Y = Ys + buf * WB_BK * PY;
    tile.product(Y, Xs + buf * WB_BK * PX);
    // dx rows 16*rg .. +15 of the chunk, two column tiles per wave, K = 192
    floatx4 dacc[2];
#pragma unroll
    for (int t = 0; t < 2; ++t) dacc[t] = floatx4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int c = 0; c < KC; ++c)
#pragma unroll
      for (int u = 0; u < 2; ++u) {
        const bf16x8 yf = *reinterpret_cast<const bf16x8*>(Y + (16 * rg + r) * PY + 64 * c + 16 * q + 8 * u);
#pragma unroll
        for (int t = 0; t < 2; ++t) {
          const bf16x8 wf = *reinterpret_cast<const bf16x8*>(Wt + (((wave >> 1) + 2 * t) * 16 + r) * PW + 64 * c + 16 * q + 8 * u);
          dacc[t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wf, yf, dacc[t], 0, 0, 0);
        }
      }
    if constexpr (RES) {
#pragma unroll
      for (int t = 0; t < 2; ++t) dacc[t] += res[t];
    }
    store_chunk(NXT, buf ^ 1, c0 + WB_BK);  // before this chunk's dx stores (stream_two_sets)
    {
      const int m = c0 + 16 * rg + r;
#pragma unroll
      for (int t = 0; t < 2; ++t)
        if (m < r1) *reinterpret_cast<floatx4*>(a.dx + (int64_t)m * LB_K + ((wave >> 1) + 2 * t) * 16 + 4 * q) = dacc[t];
    }
    load_chunk(NXT, c0 + 3 * WB_BK);
    __syncthreads();
  };
  stream_two_sets(r0, r1, load_chunk, store_chunk, step);
  // partial row of this workgroup: [dW 192 x 64 | db 192]; the column partials go over the dY images
  float* out = a.ws + (int64_t)blockIdx.x * (LB_N * LB_K + LB_N);
  tile.write(out, LB_N, LB_K);
  const float rsum = Tile::column_sum(reinterpret_cast<float*>(smem_raw), ysum, tid, LB_N);
  if (tid < LB_N) out[LB_N * LB_K + tid] = rsum;
}

// 65 KB of dynamic LDS (40 KB of staging, 25 KB of W): above the 64 KB of the CDNA parts before
// gfx950, within its 160 KB (two workgroups per CU); the library is built for gfx950 only, and
// RS_CHECK_LAUNCH reports a launch that any other target would refuse
size_t lin_bwd_lds() {
  return wb_stage_bytes(LB_N, LB_K) + (size_t)LB_K * (LB_N + 8) * 2;
}

}  // namespace
}  // namespace rs

using namespace rs;

extern "C" int rs_seq_input_bwd_bf16_supported(int M, int d, int dcat) {
  return seq_bwd_shape_ok(M, d, dcat) ? 1 : 0;
}

extern "C" int64_t rs_seq_input_bwd_bf16_ws_bytes(int M, int d, int dcat) {
  if (!seq_bwd_shape_ok(M, d, dcat)) return 0;
  return (int64_t)wgrad_row_split(M, WB_BK).blocks * ((int64_t)d * dcat + d) * (int64_t)sizeof(float);
}

extern "C" int rs_seq_input_bwd_bf16(const float* dx, const float* cat, int ldcat, const float* W, int ldw,
                                     int M, int d, int dcat, float p, const int64_t* key, int site_a,
                                     int site_b, float* dcat_out, float* dW, float* db, float* ws,
                                     void* stream) {
  RS_CHECK_ARG(M >= 0 && d == SB_D && dcat >= 8 && dcat <= 96 && dcat % 8 == 0,
               "rs_seq_input_bwd_bf16: need d == 64 and dcat a multiple of 8 up to 96 (d=%d dcat=%d)", d, dcat);
  if (M == 0) return 0;
  RS_CHECK_ARG(dx && cat && W && dcat_out && dW && db && ws, "rs_seq_input_bwd_bf16: null operand");
  RS_CHECK_ARG(p >= 0.f && p < 1.f && (p == 0.f || key), "rs_seq_input_bwd_bf16: 0 <= p < 1, key with p > 0");
  RS_CHECK_ARG(aligned16(dx) && aligned16(cat) && aligned16(dcat_out) && aligned16(ws) && ldcat >= dcat &&
                   ldcat % 4 == 0 && ldw >= dcat,
               "rs_seq_input_bwd_bf16: misaligned operand");
  SeqBwdArgs a{};
  a.dx = dx; a.cat = cat; a.W = W; a.dcat = dcat_out; a.ws = ws;
  a.M = M; a.NC = dcat; a.ldcat = ldcat; a.ldw = ldw;
  a.p = p; a.key = key; a.site_a = site_a; a.site_b = site_b;
  const RowSplit sp = wgrad_row_split(M, WB_BK);
  const int rpb = sp.rows_per_block, nblk = sp.blocks;
  const size_t lds = wb_stage_bytes(SB_D, seq_bwd_pad(dcat));
  hipStream_t st = as_stream(stream);
  switch (seq_bwd_pad(dcat)) {
    case 32: seq_input_bwd_bf16_kernel<32><<<nblk, 256, lds, st>>>(a, rpb); break;
    case 64: seq_input_bwd_bf16_kernel<64><<<nblk, 256, lds, st>>>(a, rpb); break;
    default: seq_input_bwd_bf16_kernel<96><<<nblk, 256, lds, st>>>(a, rpb); break;
  }
  RS_CHECK_LAUNCH("rs_seq_input_bwd_bf16");
  return reduce_partials(ws, nblk, d, dcat, dW, db, st);
}

// The attention out-projection's backward on the same kernel: dh = dh1 (norm1's backward, only
// read), x = att, W = Wo [64][ldw]; y = dh * keep4(site) is the dsa that ffn_bwd_bf16_kernel used to
// store for wgrad_bf16_kernel<64, 64> and the input-gradient rowgemm, whose bits these outputs carry.
extern "C" int64_t rs_outproj_bwd_bf16_ws_bytes(int M, int d) { return rs_seq_input_bwd_bf16_ws_bytes(M, d, SB_D); }

extern "C" int rs_outproj_bwd_bf16(const float* dh, const float* x, const float* W, int ldw, int M, int d,
                                   float p, const int64_t* key, int site, float* dx, float* dW, float* db,
                                   float* ws, void* stream) {
  RS_CHECK_ARG(M >= 0 && d == SB_D, "rs_outproj_bwd_bf16: need d == 64 (d=%d)", d);
  if (M == 0) return 0;
  RS_CHECK_ARG(dh && x && W && dx && dW && db && ws, "rs_outproj_bwd_bf16: null operand");
  RS_CHECK_ARG(p >= 0.f && p < 1.f && (p == 0.f || key), "rs_outproj_bwd_bf16: 0 <= p < 1, key with p > 0");
  RS_CHECK_ARG(aligned16(dh) && aligned16(x) && aligned16(dx) && aligned16(ws) && ldw >= d,
               "rs_outproj_bwd_bf16: misaligned operand");
  RS_CHECK_ARG(dx != dh && dx != x, "rs_outproj_bwd_bf16: dx may not alias an input");
  SeqBwdArgs a{};
  a.dx = dh; a.cat = x; a.W = W; a.dcat = dx; a.ws = ws;
  a.M = M; a.NC = SB_D; a.ldcat = SB_D; a.ldw = ldw;
  a.p = p; a.key = key; a.site_a = site; a.site_b = site;
  const RowSplit sp = wgrad_row_split(M, WB_BK);
  const int rpb = sp.rows_per_block, nblk = sp.blocks;
  hipStream_t st = as_stream(stream);
  seq_input_bwd_bf16_kernel<SB_D, true><<<nblk, 256, wb_stage_bytes(SB_D, SB_D), st>>>(a, rpb);
  RS_CHECK_LAUNCH("rs_outproj_bwd_bf16");
  return reduce_partials(ws, nblk, SB_D, SB_D, dW, db, st);
}

extern "C" int64_t rs_linear_bwd_bf16_ws_bytes(int M, int N, int K) {
  if (M < 1 || N != LB_N || K != LB_K) return 0;
  return (int64_t)wgrad_row_split(M, WB_BK).blocks * (LB_N * LB_K + LB_N) * (int64_t)sizeof(float);
}

extern "C" int rs_linear_bwd_bf16(const void* dy, const float* x, const float* W, int ldw, int M, int N, int K,
                                  const float* dx_in, float* dx, float* dW, float* db, float* ws,
                                  void* stream) {
  RS_CHECK_ARG(M >= 0 && N == LB_N && K == LB_K, "rs_linear_bwd_bf16: need N == 192 and K == 64 (N=%d K=%d)", N, K);
  if (M == 0) return 0;
  RS_CHECK_ARG(dy && x && W && dx && dW && db && ws, "rs_linear_bwd_bf16: null operand");
  RS_CHECK_ARG(aligned16(dy) && aligned16(x) && aligned16(W) && aligned16(dx) && aligned16(ws) &&
                   (!dx_in || aligned16(dx_in)) && ldw >= K && ldw % 4 == 0,
               "rs_linear_bwd_bf16: misaligned operand");
  LinBwdArgs a{};
  a.dy = reinterpret_cast<const __bf16*>(dy); a.x = x; a.W = W; a.dx_in = dx_in; a.dx = dx; a.ws = ws;
  a.M = M; a.ldw = ldw;
  const RowSplit sp = wgrad_row_split(M, WB_BK);
  const int rpb = sp.rows_per_block, nblk = sp.blocks;
  hipStream_t st = as_stream(stream);
  if (dx_in) linear_bwd_bf16_kernel<true><<<nblk, 256, lin_bwd_lds(), st>>>(a, rpb);
  else linear_bwd_bf16_kernel<false><<<nblk, 256, lin_bwd_lds(), st>>>(a, rpb);
  RS_CHECK_LAUNCH("rs_linear_bwd_bf16");
  return reduce_partials(ws, nblk, LB_N, LB_K, dW, db, st);
}

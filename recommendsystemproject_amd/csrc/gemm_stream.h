// Shared between gemm.hip (dispatch) and gemm_stream.hip (streaming kernels): ONE definition of
// the launch arguments, so both translation units agree on the layout.
#pragma once
#include "common.h"

namespace rs {

struct StreamArgs {
  int M, N, K;
  float alpha, beta;
  const float* A; int lda;
  const float* B; int ldb;
  float* C; int ldc;
  int epi;
  const float* bias;
  const float* aux; int ld_aux, aux_mod;
  float* rowsum;
  float* ws;
  int transB;
  int vec_epi;  // rowgemm: C / aux / bias rows 16-byte addressable -> float4 epilogue I/O
  float drop_p;
  const int64_t* drop_key;
  int site_a, site_b;
  // fused residual + LayerNorm epilogue (rowgemm LN instances, N == 64):
  //   h = drop_a(alpha*acc + bias) + aux  -> C;   y = LN(h) * gamma + beta -> ln_y
  const float* ln_gamma;
  const float* ln_beta;
  float* ln_y;
  float* ln_mean;
  float* ln_rstd;
  float ln_eps;
  // LN instances, optional: the residual row of output row m is aux row m * aux_bag + aux_rows[m]
  // (the pruned last encoder layer reads x[b, last[b]] in place instead of a gathered copy)
  const int64_t* aux_rows;
  int aux_bag;
};

// bf16: the call is in the bf16 compute mode (RS_GEMM_BF16), which has one more shape
bool rowgemm_supported(int transA, int M, int N, int K, const float* A, int lda, bool bf16 = false);
int rowgemm_launch(const StreamArgs& s, hipStream_t st);
bool rowgemm_ln_supported(int M, int N, int K, const float* A, int lda);
int rowgemm_ln_launch(const StreamArgs& s, hipStream_t st);
bool wgrad_instance(int M, int N);  // an instance exists for this (padded) dW tile
bool wgrad_supported(int transA, int transB, int M, int N, int K, const float* A, int lda,
                     const float* B, int ldb, int ldc, int epi);
int64_t wgrad_ws_bytes(int M, int N, int K);
int wgrad_launch(const StreamArgs& s, hipStream_t st);
// bf16 MFMA weight gradient; y_bf16 / x_bf16: dY (A) / X (B) are stored as bf16
int wgrad_bf16_launch(const StreamArgs& s, bool y_bf16, bool x_bf16, hipStream_t st);

// The row split of every weight-gradient kernel (fp32, bf16, and linear_bwd.hip's one-pass
// backwards): workgroups of rows_per_block rows, whole chunks of bk rows each; `blocks` partial
// tiles meet the fixed-order reduce. A fused backward has the bits of the pair it replaces only
// while both use this split, and the *_ws_bytes sizes follow it. max_blocks bounds `blocks` for
// any chunk height (rs_wgrad_ws_bytes sizes for either kernel).
struct RowSplit { int rows_per_block, blocks, max_blocks; };
RowSplit wgrad_row_split(int rows, int bk);

// bf16 weight-gradient geometry (wgrad_tile.h: the tile of wgrad_bf16_kernel and of the one-pass
// backwards)
constexpr int WB_BK = 32;  // rows per staged chunk

// LDS row pitch (bf16 elements) for a pad-wide image: the 4 rows of one transposed read must
// fall in distinct 64-byte windows of the 256-byte bank space -> pitch*2 mod 256 in {64, 192}
constexpr int wb_pitch(int pad) { return (pad % 128 == 32 || pad % 128 == 96) ? pad : pad + 32; }

// wave grid over the (MO/32) x (NO/32) tiles: the split of 4 waves with the fewest fragments
constexpr int wb_gm(int tm, int tn) {
  int best = 1, cost = 1 << 30;
  for (int gm = 1; gm <= 4; gm *= 2) {
    const int gn = 4 / gm;
    const int c = (tm + gm - 1) / gm + (tn + gn - 1) / gn + 64 * ((tm < gm) + (tn < gn));
    if (c < cost) { cost = c; best = gm; }
  }
  return best;
}

// bytes of the double-buffered bf16 staging images of Y [WB_BK][mo_pad] and X [WB_BK][no_pad]
constexpr size_t wb_stage_bytes(int mo_pad, int no_pad) {
  return (size_t)2 * WB_BK * (wb_pitch(mo_pad) + wb_pitch(no_pad)) * 2;
}

}  // namespace rs

// The weight-gradient tile of the bf16 streaming backwards (device only): dW[MO_PAD][NO_PAD] =
// Y^T X of a workgroup of 4 waves over row-major bf16 LDS images of Y and X, WB_BK rows at a time.
// wgrad_bf16_kernel (gemm_stream.hip) and the one-pass backwards (linear_bwd.hip) stage their
// chunks in their own ways and share everything behind the images: the wave grid, the transposed
// reads, the MFMA order, the partial-tile write and the bias gradient's ordered column sum. One
// definition, so a fused backward has the bits of wgrad_bf16_kernel by construction (given the
// same row split: wgrad_row_split, gemm_stream.h).
#pragma once
#include "gemm_stream.h"
#include "mfma.h"

namespace rs {

template <int MO_PAD, int NO_PAD>
struct WgradTile {
  static constexpr int PY = wb_pitch(MO_PAD), PX = wb_pitch(NO_PAD);  // image pitches (bf16)
  static constexpr int TMT = MO_PAD / 32, TNT = NO_PAD / 32;
  static constexpr int GM = wb_gm(TMT, TNT), GN = 4 / GM;  // wave grid
  static constexpr int TM = (TMT + GM - 1) / GM, TN = (TNT + GN - 1) / GN;  // 32x32 tiles per wave

  int lane, wm, wn;
  // transposed-read addresses: lane 4q+p of 16-lane group g reads row q (+4 for the second
  // half of the fragment) of the block, columns 4p..4p+3 of the 16-column half (g & 1);
  // rows 8h.. with h = g >> 1
  int trow, tcol;
  floatx16 acc[TM][TN];

  __device__ __forceinline__ explicit WgradTile(int tid) {
    lane = tid & 63;
    const int wave = tid >> 6;
    wm = wave / GN;
    wn = wave % GN;
    const int g = lane >> 4, lq = (lane & 15) >> 2, lp = lane & 3;
    trow = 8 * (g >> 1) + lq;
    tcol = 16 * (g & 1) + 4 * lp;
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
      for (int j = 0; j < TN; ++j)
#pragma unroll
        for (int e = 0; e < 16; ++e) acc[i][j][e] = 0.f;
  }

  // acc += Y^T X of one staged chunk: Y [WB_BK][PY], X [WB_BK][PX]
  __device__ __forceinline__ void product(const __bf16* Y, const __bf16* X) {
#pragma unroll
    for (int ks = 0; ks < WB_BK / 16; ++ks) {
      bf16x8 af[TM], bfr[TN];
#pragma unroll
      for (int i = 0; i < TM; ++i) {
        const int ti = wm * TM + i;
        const __bf16* p = Y + (16 * ks + trow) * PY + 32 * (ti < TMT ? ti : 0) + tcol;
        af[i] = tr_frag(p, p + 4 * PY);
      }
#pragma unroll
      for (int j = 0; j < TN; ++j) {
        const int tj = wn * TN + j;
        const __bf16* p = X + (16 * ks + trow) * PX + 32 * (tj < TNT ? tj : 0) + tcol;
        bfr[j] = tr_frag(p, p + 4 * PX);
      }
#pragma unroll
      for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int j = 0; j < TN; ++j)
          acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(af[i], bfr[j], acc[i][j], 0, 0, 0);
    }
  }

  // this workgroup's partial tile -> out[Mo][No]. Of a 32x32 accumulator a lane holds column
  // lane & 31 and, in element e, row (e & 3) + 8 * (e >> 2) + 4 * (lane >> 5). Compile-time Mo / No
  // that cover the padded tile fold the bounds checks away. (wgrad_kernel, the fp32 kernel, keeps
  // its own copy of this row map: its tiles are dealt to the waves differently, and going through
  // a shared function changed its code.)
  __device__ __forceinline__ void write(float* out, int Mo, int No) const {
#pragma unroll
    for (int i = 0; i < TM; ++i) {
      const int ti = wm * TM + i;
      if (ti >= TMT) continue;
#pragma unroll
      for (int j = 0; j < TN; ++j) {
        const int tj = wn * TN + j;
        if (tj >= TNT) continue;
        const int n = tj * 32 + (lane & 31);
        if (n >= No) continue;
#pragma unroll
        for (int e = 0; e < 16; ++e) {
          const int m = ti * 32 + (e & 3) + 8 * (e >> 2) + 4 * (lane >> 5);
          if (m < Mo) out[(int64_t)m * No + n] = acc[i][j][e];
        }
      }
    }
  }

  // Bias gradient: the threads' column partials (slot i of thread tid covers the V consecutive
  // elements from (tid + 256 i) V of the [WB_BK][MO_PAD] chunk; V = 4 for fp32, 8 for bf16 storage)
  // -> R[kk][c] (which may lie over the staging images: all reads of them are behind a barrier),
  // then the rows summed in order. Returns column tid's sum to the threads tid < Mo.
  template <int NYS, int V>
  static __device__ __forceinline__ float column_sum(float* R, const float (&ysum)[NYS][V], int tid, int Mo) {
    static_assert(NYS * 256 * V == WB_BK * MO_PAD && V % 4 == 0, "whole slots");
#pragma unroll
    for (int i = 0; i < NYS; ++i)
#pragma unroll
      for (int h = 0; h < V / 4; ++h)
        *reinterpret_cast<floatx4*>(R + (tid + i * 256) * V + 4 * h) =
            floatx4{ysum[i][4 * h], ysum[i][4 * h + 1], ysum[i][4 * h + 2], ysum[i][4 * h + 3]};
    __syncthreads();
    float rsum = 0.f;
    if (tid < Mo) {
#pragma unroll 8
      for (int kk = 0; kk < WB_BK; ++kk) rsum += R[kk * MO_PAD + tid];
    }
    return rsum;
  }
};

}  // namespace rs

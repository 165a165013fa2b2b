// A chained product from rows a wave already holds (device only): the next Linear of a 16-row
// group computed from the previous kernel stage's epilogue registers, so the rows are not read
// back from HBM by a kernel of their own.
//
// The streaming kernels end a step with lane (r = lane & 15, q = lane >> 4) holding row r of the
// wave's 16-row group at columns 16t + 4q + e (t < 4, e < 4): the C/D map of four 16x16 MFMA
// tiles with the weights on the row side. A following K = 64 product wants row r at
// k = 16q .. 16q + 15 (rowgemm_bf16_kernel's k map). rows_to_operand takes the rows through a
// per-wave LDS tile [16][CH_DP] bf16 from the one layout to the other; chain_linear_bf16 then
// computes rows . W^T + b against an LDS weight image [NT * 16][CH_DP] and stores bf16.
//
// The bits are those of rowgemm_bf16_kernel<NT, 1, false, RS_EPI_BIAS, bf16 C> fed the stored fp32
// rows: the same rounding point (the fp32 value that is stored, rounded to nearest even), the same
// k split (MFMA 0: k = 16q .. 16q+7, MFMA 1: the next 8), the same MFMA order per accumulator
// and the same bias add. No k permutation here: it would change the summation order.
#pragma once
#include "mfma.h"

namespace rs {

constexpr int CH_D = 64;         // row width
constexpr int CH_DP = CH_D + 8;  // LDS pitch (bf16): conflict-free 16-byte reads

constexpr size_t chain_tile_bytes(int waves) { return (size_t)waves * 16 * CH_DP * 2; }
constexpr size_t chain_weight_bytes(int n) { return (size_t)n * CH_DP * 2 + (size_t)n * 4; }

// tile_row: this lane's row r of its wave's tile. One wave writes and reads its own tile, and LDS
// executes a wave's operations in order: no barrier (EXEC full, every lane takes part).
__device__ __forceinline__ void rows_to_operand(__bf16* tile_row, const floatx4 (&rows)[4], int q,
                                                bf16x8 (&af)[2]) {
#pragma unroll
  for (int t = 0; t < 4; ++t) put4(tile_row + 16 * t + 4 * q, rows[t]);
  asm volatile("" ::: "memory");
  af[0] = *reinterpret_cast<const bf16x8*>(tile_row + 16 * q);
  af[1] = *reinterpret_cast<const bf16x8*>(tile_row + 16 * q + 8);
  asm volatile("" ::: "memory");
}

// out_row[16t + 4q + e] = bf16(sum_k af[k] Ws[16t + r][k] + sbias[16t + 4q + e]), t < NT
template <int NT>
__device__ __forceinline__ void chain_linear_bf16(const bf16x8 (&af)[2], const __bf16* Ws,
                                                  const float* sbias, int r, int q, __bf16* out_row) {
  static_assert(NT % 4 == 0, "four accumulator chains per step");
#pragma unroll
  for (int j0 = 0; j0 < NT; j0 += 4) {
    // keep the scheduler from hoisting every group's weight reads (register pressure)
    __builtin_amdgcn_sched_barrier(0);
    floatx4 acc[4];
    bf16x8 b[4][2];
#pragma unroll
    for (int h = 0; h < 4; ++h) {
      acc[h] = floatx4{0.f, 0.f, 0.f, 0.f};
      const __bf16* bp = Ws + ((j0 + h) * 16 + r) * CH_DP + 16 * q;
      b[h][0] = *reinterpret_cast<const bf16x8*>(bp);
      b[h][1] = *reinterpret_cast<const bf16x8*>(bp + 8);
    }
#pragma unroll
    for (int u = 0; u < 2; ++u)
#pragma unroll
      for (int h = 0; h < 4; ++h)
        acc[h] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(b[h][u], af[u], acc[h], 0, 0, 0);
#pragma unroll
    for (int h = 0; h < 4; ++h) {
      const int nl = (j0 + h) * 16 + 4 * q;
      put4(out_row + nl, acc[h] + *reinterpret_cast<const floatx4*>(sbias + nl));
    }
  }
}

}  // namespace rs

// The score-tile pieces shared by the kernels of retrieve.hip (fused top-K, target rank): the
// staging geometry, the user fragments (B operands), the global -> register -> LDS staging of an
// item tile and the MFMA loop over one. One output element of an MFMA depends only on its own A
// row, its own B column and the k order, so every kernel that forms a score through ft_mfma gets
// the same bits for the same (user, item row) whatever else shares the tile.
#pragma once
#include <type_traits>

#include "common.h"
#include "mfma.h"

namespace rs {

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

// user fragments (B operand) of lane (c, h). bf16: U[o][16 s + 8 h .. + 7] of k-step s; fp32:
// U[o][h D/2 + s] (k-step s pairs embedding columns s and D/2 + s)
template <int DP, bool F32>
struct FtUser {
  bf16x8 ub[F32 ? 1 : DP / 16];
  float uf[F32 ? DP / 2 : 1];

  __device__ __forceinline__ void load(const float* U, int64_t ldu, int o, bool o_ok, int D, int h) {
    if constexpr (F32) {
#pragma unroll
      for (int s4 = 0; s4 < DP / 8; ++s4) {
        floatx4 x = {0.f, 0.f, 0.f, 0.f};
        if (o_ok && 8 * s4 < D) x = ld4(U + (int64_t)o * ldu + h * (D / 2) + 4 * s4);
#pragma unroll
        for (int j = 0; j < 4; ++j) uf[4 * s4 + j] = x[j];
      }
    } else {
#pragma unroll
      for (int s = 0; s < DP / 16; ++s) {
        floatx4 x0 = {0.f, 0.f, 0.f, 0.f}, x1 = x0;
        if (o_ok && 16 * s < D) {
          const float* p = U + (int64_t)o * ldu + 16 * s + 8 * h;
          x0 = ld4(p);
          x1 = ld4(p + 4);
        }
        ub[s] = cvt8(x0, x1);
      }
    }
  }
};

// staging: chunk `slot` = 16 bytes `ch` of tile row `row` (the mapping of D = DP; a chunk past
// the row's end repeats its last one: same bytes to the same LDS address). Loads are
// unconditional, rows clamped to N - 1 (columns past the split's end are masked where consumed).
// c0: the tile's first catalog column; cpr = D * ESZ / 16.
template <class Cfg>
__device__ __forceinline__ void ft_load_tile(u32x4 (&r)[Cfg::SL], const void* items, int64_t ldi, int N,
                                             int64_t c0, int tid, int cpr) {
#pragma unroll
  for (int i = 0; i < Cfg::SL; ++i) {
    const int slot = tid + Cfg::NT * i;
    const int row = slot / Cfg::CPR, ch = min(slot % Cfg::CPR, cpr - 1);
    const int64_t g = min(c0 + row, (int64_t)N - 1);
    r[i] = *reinterpret_cast<const u32x4*>(reinterpret_cast<const char*>(items) + g * ldi * Cfg::ESZ + ch * 16);
  }
}

// PT: the LDS row pitch in elements (D + 4 fp32, D + 8 bf16)
template <class Cfg>
__device__ __forceinline__ void ft_store_tile(const u32x4 (&r)[Cfg::SL], void* tile, int PT, int tid, int cpr) {
#pragma unroll
  for (int i = 0; i < Cfg::SL; ++i) {
    const int slot = tid + Cfg::NT * i;
    const int row = slot / Cfg::CPR, ch = min(slot % Cfg::CPR, cpr - 1);
    *reinterpret_cast<u32x4*>(reinterpret_cast<char*>(tile) + row * PT * Cfg::ESZ + ch * 16) = r[i];
  }
}

// acc[ib] = the 32 x 32 scores of item rows T[32 ib .. + 31] (A operand, LDS, pitch PT) against
// the wave's 32 users: element e of lane (c, h) = item row 32 ib + 8 (e >> 2) + 4 h + (e & 3), user c
template <int DP, bool F32, int NB, class E>
__device__ __forceinline__ void ft_mfma(const E* T, int PT, int D, int c, int h, const FtUser<DP, F32>& u,
                                        floatx16 (&acc)[NB]) {
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
            acc[ib] = __builtin_amdgcn_mfma_f32_32x32x2f32(a4[j], u.uf[4 * s4 + j], acc[ib], 0, 0, 0);
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
          acc[ib] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(af, u.ub[s], acc[ib], 0, 0, 0);
        }
      }
    }
  }
}

}  // namespace rs

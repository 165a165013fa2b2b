// The score-tile pieces shared by the kernels of retrieve.hip (fused top-K, target rank): the
// staging geometry, the user fragments (B operands), the global -> register -> LDS staging of an
// item tile and the MFMA loop over one. One output element of an MFMA depends only on its own A
// row, its own B column and the k order, so every kernel that forms a score through ft_mfma gets
// the same bits for the same (user, item row) whatever else shares the tile.
#pragma once
#include <type_traits>

#include "common.h"
#include "e4m3.h"
#include "mfma.h"

namespace rs {

// the item rows' element: fp32, bf16, or OCP e4m3 bytes under one power-of-two scale (e4m3.h)
enum FtElem { kF32 = 0, kBF16 = 1, kE4M3 = 2 };

template <FtElem EK>
using FtStore = std::conditional_t<EK == kF32, float, std::conditional_t<EK == kBF16, __bf16, uint8_t>>;

// the LDS row pitch in elements for width D: D + 4 fp32 and D + 8 bf16 (D + 16 bytes, an odd
// number of 16-byte slots: the 16-byte A reads of 16 rows fall on 16 different slots of the
// 256-byte bank row). e4m3 rows are D bytes, an odd number of slots only after a pad of 16 or 32:
// (D + 16) | 16. An 8-byte A read is banked per 32-lane half, rows c and c + 16 of a block are then
// one slot, so rows 16 - 31 of every block are stored with the two 8-byte halves of each slot
// swapped (ft_store_slot) and read at the opposite half (ft_mfma): 32 rows, 32 different halves.
template <FtElem EK>
__device__ __forceinline__ constexpr int ft_pitch(int D) {
  return EK == kF32 ? D + 4 : EK == kBF16 ? D + 8 : ((D + 16) | 16);
}

// DP: the embedding width the registers and LDS are sized for (D <= DP); KB: the K bucket
// NARROW: 32-item tiles whatever fits (a quarter to a half of the staging registers)
template <int DP, FtElem EK, int KB, bool NARROW = false>
struct FtCfg {
  static constexpr int NW = KB == 0 ? 4 : 1;        // waves per workgroup
  static constexpr int NT = 64 * NW;
  static constexpr int ROWS = 32 * NW;              // users per workgroup
  static constexpr int CAP = KB == 0 ? 80 : 352;    // list capacity: K + 32 <= CAP - 16
  static constexpr int ESZ = EK == kF32 ? 4 : EK == kBF16 ? 2 : 1;
  static constexpr int PTMAX = EK == kF32 ? DP + 4 : EK == kBF16 ? DP + 8 : DP + 16;  // largest pitch, D <= DP
  // items per tile: two LDS buffers within 72 KB (one wave stages at most 64 rows)
  static constexpr int TI = NARROW ? 32 : (KB == 0 && 2 * 128 * PTMAX * ESZ <= 72 * 1024) ? 128
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
// U[o][h D/2 + s] (k-step s pairs embedding columns s and D/2 + s); e4m3: the bf16 elements,
// quantised to e4m3 as RNE(U[o][.] 2^e_u) with e_u from the row's absmax (the lane's own half and
// one exchange with lane ^ 32) and held as the bf16 values of those bytes (exact), and dq =
// 2^-(e_u + item_exp), the exact factor from accumulator to score
template <int DP, FtElem EK>
struct FtUser {
  bf16x8 ub[EK != kF32 ? DP / 16 : 1];
  float uf[EK == kF32 ? DP / 2 : 1];
  float dq;

  __device__ __forceinline__ void load(const float* U, int64_t ldu, int o, bool o_ok, int D, int h,
                                       int item_exp) {
    if constexpr (EK == kE4M3) {
      floatx4 x[DP / 8];
      float amax = 0.f;
#pragma unroll
      for (int s = 0; s < DP / 16; ++s) {
        x[2 * s] = floatx4{0.f, 0.f, 0.f, 0.f};
        x[2 * s + 1] = x[2 * s];
        if (o_ok && 16 * s < D) {
          const float* p = U + (int64_t)o * ldu + 16 * s + 8 * h;
          x[2 * s] = ld4(p);
          x[2 * s + 1] = ld4(p + 4);
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) amax = fmaxf(amax, fmaxf(fabsf(x[2 * s][j]), fabsf(x[2 * s + 1][j])));
      }
      amax = fmaxf(amax, __shfl_xor(amax, 32));
      const int eu = e4m3_exponent(amax);
      const float sc = e4m3_pow2(eu);
#pragma unroll
      for (int s = 0; s < DP / 16; ++s) {
        const uint32_t lo = e4m3_pack4(x[2 * s] * sc), hi = e4m3_pack4(x[2 * s + 1] * sc);
        ub[s] = e4m3_to_bf16x8((long)(((unsigned long long)hi << 32) | lo));
      }
      dq = e4m3_pow2(-eu - item_exp);
    } else if constexpr (EK == kF32) {
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

// one 16-byte slot of LDS row `row`: e4m3 rows 16 - 31 of a block hold their halves swapped (ft_pitch)
template <int ESZ>
__device__ __forceinline__ void ft_store_slot(void* tile, int PT, int row, int ch, u32x4 v) {
  if constexpr (ESZ == 1) v = (row & 16) ? u32x4{v[2], v[3], v[0], v[1]} : v;
  *reinterpret_cast<u32x4*>(reinterpret_cast<char*>(tile) + row * PT * ESZ + ch * 16) = v;
}

// PT: the LDS row pitch in elements (ft_pitch)
template <class Cfg>
__device__ __forceinline__ void ft_store_tile(const u32x4 (&r)[Cfg::SL], void* tile, int PT, int tid, int cpr) {
#pragma unroll
  for (int i = 0; i < Cfg::SL; ++i) {
    const int slot = tid + Cfg::NT * i;
    const int row = slot / Cfg::CPR, ch = min(slot % Cfg::CPR, cpr - 1);
    ft_store_slot<Cfg::ESZ>(tile, PT, row, ch, r[i]);
  }
}

// acc[ib] = the 32 x 32 scores of item rows T[32 ib .. + 31] (A operand, LDS, pitch PT) against
// the wave's 32 users: element e of lane (c, h) = item row 32 ib + 8 (e >> 2) + 4 h + (e & 3), user c
// (e4m3: already de-scaled by u.dq, a power of two, so exact)
template <int DP, FtElem EK, int NB, class E>
__device__ __forceinline__ void ft_mfma(const E* T, int PT, int D, int c, int h, const FtUser<DP, EK>& u,
                                        floatx16 (&acc)[NB]) {
#pragma unroll
  for (int ib = 0; ib < NB; ++ib)
#pragma unroll
    for (int e = 0; e < 16; ++e) acc[ib][e] = 0.f;
  if constexpr (EK == kE4M3) {
    // one 8-byte read per k-step: half h of slot s, the opposite half in the swapped rows. The
    // bytes go to the bf16 MFMA as the bf16 values they encode (4 conversions): the e4m3 MFMA
    // aligns the products of a k-step to the largest and keeps about 13 bits below it, so its
    // sums are not the fp32 sums of the format (DESIGN)
    const char* row = reinterpret_cast<const char*>(T) + c * PT + 8 * (h ^ ((c >> 4) & 1));
#pragma unroll
    for (int s = 0; s < DP / 16; ++s) {
      if (16 * s < D) {
#pragma unroll
        for (int ib = 0; ib < NB; ++ib) {
          const long af = *reinterpret_cast<const long*>(row + ib * 32 * PT + 16 * s);
          acc[ib] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(e4m3_to_bf16x8(af), u.ub[s], acc[ib], 0, 0, 0);
        }
      }
    }
#pragma unroll
    for (int ib = 0; ib < NB; ++ib)
#pragma unroll
      for (int e = 0; e < 16; ++e) acc[ib][e] *= u.dq;
  } else if constexpr (EK == kF32) {
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

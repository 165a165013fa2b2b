// The shapes the selected-row attention kernels (attn_rows.hip) take: shared with rs_attn_plan
// (attention.hip), which reports them as rows_ok.
#pragma once

namespace rs {

constexpr int kMaxChunks = 4;  // chunks of 64 keys, one per lane: L <= 256

inline bool head_dim_ok(int hd) { return hd == 8 || hd == 16 || hd == 32 || hd == 64; }
inline bool attn_rows_ok(int L, int hd) { return L <= 64 * kMaxChunks && head_dim_ok(hd); }

}  // namespace rs

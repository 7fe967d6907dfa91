// wave64 cross-lane helpers shared by the per-ray kernels (hn_render.hip, hn_regularizers.hip).
#pragma once
#include "hn_common.h"

// ------------------------------------------------------------------------------------------------
// wave64 scans — on the DPP cross-lane paths of CDNA (round 6; rounds 1-5 went through `__shfl_up` = `ds_bpermute_b32`, an
// LDS-pipe round trip per step): an inclusive scan is Kogge-Stone inside each row of 16 lanes (row_shr:1, 2, 4, 8; a lane
// without a source keeps the identity), then lane 15 of rows 0 / 2 joins rows 1 / 3 (row_bcast:15, row mask 0xa) and lane
// 31 rows 2-3 (row_bcast:31, row mask 0xc): six `v_mov_b32_dpp` + six ALU ops, no LDS traffic, no wait.
// ------------------------------------------------------------------------------------------------
template <int CTRL, int ROW_MASK>
HN_DEV float hn_dpp(float old, float src) {      // lanes whose source lane does not exist (or whose row is masked) return `old`
  return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(__builtin_bit_cast(int, old), __builtin_bit_cast(int, src),
                                                               CTRL, ROW_MASK, 0xf, false));
}
constexpr int HN_DPP_ROW_SHR = 0x110, HN_DPP_WAVE_SHR1 = 0x138, HN_DPP_BCAST15 = 0x142, HN_DPP_BCAST31 = 0x143;
HN_DEV float hn_wave_incl_scan_mul(float v, int) {
  v *= hn_dpp<HN_DPP_ROW_SHR + 1, 0xf>(1.0f, v);
  v *= hn_dpp<HN_DPP_ROW_SHR + 2, 0xf>(1.0f, v);
  v *= hn_dpp<HN_DPP_ROW_SHR + 4, 0xf>(1.0f, v);
  v *= hn_dpp<HN_DPP_ROW_SHR + 8, 0xf>(1.0f, v);
  v *= hn_dpp<HN_DPP_BCAST15, 0xa>(1.0f, v);
  v *= hn_dpp<HN_DPP_BCAST31, 0xc>(1.0f, v);
  return v;
}
HN_DEV float hn_wave_incl_scan_add(float v, int) {
  v += hn_dpp<HN_DPP_ROW_SHR + 1, 0xf>(0.0f, v);
  v += hn_dpp<HN_DPP_ROW_SHR + 2, 0xf>(0.0f, v);
  v += hn_dpp<HN_DPP_ROW_SHR + 4, 0xf>(0.0f, v);
  v += hn_dpp<HN_DPP_ROW_SHR + 8, 0xf>(0.0f, v);
  v += hn_dpp<HN_DPP_BCAST15, 0xa>(0.0f, v);
  v += hn_dpp<HN_DPP_BCAST31, 0xc>(0.0f, v);
  return v;
}
// the value of the lane below (identity in lane 0): wave_shr:1
HN_DEV float hn_wave_shr1(float v, float identity) { return hn_dpp<HN_DPP_WAVE_SHR1, 0xf>(identity, v); }
// one lane's value in every lane (`lane_idx` wave-uniform): v_readlane_b32, a scalar-register broadcast
HN_DEV float hn_wave_bcast(float v, int lane_idx) {
  return __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, v), lane_idx));
}

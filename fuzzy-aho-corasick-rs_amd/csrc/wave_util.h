// wave_util.h — device-only lane and wave helpers shared by the kernel files (search_kernels.hip,
// prefilter_kernels.hip, ...), and the f32 total-order key rank_kernels.hip and count_kernels.hip share.
// A wave is 64 lanes (gfx950).
#pragma once
#include <hip/hip_runtime.h>

namespace fac {

__device__ __forceinline__ uint32_t lane_id() { return __lane_id(); }

__device__ __forceinline__ uint32_t prefix_below(uint64_t mask) {
  return __builtin_amdgcn_mbcnt_hi((uint32_t)(mask >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)mask, 0u));
}
// Reads from a wave-uniform lane: v_readlane (scalar path), not ds_bpermute through the LDS unit.
__device__ __forceinline__ uint32_t shfl_u32(uint32_t v, int l) {
  return (uint32_t)__builtin_amdgcn_readlane((int)v, l);
}
__device__ __forceinline__ uint64_t shfl_u64(uint64_t v, int l) {
  const uint32_t lo = shfl_u32((uint32_t)v, l), hi = shfl_u32((uint32_t)(v >> 32), l);
  return ((uint64_t)hi << 32) | lo;
}

// f32 total_cmp as an unsigned key (ascending key order == total order; rank_kernels.hip's sort
// keys, count_kernels.hip's similarity order word), and the float's bits back from the key
__device__ inline uint32_t total_key(float f) {
  const uint32_t b = __float_as_uint(f);
  return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}
__host__ __device__ inline uint32_t total_key_bits(uint32_t k) { return (k & 0x80000000u) ? (k ^ 0x80000000u) : ~k; }

// Wave-wide inclusive prefix sum (DPP row shifts + row broadcasts).
__device__ __forceinline__ uint32_t wave_inclusive_sum(uint32_t v) {
  int x = (int)v;
  x += __builtin_amdgcn_update_dpp(0, x, 0x111, 0xF, 0xF, false);  // row_shr:1
  x += __builtin_amdgcn_update_dpp(0, x, 0x112, 0xF, 0xF, false);  // row_shr:2
  x += __builtin_amdgcn_update_dpp(0, x, 0x114, 0xF, 0xF, false);  // row_shr:4
  x += __builtin_amdgcn_update_dpp(0, x, 0x118, 0xF, 0xF, false);  // row_shr:8
  x += __builtin_amdgcn_update_dpp(0, x, 0x142, 0xA, 0xF, false);  // row_bcast:15
  x += __builtin_amdgcn_update_dpp(0, x, 0x143, 0xC, 0xF, false);  // row_bcast:31
  return (uint32_t)x;
}

}  // namespace fac

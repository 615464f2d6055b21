// qtx_attn_frag.h — the pieces the matrix-core attention kernels share (k_attn_mfma and
// k_attn_encq in qtx_attn.hip, k_attn_mfma_long in qtx_attn_long.hip): the staged key order
// and K-row swizzle that make the transposed scores S^T = K Q^T land as the PV MFMA's A
// operand, and the lane-pair steps of the canonical softmax trees.
#pragma once

#include <type_traits>

#include "qtx_common.h"

namespace qtx {

// 64-byte K rows, slot swizzle of qtx_gemm.hip (conflict-free ds_read_b128 fragments)
__device__ __forceinline__ int am_slot(int r, int c) { return c ^ (((r >> 3) & 1) << 1); }
// staged position of key j (an involution): bits 0-1 <-> bits 2-3
__device__ __forceinline__ int am_perm(int j) { return (j & ~15) | ((j & 3) << 2) | ((j >> 2) & 3); }

// x + (x of lane ^ 16) / (lane ^ 32): one permlane swap, the pair's sum / max
__device__ __forceinline__ float xsum16(float v) {
  const auto r = __builtin_amdgcn_permlane16_swap(__float_as_uint(v), __float_as_uint(v), false, false);
  return __uint_as_float(r[0]) + __uint_as_float(r[1]);
}
__device__ __forceinline__ float xsum32(float v) {
  const auto r = __builtin_amdgcn_permlane32_swap(__float_as_uint(v), __float_as_uint(v), false, false);
  return __uint_as_float(r[0]) + __uint_as_float(r[1]);
}
__device__ __forceinline__ float xmax16(float v) {
  const auto r = __builtin_amdgcn_permlane16_swap(__float_as_uint(v), __float_as_uint(v), false, false);
  return fmaxf(__uint_as_float(r[0]), __uint_as_float(r[1]));
}
__device__ __forceinline__ float xmax32(float v) {
  const auto r = __builtin_amdgcn_permlane32_swap(__float_as_uint(v), __float_as_uint(v), false, false);
  return fmaxf(__uint_as_float(r[0]), __uint_as_float(r[1]));
}

// Key j's 64 value bytes (four 16-byte chunks vv) as its 16 dwords of the transposed-dword V
// layout: dword f = bytes v[j][f], v[j][16+f], v[j][32+f], v[j][48+f] (f = 0..15) — the PV B
// operand of lane (f = lane & 15) for the four 16-wide dim tiles in one ds_read_b32
__device__ __forceinline__ void am_vt_row(const uint4 (&vv)[4], bool ok, uint32_t* vt) {
  const uint32_t* w0 = reinterpret_cast<const uint32_t*>(&vv[0]);
  const uint32_t* w1 = reinterpret_cast<const uint32_t*>(&vv[1]);
  const uint32_t* w2 = reinterpret_cast<const uint32_t*>(&vv[2]);
  const uint32_t* w3 = reinterpret_cast<const uint32_t*>(&vv[3]);
#pragma unroll
  for (int f = 0; f < 16; ++f) {
    const int q = f >> 2, pb = f & 3;
    const uint32_t sel = (uint32_t)pb | ((uint32_t)(pb + 4) << 8);   // [lo.pb, hi.pb]
    const uint32_t t01 = __builtin_amdgcn_perm(w1[q], w0[q], sel);
    const uint32_t t23 = __builtin_amdgcn_perm(w3[q], w2[q], sel);
    vt[f] = ok ? __builtin_amdgcn_perm(t23, t01, 0x05040100u) : 0u;
  }
}

// f(integral_constant<int, 0>) ... f(integral_constant<int, N - 1>): a loop unrolled by
// instantiation, for bodies whose register arrays need compile-time indices
template <int I, int N, class F>
__device__ __forceinline__ void static_for_(F& f) {
  if constexpr (I < N) {
    f(std::integral_constant<int, I>{});
    static_for_<I + 1, N>(f);
  }
}
template <int N, class F>
__device__ __forceinline__ void static_for(F&& f) { static_for_<0, N>(f); }

}  // namespace qtx

// qtx_tail.h — device helpers the decode tails share (qtx_decode.hip: k_argmax_embed,
// k_skinny_wide_tok, k_top2_embed; qtx_decode_wide.hip: k_tok_wide, k_top2_wide): the near-tie
// bound, the integer wave sum and the generator's per-strip record with its merge.  (Top2 and
// wave_top2, the scored tails' selection: qtx_common.h.)
#pragma once
#include "qtx_common.h"
#include "qtx_kernels.h"

namespace qtx {

// logp = (x - max) - lse with lse = log(sum) <= logf(V) < 16: (x - max) < -ARG_DELTA rounds
// below -lse, so only values above max - ARG_DELTA can tie the maximum's logp.
constexpr float ARG_DELTA = 4.0e-6f;   // >= 2 ulp(16): covers every V with logf(V) < 16
static_assert(ARG_MAXV <= WIDE_MAXV && WIDE_MAXV < 8886110, "logf(V) < 16 for every tail's V");

__device__ __forceinline__ int wave_sum_i32(int v) {
  auto d = [](int x, auto ctrl) {
    return __builtin_amdgcn_update_dpp(0, x, decltype(ctrl)::value, 0xF, 0xF, true);
  };
  v += d(v, std::integral_constant<int, 0xB1>{});
  v += d(v, std::integral_constant<int, 0x4E>{});
  v += d(v, std::integral_constant<int, 0x141>{});
  v += d(v, std::integral_constant<int, 0x140>{});
  return (__builtin_amdgcn_readlane(v, 0) + __builtin_amdgcn_readlane(v, 16)) +
         (__builtin_amdgcn_readlane(v, 32) + __builtin_amdgcn_readlane(v, 48));
}

// One record of k_generator_mfma<true> (qtx_kernels.h launch_generator_mfma), or of a union of
// strips.
struct TokRec { float m1, m2; int i1, fl; };
// the record of the union of two disjoint sets: m1 by "larger value, then smaller index", m2
// the largest of the loser's m1 and both m2, flags or'ed (commutative and associative)
__device__ __forceinline__ void tok_merge(TokRec& a, float m1, float m2, int i1, int fl) {
  const bool lead = (m1 > a.m1) | ((m1 == a.m1) & (i1 < a.i1));   // (no branches)
  const float loser = lead ? a.m1 : m1;
  a.m2 = fmaxf(fmaxf(a.m2, m2), loser);
  a.m1 = lead ? m1 : a.m1;
  a.i1 = lead ? i1 : a.i1;
  a.fl |= fl;
}
template <int CTRL>
__device__ __forceinline__ void tok_merge_dpp(TokRec& a) {   // (the partner lane's set is disjoint)
  const float m1 = dpp<CTRL>(a.m1), m2 = dpp<CTRL>(a.m2);
  const int i1 = dpp_i32<CTRL>(a.i1), fl = dpp_i32<CTRL>(a.fl);
  tok_merge(a, m1, m2, i1, fl);
}

}  // namespace qtx

// qtx_decode_ka.h — kernel-argument preload of the decode step's kernels: the 14-dword lead
// block and the decode attention's blocks (k_dec_attn in qtx_decode.hip, k_dec_attn_long in
// qtx_decode_long.hip).  Both sources are built with -amdgpu-kernarg-preload-count (qtx/_build.py).
#pragma once
#include <cstdint>

#include "qtx_kernels.h"

namespace qtx {

// =====================================================================================
// Kernel-argument preload.  gfx950 hands a wave the first 14 dwords of its kernel-argument
// segment in SGPRs at launch (16 user SGPRs less the segment pointer; the build passes
// -amdgpu-kernarg-preload-count, qtx/_build.py) — but only leading scalar parameters, never
// a by-value struct, which costs an s_load + s_waitcnt before the first address exists.  The
// step's kernels are latency-bound, so they take those 14 dwords as seven
// 64-bit scalars — a "lead" block per prologue mode, holding what the first load phase
// needs and nothing the instantiation does not read — and everything else as a trailing
// struct, fetched by s_load while the first loads are in flight.  The launchers pack the
// blocks from SkinnyArgs / DecAttnArgs; the kernels rebuild the same struct in registers.
// Pointers travel as integers and come back as global (address space 1) pointers.
// =====================================================================================
struct KaLead { uint64_t w[7]; };
#define QTX_KA_PARAMS uint64_t ka0, uint64_t ka1, uint64_t ka2, uint64_t ka3, uint64_t ka4, \
                      uint64_t ka5, uint64_t ka6
#define QTX_KA_VALS KaLead{{ka0, ka1, ka2, ka3, ka4, ka5, ka6}}
#define QTX_KA_ARGS(l) (l).w[0], (l).w[1], (l).w[2], (l).w[3], (l).w[4], (l).w[5], (l).w[6]
template <class L> KaLead ka_pack(const L& l) {
  static_assert(sizeof(L) == sizeof(KaLead), "a lead block is the 14 preloaded dwords");
  return __builtin_bit_cast(KaLead, l);
}
inline uint64_t ka_int(const void* p) { return (uint64_t)reinterpret_cast<uintptr_t>(p); }
template <class T> __device__ __forceinline__ T* ka_ptr(uint64_t v) {
  return (T*)(__attribute__((address_space(1))) T*)v;
}

// the most rows the decode attention loads: k_dec_attn_long's LDS rows (launch_dec_attn's bound)
constexpr int DEC_LONG_MAXK = 512;

// The lead blocks of k_dec_attn (kernel-argument preload, above): what the loads of phase 0
// need.  Self: the device position counter (read only by a step replayed at several
// positions, and by no load's address) stays in the tail; cross: the mask pointer does —
// its bytes are loaded behind the key rows and scales, when the tail has long arrived.
template <bool KV_NEW> struct DaLead;
template <> struct DaLead<true> {
  uint64_t y; int ldy, kv_bs; uint64_t kc, vc, skc, svc; int host_step1, zero;
};
template <> struct DaLead<false> {
  uint64_t y; int ldy, kv_bs; uint64_t kc, vc, skc, svc; int S, zero;
};
struct DaTail { const int* step; const uint8_t* mask; float* ctx; float* pmax; int B; };

template <bool KV_NEW> KaLead da_lead(const DecAttnArgs& a) {
  DaLead<KV_NEW> l{};
  l.y = ka_int(a.y); l.ldy = (int)a.ldy; l.kv_bs = (int)a.kv_bs;
  l.kc = ka_int(a.kc); l.vc = ka_int(a.vc); l.skc = ka_int(a.skc); l.svc = ka_int(a.svc);
  if constexpr (KV_NEW) l.host_step1 = a.host_step1; else l.S = a.S;
  return ka_pack(l);
}
template <bool KV_NEW>
__device__ __forceinline__ DecAttnArgs da_args(const KaLead& k, const DaTail& t) {
  const DaLead<KV_NEW> l = __builtin_bit_cast(DaLead<KV_NEW>, k);
  DecAttnArgs a{};
  a.y = ka_ptr<const float>(l.y); a.ldy = l.ldy; a.kv_bs = l.kv_bs;
  a.kc = ka_ptr<int8_t>(l.kc); a.vc = ka_ptr<int8_t>(l.vc);
  a.skc = ka_ptr<float>(l.skc); a.svc = ka_ptr<float>(l.svc);
  if constexpr (KV_NEW) a.host_step1 = l.host_step1; else a.S = l.S;
  a.step = t.step; a.mask = t.mask; a.ctx = t.ctx; a.pmax = t.pmax; a.B = t.B;
  return a;
}

}  // namespace qtx

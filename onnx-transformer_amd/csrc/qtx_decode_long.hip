// qtx_decode_long.hip — the decode step's attention for 129 to 512 keys (gfx950, wave64).
//
//   k_dec_attn_long  one query per sentence, four waves per (sentence, head): the fused step's
//                    self- and cross-attention where k_dec_attn (qtx_decode.hip, one wave, at
//                    most 128 keys in registers) cannot hold the keys
//                    attention.py:23-67, get_quantized_model.py:160-168
//
// Same arguments, cache layouts and canonical order as k_dec_attn (oracle/qtx_oracle.py
// attention(dec=True)); results are bit-identical to it wherever both apply.
#include "qtx_common.h"
#include "qtx_decode_ka.h"
#include "qtx_kernels.h"

namespace qtx {

// =====================================================================================
// k_dec_attn_long: grid (B, 8), 256 threads.  The work is split twice, because the two halves
// of the attention are bound by different orders:
//   scores   wave w owns the 128-key block [128 w, 128 w + 128): 8 key fragments loaded
//            straight into the B layout of v_mfma_i32_16x16x64_i8 (clamped loads, keys never
//            staged in LDS), lane l scores keys 128 w + l and 128 w + l + 64 — k_dec_attn's
//            wave, four times.  The int32 dots are exact, so this split is free.
//   softmax  the row maximum per wave, then across waves through LDS (a maximum has no order).
//            The denominator is NOT a sum of per-wave sums: the canonical order is lane l adding
//            e[l], e[l + 64], ..., e[l + 448] from 0 and one 64-lane tree (row_sum_lanesplit),
//            and lane l's eight keys lie in four different waves.  So the exponentials meet in
//            an LDS row E[512] (0 past the last key: x + 0 == x for the x >= 0 summed here) and
//            every wave forms the same denominator from it — no second exchange.
//   PV       wave c runs chain c (keys with (j >> 2) & 3 == c) for dim = lane: per 16-key
//            fragment one value dword (group 4 g + c: 4 keys of the lane's dim) and 4 v_fmac,
//            so the dependent chain is at most 128 fmas per lane — one chain of k_dec_attn's
//            four — and the value bytes are spread over the four waves.  The partial sums meet
//            in LDS and wave 0 forms (c0 + c1) + (c2 + c3).
// Self-attention: every wave quantizes the q / k / v rows itself (wave_absmax_n<3>,
// quant_one_n<3>: the same instructions on the same data, so the same scales in every wave
// that scores); wave 0 publishes the q and k codes in LDS and appends to the caches.  The new
// k code replaces row `step` in the fragment that holds it (wave step >> 7), the new v byte
// its byte of the group dword in the wave that owns chain (step >> 2) & 3, the new scales the
// loaded ones in the lane that scores the key — so a stale cache row at `step`, or a load that
// races the append, never reaches the result.
// The position comes from the host (host_step1) or the device counter; either way rows
// 0 .. position alone are loaded and looped over (the counter is read before the key loads:
// one more latency, against reading up to 512 rows of which a few are live), loads clamped to
// the last live row, which lies inside kv_bs.
// Cross-attention: the key loops stop at the sentence's last unmasked key (later keys give
// P == 0 and fma(0, v, acc) == acc); a fully masked row keeps all S keys.
// LDS: E 2 KiB + PS 2 KiB + partials 1 KiB + codes 128 B + 32 B of per-wave maxima / last keys.
// =====================================================================================
template <bool KV_NEW>
__global__ __launch_bounds__(256) void k_dec_attn_long(QTX_KA_PARAMS, DaTail kt) {
  const DecAttnArgs a = da_args<KV_NEW>(QTX_KA_VALS, kt);
  __shared__ __attribute__((aligned(16))) float E[DEC_LONG_MAXK];    // qexp(score - max), 0 past Sk
  __shared__ __attribute__((aligned(16))) float PS[DEC_LONG_MAXK];   // RN(P_j * s_v[j]), 0 past Sk
  __shared__ float part[4][64];                                  // the chains' partial sums
  __shared__ __attribute__((aligned(16))) int8_t qs[KV_NEW ? 128 : 64];   // q (and new k) codes
  __shared__ float wmax[4];
  __shared__ int wlast[4];
  const int b = blockIdx.x, h = blockIdx.y;
  // (the wave index as a scalar: every test on it below is then a scalar branch)
  const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63;
  const int fr = lane & 15, fg = lane >> 4;    // MFMA fragment: column (key) fr, byte chunk fg
  const float* yr = a.y + (long)b * a.ldy;

  // phase 0: this step's q (k, v) rows first, then the position, then this wave's key block,
  // scales, mask bytes and value dwords — all issued before any is consumed
  float4 yq[2], yk[2], yv[2];
#pragma unroll
  for (int c = 0; c < 2; ++c) {
    yq[c] = *reinterpret_cast<const float4*>(yr + 4 * (lane + 64 * c));
    if constexpr (KV_NEW) {
      yk[c] = *reinterpret_cast<const float4*>(yr + 512 + 4 * (lane + 64 * c));
      yv[c] = *reinterpret_cast<const float4*>(yr + 1024 + 4 * (lane + 64 * c));
    }
  }
  const float q_own = yr[h * 64 + lane];
  const float k_own = KV_NEW ? yr[512 + h * 64 + lane] : 0.0f;
  const float v_own = KV_NEW ? yr[1024 + h * 64 + lane] : 0.0f;
  __builtin_amdgcn_sched_barrier(0);
  // clamped: a stale position (a counter not reset) must not index past the cache
  const int step = !KV_NEW ? 0 : a.host_step1 > 0 ? a.host_step1 - 1 : min(max(*a.step, 0), (int)a.kv_bs - 1);
  const int nrows = KV_NEW ? step + 1 : a.S;           // rows loaded: 1 .. min(kv_bs, 512)
  const int r0 = 128 * w;                              // this wave's key block
  const int nw = min(max(nrows - r0, 0), 128);         // its live rows (0: the wave scores nothing)
  const long kvb = (long)b * a.kv_bs;
  const long vgb = (long)b * ((a.kv_bs + 3) >> 2);     // the sentence's first value group
  const int glast = (nrows - 1) >> 2;                  // the last loaded 4-key value group
  const int8_t* const kbase = a.kc + kvb * 512 + h * 64;
  const int8_t* const vbase = a.vc + vgb * 2048 + h * 256;
  uint4 kr[8];
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    kr[i] = make_uint4(0, 0, 0, 0);
    if (16 * i < nw) {                                 // wave-uniform
      const unsigned koff = (unsigned)(min(r0 + 16 * i + fr, nrows - 1) * 512 + 16 * fg);
      // non-temporal as in k_dec_attn: read once per step by one wave
      kr[i] = __builtin_bit_cast(uint4, __builtin_nontemporal_load(reinterpret_cast<const v4i*>(kbase + koff)));
    }
  }
  const int j0 = min(r0 + lane, nrows - 1), j1 = min(r0 + lane + 64, nrows - 1);
  const float* const skb = a.skc + kvb;
  const float* const svb = a.svc + kvb;
  float sk0 = skb[(unsigned)j0], sk1 = skb[(unsigned)j1];
  float sv0 = svb[(unsigned)j0], sv1 = svb[(unsigned)j1];
  bool keep0 = true, keep1 = true;
  if constexpr (!KV_NEW) {
    const uint8_t* const mb = a.mask + (long)b * a.S;
    keep0 = mb[(unsigned)j0] != 0;
    keep1 = mb[(unsigned)j1] != 0;
  }
  // chain w's value dwords: fragment g's group 4 g + w, dim = lane; 64 keys (4 fragments) per
  // wave-uniform test, groups clamped to the last loaded one
  uint32_t vg[32];
  __builtin_amdgcn_sched_barrier(0);
#pragma unroll
  for (int G = 0; G < 8; ++G)
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int g = 4 * G + q;
      vg[g] = 0u;
      // (the zero pinned to a VGPR: left to itself the register allocator keeps the unloaded
      // dwords' zeros in accumulation registers, takes all 512 registers and still spills 3 KB
      // of scratch per lane; pinned: 101 / 88 VGPRs + 14 / 12 AGPRs self / cross, no scratch,
      // -Rpass-analysis=kernel-resource-usage)
      asm("" : "+v"(vg[g]));
      if (64 * G < nrows)
        vg[g] = __builtin_nontemporal_load(
            reinterpret_cast<const uint32_t*>(vbase + (unsigned)(min(4 * g + w, glast) * 2048 + 4 * lane)));
    }
  // cross: this wave's last unmasked key + 1 (0: none)
  if constexpr (!KV_NEW) {
    const int j = r0 + lane;
    const int last = wave_max_i32(max(keep0 && j < a.S ? j + 1 : 0, keep1 && j + 64 < a.S ? j + 65 : 0));
    if (lane == 0) wlast[w] = last;
  }

  // phase 1: per-token scales of q (and k, v) over the full 512-wide rows, in every wave
  auto lmax8 = [](const float4 (&v)[2]) {
    float m = 0.0f;
#pragma unroll
    for (int c = 0; c < 2; ++c)
      m = fmaxf(m, fmaxf(fmaxf(fabsf(v[c].x), fabsf(v[c].y)), fmaxf(fabsf(v[c].z), fabsf(v[c].w))));
    return m;
  };
  float sq;
  int8_t vq = 0;
  if constexpr (KV_NEW) {
    float am[3] = {lmax8(yq), lmax8(yk), lmax8(yv)};
    wave_absmax_n<3>(am, 1e-5f);
    absmax_scale127_n<3>(am);
    const float own[3] = {q_own, k_own, v_own};
    int code[3];
    quant_one_n<3>(own, am, code);
    sq = am[0];
    const float sk = am[1], sv = am[2];
    const int8_t kq = (int8_t)code[1];
    vq = (int8_t)code[2];
    if (w == 0) {
      const long row = kvb + step;
      a.kc[row * 512 + h * 64 + lane] = kq;     // cache append (attention.py: k/v of this step)
      a.vc[((vgb + (step >> 2)) * 512 + h * 64 + lane) * 4 + (step & 3)] = vq;
      if (h == 0 && lane == 0) { a.skc[row] = sk; a.svc[row] = sv; }
      qs[lane] = (int8_t)code[0];
      qs[64 + lane] = kq;
    }
    if (r0 + lane == step) { sk0 = sk; sv0 = sv; }          // the new scales in the lane that
    if (r0 + lane + 64 == step) { sk1 = sk; sv1 = sv; }     // scores the key
  } else {
    sq = absmax_scale127(wave_absmax(lmax8(yq), 1e-5f));
    const int code = quant_one(q_own, sq);
    if (w == 0) qs[lane] = (int8_t)code;
  }
  __syncthreads();

  // phase 2: operand fragments (A: the q codes' chunk fg in every row) and the key count
  const v4i qf = *reinterpret_cast<const v4i*>(qs + 16 * fg);
  if constexpr (KV_NEW) {
    const uint4 kn = *reinterpret_cast<const uint4*>(qs + 64 + 16 * fg);
    const bool own = w == (step >> 7) && fr == (step & 15);
#pragma unroll
    for (int i = 0; i < 8; ++i)
      if (i == ((step >> 4) & 7) && own) kr[i] = kn;
  }
  int Sk = nrows;
  if constexpr (!KV_NEW) {
    // (wave-uniform by construction; said so, or the key loops below become divergent branches)
    const int last = __builtin_amdgcn_readfirstlane(max(max(wlast[0], wlast[1]), max(wlast[2], wlast[3])));
    if (last > 0) Sk = last;
  }

  // phase 3: scores of keys r0 + lane, r0 + lane + 64; the row maximum through LDS
  v4i sacc[8];
#pragma unroll
  for (int i = 0; i < 8; ++i)
    sacc[i] = __builtin_amdgcn_mfma_i32_16x16x64_i8(qf, __builtin_bit_cast(v4i, kr[i]), v4i{0, 0, 0, 0}, 0, 0, 0);
  float sc[2];
  bool live[2];
  float lmax = -3.0e38f;
#pragma unroll
  for (int u = 0; u < 2; ++u) {
    int dot = sacc[4 * u][0];
#pragma unroll
    for (int t = 1; t < 4; ++t) dot = fg == t ? sacc[4 * u + t][0] : dot;
    live[u] = r0 + lane + 64 * u < Sk;
    float s = (((float)dot * sq) * (u ? sk1 : sk0)) * 0.125f;
    if (!(u ? keep1 : keep0)) s = -1.0e9f;
    sc[u] = s;
    lmax = live[u] ? fmaxf(lmax, s) : lmax;
  }
  lmax = wave_max(lmax);
  if (lane == 0) wmax[w] = lmax;
  __syncthreads();
  const float m = fmaxf(fmaxf(wmax[0], wmax[1]), fmaxf(wmax[2], wmax[3]));
#pragma unroll
  for (int u = 0; u < 2; ++u) {
    sc[u] = qexp(sc[u] - m);
    E[r0 + lane + 64 * u] = live[u] ? sc[u] : 0.0f;
  }
  __syncthreads();
  // the denominator in the canonical lane-split order, the same in every wave
  float lsum = 0.0f;
#pragma unroll
  for (int r = 0; r < 8; ++r) lsum = lsum + E[lane + 64 * r];
  const float den = wave_sum(lsum);
  const float rden = 1.0f / den;
  // P = rint((e / den) * 127) / 127 (div_cr unguarded: den in [1, 512]), PS = RN(P * s_v)
#pragma unroll
  for (int u = 0; u < 2; ++u) {
    const float ps = div127(rintf(div_cr(sc[u], den, rden) * 127.0f)) * (u ? sv1 : sv0);
    PS[r0 + lane + 64 * u] = live[u] ? ps : 0.0f;
  }
  __syncthreads();

  // phase 4: chain w of context dim h * 64 + lane over the keys 16 g + 4 w + (0 .. 3), g in
  // key order.  A fragment past the last key inside a live 64-key chunk has PS == 0 and a
  // finite (clamped) value: fma(0, v, acc) == acc
  if constexpr (KV_NEW) {
    const int sh = 8 * (step & 3);
    const uint32_t ins = (uint32_t)(uint8_t)vq << sh, keep = ~(0xffu << sh);
    const bool mine = w == ((step >> 2) & 3);
#pragma unroll
    for (int g = 0; g < 32; ++g) vg[g] = mine && g == (step >> 4) ? (vg[g] & keep) | ins : vg[g];
  }
  auto fmac = [](float& c, float p, float x) { asm("v_fmac_f32 %0, %1, %2" : "+v"(c) : "v"(p), "v"(x)); };
  float acc = 0.0f;
#pragma unroll
  for (int G = 0; G < 8; ++G) {
    if (64 * G < Sk) {                                 // wave-uniform (Sk <= nrows: vg loaded)
      float4 p[4];
#pragma unroll
      for (int q = 0; q < 4; ++q) p[q] = *reinterpret_cast<const float4*>(PS + 16 * (4 * G + q) + 4 * w);
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const uint32_t d = vg[4 * G + q];
        fmac(acc, p[q].x, (float)(int8_t)d);
        fmac(acc, p[q].y, (float)(int8_t)(d >> 8));
        fmac(acc, p[q].z, (float)(int8_t)(d >> 16));
        fmac(acc, p[q].w, (float)(int8_t)(d >> 24));
      }
    }
  }
  part[w][lane] = acc;
  __syncthreads();

  // phase 5: (c0 + c1) + (c2 + c3), the head's 64 context values and their absmax when asked
  if (w == 0) {
    const float ctx = (part[0][lane] + part[1][lane]) + (part[2][lane] + part[3][lane]);
    st_at(a.ctx, 4u * (unsigned)(b * 512 + h * 64 + lane), ctx);
    if (a.pmax) {
      const float am = wave_max(fabsf(ctx));
      if (lane == 0) a.pmax[(long)h * a.B + b] = am;
    }
  }
}

// a (validated by launch_dec_attn) with 129 .. 512 rows to load
hipError_t launch_dec_attn_long(const DecAttnArgs& a, int B, hipStream_t st) {
  const int nrows = a.kv_new ? (a.host_step1 > 0 ? a.host_step1 : (int)a.kv_bs) : a.S;
  if (nrows <= 0 || nrows > DEC_LONG_MAXK || a.kv_bs < nrows || (long)B * 512 >= (1L << 29))
    return hipErrorInvalidValue;
  const dim3 grid(B, 8), block(256);
  const DaTail t{a.step, a.mask, a.ctx, a.pmax, a.B};
  if (a.kv_new) {
    const KaLead l = da_lead<true>(a);
    k_dec_attn_long<true><<<grid, block, 0, st>>>(QTX_KA_ARGS(l), t);
  } else {
    const KaLead l = da_lead<false>(a);
    k_dec_attn_long<false><<<grid, block, 0, st>>>(QTX_KA_ARGS(l), t);
  }
  return hipGetLastError();
}

}  // namespace qtx

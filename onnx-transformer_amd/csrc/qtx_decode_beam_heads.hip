// qtx_decode_beam_heads.hip — the beam search past 128 keys for models with 4 or 16 heads: the
// fused step's ancestry-indexed self-attention at head widths DK = 128 and 32 (gfx950, wave64).
//
//   k_dec_attn_beam_hd<DK>   1 to 512 keys; position j of row r = b * K + k is read from cache
//                            row b * K + anc[r][j] (k_beam_ancestry keeps the table,
//                            qtx_decode_beam.hip)
//
// The 64-wide k_dec_attn_beam (qtx_decode_beam.hip) and the own-slot k_dec_attn_hd
// (qtx_attn_heads.hip) are untouched; launch_dec_attn_beam dispatches here when the argument
// block's head width is not 64.  Arguments, cache layouts, canonical order and results of
// k_dec_attn_hd<DK, true>: on the caches gathered through the table the two agree bit for bit.
//
// Grid (R, 8), 256 threads; workgroup (r, blk) owns the 64-column block blk of row r's context
// and writes that block's absmax to pmax [8][B].
//   split    k_dec_attn_hd's: DK = 32 two heads per workgroup, both in ONE
//            v_mfma_i32_16x16x64_i8 issue per key fragment (query rows alternate head 0 / head 1,
//            the other head's 32 bytes zeroed; two E / PS rows, two maxima); DK = 128 two
//            workgroups per head, each forming the full 128-deep dot (two chained issues) and
//            running PV on — and appending — its own 64 columns.  Wave w scores the 128-key block
//            [128 w, 128 w + 128), each head's one denominator is the lane-split sum over
//            E[512], wave c runs PV chain c and wave 0 sums (c0 + c1) + (c2 + c3).
//   score    ((float(acc) * s_q) * s_k[j]) / c, c = RN32(sqrt(DK)), the correctly rounded
//            quotient (div_const_n), never a product with a reciprocal.
//   table    k_dec_attn_beam's: anc[r][0 .. kv_bs) is loaded with the step's y rows (two byte
//            loads per thread, no address depends on the position), clamped to K - 1 and stored
//            in LDS behind one barrier: a stale table gives wrong numbers, never an address
//            outside the sentence's K cache rows.
//   keys     the lane that loads key j reads slot A[j] from LDS and forms its own base, 32-bit
//            offsets inside the sentence's K rows; DK = 128 reads both 64-byte k-steps of the row
//            through the one slot.  The scales skc / svc go through the same slot.
//   values   the four slots of a group are one aligned LDS dword; the dead bytes of the
//            position's own group take their predecessor's slot; a wave-uniform vote picks one
//            dword load per group (every live group of one slot) or the mixed path: 16 loads per
//            64-key chunk, byte selects, chunk G + 1's loads issued before chunk G is assembled.
//   append   row `step` of the row's OWN slot (cache row r).
//
// DK = 128 and the registers.  Beside k_dec_attn_beam's 8 key fragments it holds a second set
// (kr[8][2], 64 dwords), both indexed through the table.  The schedule kept is
// k_dec_attn_beam's — every key load issued first, then the slot vote, two value chunks in
// flight on the mixed path — because the compiler's report (the build's flags,
// -Rpass-analysis=kernel-resource-usage) shows it fits with no scratch and no spill, at the
// two waves per SIMD k_dec_attn_beam already runs at (above 128 VGPRs the next step down is at
// 256), so neither one chunk in flight nor key loads ordered behind the vote would buy a wave:
//   k_dec_attn_beam_hd<128>  200 VGPRs, 20 AGPRs, no scratch, no spill, LDS 5904 bytes
//   k_dec_attn_beam_hd<32>   168 VGPRs, 24 AGPRs, no scratch, no spill, LDS 9888 bytes (the
//                            second E / PS row)
// (k_dec_attn_beam: 166 VGPRs, 14 AGPRs, LDS 5776 bytes; DESIGN.md §4 has the figures.)
#include "qtx_common.h"
#include "qtx_decode_ka.h"
#include "qtx_kernels.h"

namespace qtx {

template <int DK> struct BhdC;
template <> struct BhdC<128> { static constexpr float c = 0x1.6a09e6p+3f; };   // RN32(sqrt(128))
template <> struct BhdC<32> { static constexpr float c = 0x1.6a09e6p+2f; };    // RN32(sqrt(32))
static_assert(__builtin_bit_cast(uint32_t, BhdC<128>::c) == 0x413504F3u &&
              __builtin_bit_cast(uint32_t, BhdC<32>::c) == 0x40B504F3u, "c = RN32(sqrt(DK))");

struct DaBeamHdTail { DaTail t; const uint8_t* anc; int K; };

//   NH  heads per workgroup (DK = 32: 2; DK = 128: 1)
//   KS  64-byte k-steps per key fragment (DK = 128: 2; DK = 32: 1 — the block's 64 columns are
//       its two heads)
template <int DK>
__global__ __launch_bounds__(256) void k_dec_attn_beam_hd(QTX_KA_PARAMS, DaBeamHdTail bt) {
  static_assert(DK == 32 || DK == 128, "head widths 32 and 128");
  constexpr int NH = DK == 32 ? 2 : 1;
  constexpr int KS = DK == 128 ? 2 : 1;
  const DecAttnArgs a = da_args<true>(QTX_KA_VALS, bt.t);
  __shared__ __attribute__((aligned(16))) float E[NH][DEC_LONG_MAXK];    // qexp(score - max), 0 past Sk
  __shared__ __attribute__((aligned(16))) float PS[NH][DEC_LONG_MAXK];   // RN(P_j * s_v[j]), 0 past Sk
  __shared__ float part[4][64];                                      // the chains' partial sums
  __shared__ __attribute__((aligned(16))) int8_t qs[2 * 64 * KS];    // q codes, then the new k codes
  __shared__ __attribute__((aligned(16))) uint8_t A[DEC_LONG_MAXK];  // the row's slots, clamped
  __shared__ float wmax[NH][4];
  const int b = blockIdx.x, blk = blockIdx.y;      // blk: the 64-column block this workgroup owns
  const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63;
  const int fr = lane & 15, fg = lane >> 4;    // MFMA fragment: column (key) fr, byte chunk fg
  const int c0 = DK == 128 ? (blk >> 1) * 128 : blk * 64;   // first column the scores read
  const int hd = DK == 32 ? lane >> 5 : 0;     // the head (of the block) of column `lane`
  const float* yr = a.y + (long)b * a.ldy;
  const int K = bt.K, kvn = (int)a.kv_bs;
  const int b0 = b - b % K;                    // the sentence's first cache row

  // phase 0a: this step's q, k, v rows, the table row and the position
  float4 yq[2], yk[2], yv[2];
#pragma unroll
  for (int c = 0; c < 2; ++c) {
    yq[c] = *reinterpret_cast<const float4*>(yr + 4 * (lane + 64 * c));
    yk[c] = *reinterpret_cast<const float4*>(yr + 512 + 4 * (lane + 64 * c));
    yv[c] = *reinterpret_cast<const float4*>(yr + 1024 + 4 * (lane + 64 * c));
  }
  float q_own[KS], k_own[KS];
#pragma unroll
  for (int t = 0; t < KS; ++t) {
    q_own[t] = yr[c0 + 64 * t + lane];
    k_own[t] = yr[512 + c0 + 64 * t + lane];
  }
  const float v_own = yr[1024 + blk * 64 + lane];
  const uint8_t* const ar = bt.anc + (long)b * kvn;
  const int tid = threadIdx.x;
  const uint8_t a0 = ar[min(tid, kvn - 1)], a1 = ar[min(tid + 256, kvn - 1)];
  __builtin_amdgcn_sched_barrier(0);
  // clamped: a stale position (a counter not reset) must not index past the cache
  const int step = a.host_step1 > 0 ? a.host_step1 - 1 : min(max(*a.step, 0), kvn - 1);
  A[tid] = (uint8_t)min((int)a0, K - 1);       // (entries past kv_bs - 1: the last one's copy)
  A[tid + 256] = (uint8_t)min((int)a1, K - 1);
  __syncthreads();

  // phase 0b: this wave's key block (both k-steps), scales and value dwords through the table
  const int nrows = step + 1;                          // rows loaded: 1 .. min(kv_bs, 512)
  const int r0 = 128 * w;                              // this wave's key block
  const int nw = min(max(nrows - r0, 0), 128);         // its live rows (0: the wave scores nothing)
  const long kvb = (long)b0 * kvn;                     // the sentence's first position
  const int G4 = (kvn + 3) >> 2;                       // value groups per cache row
  const int glast = (nrows - 1) >> 2;                  // the last loaded 4-key value group
  const int8_t* const kbase = a.kc + kvb * 512 + c0;
  const int8_t* const vbase = a.vc + (long)b0 * G4 * 2048 + blk * 256;
  uint4 kr[8][KS];
#pragma unroll
  for (int i = 0; i < 8; ++i) {
#pragma unroll
    for (int t = 0; t < KS; ++t) kr[i][t] = make_uint4(0, 0, 0, 0);
    if (16 * i < nw) {                                 // wave-uniform
      const int j = min(r0 + 16 * i + fr, nrows - 1);
      const unsigned koff = (unsigned)(((int)A[j] * kvn + j) * 512 + 16 * fg);
#pragma unroll
      for (int t = 0; t < KS; ++t)
        kr[i][t] = __builtin_bit_cast(uint4, __builtin_nontemporal_load(
                                                 reinterpret_cast<const v4i*>(kbase + koff + 64 * t)));
    }
  }
  const int j0 = min(r0 + lane, nrows - 1), j1 = min(r0 + lane + 64, nrows - 1);
  const float* const skb = a.skc + kvb;
  const float* const svb = a.svc + kvb;
  const unsigned o0 = (unsigned)((int)A[j0] * kvn + j0), o1 = (unsigned)((int)A[j1] * kvn + j1);
  float sk0 = skb[o0], sk1 = skb[o1];
  float sv0 = svb[o0], sv1 = svb[o1];
  // the slots of chain w's groups: lane g holds group min(4 g + w, glast)'s four, the dead
  // bytes of the position's own group set to their predecessor's slot
  uint32_t sl = reinterpret_cast<const uint32_t*>(A)[min(4 * (lane & 31) + w, glast)];
  if (min(4 * (lane & 31) + w, glast) == glast) {
    const int q0 = step & 3;                           // bytes q0 .. 3: patched, or PS == 0
    const uint32_t low = q0 ? 0xffffffffu >> (8 * (4 - q0)) : 0u;
    const uint32_t ref = q0 ? (sl >> (8 * (q0 - 1))) & 0xffu : sl & 0xffu;
    sl = (sl & low) | ((ref * 0x01010101u) & ~low);
  }
  const bool uni = __builtin_amdgcn_ballot_w64(sl != (sl & 0xffu) * 0x01010101u) == 0ull;
  auto vload = [&](int g, uint32_t slot) {
    return __builtin_nontemporal_load(reinterpret_cast<const uint32_t*>(
        vbase + (unsigned)(((int)slot * G4 + min(4 * g + w, glast)) * 2048 + 4 * lane)));
  };
  uint32_t vg[32];
  __builtin_amdgcn_sched_barrier(0);
#pragma unroll
  for (int g = 0; g < 32; ++g) {
    vg[g] = 0u;
    asm("" : "+v"(vg[g]));     // (the zero pinned to a VGPR: k_dec_attn_long's note)
  }
  if (uni) {
#pragma unroll
    for (int G = 0; G < 8; ++G)
      if (64 * G < nrows) {
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          const int g = 4 * G + q;
          vg[g] = vload(g, (uint32_t)__builtin_amdgcn_readlane((int)sl, g) & 0xffu);
        }
      }
  } else {
    // byte e of group g from slot (s >> 8 e) & 255; chunk G + 1 in flight while G is assembled
    uint32_t cur[16], nxt[16] = {};
    auto issue = [&](int G, uint32_t (&d)[16]) {
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const uint32_t s = (uint32_t)__builtin_amdgcn_readlane((int)sl, 4 * G + q);
#pragma unroll
        for (int e = 0; e < 4; ++e) d[4 * q + e] = vload(4 * G + q, (s >> (8 * e)) & 0xffu);
      }
    };
    issue(0, cur);
#pragma unroll
    for (int G = 0; G < 8; ++G) {
      if (64 * G < nrows) {
        if (G + 1 < 8 && 64 * (G + 1) < nrows) issue(G + 1, nxt);
#pragma unroll
        for (int q = 0; q < 4; ++q)
          vg[4 * G + q] = (cur[4 * q] & 0x000000ffu) | (cur[4 * q + 1] & 0x0000ff00u) |
                          (cur[4 * q + 2] & 0x00ff0000u) | (cur[4 * q + 3] & 0xff000000u);
#pragma unroll
        for (int e = 0; e < 16; ++e) cur[e] = nxt[e];
      }
    }
  }

  // phase 1: per-token scales of q, k, v over the full 512-wide rows, in every wave
  auto lmax8 = [](const float4 (&v)[2]) {
    float m = 0.0f;
#pragma unroll
    for (int c = 0; c < 2; ++c)
      m = fmaxf(m, fmaxf(fmaxf(fabsf(v[c].x), fabsf(v[c].y)), fmaxf(fabsf(v[c].z), fabsf(v[c].w))));
    return m;
  };
  float am[3] = {lmax8(yq), lmax8(yk), lmax8(yv)};
  wave_absmax_n<3>(am, 1e-5f);
  absmax_scale127_n<3>(am);
  const float sq = am[0], sk = am[1], sv = am[2];
  int8_t kq[KS], qq[KS], vq = 0;
#pragma unroll
  for (int t = 0; t < KS; ++t) {
    const float own[3] = {q_own[t], k_own[t], v_own};
    int code[3];
    quant_one_n<3>(own, am, code);
    qq[t] = (int8_t)code[0];
    kq[t] = (int8_t)code[1];
    vq = (int8_t)code[2];
  }
  if (w == 0) {
    const long row = (long)b * kvn + step;      // the append: the row's own slot, this
    const int to = DK == 128 ? blk & 1 : 0;     // workgroup's 64 columns (DK = 128: its half)
    a.kc[row * 512 + blk * 64 + lane] = kq[to];
    a.vc[(((long)b * G4 + (step >> 2)) * 512 + blk * 64 + lane) * 4 + (step & 3)] = vq;
    if (blk == 0 && lane == 0) { a.skc[row] = sk; a.svc[row] = sv; }
#pragma unroll
    for (int t = 0; t < KS; ++t) {
      qs[64 * t + lane] = qq[t];
      qs[64 * KS + 64 * t + lane] = kq[t];
    }
  }
  if (r0 + lane == step) { sk0 = sk; sv0 = sv; }          // the new scales in the lane that
  if (r0 + lane + 64 == step) { sk1 = sk; sv1 = sv; }     // scores the key
  __syncthreads();

  // phase 2: operand fragments (A: the q codes' chunk fg in every row — DK = 32: row parity
  // picks the head, the other head's bytes zero), the new key patched in
  v4i qf[KS];
#pragma unroll
  for (int t = 0; t < KS; ++t) qf[t] = *reinterpret_cast<const v4i*>(qs + 64 * t + 16 * fg);
  if constexpr (DK == 32)
    if ((fr & 1) != (fg >> 1)) qf[0] = v4i{0, 0, 0, 0};
  {
    const bool own = w == (step >> 7) && fr == (step & 15);
#pragma unroll
    for (int t = 0; t < KS; ++t) {
      const uint4 kn = *reinterpret_cast<const uint4*>(qs + 64 * KS + 64 * t + 16 * fg);
#pragma unroll
      for (int i = 0; i < 8; ++i)
        if (i == ((step >> 4) & 7) && own) kr[i][t] = kn;
    }
  }
  const int Sk = nrows;

  // phase 3: scores of keys r0 + lane, r0 + lane + 64 (output row hh of fragment 4 u + fg,
  // column fr, is head hh's dot); the row maxima through LDS
  v4i sacc[8];
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    sacc[i] = v4i{0, 0, 0, 0};
#pragma unroll
    for (int t = 0; t < KS; ++t)
      sacc[i] = __builtin_amdgcn_mfma_i32_16x16x64_i8(qf[t], __builtin_bit_cast(v4i, kr[i][t]), sacc[i], 0, 0, 0);
  }
  float sc[NH][2];
  bool live[2];
#pragma unroll
  for (int u = 0; u < 2; ++u) {
    live[u] = r0 + lane + 64 * u < Sk;
#pragma unroll
    for (int hh = 0; hh < NH; ++hh) {
      int dot = sacc[4 * u][hh];
#pragma unroll
      for (int t = 1; t < 4; ++t) dot = fg == t ? sacc[4 * u + t][hh] : dot;
      sc[hh][u] = ((float)dot * sq) * (u ? sk1 : sk0);
    }
  }
  {
    float flat[NH * 2];
#pragma unroll
    for (int hh = 0; hh < NH; ++hh) { flat[2 * hh] = sc[hh][0]; flat[2 * hh + 1] = sc[hh][1]; }
    div_const_n<NH * 2>(flat, BhdC<DK>::c);    // the correctly rounded quotients
#pragma unroll
    for (int hh = 0; hh < NH; ++hh) { sc[hh][0] = flat[2 * hh]; sc[hh][1] = flat[2 * hh + 1]; }
  }
#pragma unroll
  for (int hh = 0; hh < NH; ++hh) {
    float lmax = -3.0e38f;
#pragma unroll
    for (int u = 0; u < 2; ++u) lmax = live[u] ? fmaxf(lmax, sc[hh][u]) : lmax;
    lmax = wave_max(lmax);
    if (lane == 0) wmax[hh][w] = lmax;
  }
  __syncthreads();
#pragma unroll
  for (int hh = 0; hh < NH; ++hh) {
    const float m = fmaxf(fmaxf(wmax[hh][0], wmax[hh][1]), fmaxf(wmax[hh][2], wmax[hh][3]));
#pragma unroll
    for (int u = 0; u < 2; ++u) {
      sc[hh][u] = qexp(sc[hh][u] - m);
      E[hh][r0 + lane + 64 * u] = live[u] ? sc[hh][u] : 0.0f;
    }
  }
  __syncthreads();
  // the denominators in the canonical lane-split order, the same in every wave
#pragma unroll
  for (int hh = 0; hh < NH; ++hh) {
    float lsum = 0.0f;
#pragma unroll
    for (int r = 0; r < 8; ++r) lsum = lsum + E[hh][lane + 64 * r];
    const float den = wave_sum(lsum);
    const float rden = 1.0f / den;
    // P = rint((e / den) * 127) / 127 (div_cr unguarded: den in [1, 512]), PS = RN(P * s_v)
#pragma unroll
    for (int u = 0; u < 2; ++u) {
      const float ps = div127(rintf(div_cr(sc[hh][u], den, rden) * 127.0f)) * (u ? sv1 : sv0);
      PS[hh][r0 + lane + 64 * u] = live[u] ? ps : 0.0f;
    }
  }
  __syncthreads();

  // phase 4: chain w of context column blk * 64 + lane (head hd of the block) over the keys
  // 16 g + 4 w + (0 .. 3), g in key order, the new v byte in place of the cached one
  {
    const int sh = 8 * (step & 3);
    const uint32_t ins = (uint32_t)(uint8_t)vq << sh, keep = ~(0xffu << sh);
    const bool mine = w == ((step >> 2) & 3);
#pragma unroll
    for (int g = 0; g < 32; ++g) vg[g] = mine && g == (step >> 4) ? (vg[g] & keep) | ins : vg[g];
  }
  auto fmac = [](float& c, float p, float x) { asm("v_fmac_f32 %0, %1, %2" : "+v"(c) : "v"(p), "v"(x)); };
  const float* const psr = &PS[0][0] + hd * DEC_LONG_MAXK;
  float acc = 0.0f;
#pragma unroll
  for (int G = 0; G < 8; ++G) {
    if (64 * G < Sk) {                                 // wave-uniform (vg loaded)
      float4 p[4];
#pragma unroll
      for (int q = 0; q < 4; ++q) p[q] = *reinterpret_cast<const float4*>(psr + 16 * (4 * G + q) + 4 * w);
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

  // phase 5: (c0 + c1) + (c2 + c3), the block's 64 context values and their absmax when asked
  if (w == 0) {
    const float ctx = (part[0][lane] + part[1][lane]) + (part[2][lane] + part[3][lane]);
    st_at(a.ctx, 4u * (unsigned)(b * 512 + blk * 64 + lane), ctx);
    if (a.pmax) {
      const float amx = wave_max(fabsf(ctx));
      if (lane == 0) a.pmax[(long)blk * a.B + b] = amx;
    }
  }
}

// a (validated by launch_dec_attn_beam, which dispatches here) with a.dk 32 or 128; the vector
// loads of the y rows and key fragments need 16-byte aligned rows
hipError_t launch_dec_attn_beam_hd(const DecAttnArgs& a, const uint8_t* anc, int K, int B, hipStream_t st) {
  if ((a.dk != 32 && a.dk != 128) || (reinterpret_cast<uintptr_t>(a.y) & 15) || (a.ldy & 3) ||
      (reinterpret_cast<uintptr_t>(a.kc) & 15) || (reinterpret_cast<uintptr_t>(a.vc) & 3))
    return hipErrorInvalidValue;
  const KaLead l = da_lead<true>(a);
  const DaBeamHdTail t{{a.step, a.mask, a.ctx, a.pmax, a.B}, anc, K};
  if (a.dk == 128) k_dec_attn_beam_hd<128><<<dim3(B, 8), dim3(256), 0, st>>>(QTX_KA_ARGS(l), t);
  else k_dec_attn_beam_hd<32><<<dim3(B, 8), dim3(256), 0, st>>>(QTX_KA_ARGS(l), t);
  return hipGetLastError();
}

}  // namespace qtx

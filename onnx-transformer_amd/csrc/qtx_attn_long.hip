// qtx_attn_long.hip — encoder / decoder-module attention for 129 to 512 keys on the matrix
// cores (gfx950, wave64).
//
//   k_attn_mfma_long<DEC, NB>   the attention of k_attn_mfma (qtx_attn.hip: same AttnArgs, both
//                               mask forms, both PV orders, fp32 context) where its 128 key
//                               slots do not hold the keys; NB = ceil(Sk / 128) = 2, 3, 4
//                               attention.py:23-36, canonical order of oracle/qtx_oracle.py
//
// Workgroup = (head h, sentence b, block of 64 query rows), 4 waves, wave w owns query rows
// 16 w .. 16 w + 15 of the block and ALL the keys: a row's scores, exponentials and P codes
// never leave the lane that computed them (x[8 NB][4]: 64 / 96 / 128 registers), so the one
// exchange of the whole kernel is the staging barrier.
//   staging  K, V, both scale vectors and the key mask of the head, once per workgroup, every
//            thread a whole key at a time (keys tid, tid + 256): K rows in the staged key order
//            am_perm with am_slot's swizzle, V in the transposed-dword layout, sks / mks in
//            staged order, svs in key order.  Only the slots the kernel reads are staged —
//            Sk rounded up to a 16-key tile — and those past Sk hold zeros with scale 0 (from
//            clamped unconditional loads).  At 512 keys: 32 KB + 32 KB + 4 KB + 512 B, two
//            workgroups per CU.
//   scores   S^T = K Q^T, one v_mfma_i32_16x16x64_i8 per 16-key tile kt < 8 NB: lane (fr, fg)
//            gets row fr at keys 16 kt + 4 e + fg — the A operand of PV step s = 4 kt + e.
//   softmax  max: in the lane, then lanes xor 16 / xor 32.  The denominator is the canonical
//            lane-split sum (oracle row_sum_lanesplit): position L = j mod 64 adds
//            e[L], e[L + 64], ... in order from 0, then the 64-position tree, bit 0 first.
//            Here L = 16 (kt & 3) + 4 e + fg, so position (kt & 3, e)'s partial is the in-lane
//            sum over r = kt >> 2 = 0 .. 2 NB - 1 (absent keys add +0: exact) and the tree is
//            k_attn_mfma's: xsum16, xsum32, over e, over kt & 3.  (A sum of per-128-block sums
//            is another number in about a third of random 512-key rows)
//   PV       v_mfma_f32_16x16x4f32 over the steps s < ceil(Sk / 4) in key order from 0: one
//            chain per 16-wide dim tile (four independent chains side by side), or DEC: step s
//            to chain s & 3 of four per dim tile, summed (c0 + c1) + (c2 + c3).  DEC takes the
//            dim tiles in two passes of two (register budget, below).  The V dwords and scales
//            of a chunk of 8 steps are read ahead of its MFMAs wherever the whole chunk exists.
// A causal query's mask row is read from global memory byte by byte (mask strides are the
// caller's: nothing to vectorize on).
#include "qtx_attn_frag.h"
#include "qtx_common.h"
#include "qtx_kernels.h"

namespace qtx {

constexpr int AML_MAXK = 512;

template <bool DEC, int NB>
__global__ __launch_bounds__(256, 2) void k_attn_mfma_long(AttnArgs a) {
  constexpr int NK = 128 * NB;             // key slots
  constexpr int NT = 8 * NB;               // 16-key score tiles
  __shared__ __attribute__((aligned(16))) uint8_t Ks[NK * 64];
  __shared__ __attribute__((aligned(16))) int8_t Vs[NK * 64];
  __shared__ __attribute__((aligned(16))) float sks[NK];     // staged order (am_perm)
  __shared__ __attribute__((aligned(16))) float svs[NK];     // key order
  __shared__ __attribute__((aligned(16))) uint8_t mks[NK];   // per-key mask, staged order
  const int h = blockIdx.x, b = blockIdx.y;
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int fr = lane & 15, fg = lane >> 4;
  const int Sk = a.Sk, Sq = a.Sq, hoff = h * 64;
  const int nk4 = (Sk + 3) & ~3;            // keys rounded up to the PV MFMA k step
  const int nk16 = (Sk + 15) & ~15;         // ... to a score tile: the slots anything reads
  const int r0 = blockIdx.z * 64 + wave * 16;
  const bool row_mask = a.mask && a.m_is != 0;   // per-query mask rows (causal decoder)

  // ---- stage K, V, scales, mask of the key slots below nk16 (slots >= Sk zero) -----------
  const int8_t* kb = a.k + b * a.k_bs + hoff;
  const int8_t* vb = a.v + b * a.v_bs + hoff;
#pragma unroll
  for (int it = 0; it < (NB + 1) / 2; ++it) {
    const int j = tid + 256 * it;
    if (j < nk16) {                         // (nk16 <= NK: Sk <= 128 NB)
      const int jc = min(j, Sk - 1), pj = am_perm(j);
      const bool ok = j < Sk;
      uint4 kv[4], vv[4];
#pragma unroll
      for (int c = 0; c < 4; ++c) {         // clamped, unconditional loads; zeroed if j >= Sk
        kv[c] = *reinterpret_cast<const uint4*>(kb + (long)jc * a.k_ld + 16 * c);
        vv[c] = *reinterpret_cast<const uint4*>(vb + (long)jc * a.v_ld + 16 * c);
      }
      const float skj = a.sk[b * a.sk_bs + jc], svj = a.sv[b * a.sv_bs + jc];
      const uint8_t mj = (a.mask && !row_mask) ? a.mask[b * a.m_bs + jc] : (uint8_t)1;
#pragma unroll
      for (int c = 0; c < 4; ++c)
        *reinterpret_cast<uint4*>(Ks + pj * 64 + 16 * am_slot(pj, c)) = ok ? kv[c] : make_uint4(0, 0, 0, 0);
      am_vt_row(vv, ok, reinterpret_cast<uint32_t*>(Vs + j * 64));
      sks[pj] = ok ? skj : 0.0f;
      svs[j] = ok ? svj : 0.0f;
      mks[pj] = ok ? mj : (uint8_t)1;
    }
  }
  // this wave's query fragment (MFMA B operand: query row fr, bytes 16*fg..) and row scale
  const int qrow = min(r0 + fr, Sq - 1);
  const v4i qf = *reinterpret_cast<const v4i*>(a.q + b * a.q_bs + (long)qrow * a.q_ld + hoff + 16 * fg);
  const float sqr = a.sq[b * a.sq_bs + qrow];
  const uint8_t* mrow = row_mask ? a.mask + b * a.m_bs + (long)qrow * a.m_is : nullptr;
  __syncthreads();
  if (r0 >= Sq) return;                    // (after the only block-wide barrier)

  // ---- scores S^T: C[staged row 4fg + e = key 16kt + 4e + fg][query fr] ------------------
  // masked: -1e9; absent (>= Sk): -3e38, whose exponential and P are exactly 0
  float x[NT][4];
#pragma unroll
  for (int kt = 0; kt < NT; ++kt) {
    if (16 * kt < Sk) {
      const int krow = kt * 16 + fr;
      const v4i kf = *reinterpret_cast<const v4i*>(Ks + krow * 64 + 16 * am_slot(krow, fg));
      const v4i sc4 = __builtin_amdgcn_mfma_i32_16x16x64_i8(kf, qf, v4i{0, 0, 0, 0}, 0, 0, 0);
      const int k0 = 16 * kt + 4 * fg;         // staged rows k0..k0+3
      const float4 skv = *reinterpret_cast<const float4*>(sks + k0);
      const uint32_t mk = *reinterpret_cast<const uint32_t*>(mks + k0);
      const float skk[4] = {skv.x, skv.y, skv.z, skv.w};
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const int key = 16 * kt + 4 * e + fg;
        float sc = (((float)sc4[e] * sqr) * skk[e]) * 0.125f;
        bool keep = ((mk >> (8 * e)) & 0xffu) != 0u;
        if (row_mask) keep = mrow[min(key, Sk - 1)] != 0;
        if (!keep) sc = -1.0e9f;
        x[kt][e] = key < Sk ? sc : -3.0e38f;
      }
    } else {
#pragma unroll
      for (int e = 0; e < 4; ++e) x[kt][e] = -3.0e38f;
    }
  }

  // ---- softmax of row fr over its key slots (32 NB in the lane, 4 lanes) -----------------
  float m = x[0][0];
#pragma unroll
  for (int kt = 0; kt < NT; ++kt)
#pragma unroll
    for (int e = 0; e < 4; ++e) m = fmaxf(m, x[kt][e]);
  m = xmax16(m);
  m = xmax32(m);
#pragma unroll
  for (int kt = 0; kt < NT; ++kt) {
#pragma unroll
    for (int e = 0; e < 4; ++e) x[kt][e] = qexp(x[kt][e] - m);   // absent: qexp(-3e38 - m) == 0
    __builtin_amdgcn_sched_barrier(0);
  }
  float t[4];
#pragma unroll
  for (int kq = 0; kq < 4; ++kq) {
    float u[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      float part = 0.0f;                 // position L = 16 kq + 4 e + fg: e[L], e[L + 64], ...
#pragma unroll
      for (int r = 0; r < 2 * NB; ++r) part = part + x[kq + 4 * r][e];
      u[e] = xsum32(xsum16(part));       // tree levels 1-2 (lanes)
    }
    t[kq] = (u[0] + u[1]) + (u[2] + u[3]);
  }
  const float den = (t[0] + t[1]) + (t[2] + t[3]);
  // e/den correctly rounded via the shared reciprocal (div_cr) unless some e is outside
  // its range (then the true division, wave-uniform); q/127 by div127 (exact for the codes)
  DivRange rg;
#pragma unroll
  for (int kt = 0; kt < NT; ++kt)
#pragma unroll
    for (int e = 0; e < 4; ++e) rg.add(x[kt][e]);
  const bool fast = __ballot(!(rg.ok() && divisor_ok(den))) == 0ull;
  const float rden = 1.0f / den;
  // (the wave-uniform choice taken per score tile, not once around two loops over all 32 NB
  // slots: the two 128-value results meeting after such a pair of loops cost the NB = 4
  // instances ten registers more than the 256 that two waves per SIMD leave, i.e. scratch)
#pragma unroll
  for (int kt = 0; kt < NT; ++kt) {
    float qt[4];
    if (fast) {
#pragma unroll
      for (int e = 0; e < 4; ++e) qt[e] = div_cr(x[kt][e], den, rden);
    } else {
#pragma unroll
      for (int e = 0; e < 4; ++e) qt[e] = x[kt][e] / den;
    }
#pragma unroll
    for (int e = 0; e < 4; ++e) x[kt][e] = div127(rintf(qt[e] * 127.0f));   // keys >= Sk: e == 0, P = 0
  }

  // ---- PV on fp32 MFMA: A = P[row fr][k] (the lane's x[s/4][s%4], k = 4s + fg),
  // B = float(v[k][d]) * s_v[k].  DEC (the decoder's PV order, oracle attention_pv dec):
  // A = RN(P * s_v[k]), B = float(v[k][d]), and step s goes to chain s & 3 — one MFMA step is
  // one chain's 4 keys in order — the four chains summed (c0 + c1) + (c2 + c3) ----------------
  // DEC holds four accumulators per dim tile, so it takes the dim tiles in two passes of two
  // (32 accumulators beside the 32 NB P values, not 64: the NB = 4 instance stays under the
  // 256 registers of two waves per SIMD with no scratch); the second pass repeats only the
  // P * s_v products and the LDS reads
  constexpr int NCH = DEC ? 4 : 1;         // chains per dim tile
  constexpr int NDT = DEC ? 2 : 4;         // dim tiles per pass
  const uint32_t* vt32 = reinterpret_cast<const uint32_t*>(Vs);
  static_for<4 / NDT>([&](auto pc) {
    constexpr int dt0 = NDT * decltype(pc)::value;
    v4f acc[NCH][NDT];
#pragma unroll
    for (int c = 0; c < NCH; ++c)
#pragma unroll
      for (int d = 0; d < NDT; ++d) acc[c][d] = v4f{0, 0, 0, 0};
    auto step = [&](auto sc, float svk, uint32_t vd) {
      constexpr int s4 = decltype(sc)::value;
      const float pa = DEC ? x[s4 >> 2][s4 & 3] * svk : x[s4 >> 2][s4 & 3];
#pragma unroll
      for (int d = 0; d < NDT; ++d) {
        const float vf = (float)(int8_t)(vd >> (8 * (dt0 + d)));
        const float vb2 = DEC ? vf : vf * svk;
        acc[s4 % NCH][d] = __builtin_amdgcn_mfma_f32_16x16x4f32(pa, vb2, acc[s4 % NCH][d], 0, 0, 0);
      }
    };
    static_for<4 * NB>([&](auto cc) {      // chunks of 8 steps (32 keys)
      constexpr int c = decltype(cc)::value;
      if (32 * c + 32 <= nk4) {            // the whole chunk: operands first, then the MFMAs
        float svk[8];
        uint32_t vd[8];
#pragma unroll
        for (int i = 0; i < 8; ++i) {
          const int k = 4 * (8 * c + i) + fg;
          svk[i] = svs[k];
          vd[i] = vt32[k * 16 + fr];
        }
        static_for<8>([&](auto ic) {
          constexpr int i = decltype(ic)::value;
          step(std::integral_constant<int, 8 * c + i>{}, svk[i], vd[i]);
        });
      } else {                             // the ragged chunk: only steps below ceil(Sk / 4)
        static_for<8>([&](auto ic) {
          constexpr int s4 = 8 * c + decltype(ic)::value;
          if (4 * s4 < nk4) {
            const int k = 4 * s4 + fg;
            step(std::integral_constant<int, s4>{}, svs[k], vt32[k * 16 + fr]);
          }
        });
      }
    });
#pragma unroll
    for (int d = 0; d < NDT; ++d)
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const int row = r0 + 4 * fg + e;
        const float cv = DEC ? (acc[0][d][e] + acc[1 % NCH][d][e]) + (acc[2 % NCH][d][e] + acc[3 % NCH][d][e])
                             : acc[0][d][e];
        if (row < Sq) a.ctx[b * a.c_bs + (long)row * a.c_ld + hoff + (dt0 + d) * 16 + fr] = cv;
      }
  });
}

template <bool DEC>
static hipError_t launch_nb(const AttnArgs& a, hipStream_t st) {
  const dim3 grid(a.H, a.B, (a.Sq + 63) / 64), block(256);
  switch ((a.Sk + 127) / 128) {
    case 2: k_attn_mfma_long<DEC, 2><<<grid, block, 0, st>>>(a); break;
    case 3: k_attn_mfma_long<DEC, 3><<<grid, block, 0, st>>>(a); break;
    default: k_attn_mfma_long<DEC, 4><<<grid, block, 0, st>>>(a); break;
  }
  return hipGetLastError();
}

// Returns hipErrorNotSupported for shapes it does not take (caller keeps k_attention).
hipError_t launch_attention_mfma_long(const AttnArgs& a, hipStream_t st) {
  if (a.sk_dev || a.qpos_dev || a.H * 64 > 4096 || a.Sk <= 128 || a.Sk > AML_MAXK)
    return hipErrorNotSupported;
  return a.dec ? launch_nb<true>(a, st) : launch_nb<false>(a, st);
}

}  // namespace qtx

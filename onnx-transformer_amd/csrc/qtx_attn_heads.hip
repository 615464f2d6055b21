// qtx_attn_heads.hip — attention for models with 4 or 16 heads at d_model 512: head widths
// DK = 128 and 32 (gfx950, wave64).  The 64-wide kernels (qtx_attn.hip, qtx_attn_long.hip,
// qtx_decode.hip, qtx_decode_long.hip, k_attention) are untouched; launch_attention /
// launch_dec_attn dispatch here when the argument block's head width is not 64.
//
//   k_attn_mfma_hd<DK, DEC, NB>  full-prefix attention, 1 .. 512 keys (NB = ceil(Sk / 128))
//   k_dec_attn_hd<DK, KV_NEW>    the KV-cached step's attention, 1 .. 512 keys
//   k_attention_hd<DK>           the VALU kernel of the device-counter forms
//
// The canonical order is the 64-wide kernels' (oracle/qtx_oracle.py attention); only the
// score differs: s = ((float(acc) * s_q) * s_k[j]) / c with c = RN32(sqrt(DK)), acc the exact
// int32 dot over the head's DK columns.  c is no power of two, so the quotient is the
// correctly rounded fp32 division (div_const_n: div_cr behind its range vote, else `/`),
// never a product with RN(1 / c).
//
// k_attn_mfma_hd: workgroup = (head, sentence, block of 64 query rows), 4 waves, wave w owns
// query rows 16 w .. 16 w + 15 and ALL the keys, exactly k_attn_mfma_long's split: a row's
// scores, exponentials and P codes stay in the lane that computed them, the denominator is the
// one canonical lane-split sum over all keys (never a sum of per-block sums: qtx_attn_long.hip's
// header says why), and the only exchange is the staging barrier.
//   staging  K rows of DK bytes in the staged key order am_perm; DK = 128: the eight 16-byte
//            chunks of row r at chunk ^ (r & 7) (the fragment reads of 8 consecutive rows then
//            touch 8 different chunk columns).  V in the transposed layout of am_vt_row, one
//            dword per (key, 64-column half, f) for DK = 128 — the halves of key k swapped when
//            (k >> 1) & 1, so the four keys of a PV step read four different bank groups — and
//            one 16-bit pair (v[f], v[16 + f]) per (key, f) for DK = 32.
//   scores   S^T = K Q^T.  DK = 128: two chained v_mfma_i32_16x16x64_i8 per 16-key tile (the
//            64-byte halves of the rows).  DK = 32: one v_mfma_i32_16x16x32_i8 per tile — the
//            32-deep form, 8 bytes per lane, so no issue runs half empty.
//   PV       v_mfma_f32_16x16x4f32 over DK / 16 dim tiles, steps in key order from 0, in
//            k_attn_mfma_long's chain order (DEC: step s to chain s & 3, (c0 + c1) + (c2 + c3)).
//            The dim tiles go in passes (4 per pass, DEC 2) so the accumulators beside the
//            32 NB P values stay what the 64-wide kernel holds.
// One kernel template serves the whole key range; NB only sizes the register array of P values
// (32 NB per lane) and the LDS (DK = 128, NB = 4: 64 KB + 64 KB + 4.5 KB, one workgroup per CU,
// which is what bounds it: a 512-key head of 128 columns is 128 KB of K and V).  Resource
// figures: DESIGN.md §4.
//
// k_dec_attn_hd: grid (B, 8), 256 threads, k_dec_attn_long's split (key blocks per wave for
// the scores, one LDS row of exponentials per head for the one denominator, one PV chain per
// wave) at every key count.  A workgroup owns one whole 64-column block of the context, so it
// writes that block's absmax into pmax [8][B] with no exchange between workgroups and the
// consumer GEMM does not change:
//   DK = 32   two heads per workgroup, both in ONE 16x16x64 issue per key fragment: the query
//             operand's rows alternate head 0 / head 1 with the other head's 32 bytes zeroed,
//             so output rows 0 / 1 are the two heads' dots of the key.
//   DK = 128  two workgroups per head: each forms the full 128-deep dot products (two chained
//             issues) and runs PV on its own 64 columns.  The other choice — one workgroup per
//             head writing two maxima — halves the grid of a latency-bound step and doubles
//             each lane's PV chain work; the duplicated scores cost 64 more key bytes per lane.
// Cache layouts, clamped loads, append rules and position handling are k_dec_attn_long's.
#include "qtx_attn_frag.h"
#include "qtx_common.h"
#include "qtx_decode_ka.h"
#include "qtx_kernels.h"

namespace qtx {

template <int DK> struct HdC;
template <> struct HdC<128> { static constexpr float c = 0x1.6a09e6p+3f; };   // RN32(sqrt(128))
template <> struct HdC<32> { static constexpr float c = 0x1.6a09e6p+2f; };    // RN32(sqrt(32))
static_assert(__builtin_bit_cast(uint32_t, HdC<128>::c) == 0x413504F3u &&
              __builtin_bit_cast(uint32_t, HdC<32>::c) == 0x40B504F3u, "c = RN32(sqrt(DK))");

constexpr int AMH_MAXK = 512;

// =====================================================================================
// k_attn_mfma_hd
// =====================================================================================
template <int DK, bool DEC, int NB>
__global__ __launch_bounds__(256) void k_attn_mfma_hd(AttnArgs a) {
  static_assert(DK == 32 || DK == 128, "head widths 32 and 128");
  constexpr int NK = 128 * NB;             // key slots
  constexpr int NT = 8 * NB;               // 16-key score tiles
  constexpr int KCH = DK / 16;             // 16-byte chunks of a row
  __shared__ __attribute__((aligned(16))) uint8_t Ks[NK * DK];
  __shared__ __attribute__((aligned(16))) uint8_t Vs[NK * DK];
  __shared__ __attribute__((aligned(16))) float sks[NK];     // staged order (am_perm)
  __shared__ __attribute__((aligned(16))) float svs[NK];     // key order
  __shared__ __attribute__((aligned(16))) uint8_t mks[NK];   // per-key mask, staged order
  const int h = blockIdx.x, b = blockIdx.y;
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int fr = lane & 15, fg = lane >> 4;
  const int Sk = a.Sk, Sq = a.Sq, hoff = h * DK;
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
      uint4 kv[KCH], vv[KCH];
#pragma unroll
      for (int c = 0; c < KCH; ++c) {       // clamped, unconditional loads; zeroed if j >= Sk
        kv[c] = *reinterpret_cast<const uint4*>(kb + (long)jc * a.k_ld + 16 * c);
        vv[c] = *reinterpret_cast<const uint4*>(vb + (long)jc * a.v_ld + 16 * c);
      }
      const float skj = a.sk[b * a.sk_bs + jc], svj = a.sv[b * a.sv_bs + jc];
      const uint8_t mj = (a.mask && !row_mask) ? a.mask[b * a.m_bs + jc] : (uint8_t)1;
#pragma unroll
      for (int c = 0; c < KCH; ++c) {
        const int slot = DK == 128 ? c ^ (pj & 7) : c;
        *reinterpret_cast<uint4*>(Ks + pj * DK + 16 * slot) = ok ? kv[c] : make_uint4(0, 0, 0, 0);
      }
      if constexpr (DK == 128) {
        const int sw = (j >> 1) & 1;
        uint32_t* vt = reinterpret_cast<uint32_t*>(Vs + j * 128);
        const uint4 lo[4] = {vv[0], vv[1], vv[2], vv[3]}, hi[4] = {vv[4], vv[5], vv[6], vv[7]};
        am_vt_row(lo, ok, vt + 16 * sw);
        am_vt_row(hi, ok, vt + 16 * (1 ^ sw));
      } else {
        // pair f = (v[f], v[16 + f]), two pairs per dword
        const uint32_t w[8] = {vv[0].x, vv[0].y, vv[0].z, vv[0].w, vv[1].x, vv[1].y, vv[1].z, vv[1].w};
        uint32_t o[8];
#pragma unroll
        for (int p = 0; p < 8; ++p) {
          const int f0 = 2 * p, f1 = 2 * p + 1;
          const uint32_t a0 = (w[f0 >> 2] >> (8 * (f0 & 3))) & 0xffu, b0 = (w[4 + (f0 >> 2)] >> (8 * (f0 & 3))) & 0xffu;
          const uint32_t a1 = (w[f1 >> 2] >> (8 * (f1 & 3))) & 0xffu, b1 = (w[4 + (f1 >> 2)] >> (8 * (f1 & 3))) & 0xffu;
          o[p] = ok ? (a0 | (b0 << 8) | (a1 << 16) | (b1 << 24)) : 0u;
        }
        uint4* vt = reinterpret_cast<uint4*>(Vs + j * 32);
        vt[0] = make_uint4(o[0], o[1], o[2], o[3]);
        vt[1] = make_uint4(o[4], o[5], o[6], o[7]);
      }
      sks[pj] = ok ? skj : 0.0f;
      svs[j] = ok ? svj : 0.0f;
      mks[pj] = ok ? mj : (uint8_t)1;
    }
  }
  // this wave's query fragment (MFMA B operand: query row fr) and row scale
  const int qrow = min(r0 + fr, Sq - 1);
  const int8_t* qp = a.q + b * a.q_bs + (long)qrow * a.q_ld + hoff;
  v4i qf[2] = {v4i{0, 0, 0, 0}, v4i{0, 0, 0, 0}};
  long qf8 = 0;
  if constexpr (DK == 128) {
    qf[0] = *reinterpret_cast<const v4i*>(qp + 16 * fg);
    qf[1] = *reinterpret_cast<const v4i*>(qp + 64 + 16 * fg);
  } else {
    qf8 = *reinterpret_cast<const long*>(qp + 8 * fg);
  }
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
      v4i sc4 = v4i{0, 0, 0, 0};
      if constexpr (DK == 128) {
#pragma unroll
        for (int t = 0; t < 2; ++t) {
          const v4i kf = *reinterpret_cast<const v4i*>(Ks + krow * 128 + 16 * ((4 * t + fg) ^ (krow & 7)));
          sc4 = __builtin_amdgcn_mfma_i32_16x16x64_i8(kf, qf[t], sc4, 0, 0, 0);
        }
      } else {
        const long kf = *reinterpret_cast<const long*>(Ks + krow * 32 + 8 * fg);
        sc4 = __builtin_amdgcn_mfma_i32_16x16x32_i8(kf, qf8, sc4, 0, 0, 0);
      }
      const int k0 = 16 * kt + 4 * fg;         // staged rows k0..k0+3
      const float4 skv = *reinterpret_cast<const float4*>(sks + k0);
      const uint32_t mk = *reinterpret_cast<const uint32_t*>(mks + k0);
      float s4[4] = {((float)sc4[0] * sqr) * skv.x, ((float)sc4[1] * sqr) * skv.y,
                     ((float)sc4[2] * sqr) * skv.z, ((float)sc4[3] * sqr) * skv.w};
      div_const_n<4>(s4, HdC<DK>::c);          // the correctly rounded quotients (wave-uniform vote)
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const int key = 16 * kt + 4 * e + fg;
        float sc = s4[e];
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

  // ---- softmax of row fr over its key slots (32 NB in the lane, 4 lanes): the canonical
  // trees of k_attn_mfma_long ----------------------------------------------------------------
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
  DivRange rg;
#pragma unroll
  for (int kt = 0; kt < NT; ++kt)
#pragma unroll
    for (int e = 0; e < 4; ++e) rg.add(x[kt][e]);
  const bool fast = __ballot(!(rg.ok() && divisor_ok(den))) == 0ull;
  const float rden = 1.0f / den;
#pragma unroll
  for (int kt = 0; kt < NT; ++kt) {      // (the choice per tile: k_attn_mfma_long's register note)
    float qt[4];
    if (fast) {
#pragma unroll
      for (int e = 0; e < 4; ++e) qt[e] = div_cr(x[kt][e], den, rden);
    } else {
#pragma unroll
      for (int e = 0; e < 4; ++e) qt[e] = x[kt][e] / den;
    }
#pragma unroll
    for (int e = 0; e < 4; ++e) x[kt][e] = div127(rintf(qt[e] * 127.0f));   // keys >= Sk: P = 0
  }

  // ---- PV on fp32 MFMA: A = P[row fr][k] (the lane's x[s/4][s%4], k = 4s + fg),
  // B = float(v[k][d]) * s_v[k]; DEC: A = RN(P * s_v[k]), B = float(v[k][d]), step s to chain
  // s & 3, summed (c0 + c1) + (c2 + c3).  TILES dim tiles in passes of NDT ---------------------
  constexpr int TILES = DK / 16;
  constexpr int NCH = DEC ? 4 : 1;
  constexpr int NDT = DEC ? 2 : (TILES < 4 ? TILES : 4);
  auto vread = [&](int k, int dt0) -> uint32_t {   // the V bytes of key k, column f = fr
    if constexpr (DK == 128)
      return reinterpret_cast<const uint32_t*>(Vs)[k * 32 + 16 * ((dt0 >> 2) ^ ((k >> 1) & 1)) + fr];
    else
      return reinterpret_cast<const uint16_t*>(Vs)[k * 16 + fr];
  };
  static_for<TILES / NDT>([&](auto pc) {
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
        const float vf = (float)(int8_t)(vd >> (8 * ((dt0 + d) & 3)));
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
          vd[i] = vread(k, dt0);
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
            step(std::integral_constant<int, s4>{}, svs[k], vread(k, dt0));
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

template <int DK, bool DEC>
static hipError_t launch_hd_nb(const AttnArgs& a, hipStream_t st) {
  const dim3 grid(a.H, a.B, (a.Sq + 63) / 64), block(256);
  switch ((a.Sk + 127) / 128) {
    case 1: k_attn_mfma_hd<DK, DEC, 1><<<grid, block, 0, st>>>(a); break;
    case 2: k_attn_mfma_hd<DK, DEC, 2><<<grid, block, 0, st>>>(a); break;
    case 3: k_attn_mfma_hd<DK, DEC, 3><<<grid, block, 0, st>>>(a); break;
    default: k_attn_mfma_hd<DK, DEC, 4><<<grid, block, 0, st>>>(a); break;
  }
  return hipGetLastError();
}

// a.dk 32 or 128, host-known counts, 1 .. 512 keys; rows 16-byte aligned (vector loads)
hipError_t launch_attention_mfma_hd(const AttnArgs& a, hipStream_t st) {
  if (a.sk_dev || a.qpos_dev || a.Sk <= 0 || a.Sk > AMH_MAXK || a.H <= 0 || a.H > 65535 ||
      (a.dk != 32 && a.dk != 128) || (a.q_ld % 16) || (a.k_ld % 16) || (a.v_ld % 16) ||
      (a.q_bs % 16) || (a.k_bs % 16) || (a.v_bs % 16))
    return hipErrorInvalidValue;
  if (a.dk == 128) return a.dec ? launch_hd_nb<128, true>(a, st) : launch_hd_nb<128, false>(a, st);
  return a.dec ? launch_hd_nb<32, true>(a, st) : launch_hd_nb<32, false>(a, st);
}

// =====================================================================================
// k_attention_hd: k_attention (qtx_kernels.hip) with the head width as a parameter — one
// workgroup (4 waves) per (head, batch), K (rows padded by one dword), V and the key scales
// staged once, each wave walking query rows; the device-counter forms (sk_dev / qpos_dev) of
// the unfused step.  PV: lane = column; DK = 128 two columns per lane, DK = 32 half the lanes.
// Like k_attention it declares LDS for 512 keys whatever Sk is (DK = 128: 142 KB, one workgroup
// per CU even at a handful of keys): accepted for the unfused step, which is no hot path.
// =====================================================================================
template <int DK>
__global__ __launch_bounds__(256) void k_attention_hd(AttnArgs a) {
  constexpr int KW = DK / 4;               // dwords of a row
  constexpr int NC = DK == 128 ? 2 : 1;    // columns per lane
  __shared__ uint32_t Ks[AMH_MAXK * (KW + 1)];
  __shared__ uint8_t Vs[AMH_MAXK * DK];
  __shared__ float sks[AMH_MAXK], svs[AMH_MAXK];
  __shared__ float Pb[4][AMH_MAXK];
  const int h = blockIdx.x, b = blockIdx.y;
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int Sk = min(max(a.sk_dev ? (*a.sk_dev + a.sk_add) : a.Sk, 0), AMH_MAXK);
  const int hoff = h * DK;

  const int8_t* kb = a.k + b * a.k_bs + hoff;
  const int8_t* vb = a.v + b * a.v_bs + hoff;
  for (int idx = tid; idx < Sk * KW; idx += 256) {
    const int j = idx / KW, w = idx % KW;
    Ks[j * (KW + 1) + w] = *reinterpret_cast<const uint32_t*>(kb + (long)j * a.k_ld + 4 * w);
    *reinterpret_cast<uint32_t*>(Vs + j * DK + 4 * w) =
        *reinterpret_cast<const uint32_t*>(vb + (long)j * a.v_ld + 4 * w);
  }
  for (int j = tid; j < Sk; j += 256) {
    sks[j] = a.sk[b * a.sk_bs + j];
    svs[j] = a.sv[b * a.sv_bs + j];
  }
  __syncthreads();

  float* P = Pb[wave];
  for (int i = wave; i < a.Sq; i += 4) {
    const int8_t* qr = a.q + b * a.q_bs + (long)i * a.q_ld + hoff;
    uint32_t qd[KW];
#pragma unroll
    for (int w = 0; w < KW / 4; ++w) {
      const uint4 t = *reinterpret_cast<const uint4*>(qr + 16 * w);
      qd[4 * w] = t.x; qd[4 * w + 1] = t.y; qd[4 * w + 2] = t.z; qd[4 * w + 3] = t.w;
    }
    const float sqi = a.sq[b * a.sq_bs + i];
    const int mrow = a.qpos_dev ? (*a.qpos_dev + i) : i;
    const uint8_t* mk = a.mask ? a.mask + b * a.m_bs + (long)mrow * a.m_is : nullptr;
    float lmax = -3.0e38f;
    for (int j = lane; j < Sk; j += 64) {
      int acc = 0;
#pragma unroll
      for (int w = 0; w < KW; ++w) acc = __builtin_amdgcn_sdot4(qd[w], Ks[j * (KW + 1) + w], acc, false);
      float s = (((float)acc * sqi) * sks[j]) / HdC<DK>::c;
      if (mk && mk[j] == 0) s = -1.0e9f;
      P[j] = s;
      lmax = fmaxf(lmax, s);
    }
    const float m = wave_max(lmax);
    float lsum = 0.0f;
    for (int j = lane; j < Sk; j += 64) {
      const float e = qexp(P[j] - m);
      P[j] = e;
      lsum = lsum + e;
    }
    const float den = wave_sum(lsum);
    for (int j = lane; j < Sk; j += 64) P[j] = rintf((P[j] / den) * 127.0f) / 127.0f;
    __builtin_amdgcn_wave_barrier();
#pragma unroll
    for (int cc = 0; cc < NC; ++cc) {
      const int col = lane + 64 * cc;
      if (col < DK) {
        float acc = 0.0f;
        if (a.dec) {   // the decoder's PV order (qtx_common.h pv_dec_chains)
          acc = pv_dec_chains(Sk, [&](int j) { return P[j] * svs[j]; },
                              [&](int j) { return (float)(int8_t)Vs[j * DK + col]; });
        } else {
          for (int j = 0; j < Sk; ++j)
            acc = fmaf(P[j], (float)(int8_t)Vs[j * DK + col] * svs[j], acc);
        }
        a.ctx[b * a.c_bs + (long)i * a.c_ld + hoff + col] = acc;
      }
    }
    __builtin_amdgcn_wave_barrier();
  }
}

hipError_t launch_attention_valu_hd(const AttnArgs& a, hipStream_t st) {
  if ((a.dk != 32 && a.dk != 128) || a.H <= 0 || a.H > 65535 || (a.q_ld % 16) || (a.k_ld % 4) ||
      (a.v_ld % 4) || (a.q_bs % 16) || (a.k_bs % 4) || (a.v_bs % 4) ||
      (!a.sk_dev && (a.Sk <= 0 || a.Sk > AMH_MAXK)))
    return hipErrorInvalidValue;
  const dim3 grid(a.H, a.B), block(256);
  if (a.dk == 128) k_attention_hd<128><<<grid, block, 0, st>>>(a);
  else k_attention_hd<32><<<grid, block, 0, st>>>(a);
  return hipGetLastError();
}

// =====================================================================================
// k_dec_attn_hd (header comment above; phases as k_dec_attn_long, qtx_decode_long.hip)
//   NH  heads per workgroup (DK = 32: 2; DK = 128: 1)
//   KS  64-byte k-steps per key fragment (DK = 128: 2; DK = 32: 1 — the block's 64 columns
//       are its two heads)
// =====================================================================================
template <int DK, bool KV_NEW>
__global__ __launch_bounds__(256) void k_dec_attn_hd(QTX_KA_PARAMS, DaTail kt) {
  static_assert(DK == 32 || DK == 128, "head widths 32 and 128");
  constexpr int NH = DK == 32 ? 2 : 1;
  constexpr int KS = DK == 128 ? 2 : 1;
  const DecAttnArgs a = da_args<KV_NEW>(QTX_KA_VALS, kt);
  __shared__ __attribute__((aligned(16))) float E[NH][DEC_LONG_MAXK];    // qexp(score - max), 0 past Sk
  __shared__ __attribute__((aligned(16))) float PS[NH][DEC_LONG_MAXK];   // RN(P_j * s_v[j]), 0 past Sk
  __shared__ float part[4][64];                                      // the chains' partial sums
  __shared__ __attribute__((aligned(16))) int8_t qs[2 * 64 * KS];    // q codes, then the new k codes
  __shared__ float wmax[NH][4];
  __shared__ int wlast[4];
  const int b = blockIdx.x, blk = blockIdx.y;      // blk: the 64-column block this workgroup owns
  const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63;
  const int fr = lane & 15, fg = lane >> 4;    // MFMA fragment: column (key) fr, byte chunk fg
  const int c0 = DK == 128 ? (blk >> 1) * 128 : blk * 64;   // first column the scores read
  const int hd = DK == 32 ? lane >> 5 : 0;     // the head (of the block) of column `lane`
  const float* yr = a.y + (long)b * a.ldy;

  // phase 0: this step's q (k, v) rows, the position, this wave's key block, scales, mask
  // bytes and value dwords — all issued before any is consumed
  float4 yq[2], yk[2], yv[2];
#pragma unroll
  for (int c = 0; c < 2; ++c) {
    yq[c] = *reinterpret_cast<const float4*>(yr + 4 * (lane + 64 * c));
    if constexpr (KV_NEW) {
      yk[c] = *reinterpret_cast<const float4*>(yr + 512 + 4 * (lane + 64 * c));
      yv[c] = *reinterpret_cast<const float4*>(yr + 1024 + 4 * (lane + 64 * c));
    }
  }
  float q_own[KS], k_own[KS];
#pragma unroll
  for (int t = 0; t < KS; ++t) {
    q_own[t] = yr[c0 + 64 * t + lane];
    k_own[t] = KV_NEW ? yr[512 + c0 + 64 * t + lane] : 0.0f;
  }
  const float v_own = KV_NEW ? yr[1024 + blk * 64 + lane] : 0.0f;
  __builtin_amdgcn_sched_barrier(0);
  // clamped: a stale position (a counter not reset) must not index past the cache
  const int step = !KV_NEW ? 0 : a.host_step1 > 0 ? a.host_step1 - 1 : min(max(*a.step, 0), (int)a.kv_bs - 1);
  const int nrows = KV_NEW ? step + 1 : a.S;           // rows loaded: 1 .. min(kv_bs, 512)
  const int r0 = 128 * w;                              // this wave's key block
  const int nw = min(max(nrows - r0, 0), 128);         // its live rows (0: the wave scores nothing)
  const long kvb = (long)b * a.kv_bs;
  const long vgb = (long)b * ((a.kv_bs + 3) >> 2);     // the sentence's first value group
  const int glast = (nrows - 1) >> 2;                  // the last loaded 4-key value group
  const int8_t* const kbase = a.kc + kvb * 512 + c0;
  const int8_t* const vbase = a.vc + vgb * 2048 + blk * 256;
  uint4 kr[8][KS];
#pragma unroll
  for (int i = 0; i < 8; ++i)
#pragma unroll
    for (int t = 0; t < KS; ++t) {
      kr[i][t] = make_uint4(0, 0, 0, 0);
      if (16 * i < nw) {                               // wave-uniform
        const unsigned koff = (unsigned)(min(r0 + 16 * i + fr, nrows - 1) * 512 + 64 * t + 16 * fg);
        kr[i][t] = __builtin_bit_cast(uint4, __builtin_nontemporal_load(reinterpret_cast<const v4i*>(kbase + koff)));
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
  // chain w's value dwords: fragment g's group 4 g + w, column = lane; groups clamped to the
  // last loaded one
  uint32_t vg[32];
  __builtin_amdgcn_sched_barrier(0);
#pragma unroll
  for (int G = 0; G < 8; ++G)
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int g = 4 * G + q;
      vg[g] = 0u;
      asm("" : "+v"(vg[g]));     // (the zero pinned to a VGPR: k_dec_attn_long's note)
      if (64 * G < nrows)
        vg[g] = __builtin_nontemporal_load(
            reinterpret_cast<const uint32_t*>(vbase + (unsigned)(min(4 * g + w, glast) * 2048 + 4 * lane)));
    }
  if constexpr (!KV_NEW) {       // cross: this wave's last unmasked key + 1 (0: none)
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
    sq = am[0];
    const float sk = am[1], sv = am[2];
    int8_t kq[KS], qq[KS];
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
      const long row = kvb + step;
      // cache append: this workgroup's 64 columns (DK = 128: its half of the head's key)
      const int to = DK == 128 ? blk & 1 : 0;
      a.kc[row * 512 + blk * 64 + lane] = kq[to];
      a.vc[((vgb + (step >> 2)) * 512 + blk * 64 + lane) * 4 + (step & 3)] = vq;
      if (blk == 0 && lane == 0) { a.skc[row] = sk; a.svc[row] = sv; }
#pragma unroll
      for (int t = 0; t < KS; ++t) {
        qs[64 * t + lane] = qq[t];
        qs[64 * KS + 64 * t + lane] = kq[t];
      }
    }
    if (r0 + lane == step) { sk0 = sk; sv0 = sv; }          // the new scales in the lane that
    if (r0 + lane + 64 == step) { sk1 = sk; sv1 = sv; }     // scores the key
  } else {
    sq = absmax_scale127(wave_absmax(lmax8(yq), 1e-5f));
#pragma unroll
    for (int t = 0; t < KS; ++t) {
      const int code = quant_one(q_own[t], sq);
      if (w == 0) qs[64 * t + lane] = (int8_t)code;
    }
  }
  __syncthreads();

  // phase 2: operand fragments and the key count.  A: the q codes' chunk fg in every row —
  // DK = 32: row parity picks the head, the other head's bytes zero
  v4i qf[KS];
#pragma unroll
  for (int t = 0; t < KS; ++t) qf[t] = *reinterpret_cast<const v4i*>(qs + 64 * t + 16 * fg);
  if constexpr (DK == 32)
    if ((fr & 1) != (fg >> 1)) qf[0] = v4i{0, 0, 0, 0};
  if constexpr (KV_NEW) {
    const bool own = w == (step >> 7) && fr == (step & 15);
#pragma unroll
    for (int t = 0; t < KS; ++t) {
      const uint4 kn = *reinterpret_cast<const uint4*>(qs + 64 * KS + 64 * t + 16 * fg);
#pragma unroll
      for (int i = 0; i < 8; ++i)
        if (i == ((step >> 4) & 7) && own) kr[i][t] = kn;
    }
  }
  int Sk = nrows;
  if constexpr (!KV_NEW) {
    const int last = __builtin_amdgcn_readfirstlane(max(max(wlast[0], wlast[1]), max(wlast[2], wlast[3])));
    if (last > 0) Sk = last;
  }

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
    div_const_n<NH * 2>(flat, HdC<DK>::c);     // the correctly rounded quotients
#pragma unroll
    for (int hh = 0; hh < NH; ++hh) { sc[hh][0] = flat[2 * hh]; sc[hh][1] = flat[2 * hh + 1]; }
  }
#pragma unroll
  for (int hh = 0; hh < NH; ++hh) {
    float lmax = -3.0e38f;
#pragma unroll
    for (int u = 0; u < 2; ++u) {
      if (!(u ? keep1 : keep0)) sc[hh][u] = -1.0e9f;
      lmax = live[u] ? fmaxf(lmax, sc[hh][u]) : lmax;
    }
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
  // 16 g + 4 w + (0 .. 3), g in key order
  if constexpr (KV_NEW) {
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
    if (64 * G < Sk) {                                 // wave-uniform (Sk <= nrows: vg loaded)
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
      const float am = wave_max(fabsf(ctx));
      if (lane == 0) a.pmax[(long)blk * a.B + b] = am;
    }
  }
}

template <int DK>
static hipError_t launch_dec_hd(const DecAttnArgs& a, int B, hipStream_t st) {
  const dim3 grid(B, 8), block(256);
  const DaTail t{a.step, a.mask, a.ctx, a.pmax, a.B};
  if (a.kv_new) {
    const KaLead l = da_lead<true>(a);
    k_dec_attn_hd<DK, true><<<grid, block, 0, st>>>(QTX_KA_ARGS(l), t);
  } else {
    const KaLead l = da_lead<false>(a);
    k_dec_attn_hd<DK, false><<<grid, block, 0, st>>>(QTX_KA_ARGS(l), t);
  }
  return hipGetLastError();
}

// a (validated by launch_dec_attn) with a.dk 32 or 128 and 1 .. 512 rows to load
hipError_t launch_dec_attn_hd(const DecAttnArgs& a, int B, hipStream_t st) {
  const int nrows = a.kv_new ? (a.host_step1 > 0 ? a.host_step1 : (int)a.kv_bs) : a.S;
  if (nrows <= 0 || nrows > DEC_LONG_MAXK || a.kv_bs < nrows || (long)B * 512 >= (1L << 29) ||
      (a.dk != 32 && a.dk != 128))
    return hipErrorInvalidValue;
  return a.dk == 128 ? launch_dec_hd<128>(a, B, st) : launch_dec_hd<32>(a, B, st);
}

}  // namespace qtx

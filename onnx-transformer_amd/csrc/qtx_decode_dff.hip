// qtx_decode_dff.hip — the decode step's FFN2 for the feed-forward widths between the two
// flagship ones: K = d_ff = 256 q, q = 1, 3, 4, 5, 6, 7 (gfx950, wave64; q = 2 and 8 are
// qtx_decode.hip's K = 512 and 2048).
//
//   k_skinny8_dff   M <= QTX_SKINNY8_MAXM rows: the fp32 hidden quantized per token in the
//                   prologue (quant_linear.py:30-43), 8 waves, the 4 q MFMA k-steps dealt
//                   round-robin to them, residual epilogue — k_skinny8_ffn2's work split at any q
//   k_skinny<K>     the other row regimes: the K-split template of qtx_skinny.h at the new K
//
// Same int32 sums (any split of an integer sum is exact) and the same epilogue expression as
// k_skinny: bit for bit its results, and the oracle's.
#include "qtx_common.h"
#include "qtx_decode_ka.h"
#include "qtx_kernels.h"
#include "qtx_knobs.h"
#include "qtx_skinny.h"

namespace qtx {

// =====================================================================================
// k_skinny8_dff<Q, OWN>: out[4 rows, 16 columns] = res + (quant(X) . W^T) s_a s_w + bias,
// K = 256 Q, one 8-wave workgroup per tile (the latency-bound step is fastest with many
// small workgroups: qtx_decode.hip, above skinny_mode).
//   quantization  row r belongs to waves 2 r and 2 r + 1; each quantizes one half of it,
//                 128 Q floats = 2 Q per lane: Q / 2 float4 loads for even Q, Q float2 loads
//                 for odd Q (the half row is then no multiple of 256 floats).  OWN (A_F32R):
//                 the wave loads the other half too, for the row maximum alone, so the two
//                 waves of a row agree on the scale without meeting in LDS; else (A_F32Q) both
//                 reduce FFN1's per-tile maxima.
//   k-steps       K / 64 = 4 Q steps of v_mfma_i32_16x16x64_i8, step s to wave s mod 8: at
//                 most ceil(Q / 2) <= 4 weight fragments (uint4) per lane.  For odd Q waves
//                 0-3 carry one step more than waves 4-7 (their fragment load of that round
//                 is clamped to the last step and not used); for Q = 1 waves 4-7 carry none
//                 and stay out of the reduction.
//   reduction     exact int32 over the carrying waves in LDS; wave 0 writes one output per lane.
// Order of the global loads: the A rows, then the weight fragments and the epilogue operands —
// all issued before the first is consumed (qtx_skinny.h, skinny_prologue).
// LDS: A panel 16 x (K + 16) bytes (rows 4-15 are never written: their C rows are not read),
// 4 scales, min(8, 4 Q) x 1 KB of partial sums.  No scratch.
// =====================================================================================
template <int Q, bool OWN>
__global__ __launch_bounds__(512) void k_skinny8_dff(QTX_KA_PARAMS, SkTail kt) {
  const SkinnyArgs g = sk_args<OWN ? A_F32R : A_F32Q>(QTX_KA_VALS, kt);
  constexpr int K = 256 * Q, RB = 4, LDA = K + 16;
  constexpr int NST = K / 64;              // k-steps in all
  constexpr int NS = (NST + 7) / 8;        // rounds: the most steps one wave carries
  constexpr int NW = NST < 8 ? NST : 8;    // waves that carry a step
  constexpr bool V4 = Q % 2 == 0;          // float4 loads (else float2)
  constexpr int VW = V4 ? 4 : 2, NC = 2 * Q / VW, HALF = 128 * Q;
  static_assert(Q >= 1 && Q <= 8 && NS <= 4, "at most 4 weight fragments per lane");
  __shared__ __attribute__((aligned(16))) uint8_t As[16 * LDA];
  __shared__ float sas[RB];
  __shared__ v4i red[NW][64];
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int fr = lane & 15, fg = lane >> 4;
  const int n0 = blockIdx.x * 16, m0 = blockIdx.y * RB;
  // 1. the A operand's loads first: row r = wave / 2, half h = wave & 1 (columns HALF h ..)
  const int r = wave >> 1, half = wave & 1;
  const int m = min(m0 + r, g.M - 1);
  auto load_half = [&](int h, float (&v)[2 * Q]) {
#pragma unroll
    for (int c = 0; c < NC; ++c) {
      const unsigned off = 4u * (unsigned)(m * (int)g.ldx + HALF * h + VW * (lane + 64 * c));
      if constexpr (V4) {
        const float4 u = ld_at(reinterpret_cast<const float4*>(g.X), off);
        v[4 * c] = u.x; v[4 * c + 1] = u.y; v[4 * c + 2] = u.z; v[4 * c + 3] = u.w;
      } else {
        const float2 u = ld_at(reinterpret_cast<const float2*>(g.X), off);
        v[2 * c] = u.x; v[2 * c + 1] = u.y;
      }
    }
  };
  float t[2 * Q], to[2 * Q];   // to: OWN, the row's other half
  float pm[2] = {0.0f, 0.0f};
  load_half(half, t);
  if constexpr (OWN) {
    load_half(half ^ 1, to);
  } else {
#pragma unroll
    for (int u = 0; u < 2; ++u)   // partials lane, lane + 64 (clamped: max-safe)
      pm[u] = ld_at(g.pmax_in, 4u * (unsigned)(min(lane + 64 * u, g.pmax_n - 1) * g.M + m));
  }
  // 2. then this wave's weight fragments: round j is step wave + 8 j
  const int n = min(n0 + fr, g.N - 1);
  uint4 wf[NS];
#pragma unroll
  for (int j = 0; j < NS; ++j) {
    const int s = min(wave + 8 * j, NST - 1);   // (a round not every wave carries: clamped)
    wf[j] = ld_at(reinterpret_cast<const uint4*>(g.W), (unsigned)(n * (int)g.ldw + 64 * s + 16 * fg));
  }
  const int col = n0 + fr, cc = min(col, g.N - 1);
  const bool cok = col < g.N;
  const float swc = ld_at(g.sw, 4u * cc);
  __builtin_amdgcn_sched_barrier(0);   // as in k_skinny: trailing arguments from here on
  // the epilogue's output of this lane (wave 0): row m0 + (lane >> 4), column n0 + (lane & 15)
  const float rv = ld_at(g.res, 4u * (unsigned)(min(m0 + fg, g.M - 1) * (int)g.ldr + cc));
  const float bc = ld_at(g.bias, 4u * cc);
  // 3. per-token quantization of the half row into LDS
  {
    const bool ok = m0 + r < g.M;
    float sc;
    if constexpr (OWN) {
      float lm = 0.0f;     // (>= +0, NaN dropped: wave_absmax's precondition)
#pragma unroll
      for (int i = 0; i < 2 * Q; ++i) lm = fmaxf(lm, fmaxf(fabsf(t[i]), fabsf(to[i])));
      sc = absmax_scale127(wave_absmax(lm, 1e-5f));   // quant_scale, its 1e-5 floor in the maximum
    } else {
      sc = quant_scale(wave_max(fmaxf(pm[0], pm[1])), 127.0f);
    }
    if constexpr (V4) {
      uint32_t qd[NC];
      quant_pack<2 * Q>(t, sc, qd);
      uint32_t* dst = reinterpret_cast<uint32_t*>(As + r * LDA + HALF * half);
#pragma unroll
      for (int c = 0; c < NC; ++c) dst[lane + 64 * c] = ok ? qd[c] : 0u;
    } else {
      // 2 Q values are no whole number of dwords: two zeros fill the last one (code 0, no part
      // in the near-tie vote), and load c's two codes are one halfword of dword c / 2
      float tf[2 * Q + 2];
#pragma unroll
      for (int i = 0; i < 2 * Q; ++i) tf[i] = t[i];
      tf[2 * Q] = tf[2 * Q + 1] = 0.0f;
      uint32_t qd[(Q + 1) / 2];
      quant_pack<2 * Q + 2>(tf, sc, qd);
      uint16_t* dst = reinterpret_cast<uint16_t*>(As + r * LDA + HALF * half);
#pragma unroll
      for (int c = 0; c < NC; ++c)
        dst[lane + 64 * c] = ok ? (uint16_t)(qd[c >> 1] >> (16 * (c & 1))) : (uint16_t)0;
    }
    if (lane == 0 && half == 0) sas[r] = ok ? sc : 0.0f;
  }
  __syncthreads();
  // 4. MFMA over this wave's k-steps, exact int32 reduction over the carrying waves
  v4i acc = v4i{0, 0, 0, 0};
#pragma unroll
  for (int j = 0; j < NS; ++j) {
    const int s = wave + 8 * j;
    if (8 * j + 7 < NST || s < NST) {   // (wave-uniform; every wave carries a full round)
      const v4i afr = *reinterpret_cast<const v4i*>(As + fr * LDA + 64 * s + 16 * fg);
      acc = __builtin_amdgcn_mfma_i32_16x16x64_i8(afr, __builtin_bit_cast(v4i, wf[j]), acc, 0, 0, 0);
    }
  }
  if (NW == 8 || wave < NW) red[wave][lane] = acc;
  __syncthreads();
  if (wave != 0) return;
  // 5. epilogue: out = res + y, as k_skinny8_ffn2's.  The 4 useful rows of the 16-row tile sit
  //    in lanes 0-15 (element e = row); lane l takes row e = l >> 4 of column l & 15, summing
  //    element e of lane l & 15 over the carrying waves
  {
    const int e = fg, src = fr;
    int sum = 0;
#pragma unroll
    for (int w = 0; w < NW; ++w) sum += reinterpret_cast<const int*>(&red[w][src])[e];
    const int row = m0 + e;
    const float y = ((float)sum * sas[e]) * swc + bc;
    if (cok && row < g.M) st_at(g.out, 4u * (unsigned)(row * (int)g.ldo + col), rv + y);
  }
}

// ---- dispatch ---------------------------------------------------------------------------
// k_skinny at the new K: the epilogues the step and the per-op entry use (none, residual)
template <int K, int AM, int RB>
hipError_t dff_flags(const SkinnyArgs& g, hipStream_t st) {
  const dim3 grid(g.N / 16, (g.M + RB - 1) / RB);
  if (g.flags == 0) QTX_SK_LAUNCH(AM, grid, 256, k_skinny<1, RB, K, 8, AM, 0>);
  else if (g.flags == EPI_RESIDUAL) QTX_SK_LAUNCH(AM, grid, 256, k_skinny<1, RB, K, 8, AM, EPI_RESIDUAL>);
  else return hipErrorInvalidValue;
  return hipGetLastError();
}
// the fp32 prologues with 4-, 8- and 16-row blocks; the int8 panel (the >= 96-row path's
// quantizer kernel, QTX_FFN_QKERNEL) with 4- and 16-row blocks
template <int K, int AM>
hipError_t dff_rb(const SkinnyArgs& g, int rb, hipStream_t st) {
  switch (rb) {
    case 4: return dff_flags<K, AM, 4>(g, st);
    case 8: if constexpr (AM != A_I8) return dff_flags<K, AM, 8>(g, st); else break;
    case 16: return dff_flags<K, AM, 16>(g, st);
  }
  return hipErrorInvalidValue;
}

template <int Q>
hipError_t dff_mode(const SkinnyArgs& g, hipStream_t st) {
  constexpr int K = 256 * Q;
  const Knobs& kn = knobs();     // QTX_RB_* / QTX_SKINNY8_MAXM: QTX_DIAG build
  // the step's FFN2 (fp32 hidden, residual) at M <= QTX_SKINNY8_MAXM (default 32), as K = 2048
  if (g.M <= kn.skinny8_maxm && g.flags == EPI_RESIDUAL &&
      ((g.amode == A_F32Q && g.pmax_n <= 128) || g.amode == A_F32R)) {
    const dim3 grid(g.N / 16, (g.M + 3) / 4);
    if (g.amode == A_F32R) QTX_SK_LAUNCH(A_F32R, grid, 512, k_skinny8_dff<Q, true>);
    else QTX_SK_LAUNCH(A_F32Q, grid, 512, k_skinny8_dff<Q, false>);
    return hipGetLastError();
  }
  // rows per workgroup by M exactly as skinny_mode's K = 2048 branch
  const bool big = g.M >= 96;
  const int rb_i8 = kn.rb_i8_2048 > 0 ? kn.rb_i8_2048 : (big ? 16 : 4);
  const int rb_f = kn.rb_f32q > 0 ? kn.rb_f32q : (g.M >= 192 ? 16 : big ? 8 : 4);
  if (g.amode == A_I8) return dff_rb<K, A_I8>(g, rb_i8, st);
  if (g.amode == A_F32Q) return dff_rb<K, A_F32Q>(g, rb_f, st);
  if (g.amode == A_F32R) return dff_rb<K, A_F32R>(g, rb_f, st);
  return hipErrorInvalidValue;   // (the LayerNorm prologue is K = 512 only)
}

hipError_t launch_skinny_dff(const SkinnyArgs& g, hipStream_t st) {
  switch (g.K) {
    case 256: return dff_mode<1>(g, st);
    case 768: return dff_mode<3>(g, st);
    case 1024: return dff_mode<4>(g, st);
    case 1280: return dff_mode<5>(g, st);
    case 1536: return dff_mode<6>(g, st);
    case 1792: return dff_mode<7>(g, st);
    default: return hipErrorInvalidValue;
  }
}

}  // namespace qtx

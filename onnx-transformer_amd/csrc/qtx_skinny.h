// qtx_skinny.h — the skinny GEMM's shared pieces: the lead blocks of its kernel-argument
// preload, the A-operand prologue and k_skinny itself.  qtx_decode.hip instantiates them for
// K = 512 and 2048, qtx_decode_dff.hip for the other FFN2 widths (K = d_ff = 256 q); both are
// built with -amdgpu-kernarg-preload-count (qtx/_build.py).
#pragma once
#include "qtx_common.h"
#include "qtx_decode_ka.h"
#include "qtx_kernels.h"

namespace qtx {

__device__ __forceinline__ uint4 unpack_i4(uint2 h) {
  auto sext = [](uint32_t v) { return v | ((v & 0x08080808u) * 0x1Eu); };
  const uint32_t lo0 = sext(h.x & 0x0F0F0F0Fu), hi0 = sext((h.x >> 4) & 0x0F0F0F0Fu);
  const uint32_t lo1 = sext(h.y & 0x0F0F0F0Fu), hi1 = sext((h.y >> 4) & 0x0F0F0F0Fu);
  uint4 o;
  o.x = __builtin_amdgcn_perm(hi0, lo0, 0x05010400u);
  o.y = __builtin_amdgcn_perm(hi0, lo0, 0x07030602u);
  o.z = __builtin_amdgcn_perm(hi1, lo1, 0x05010400u);
  o.w = __builtin_amdgcn_perm(hi1, lo1, 0x07030602u);
  return o;
}

// The skinny GEMMs' lead blocks (no padding: every byte is a field), roughly in order of first
// use (all 14 dwords arrive together); strides are 32-bit (launch_skinny bounds every offset
// by 2^30).  What does not fit — the bias, and for the LayerNorm / partial-maxima prologues the
// residual — is loaded last in the first load burst, after the wait for SkTail.
template <int AMODE> struct SkLead;
template <> struct SkLead<A_I8> {     // (sa is read after the weights are issued: SkTail)
  uint64_t A; int M, N; uint64_t W; int ldw, ldr; uint64_t sw, bias, res;
};
template <> struct SkLead<A_LN> {
  uint64_t X; int M, ldx; uint64_t ln_a, ln_b, W; int ldw, N; uint64_t sw;
};
template <> struct SkLead<A_F32Q> {
  uint64_t X; int M, ldx; uint64_t pmax_in; int pmax_n, ldw; uint64_t W; int N, ldo; uint64_t sw;
};
template <> struct SkLead<A_F32R> {
  uint64_t X; int M, ldx; uint64_t W; int ldw, N; uint64_t sw, res; int ldr, ldo;
};
struct SkTail {   // the epilogue's operands (where a lead block holds one too, the kernel takes that)
  const float* sa; const float* bias; const float* res; float* out; float* pmax_out;
  int ldo, ldr;
};

template <int AMODE> KaLead sk_lead(const SkinnyArgs& g) {
  SkLead<AMODE> l{};
  l.M = g.M; l.N = g.N; l.W = ka_int(g.W); l.ldw = (int)g.ldw; l.sw = ka_int(g.sw);
  if constexpr (AMODE == A_I8) {
    l.A = ka_int(g.A); l.ldr = (int)g.ldr; l.bias = ka_int(g.bias); l.res = ka_int(g.res);
  } else {
    l.X = ka_int(g.X); l.ldx = (int)g.ldx;
    if constexpr (AMODE == A_LN) { l.ln_a = ka_int(g.ln_a); l.ln_b = ka_int(g.ln_b); }
    if constexpr (AMODE == A_F32Q) { l.pmax_in = ka_int(g.pmax_in); l.pmax_n = g.pmax_n; l.ldo = (int)g.ldo; }
    if constexpr (AMODE == A_F32R) { l.res = ka_int(g.res); l.ldr = (int)g.ldr; l.ldo = (int)g.ldo; }
  }
  return ka_pack(l);
}
inline SkTail sk_tail(const SkinnyArgs& g) {
  return SkTail{g.sa, g.bias, g.res, g.out, g.pmax_out, (int)g.ldo, (int)g.ldr};
}
// the kernel's view: SkinnyArgs again (amode / K / flags are template parameters there)
template <int AMODE>
__device__ __forceinline__ SkinnyArgs sk_args(const KaLead& k, const SkTail& t) {
  const SkLead<AMODE> l = __builtin_bit_cast(SkLead<AMODE>, k);
  SkinnyArgs g{};
  g.sa = t.sa; g.bias = t.bias; g.res = t.res; g.out = t.out; g.pmax_out = t.pmax_out;
  g.ldo = t.ldo; g.ldr = t.ldr;
  g.M = l.M; g.N = l.N; g.W = ka_ptr<const int8_t>(l.W); g.ldw = l.ldw;
  g.sw = ka_ptr<const float>(l.sw);
  if constexpr (AMODE == A_I8) {
    g.A = ka_ptr<const int8_t>(l.A); g.ldr = l.ldr; g.bias = ka_ptr<const float>(l.bias);
    g.res = ka_ptr<const float>(l.res);
  } else {
    g.X = ka_ptr<const float>(l.X); g.ldx = l.ldx;
    if constexpr (AMODE == A_LN) { g.ln_a = ka_ptr<const float>(l.ln_a); g.ln_b = ka_ptr<const float>(l.ln_b); }
    if constexpr (AMODE == A_F32Q) { g.pmax_in = ka_ptr<const float>(l.pmax_in); g.pmax_n = l.pmax_n; g.ldo = l.ldo; }
    if constexpr (AMODE == A_F32R) { g.res = ka_ptr<const float>(l.res); g.ldr = l.ldr; g.ldo = l.ldo; }
  }
  return g;
}
// <<<>>> with the blocks unpacked (kernel name last: its template arguments hold commas)
#define QTX_SK_LAUNCH(AM, grid, block, ...)                                          \
  do {                                                                               \
    const KaLead ka_l_ = sk_lead<AM>(g);                                             \
    __VA_ARGS__<<<grid, block, 0, st>>>(QTX_KA_ARGS(ka_l_), sk_tail(g));             \
  } while (0)

// =====================================================================================
// k_skinny
// =====================================================================================
// The A operand of a skinny GEMM workgroup (rows m0 .. m0 + RB - 1) into LDS: int8 rows
// (A_I8), LayerNorm + per-token quant of fp32 rows (A_LN), or per-token quant of fp32 rows
// from their partial maxima (A_F32Q).  Rows >= M are zero; sas = per-row scales.  Every
// branch issues all of its global loads before consuming any (one memory latency, not one
// per row).  Wave w takes rows w, w + 4, ...  issue_rest() (the weight fragments and the
// epilogue operands) is called right after the A operand's loads are issued: vmcnt retires
// in issue order, so the LayerNorm / quantization then waits for its own rows only and
// runs while the weights are in flight (measured: issuing the weights first made the two
// latencies add up, ~0.7 us per launch).
template <int RB, int K, int AMODE, class F>
__device__ __forceinline__ void skinny_prologue(const SkinnyArgs& g, uint8_t* As, float* sas,
                                                int m0, int tid, int wave, int lane,
                                                F&& issue_rest) {
  constexpr int LDA = K + 16;
  constexpr int BM = RB <= 16 ? 16 : 32;
  constexpr int RPW = RB / 4;  // rows per wave: r = wave + 4*j
  if constexpr (AMODE == A_I8) {
    // the panel is RB*K/16 uint4; the index is clamped (a duplicate load, no divergent
    // branch around the load) and only in-range indices are stored
    constexpr int CPR = K / 16, TOT = RB * CPR, NLD = (TOT + 255) / 256;
    uint4 v[NLD];
#pragma unroll
    for (int j = 0; j < NLD; ++j) {
      const int idx = min(tid + 256 * j, TOT - 1), m = min(m0 + idx / CPR, g.M - 1);
      v[j] = ld_at(reinterpret_cast<const uint4*>(g.A), (unsigned)(m * K + 16 * (idx % CPR)));
    }
    issue_rest();
    if (tid < BM) sas[tid] = (tid < RB && m0 + tid < g.M) ? g.sa[m0 + tid] : 0.0f;
#pragma unroll
    for (int j = 0; j < NLD; ++j) {
      const int idx = tid + 256 * j, r = idx / CPR;
      if (TOT % 256 == 0 || idx < TOT)
        *reinterpret_cast<uint4*>(As + r * LDA + 16 * (idx % CPR)) =
            (m0 + r < g.M) ? v[j] : make_uint4(0, 0, 0, 0);
    }
  } else if constexpr (AMODE == A_LN) {
    float v[RPW][2][4];
#pragma unroll
    for (int j = 0; j < RPW; ++j) {
      const int m = min(m0 + wave + 4 * j, g.M - 1);
#pragma unroll
      for (int c = 0; c < 2; ++c) {
        const float4 t = ld_at(reinterpret_cast<const float4*>(g.X), 4u * (unsigned)(m * (int)g.ldx + 4 * (lane + 64 * c)));
        v[j][c][0] = t.x; v[j][c][1] = t.y; v[j][c][2] = t.z; v[j][c][3] = t.w;
      }
    }
    float ga[2][4], gb[2][4];
    ln_params512(g.ln_a, g.ln_b, lane, ga, gb);
    issue_rest();
    uint32_t q[RPW][2];
    float sc[RPW];
#if defined(QTX_ABL) && (QTX_ABL & 2)   // diagnostic builds only: no LayerNorm / quant chain
#pragma unroll
    for (int j = 0; j < RPW; ++j) {
      q[j][0] = __float_as_uint(v[j][0][0]); q[j][1] = __float_as_uint(v[j][1][0]); sc[j] = v[j][0][1];
    }
#else
    ln_rows512<RPW>(v, ga, gb);
    quant_rows512<RPW, true>(v, q, sc);
#endif
#pragma unroll
    for (int j = 0; j < RPW; ++j) {
      const int r = wave + 4 * j;
      const bool ok = m0 + r < g.M;
      uint32_t* dst = reinterpret_cast<uint32_t*>(As + r * LDA);
      dst[lane] = ok ? q[j][0] : 0u;
      dst[lane + 64] = ok ? q[j][1] : 0u;
      if (lane == 0) sas[r] = ok ? sc[j] : 0.0f;
    }
  } else {  // A_F32Q: each wave's rows (<= 4 at a time) with their partial maxima
            // A_F32R: the same rows, the row maximum from the row itself
    constexpr bool OWN = AMODE == A_F32R;
    constexpr int NC = K / 256, RBT = RPW < 4 ? RPW : 4;
#pragma unroll
    for (int j0 = 0; j0 < RPW; j0 += RBT) {
      float4 t[RBT][NC];
      float pm[RBT][2];
#pragma unroll
      for (int jb = 0; jb < RBT; ++jb) {
        const int m = min(m0 + wave + 4 * (j0 + jb), g.M - 1);
#pragma unroll
        for (int c = 0; c < NC; ++c)
          t[jb][c] = ld_at(reinterpret_cast<const float4*>(g.X), 4u * (unsigned)(m * (int)g.ldx + 4 * (lane + 64 * c)));
        if constexpr (!OWN)
#pragma unroll
          for (int u = 0; u < 2; ++u)   // lane takes partials lane, lane+64 (clamped: max-safe)
            pm[jb][u] = ld_at(g.pmax_in, 4u * (unsigned)(min(lane + 64 * u, g.pmax_n - 1) * g.M + m));
      }
      if (j0 == 0) issue_rest();
#pragma unroll
      for (int jb = 0; jb < RBT; ++jb) {
        const int r = wave + 4 * (j0 + jb);
        const bool ok = m0 + r < g.M;
        float lm;
        if constexpr (OWN) {   // |x| max of this lane's values (fmaxf: NaN drops out as in
          lm = 0.0f;           // the partial maxima the producer would have formed)
#pragma unroll
          for (int c = 0; c < NC; ++c)
            lm = fmaxf(lm, fmaxf(fmaxf(fabsf(t[jb][c].x), fabsf(t[jb][c].y)),
                                 fmaxf(fabsf(t[jb][c].z), fabsf(t[jb][c].w))));
        } else {
          lm = fmaxf(pm[jb][0], pm[jb][1]);
        }
        // (OWN: lm >= +0 and no NaN — wave_absmax, the 1e-5 floor of quant_scale inside
        // it; the partial maxima come from memory, where a caller may have put NaN)
        float sc;
        if constexpr (OWN) sc = absmax_scale127(wave_absmax(lm, 1e-5f));
        else sc = quant_scale(wave_max(lm), 127.0f);
        uint32_t* dst = reinterpret_cast<uint32_t*>(As + r * LDA);
        float tf[4 * NC];
#pragma unroll
        for (int c = 0; c < NC; ++c) {
          tf[4 * c] = t[jb][c].x; tf[4 * c + 1] = t[jb][c].y;
          tf[4 * c + 2] = t[jb][c].z; tf[4 * c + 3] = t[jb][c].w;
        }
        uint32_t qd[NC];
#if defined(QTX_ABL) && (QTX_ABL & 8)   // diagnostic builds only: no per-token quantization
#pragma unroll
        for (int c = 0; c < NC; ++c) qd[c] = __float_as_uint(tf[4 * c] * sc);
#else
        quant_pack<4 * NC>(tf, sc, qd);
#endif
#pragma unroll
        for (int c = 0; c < NC; ++c) dst[lane + 64 * c] = ok ? qd[c] : 0u;
        if (lane == 0) sas[r] = ok ? sc : 0.0f;
      }
    }
  }
}

template <int MF, int RB, int K, int WBITS, int AMODE, int FLAGS>
__global__ __launch_bounds__(256) void k_skinny(QTX_KA_PARAMS, SkTail kt) {
  const SkinnyArgs g = sk_args<AMODE>(QTX_KA_VALS, kt);
  constexpr int BM = 16 * MF;     // MFMA rows (rows >= RB of the A panel are don't-care)
  static_assert(RB % 4 == 0 && RB <= BM, "rows per block");
  constexpr int KW = K / 4;       // K range of one wave
  constexpr int NS = KW / 64;     // MFMA k-steps per wave
  constexpr int LDA = K + 16;     // padded LDS row (bytes)
  __shared__ __attribute__((aligned(16))) uint8_t As[BM * LDA];
  __shared__ float sas[BM];
  __shared__ v4i red[4][MF][64];

  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int fr = lane & 15, fg = lane >> 4;
  const int n0 = blockIdx.x * 16, m0 = blockIdx.y * RB;

  QTX_STAMP(0);

  // 1. this lane's W fragments for its wave's K range, and the epilogue operands of wave 0
  //    (it finishes the tile: a load first issued after the reduction barrier would add a
  //    whole memory round trip) — issued right after the A operand's loads (prologue)
  const int n = min(n0 + fr, g.N - 1);
  uint4 wf[NS];
  uint2 wp[NS];
  const int col = n0 + fr;
  const bool cok = col < g.N;
  float swc = 0.0f, bc = 0.0f, rv[MF];
  constexpr bool resid = FLAGS & EPI_RESIDUAL;
  auto issue_rest = [&]() {
#pragma unroll
    for (int s = 0; s < NS; ++s) {
      const int k = wave * KW + 64 * s + 16 * fg;
#if defined(QTX_ABL) && (QTX_ABL & 1)   // diagnostic builds only: no weight loads
      wf[s] = make_uint4(n + k, k, n, 1); wp[s] = make_uint2(n, k);
#else
      if constexpr (WBITS == 8)
        wf[s] = ld_at(reinterpret_cast<const uint4*>(g.W), (unsigned)(n * (int)g.ldw + k));
      else
        wp[s] = ld_at(reinterpret_cast<const uint2*>(g.W), (unsigned)(n * (int)g.ldw + (k >> 1)));
#endif
    }
    // every wave, unconditionally, at clamped addresses (values of rows / columns outside
    // the tile are never stored): a load under a branch makes the compiler's vmcnt for the
    // prologue's own loads count the branch-free path, i.e. wait for the weights too
    const int cc = min(col, g.N - 1);
    swc = ld_at(g.sw, 4u * cc);
    // up to here every address came from preloaded arguments; what follows may wait for the
    // trailing ones (SkTail), and must not be scheduled above the weights' loads for that
    __builtin_amdgcn_sched_barrier(0);
    if constexpr (resid) {   // the rows this wave finishes: 4 fg + wave of each tile
#pragma unroll
      for (int i = 0; i < MF; ++i) {
        const int row = min(m0 + 16 * i + 4 * fg + wave, g.M - 1);
        rv[i] = ld_at(g.res, 4u * (unsigned)(row * (int)g.ldr + cc));
      }
    }
    bc = ld_at(g.bias, 4u * cc);
  };

  // 2. A panel (int8) and per-row scales into LDS
  skinny_prologue<RB, K, AMODE>(g, As, sas, m0, tid, wave, lane, issue_rest);
  __syncthreads();

  QTX_STAMP(1);
  // 3. MFMA over this wave's K range
  v4i acc[MF];
#pragma unroll
  for (int i = 0; i < MF; ++i) acc[i] = v4i{0, 0, 0, 0};
#pragma unroll
  for (int s = 0; s < NS; ++s) {
    v4i bfr;
    if constexpr (WBITS == 8) {
      bfr = __builtin_bit_cast(v4i, wf[s]);
    } else {
      bfr = __builtin_bit_cast(v4i, unpack_i4(wp[s]));
    }
    const int k = wave * KW + 64 * s + 16 * fg;
#pragma unroll
    for (int i = 0; i < MF; ++i) {
      const v4i afr = *reinterpret_cast<const v4i*>(As + (16 * i + fr) * LDA + k);
#if defined(QTX_ABL) && (QTX_ABL & 4)   // diagnostic builds only: no matrix work
      acc[i] += afr ^ bfr;
#else
      acc[i] = __builtin_amdgcn_mfma_i32_16x16x64_i8(afr, bfr, acc[i], 0, 0, 0);
#endif
    }
  }

  // 4. exact int32 reduction of the 4 K ranges
#pragma unroll
  for (int i = 0; i < MF; ++i) red[wave][i][lane] = acc[i];
  __syncthreads();
  QTX_STAMP(2);
  // 5. epilogue, split over the waves: wave w finishes element e = w of every lane's four
  //    (C layout: col = lane & 15, row = 4*(lane>>4) + e), its int32 sum over the 4 K ranges
  //    exact in any order
  constexpr bool relu = FLAGS & EPI_RELU, rmax = FLAGS & EPI_ROWMAX;
  const int e = wave;
#pragma unroll
  for (int i = 0; i < MF; ++i) {
    {
      int sum = 0;
#pragma unroll
      for (int w = 0; w < 4; ++w) sum += reinterpret_cast<const int*>(&red[w][i][lane])[e];
      const int r = 16 * i + 4 * fg + e, row = m0 + r;
      const bool ok = cok && r < RB && row < g.M;
      float y = ((float)sum * sas[r]) * swc + bc;
      if constexpr (relu) y = y > 0.0f ? y : 0.0f;
      if constexpr (resid) y = rv[i] + y;
      if (ok) st_at(g.out, 4u * (unsigned)(row * (int)g.ldo + col), y);
      if constexpr (rmax) {
        float am = ok ? fabsf(y) : 0.0f;   // max over the 16 lanes (columns) of this row
        am = fmaxf(am, dpp<0xB1>(am));
        am = fmaxf(am, dpp<0x4E>(am));
        am = fmaxf(am, dpp<0x141>(am));
        am = fmaxf(am, dpp<0x140>(am));
        if (fr == 0 && r < RB && row < g.M) g.pmax_out[(long)blockIdx.x * g.M + row] = am;
      }
    }
  }
  QTX_STAMP(3);
}

}  // namespace qtx

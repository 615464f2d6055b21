// qtx_decode.hip — fused kernels of the KV-cached greedy decode step (gfx950, wave64).
//
//   k_skinny        M<=32-row int8 GEMM, 16 columns per workgroup, K split over 4 waves,
//                   A operand built in the prologue (int8 | LayerNorm+quant | rowmax-quant)
//                   quant_linear.py:111-119, layer_norm.py:12-15, position_feed_forward.py:12
//   k_dec_attn      one query per sentence, one wave per (sentence, head); quantizes q/k/v
//                   per token, appends k/v to the cache, attention; fp32 context + per-head
//                   absmax for the next GEMM's per-token quantization
//                   attention.py:23-67, get_quantized_model.py:160-168
//   k_generator_mfma final LayerNorm fused into the fp32 generator projection on fp32 MFMA
//                   generator.py:14-15, decoder.py:16
//   k_argmax_embed  log_softmax + first argmax + next-token embedding + step advance
//                   onnx_reference_inference.py:632,640-643
//   k_skinny_wide_tok  the same decision folded into the next step's first launch (layer 0's
//                   LN+QKV), from the generator's per-strip top-2 records
//   k_top2_embed    its scored form: the two best (id, logp) of the row as well
//                   parallelized_inject_onnx_transformer.py:718-740
//
// All float steps follow the canonical order shared with oracle/qtx_oracle.py.
#include <cstdlib>

#include "qtx_common.h"
#include "qtx_kernels.h"
#include "qtx_knobs.h"

QTX_STAMP_SETTER(decode)

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

// =====================================================================================
// k_skinny8: the decode FFN2 (K = 2048, fp32 hidden quantized per token from its partial
// maxima, residual epilogue) on 8 waves: two waves per row quantize one half of it each
// (16 values per lane: half the dependent quantization chain of k_skinny's one row per
// wave), K split 8 ways (4 weight fragments per lane), exact int32 reduction over the 8
// waves.  Rows per workgroup 4, 16 columns.  Bit-identical to k_skinny.
// OWN (A_F32R): the row maximum from the row itself instead of FFN1's per-tile partial
// maxima — each wave loads the row's other half as well (8 float4 loads issued together
// instead of 4) and forms the whole row's maximum, so the two waves of a row agree on the
// scale without meeting in LDS behind a barrier of the 8 waves.
// =====================================================================================
template <bool OWN>
__global__ __launch_bounds__(512) void k_skinny8_ffn2(QTX_KA_PARAMS, SkTail kt) {
  const SkinnyArgs g = sk_args<OWN ? A_F32R : A_F32Q>(QTX_KA_VALS, kt);
  constexpr int K = 2048, RB = 4, KW = K / 8, NS = KW / 64, LDA = K + 16;
  __shared__ __attribute__((aligned(16))) uint8_t As[16 * LDA];
  __shared__ float sas[16];
  __shared__ v4i red[8][64];
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int fr = lane & 15, fg = lane >> 4;
  const int n0 = blockIdx.x * 16, m0 = blockIdx.y * RB;
  // 1. the A operand's loads first: row r = wave / 2, half = wave & 1 (1024 values)
  const int r = wave >> 1, half = wave & 1;
  const int m = min(m0 + r, g.M - 1);
  float4 t[4];
#pragma unroll
  for (int c = 0; c < 4; ++c)
    t[c] = ld_at(reinterpret_cast<const float4*>(g.X), 4u * (unsigned)(m * (int)g.ldx + 4 * (lane + 64 * (4 * half + c))));
  float pm[2] = {0.0f, 0.0f};
  float4 to[4] = {};   // OWN: the row's other half, for the row maximum alone
  if constexpr (!OWN) {
#pragma unroll
    for (int u = 0; u < 2; ++u) pm[u] = ld_at(g.pmax_in, 4u * (unsigned)(min(lane + 64 * u, g.pmax_n - 1) * g.M + m));
  } else {
#pragma unroll
    for (int c = 0; c < 4; ++c)
      to[c] = ld_at(reinterpret_cast<const float4*>(g.X), 4u * (unsigned)(m * (int)g.ldx + 4 * (lane + 64 * (4 * (half ^ 1) + c))));
  }
  // 2. then this wave's weight fragments and (wave 0) the epilogue operands
  const int n = min(n0 + fr, g.N - 1);
  uint4 wf[NS];
#pragma unroll
  for (int s = 0; s < NS; ++s)
    wf[s] = ld_at(reinterpret_cast<const uint4*>(g.W), (unsigned)(n * (int)g.ldw + wave * KW + 64 * s + 16 * fg));
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
      for (int c = 0; c < 4; ++c) {
        lm = fmaxf(lm, fmaxf(fmaxf(fabsf(t[c].x), fabsf(t[c].y)), fmaxf(fabsf(t[c].z), fabsf(t[c].w))));
        lm = fmaxf(lm, fmaxf(fmaxf(fabsf(to[c].x), fabsf(to[c].y)), fmaxf(fabsf(to[c].z), fabsf(to[c].w))));
      }
      sc = absmax_scale127(wave_absmax(lm, 1e-5f));   // quant_scale, its 1e-5 floor in the maximum
    } else {
      sc = quant_scale(wave_max(fmaxf(pm[0], pm[1])), 127.0f);
    }
    float tf[16];
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      tf[4 * c] = t[c].x; tf[4 * c + 1] = t[c].y; tf[4 * c + 2] = t[c].z; tf[4 * c + 3] = t[c].w;
    }
    uint32_t qd[4];
    quant_pack<16>(tf, sc, qd);
    uint32_t* dst = reinterpret_cast<uint32_t*>(As + r * LDA);
#pragma unroll
    for (int c = 0; c < 4; ++c) dst[lane + 64 * (4 * half + c)] = ok ? qd[c] : 0u;
    if (lane == 0 && half == 0) sas[r] = ok ? sc : 0.0f;
  }
  __syncthreads();
  // 4. MFMA over this wave's K range, exact int32 reduction of the 8 ranges
  v4i acc = v4i{0, 0, 0, 0};
#pragma unroll
  for (int s = 0; s < NS; ++s) {
    const v4i afr = *reinterpret_cast<const v4i*>(As + fr * LDA + wave * KW + 64 * s + 16 * fg);
    acc = __builtin_amdgcn_mfma_i32_16x16x64_i8(afr, __builtin_bit_cast(v4i, wf[s]), acc, 0, 0, 0);
  }
  red[wave][lane] = acc;
  __syncthreads();
  if (wave != 0) return;
  // 5. epilogue: out = res + y.  The RB = 4 useful rows of the 16-row tile sit in lanes
  //    0-15 (element e = row); wave 0 takes one output per lane — lane l: row e = l >> 4,
  //    column l & 15 — summing element e of lane l & 15 over the 8 K ranges (exact int32;
  //    conflict-free LDS reads)
  {
    const int e = fg, src = fr;
    int sum = 0;
#pragma unroll
    for (int w = 0; w < 8; ++w) sum += reinterpret_cast<const int*>(&red[w][src])[e];
    const int row = m0 + e;
    const float y = ((float)sum * sas[e]) * swc + bc;
    if (cok && row < g.M) st_at(g.out, 4u * (unsigned)(row * (int)g.ldo + col), rv + y);
  }
}

// =====================================================================================
// k_skinny_wide: the K = 512 skinny GEMM with N split over the 4 waves instead of K — a
// workgroup covers 64 columns (wave w: columns n0 + 16w .. +15, all 8 K steps, 8 weight
// fragments = 128 B per lane in flight) and its RB rows; no cross-wave reduction.  The
// prologue (LayerNorm + quant of the RB rows, or their per-token quant) then serves 64
// columns instead of 16: 4x fewer redundant LayerNorms per launch.  Same int32 sums, same
// epilogue arithmetic: bit-identical to k_skinny.
// =====================================================================================
template <int RB, int WBITS, int AMODE, int FLAGS>
__global__ __launch_bounds__(256) void k_skinny_wide(QTX_KA_PARAMS, SkTail kt) {
  const SkinnyArgs g = sk_args<AMODE>(QTX_KA_VALS, kt);
  constexpr int K = 512, NS = K / 64, LDA = K + 16;
  static_assert(RB % 4 == 0 && RB <= 16, "rows per block");
  __shared__ __attribute__((aligned(16))) uint8_t As[16 * LDA];
  __shared__ float sas[16];
  // RB = 4 / 8: each wave's useful C rows (lanes 0 .. 4 RB - 1), remapped through LDS
  constexpr int RPL = RB / 4;                        // outputs per lane after the remap
  constexpr bool REMAP = RB == 4 || RB == 8;
  __shared__ v4i tail[REMAP ? 4 : 1][REMAP ? 4 * RB : 1];
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int fr = lane & 15, fg = lane >> 4;
  const int n0 = blockIdx.x * 64 + 16 * wave, m0 = blockIdx.y * RB;
  QTX_STAMP(0);
  // 1. this lane's W fragments (all of K) and the epilogue operands of the wave's 16
  //    columns — issued right after the A operand's loads (prologue)
  const int n = min(n0 + fr, g.N - 1);
  uint4 wf[NS];
  uint2 wp[NS];
  const int col = n0 + fr;
  const bool cok = col < g.N;
  constexpr bool resid = FLAGS & EPI_RESIDUAL;
  float swc, bc, rv[4];
  auto issue_rest = [&]() {
#pragma unroll
    for (int s = 0; s < NS; ++s) {
      const int k = 64 * s + 16 * fg;
#if defined(QTX_ABL) && (QTX_ABL & 1)   // diagnostic builds only: no weight loads
      wf[s] = make_uint4(n + k, k, n, 1); wp[s] = make_uint2(n, k);
#else
      if constexpr (WBITS == 8)
        wf[s] = ld_at(reinterpret_cast<const uint4*>(g.W), (unsigned)(n * (int)g.ldw + k));
      else
        wp[s] = ld_at(reinterpret_cast<const uint2*>(g.W), (unsigned)(n * (int)g.ldw + (k >> 1)));
#endif
    }
    swc = cok ? ld_at(g.sw, 4u * col) : 0.0f;
    __builtin_amdgcn_sched_barrier(0);   // as in k_skinny: trailing arguments from here on
    bc = cok ? ld_at(g.bias, 4u * col) : 0.0f;
    if constexpr (RB == 4) {   // the epilogue's one output per lane: row m0 + fg
      rv[0] = (resid && cok && m0 + fg < g.M) ? ld_at(g.res, 4u * (unsigned)((m0 + fg) * (int)g.ldr + col)) : 0.0f;
    } else if constexpr (RB == 8) {   // its two: rows m0 + fg, m0 + fg + 4
#pragma unroll
      for (int j = 0; j < 2; ++j) {
        const int row = m0 + fg + 4 * j;
        rv[j] = (resid && cok && row < g.M) ? ld_at(g.res, 4u * (unsigned)(row * (int)g.ldr + col)) : 0.0f;
      }
    } else {
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const int r = 4 * fg + e, row = m0 + r;
        rv[e] = (resid && cok && r < RB && row < g.M) ? ld_at(g.res, 4u * (unsigned)(row * (int)g.ldr + col)) : 0.0f;
      }
    }
  };
  // 2. A panel and per-row scales into LDS
  skinny_prologue<RB, K, AMODE>(g, As, sas, m0, tid, wave, lane, issue_rest);
  __syncthreads();
  QTX_STAMP(1);
  // 3. MFMA over all of K
  v4i acc = v4i{0, 0, 0, 0};
#pragma unroll
  for (int s = 0; s < NS; ++s) {
    v4i bfr;
    if constexpr (WBITS == 8) bfr = __builtin_bit_cast(v4i, wf[s]);
    else bfr = __builtin_bit_cast(v4i, unpack_i4(wp[s]));
    const v4i afr = *reinterpret_cast<const v4i*>(As + fr * LDA + 64 * s + 16 * fg);
#if defined(QTX_ABL) && (QTX_ABL & 4)   // diagnostic builds only: no matrix work
    acc += afr ^ bfr;
#else
    acc = __builtin_amdgcn_mfma_i32_16x16x64_i8(afr, bfr, acc, 0, 0, 0);
#endif
  }
  QTX_STAMP(2);
  // 4. epilogue (C layout: col = lane & 15, row = 4*(lane>>4) + e)
  constexpr bool relu = FLAGS & EPI_RELU, rmax = FLAGS & EPI_ROWMAX;
  if constexpr (RB == 4) {
    // the 4 useful rows are elements 0-3 of lanes 0-15: through the wave's own LDS slot
    // (in-order within the wave, conflict-free) lane l takes row l >> 4 of column l & 15 —
    // one output per lane instead of four on a quarter of the lanes
    if (fg == 0) tail[wave][fr] = acc;
    // (no instruction: keeps the compiler from moving the other lanes' reads above the
    // store — the hardware keeps one wave's LDS operations in order)
    __builtin_amdgcn_wave_barrier();
    const int v = reinterpret_cast<const int*>(&tail[wave][fr])[fg];
    const int row = m0 + fg;
    const bool ok = cok && row < g.M;
    float y = ((float)v * sas[fg]) * swc + bc;
    if constexpr (relu) y = y > 0.0f ? y : 0.0f;
    if constexpr (resid) y = rv[0] + y;
    if (ok) st_at(g.out, 4u * (unsigned)(row * (int)g.ldo + col), y);
    if constexpr (rmax) {
      float am = ok ? fabsf(y) : 0.0f;   // max over the 16 lanes (columns) of this row
      am = fmaxf(am, dpp<0xB1>(am));
      am = fmaxf(am, dpp<0x4E>(am));
      am = fmaxf(am, dpp<0x141>(am));
      am = fmaxf(am, dpp<0x140>(am));
      if (fr == 0 && row < g.M) g.pmax_out[(long)(n0 >> 4) * g.M + row] = am;
    }
    QTX_STAMP(3);
    return;
  }
  if constexpr (RB == 8) {
    // the 8 useful rows are elements 0-3 of lanes 0-31 (row 4 (l >> 4) + e): the same
    // remap, lane l takes rows (l >> 4) and (l >> 4) + 4 of column l & 15 — two outputs per
    // lane instead of four on half of the lanes
    if (fg < RPL) tail[wave][16 * fg + fr] = acc;
    __builtin_amdgcn_wave_barrier();      // as at RB == 4
#pragma unroll
    for (int j = 0; j < RPL; ++j) {
      const int v = reinterpret_cast<const int*>(&tail[wave][16 * j + fr])[fg];
      const int r = fg + 4 * j, row = m0 + r;
      const bool ok = cok && row < g.M;
      float y = ((float)v * sas[r]) * swc + bc;
      if constexpr (relu) y = y > 0.0f ? y : 0.0f;
      if constexpr (resid) y = rv[j] + y;
      if (ok) st_at(g.out, 4u * (unsigned)(row * (int)g.ldo + col), y);
      if constexpr (rmax) {
        float am = ok ? fabsf(y) : 0.0f;   // max over the 16 lanes (columns) of this row
        am = fmaxf(am, dpp<0xB1>(am));
        am = fmaxf(am, dpp<0x4E>(am));
        am = fmaxf(am, dpp<0x141>(am));
        am = fmaxf(am, dpp<0x140>(am));
        if (fr == 0 && row < g.M) g.pmax_out[(long)(n0 >> 4) * g.M + row] = am;
      }
    }
    QTX_STAMP(3);
    return;
  }
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    const int r = 4 * fg + e, row = m0 + r;
    const bool ok = cok && r < RB && row < g.M;
    float y = ((float)acc[e] * sas[r]) * swc + bc;
    if constexpr (relu) y = y > 0.0f ? y : 0.0f;
    if constexpr (resid) y = rv[e] + y;
    if (ok) st_at(g.out, 4u * (unsigned)(row * (int)g.ldo + col), y);
    if constexpr (rmax) {
      float am = ok ? fabsf(y) : 0.0f;   // max over the 16 lanes (columns) of this row
      am = fmaxf(am, dpp<0xB1>(am));
      am = fmaxf(am, dpp<0x4E>(am));
      am = fmaxf(am, dpp<0x141>(am));
      am = fmaxf(am, dpp<0x140>(am));
      if (fr == 0 && r < RB && row < g.M) g.pmax_out[(long)(n0 >> 4) * g.M + row] = am;
    }
  }
  QTX_STAMP(3);
}

template <int RB, int WB, int AM>
hipError_t skinny_wide_flags(const SkinnyArgs& g, hipStream_t st) {
  const dim3 grid(g.N / 64, (g.M + RB - 1) / RB);
  switch (g.flags) {
    case 0: QTX_SK_LAUNCH(AM, grid, 256, k_skinny_wide<RB, WB, AM, 0>); break;
    case EPI_RELU: QTX_SK_LAUNCH(AM, grid, 256, k_skinny_wide<RB, WB, AM, EPI_RELU>); break;
    case EPI_RESIDUAL: QTX_SK_LAUNCH(AM, grid, 256, k_skinny_wide<RB, WB, AM, EPI_RESIDUAL>); break;
    case EPI_RELU | EPI_ROWMAX:
      QTX_SK_LAUNCH(AM, grid, 256, k_skinny_wide<RB, WB, AM, EPI_RELU | EPI_ROWMAX>);
      break;
    default: return hipErrorInvalidValue;
  }
  return hipGetLastError();
}
template <int WB, int AM>
hipError_t skinny_wide_rb(const SkinnyArgs& g, int rb, hipStream_t st) {
  switch (rb) {
    case 4: return skinny_wide_flags<4, WB, AM>(g, st);
    case 8: return skinny_wide_flags<8, WB, AM>(g, st);
    case 16: return skinny_wide_flags<16, WB, AM>(g, st);
    default: return hipErrorInvalidValue;
  }
}

// dispatch: the prologue mode and epilogue flags are template parameters (no runtime
// branches per output element).  Supported: K 512 with A_I8 / A_LN, K 2048 with A_I8 /
// A_F32Q; flags 0, RELU, RESIDUAL, RELU|ROWMAX.  Rows per workgroup RB: 16*MF for an int8
// A panel; 4 (one row per wave) for the LayerNorm prologue, which re-normalizes its rows
// in every column workgroup — few rows per workgroup keeps that short and spreads the
// fp32 row reads over many CUs (measured: RB 32 -> 8 -> 4 = 11.0 -> 5.1 -> 4.6 us for
// N=1536, M=32; in the decode step the fused form beats LN kernel + GEMM).
template <int MF, int RB, int K, int WB, int AM>
hipError_t skinny_flags(const SkinnyArgs& g, hipStream_t st) {
  const dim3 grid(g.N / 16, (g.M + RB - 1) / RB);
  switch (g.flags) {
    case 0: QTX_SK_LAUNCH(AM, grid, 256, k_skinny<MF, RB, K, WB, AM, 0>); break;
    case EPI_RELU: QTX_SK_LAUNCH(AM, grid, 256, k_skinny<MF, RB, K, WB, AM, EPI_RELU>); break;
    case EPI_RESIDUAL: QTX_SK_LAUNCH(AM, grid, 256, k_skinny<MF, RB, K, WB, AM, EPI_RESIDUAL>); break;
    case EPI_RELU | EPI_ROWMAX:
      QTX_SK_LAUNCH(AM, grid, 256, k_skinny<MF, RB, K, WB, AM, EPI_RELU | EPI_ROWMAX>);
      break;
    default: return hipErrorInvalidValue;
  }
  return hipGetLastError();
}
template <int K, int WB, int AM>
hipError_t skinny_rb(const SkinnyArgs& g, int rb, hipStream_t st) {
  switch (rb) {
    case 4: return skinny_flags<1, 4, K, WB, AM>(g, st);
    case 8: return skinny_flags<1, 8, K, WB, AM>(g, st);
    case 16: return skinny_flags<1, 16, K, WB, AM>(g, st);
    case 32: return skinny_flags<2, 32, K, WB, AM>(g, st);
    default: return hipErrorInvalidValue;
  }
}
// Rows per workgroup (decode step, M = 32, measured in bench.py; tools/rb_sweep.sh: the
// K = 512 int8 / F32Q row block 8 -> 4 took the step 234.8 -> 230.3 us): small row blocks spread
// the A-panel and weight reads over more CUs — each CU sustains only a few KB in flight,
// so a latency-bound kernel is fastest when every workgroup touches ~10-40 KB.
template <int WB>
hipError_t skinny_mode(const SkinnyArgs& g, hipStream_t st) {
  // The N-split workgroup (k_skinny_wide) for the LayerNorm-prologue GEMMs with N >= 1024
  // (LN+QKV, LN+FFN1): measured in the decode graph at M = 32 (tools/kernel_chain.py)
  // 4.50 -> 3.67 and 5.26 -> 3.95 us per launch; at N = 512 the K-split one is faster
  // (64 workgroups of 32 KB each vs 256 of 8 KB: 3.09 vs 3.60 us).  QTX_SKINNY_WIDE=0: never,
  // =<rb>: every K = 512 launch (experiments).
  // From M >= 96 (the decode of >= 96 sentences per sub-batch, e.g. cfg5's 256 per GPU) the
  // small blocks re-read W once per 4 rows: there every K = 512 GEMM runs N-split with 8-row
  // blocks, and FFN2 (whose hidden the decode step then quantizes with its own kernel,
  // qtx_api.hip greedy_step_fused) takes 16-row blocks — or 8 / 16 with the fp32 prologue
  // (tools/rb_sweep256.py, profiles/r05_rb_sweep.md: B = 256 decode 35.0 -> 27.5 ms,
  // B = 128 23.1 -> 21.0 ms; at B = 32 / 64 the small blocks stay faster).
  const Knobs& kn = knobs();     // QTX_SKINNY_WIDE / QTX_RB_* / QTX_SKINNY8_MAXM: QTX_DIAG build
  const bool big = g.M >= 96;
  const int wide_env = kn.skinny_wide;
  const bool wide = wide_env < 0 ? ((g.amode == A_LN && g.N >= 1024) || big) : wide_env > 0;
  if (wide && g.K == 512 && g.N % 64 == 0) {
    const int rb = wide_env > 0 && g.M > 4 ? wide_env : (big ? 8 : 4);
    if (g.amode == A_I8) return skinny_wide_rb<WB, A_I8>(g, rb, st);
    if (g.amode == A_LN) return skinny_wide_rb<WB, A_LN>(g, rb, st);
    if (g.amode == A_F32Q) return skinny_wide_rb<WB, A_F32Q>(g, rb, st);
    if (g.amode == A_F32R) return skinny_wide_rb<WB, A_F32R>(g, rb, st);
  }
  if (g.K == 512) {
    const int rb_i8 = kn.rb_i8_512, rb_ln = kn.rb_ln;
    if (g.amode == A_I8) return skinny_rb<512, WB, A_I8>(g, g.M <= 4 ? 4 : rb_i8, st);
    if (g.amode == A_LN) return skinny_rb<512, WB, A_LN>(g, rb_ln, st);
    if (g.amode == A_F32Q) return skinny_rb<512, WB, A_F32Q>(g, g.M <= 4 ? 4 : rb_i8, st);
    if (g.amode == A_F32R) return skinny_rb<512, WB, A_F32R>(g, g.M <= 4 ? 4 : rb_i8, st);
  } else if (g.K == 2048) {
    // the decode FFN2 (fp32 hidden, residual, 8-bit weights) at M <= QTX_SKINNY8_MAXM
    // (default 32): 8 waves (measured: B = 32 decode 14.45 -> 14.40 ms; at B = 256 the
    // 4-wave kernel is faster, 35.1 vs 36.8 ms)
    const int sk8_maxm = kn.skinny8_maxm;
    if (g.M <= sk8_maxm && WB == 8 && g.flags == EPI_RESIDUAL &&
        ((g.amode == A_F32Q && g.pmax_n <= 128) || g.amode == A_F32R)) {
      if (g.amode == A_F32R)
        QTX_SK_LAUNCH(A_F32R, dim3(g.N / 16, (g.M + 3) / 4), 512, k_skinny8_ffn2<true>);
      else
        QTX_SK_LAUNCH(A_F32Q, dim3(g.N / 16, (g.M + 3) / 4), 512, k_skinny8_ffn2<false>);
      return hipGetLastError();
    }
    const int rb_i8 = kn.rb_i8_2048 > 0 ? kn.rb_i8_2048 : (big ? 16 : 4);
    const int rb_f = kn.rb_f32q > 0 ? kn.rb_f32q : (g.M >= 192 ? 16 : big ? 8 : 4);
    if (g.amode == A_I8) return skinny_rb<2048, WB, A_I8>(g, rb_i8, st);
    if (g.amode == A_F32Q) return skinny_rb<2048, WB, A_F32Q>(g, rb_f, st);
    if (g.amode == A_F32R) return skinny_rb<2048, WB, A_F32R>(g, rb_f, st);
  }
  return hipErrorInvalidValue;
}

hipError_t launch_skinny(const SkinnyArgs& g, int wbits, hipStream_t st) {
  if (g.M <= 0) return hipSuccess;
  if (g.N % 16) return hipErrorInvalidValue;
  // the kernels address X / res / A / W with 32-bit byte offsets (ld_at)
  const long lim = 1L << 30;
  if ((long)g.M * (g.ldx > g.K ? g.ldx : g.K) >= lim || (long)g.M * g.ldr >= lim ||
      (long)g.M * g.ldo >= lim || (long)g.N * g.ldw >= lim || (long)g.M * g.pmax_n >= lim)
    return hipErrorInvalidValue;
  if (wbits == 8) return skinny_mode<8>(g, st);
  if (wbits == 4) return skinny_mode<4>(g, st);
  return hipErrorInvalidValue;
}

// =====================================================================================
// k_dec_attn: one wave per (sentence, head) — 8*B workgroups, so the cached keys/values
// (the bulk of the bytes) are spread over many CUs instead of one CU per sentence.  Each
// wave quantizes the q (and new k/v) row itself (full-row maxima recomputed per head:
// 2-6 KB of reads), attends over its head and writes its 64 fp32 context values plus
// their absmax; the per-token quantization of the context row happens in the prologue of
// the output-projection GEMM (A_F32Q), so no cross-workgroup step is needed here.
// At most 128 keys.  The scores run on the int8 MFMA (round 9): the head dimension, 64, is one
// K-step of v_mfma_i32_16x16x64_i8, and its B operand for 16 keys is one uint4 per lane (key
// 16 i + lane % 16, byte chunk lane / 16), so the key rows are loaded straight into fragment
// layout and never staged in LDS; the A operand repeats the q codes in all 16 rows.
// Grid (B, 8): the 8 heads of sentence b share blockIdx.x,
// so with B % 8 == 0 they land on one XCD (workgroups go round-robin over the 8 XCDs).
// The value cache is kept in groups of 4 keys (round 6): byte ((b * G4 + j / 4) * 512 + d) * 4
// + j % 4 holds v[b][j][d] (G4 = ceil(kv_bs / 4)), so one dword is 4 consecutive keys of one
// dim — the PV's 4-key step is one dword and 4 SDWA conversions, and the dword of (group,
// dim = lane) is a coalesced load straight into the register the chain reads (round 10: the
// value rows are not staged in LDS either).
// =====================================================================================
constexpr int DEC_MAXK = 128;

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

template <bool KV_NEW, int NIT>
__global__ __launch_bounds__(64) void k_dec_attn(QTX_KA_PARAMS, DaTail kt) {
  const DecAttnArgs a = da_args<KV_NEW>(QTX_KA_VALS, kt);
  __shared__ __attribute__((aligned(16))) float PS[DEC_MAXK];   // RN(P_j * s_v[j]), 0 past Sk
  // this step's q codes and (self) k codes of the head: 64 B each, read back as MFMA fragments
  __shared__ __attribute__((aligned(16))) int8_t qs[KV_NEW ? 128 : 64];
  const int b = blockIdx.x, h = blockIdx.y, lane = threadIdx.x;
  const int fr = lane & 15, fg = lane >> 4;    // MFMA fragment: column (key) fr, byte chunk fg
  QTX_STAMP(0);
  const float* yr = a.y + (long)b * a.ldy;

  // phase 0: every global load first (one memory latency): this step's q (k, v) rows
  // first — vmcnt retires in issue order, so their quantization (phase 1) then runs while
  // the cached keys and values are in flight — then the key rows of this head (row r
  // = 4 uint4; lane takes row 16*i + lane%16, chunk lane/16 — the B fragment of the int8
  // 16x16x64 MFMA for keys 16i .. 16i + 15, so the keys are never staged; the same 16 rows x
  // 64 B per load instruction as any other lane <-> (row, chunk) map; clamped: no divergent
  // loads)
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
  // (the y row's loads go out before the scalar arithmetic of the cache rows' bases: left to
  // itself the scheduler puts all of that, ~40 scalar instructions, ahead of the first load)
  __builtin_amdgcn_sched_barrier(0);
  // rows staged (self: rows 0 .. the position when the host passes it, else all allocated)
  const int nrows = KV_NEW ? (a.host_step1 > 0 ? a.host_step1 : (int)a.kv_bs) : a.S;
  const long kvb = (long)b * a.kv_bs;
  const long vgb = (long)b * ((a.kv_bs + 3) >> 2);     // the sentence's first value group
  const int glast = (nrows - 1) >> 2;                  // the last staged 4-key value group
  // wave-uniform bases of this head's rows and 32-bit lane offsets: the loads take the
  // scalar-base + vector-offset form instead of 64-bit address arithmetic per load
  const int8_t* const kbase = a.kc + kvb * 512 + h * 64;
  const int8_t* const vbase = a.vc + vgb * 2048 + h * 256;
  uint4 kr[NIT];
#pragma unroll
  for (int i = 0; i < NIT; ++i) {
    const unsigned koff = (unsigned)(min(16 * i + fr, nrows - 1) * 512 + 16 * fg);
    // non-temporal: each K/V row is read once per step by one wave, so it should not push
    // the weights (re-read every step) out of the XCD's L2 (B = 256: 36.2 -> 35.1 ms; the
    // default policy re-measured in round 6: B = 32 12.87 vs 12.84, B = 256 26.25 vs 25.58 ms)
    kr[i] = __builtin_bit_cast(uint4, __builtin_nontemporal_load(reinterpret_cast<const v4i*>(kbase + koff)));
  }
  const int j0 = min(lane, nrows - 1), j1 = min(lane + 64, nrows - 1);
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
  // the value rows straight into the registers the PV chains read (phase 4), never staged
  // in LDS: in the 4-key group layout the dword of group 4 g + q and dim = lane is vg4[g][q],
  // one coalesced 256-byte load per group.  Issued last (the barrier keeps the scheduler from
  // moving them ahead of a key row), so no wait ahead of the PV phase includes them.
  // Non-temporal as the key rows.  The groups are clamped to the last staged one (wave-
  // uniform): in the last fragment each group; a fragment ahead of it lies wholly inside the
  // staged rows (NIT = ceil(nrows / 16), dec_attn_nit: NIT >= 2 means nrows > 16, glast >= 4),
  // so its four groups share one clamp — the identity — and sit at constant offsets from it.
  uint32_t vg4[NIT][4];
  __builtin_amdgcn_sched_barrier(0);
#pragma unroll
  for (int g = 0; g < NIT; ++g)
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int grp = g < NIT - 1 ? min(4 * g, max(glast - 3, 0)) + q : min(4 * g + q, glast);
      vg4[g][q] = __builtin_nontemporal_load(
          reinterpret_cast<const uint32_t*>(vbase + (unsigned)(grp * 2048 + 4 * lane)));
    }
  // the position (no load's address depends on it: read after they are issued; the counter's
  // pointer comes with the trailing arguments).  Clamped: a stale position (a counter not
  // reset) must not index past the cache
  const int step = !KV_NEW ? 0 : a.host_step1 > 0 ? a.host_step1 - 1 : min(max(*a.step, 0), (int)a.kv_bs - 1);
  // cross: keys past the sentence's last unmasked one contribute exactly nothing (score
  // -1e9 -> qexp 0 -> P 0, and fma(0, v, acc) == acc), so the key loops stop there; a
  // fully masked row keeps all S keys (the reference's uniform softmax over -1e9 scores)
  int Sk = KV_NEW ? step + 1 : a.S;
  if constexpr (!KV_NEW) {
    const int last = wave_max_i32(max(keep0 && lane < a.S ? lane + 1 : 0,
                                      NIT > 4 && keep1 && lane + 64 < a.S ? lane + 65 : 0));
    if (last > 0) Sk = last;
  }

  // phase 1: per-token scales of q (and k, v) over the full 512-wide rows
  // (the lane's |x| maximum: >= +0, NaN dropped — wave_absmax's precondition)
  auto lmax8 = [](const float4 (&v)[2]) {
    float m = 0.0f;
#pragma unroll
    for (int c = 0; c < 2; ++c)
      m = fmaxf(m, fmaxf(fmaxf(fabsf(v[c].x), fabsf(v[c].y)), fmaxf(fabsf(v[c].z), fabsf(v[c].w))));
    return m;
  };
  float sq;
  int8_t kq = 0, vq = 0;
  float sk = 0.0f, sv = 0.0f;
  if constexpr (KV_NEW) {
    // self: the q, k and v chains in one pass — three maxima through one DPP tree, the three
    // scales behind one range test (absmax_scale127_n) and the three codes behind one near-tie
    // vote (quant_one_n), so the chains interleave instead of running one after another
    // between six rarely taken branches.  Where a vote fails all three take the true
    // division, which equals the short form wherever that is exact: the same scales and codes
    float am[3] = {lmax8(yq), lmax8(yk), lmax8(yv)};
    wave_absmax_n<3>(am, 1e-5f);
    absmax_scale127_n<3>(am);
    const float own[3] = {q_own, k_own, v_own};
    int code[3];
    quant_one_n<3>(own, am, code);
    sq = am[0]; sk = am[1]; sv = am[2];
    qs[lane] = (int8_t)code[0];
    kq = (int8_t)code[1];
    vq = (int8_t)code[2];
  } else {   // cross: q alone (the row absmax with quant_scale's 1e-5 floor in it)
    sq = absmax_scale127(wave_absmax(lmax8(yq), 1e-5f));
    qs[lane] = (int8_t)quant_one(q_own, sq);
  }
  if constexpr (KV_NEW) {
    const long row = kvb + step;
    a.kc[row * 512 + h * 64 + lane] = kq;     // cache append (attention.py: k/v of this step)
    a.vc[((vgb + (step >> 2)) * 512 + h * 64 + lane) * 4 + (step & 3)] = vq;
    if (h == 0 && lane == 0) { a.skc[row] = sk; a.svc[row] = sv; }
    qs[64 + lane] = kq;
    if (lane == step) { sk0 = sk; sv0 = sv; }            // the key and value scales stay in the
    if (lane + 64 == step) { sk1 = sk; sv1 = sv; }       // lane that scores the key (lane + 64 u)
  }

  // phase 2: the operand fragments.  A: the q codes' chunk fg in every row, so each of the 16
  // rows of C holds the scores.  B: kr[i] as loaded; (self) this step's k codes replace the
  // stale row `step` in the lanes that hold it (fragment step / 16, wave-uniform; column
  // step % 16)
  __syncthreads();
  const v4i qf = *reinterpret_cast<const v4i*>(qs + 16 * fg);
  if constexpr (KV_NEW) {
    const uint4 kn = *reinterpret_cast<const uint4*>(qs + 64 + 16 * fg);
    const bool own = fr == (step & 15);
#pragma unroll
    for (int i = 0; i < NIT; ++i)
      if (i == (step >> 4) && own) kr[i] = kn;
  }
  QTX_STAMP(1);

  // phase 3: scores (lane owns keys lane, lane+64), softmax, P quantization.  One MFMA per 16
  // keys, independent accumulators; int32 dot products, exact in any order
  v4i sacc[NIT];
#pragma unroll
  for (int i = 0; i < NIT; ++i)
    sacc[i] = __builtin_amdgcn_mfma_i32_16x16x64_i8(qf, __builtin_bit_cast(v4i, kr[i]), v4i{0, 0, 0, 0}, 0, 0, 0);
  // key 16 i + fr is column fr of sacc[i] (C: column lane % 16, all rows equal): lane's key
  // lane is in sacc[fg], key lane + 64 in sacc[4 + fg]
  constexpr int NU = NIT > 4 ? 2 : 1;     // up to 64 rows: no second key slot
  int dot[NU];
#pragma unroll
  for (int u = 0; u < NU; ++u) {
    dot[u] = sacc[4 * u][0];
#pragma unroll
    for (int t = 1; t < 4; ++t)
      if (4 * u + t < NIT) dot[u] = fg == t ? sacc[4 * u + t][0] : dot[u];
  }
  // (the scores and exponentials stay in registers: lane owns keys lane, lane + 64).  Both
  // key slots go through the same straight-line arithmetic and a lane without a key (j >=
  // Sk) drops its value by a select, so the two slots' chains interleave instead of running
  // one after the other under two exec masks; what such a lane computes (from a stale
  // scale, say) never reaches a sum: max and sum take it through the select alone, and
  // x + 0.0f == x for the x >= 0 summed here
  float sc[NU];
  bool live[NU];
  float lmax = -3.0e38f;
#pragma unroll
  for (int u = 0; u < NU; ++u) {
    live[u] = lane + 64 * u < Sk;
    const int acc = dot[u];
    float s = (((float)acc * sq) * (u ? sk1 : sk0)) * 0.125f;
    if (!(u ? keep1 : keep0)) s = -1.0e9f;
    sc[u] = s;
    lmax = live[u] ? fmaxf(lmax, s) : lmax;
  }
  const float m = wave_max(lmax);
  float lsum = 0.0f;
#pragma unroll
  for (int u = 0; u < NU; ++u) {
    const float e = qexp(sc[u] - m);
    sc[u] = e;
    lsum = lsum + (live[u] ? e : 0.0f);
  }
  // P = rint((e / den) * 127) / 127: e / den by div_cr, unguarded (den in [1, Sk]: the
  // row max contributes qexp(0) == 1; e >= 2^-60 gives the correctly rounded quotient and
  // e < 2^-60 a P of 0 through either), / 127 by div127 — no true division per key; the PV
  // term's P * s_v once per key (the decoder's PV order, oracle attention_pv dec), and 0
  // for the padded keys Sk .. nk16 - 1 of the last 16-key group
  const float den = wave_sum(lsum);
  const float rden = 1.0f / den;
  const int nk16 = (Sk + 15) & ~15;
#pragma unroll
  for (int u = 0; u < NU; ++u) {
    const int j = lane + 64 * u;
    const float ps = div127(rintf(div_cr(sc[u], den, rden) * 127.0f)) * (u ? sv1 : sv0);
    if (j < nk16) PS[j] = live[u] ? ps : 0.0f;
  }
  __syncthreads();
  QTX_STAMP(2);

  // phase 4: context dim h*64 + lane in the decoder's PV order: four chains, chain c over
  // the keys j with (j >> 2) & 3 == c in key order, term fma(PS[j], float(v_j), acc_c),
  // summed (c0 + c1) + (c2 + c3).  Per 16-key group the four chains' fmas are independent,
  // so the lone wave's dependent chain is a quarter of the keys (it was one fma per key,
  // 26-46 cycles each).  Padded keys: PS == 0 and a finite v, fma(0, v, acc) == acc.
  // The values of 4 keys of the lane's dim in one dword (the 4-key group layout, vg4 as
  // loaded in phase 0): each byte converted by one SDWA v_cvt_f32_i32.
  float c0 = 0.0f, c1 = 0.0f, c2 = 0.0f, c3 = 0.0f;
  if constexpr (KV_NEW) {
    // (self) this step's value code over the stale byte: key `step` is byte step & 3 of the
    // dword of group step >> 2, i.e. of vg4[step >> 4][(step >> 2) & 3].  With the position
    // from the host nrows == step + 1, so that fragment is the last one; a step replayed at
    // several positions (device counter) selects over all fragments
    const int pq = (step >> 2) & 3, sh = 8 * (step & 3);
    const uint32_t ins = (uint32_t)(uint8_t)vq << sh, keep = ~(0xffu << sh);
    auto patch = [&](uint32_t (&f)[4], bool here) {
#pragma unroll
      for (int q = 0; q < 4; ++q) f[q] = here && q == pq ? (f[q] & keep) | ins : f[q];
    };
    if (a.host_step1 > 0) {
      patch(vg4[NIT - 1], true);
    } else {
#pragma unroll
      for (int g = 0; g < NIT; ++g) patch(vg4[g], g == (step >> 4));
    }
  }
  // every 16-key group's PS operands are read first (the NIT groups that cover the staged
  // rows; those at or past nk16 are read and not used), so the chains pay the LDS latency once
  // instead of once per group (a rolled loop waited on its reads every 16 keys)
  float4 pg[NIT][4];
#pragma unroll
  for (int g = 0; g < NIT; ++g) {
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      pg[g][q] = *reinterpret_cast<const float4*>(PS + 16 * g + 4 * q);
    }
    // in group order (LDS returns in issue order: the first chains then wait for group 0
    // alone, which the scheduler would otherwise issue last)
    __builtin_amdgcn_sched_barrier(0);
  }
  // each fma an asm v_fmac_f32 (the IEEE fused multiply-add, as fmaf): left to itself the
  // compiler SLP-packs the four chains into v_pk_fma_f32 pairs — no faster on gfx950 (a
  // packed fp32 op issues at half rate) — and assembles their operand pairs with ~1 v_mov
  // per fma
  auto fmac = [](float& c, float p, float x) { asm("v_fmac_f32 %0, %1, %2" : "+v"(c) : "v"(p), "v"(x)); };
#pragma unroll
  for (int g = 0; g < NIT; ++g) {
    if (g == 0 || 16 * g < nk16) {       // (Sk >= 1: group 0 always)
      float v[16];
#pragma unroll
      for (int q = 0; q < 4; ++q)
#pragma unroll
        for (int e = 0; e < 4; ++e) v[4 * q + e] = (float)(int8_t)(vg4[g][q] >> (8 * e));
      const float4 p0 = pg[g][0], p1 = pg[g][1], p2 = pg[g][2], p3 = pg[g][3];
      fmac(c0, p0.x, v[0]);  fmac(c1, p1.x, v[4]);  fmac(c2, p2.x, v[8]);  fmac(c3, p3.x, v[12]);
      fmac(c0, p0.y, v[1]);  fmac(c1, p1.y, v[5]);  fmac(c2, p2.y, v[9]);  fmac(c3, p3.y, v[13]);
      fmac(c0, p0.z, v[2]);  fmac(c1, p1.z, v[6]);  fmac(c2, p2.z, v[10]); fmac(c3, p3.z, v[14]);
      fmac(c0, p0.w, v[3]);  fmac(c1, p1.w, v[7]);  fmac(c2, p2.w, v[11]); fmac(c3, p3.w, v[15]);
    }
  }
  const float acc = (c0 + c1) + (c2 + c3);
  QTX_STAMP(3);

  // phase 5: this head's 64 context values (and their absmax when asked for: the consumer
  // GEMM then takes the row maximum over the 8 heads, A_F32Q; the fused decode's consumer
  // forms it from the row itself, A_F32R)
  st_at(a.ctx, 4u * (unsigned)(b * 512 + h * 64 + lane), acc);
  if (a.pmax) {
    const float am = wave_max(fabsf(acc));
    if (lane == 0) a.pmax[(long)h * a.B + b] = am;
  }
  QTX_STAMP(4);
}

template <bool KV_NEW>
hipError_t dec_attn_nit(const DecAttnArgs& a, int B, int nrows, hipStream_t st) {
  const dim3 grid(B, 8), block(64);
  const KaLead l = da_lead<KV_NEW>(a);
  const DaTail t{a.step, a.mask, a.ctx, a.pmax, a.B};
  switch ((nrows + 15) / 16) {
    case 1: k_dec_attn<KV_NEW, 1><<<grid, block, 0, st>>>(QTX_KA_ARGS(l), t); break;
    case 2: k_dec_attn<KV_NEW, 2><<<grid, block, 0, st>>>(QTX_KA_ARGS(l), t); break;
    case 3: k_dec_attn<KV_NEW, 3><<<grid, block, 0, st>>>(QTX_KA_ARGS(l), t); break;
    case 4: k_dec_attn<KV_NEW, 4><<<grid, block, 0, st>>>(QTX_KA_ARGS(l), t); break;
    case 5: k_dec_attn<KV_NEW, 5><<<grid, block, 0, st>>>(QTX_KA_ARGS(l), t); break;
    case 6: k_dec_attn<KV_NEW, 6><<<grid, block, 0, st>>>(QTX_KA_ARGS(l), t); break;
    case 7: k_dec_attn<KV_NEW, 7><<<grid, block, 0, st>>>(QTX_KA_ARGS(l), t); break;
    case 8: k_dec_attn<KV_NEW, 8><<<grid, block, 0, st>>>(QTX_KA_ARGS(l), t); break;
    default: return hipErrorInvalidValue;
  }
  return hipGetLastError();
}

hipError_t launch_dec_attn(const DecAttnArgs& a, int B, hipStream_t st) {
  if (B <= 0) return hipSuccess;
  if (!a.ctx || a.B != B) return hipErrorInvalidValue;
  if (a.ldy < 0 || a.ldy >= (1L << 31) || a.kv_bs >= (1L << 31)) return hipErrorInvalidValue;   // 32-bit in the lead block
  if (a.kv_new) {
    if (a.kv_bs <= 0 || a.kv_bs > DEC_MAXK || a.host_step1 < 0 || a.host_step1 > a.kv_bs)
      return hipErrorInvalidValue;
    return dec_attn_nit<true>(a, B, a.host_step1 > 0 ? a.host_step1 : (int)a.kv_bs, st);
  }
  if (a.S <= 0 || a.S > DEC_MAXK) return hipErrorInvalidValue;
  return dec_attn_nit<false>(a, B, a.S, st);
}

// k_vgroup4: a [B * S, 512] int8 value matrix (L layers, layer stride v_ls) into k_dec_attn's
// 4-key group layout (byte ((b * G4 + g) * 512 + d) * 4 + e = v[b * S + 4 g + e][d], 0 past
// S; G4 = ceil(S / 4); layer stride o_ls): the decode's cross values, once per decode.
__global__ void k_vgroup4(const int8_t* v, long v_ls, int B, int S, int8_t* out, long o_ls) {
  const int G4 = (S + 3) >> 2;
  const long n = (long)B * G4 * 512;
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const int d = (int)(i & 511);
  const long bg = i >> 9;
  const int g = (int)(bg % G4), b = (int)(bg / G4);
  const int8_t* src = v + (long)blockIdx.y * v_ls;
  uint32_t w = 0;
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    const int j = 4 * g + e;
    const uint32_t byte = j < S ? (uint8_t)src[((long)b * S + j) * 512 + d] : 0u;
    w |= byte << (8 * e);
  }
  reinterpret_cast<uint32_t*>(out + (long)blockIdx.y * o_ls)[i] = w;
}

hipError_t launch_vgroup4(const int8_t* v, long v_ls, int L, int B, int S, int8_t* out,
                          long o_ls, hipStream_t st) {
  if (B <= 0 || S <= 0 || L <= 0) return hipSuccess;
  const long n = (long)B * ((S + 3) / 4) * 512;
  k_vgroup4<<<dim3((unsigned)((n + 255) / 256), L), dim3(256), 0, st>>>(v, v_ls, B, S, out, o_ls);
  return hipGetLastError();
}

// =====================================================================================
// k_quant_h2048: per-token quantization of fp32 rows of 2048 (the decode FFN's hidden from
// B >= 96, quant_linear.py:30-43): one 4-wave workgroup per row, wave w quarter w (8 values
// per lane), the row maximum met in LDS — a quarter of k_rows' one-wave-per-row chain.  The
// same scale (quant_scale of the row absmax, order-free) and codes (quant_pack).
// =====================================================================================
__global__ __launch_bounds__(256) void k_quant_h2048(const float* X, long ldx, int M,
                                                     int8_t* q, float* s) {
  __shared__ float wm[4];
  const int m = blockIdx.x, tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const float* xr = X + (long)m * ldx + 512 * wave;
  float4 t[2];
#pragma unroll
  for (int c = 0; c < 2; ++c) t[c] = *reinterpret_cast<const float4*>(xr + 4 * (lane + 64 * c));
  float lm = 0.0f;
#pragma unroll
  for (int c = 0; c < 2; ++c)
    lm = fmaxf(lm, fmaxf(fmaxf(fabsf(t[c].x), fabsf(t[c].y)), fmaxf(fabsf(t[c].z), fabsf(t[c].w))));
  lm = wave_absmax(lm);
  if (lane == 0) wm[wave] = lm;
  __syncthreads();
  const float sc = quant_scale(fmaxf(fmaxf(wm[0], wm[1]), fmaxf(wm[2], wm[3])), 127.0f);
  float tf[8];
#pragma unroll
  for (int c = 0; c < 2; ++c) {
    tf[4 * c] = t[c].x; tf[4 * c + 1] = t[c].y; tf[4 * c + 2] = t[c].z; tf[4 * c + 3] = t[c].w;
  }
  uint32_t qd[2];
  quant_pack<8>(tf, sc, qd);
  uint32_t* dst = reinterpret_cast<uint32_t*>(q + (long)m * 2048 + 512 * wave);
#pragma unroll
  for (int c = 0; c < 2; ++c) dst[lane + 64 * c] = qd[c];
  if (tid == 0) s[m] = sc;
}

hipError_t launch_quant_h2048(const float* X, long ldx, int M, int8_t* q, float* s,
                              hipStream_t st) {
  if (M <= 0) return hipSuccess;
  k_quant_h2048<<<dim3(M), dim3(256), 0, st>>>(X, ldx, M, q, s);
  return hipGetLastError();
}

// =====================================================================================
// k_generator_mfma: the canonical generator order on the fp32 matrix cores.
// logits[m, v] = ((c0 + c1) + (c2 + c3)) + b[v] with c_q the k-ordered fma chain over
// k in [128q, 128q + 128) from 0 (oracle OracleModel.logits): v_mfma_f32_16x16x4_f32 chained
// over a quarter (32 instructions, C starting at 0) is bit-for-bit that chain
// (cdna_hip_programming.md §3 "FP32-input MFMA").
// Block = 16 token rows x 64 vocab columns, 16 waves: wave w takes strip w & 3 (16
// columns) and k-quarter w >> 2, so the dependent MFMA chain per wave is 32 long (a lone
// 128-long chain cost ~6,100 cycles, ~48 per dependent MFMA: tools/stamp_bench.py).  A
// operand = the LayerNormed rows in LDS (one row per wave); B operand = the weight packed at
// load in MFMA order (k_pack_gen: per strip, per group of 4 k-steps, per lane one float4),
// each wave streaming its quarter strip (8 KB) with 8 coalesced 1 KB loads issued before
// the LayerNorm.  The quarters' partial tiles meet in LDS; the waves of quarter 0 add them
// in the canonical order and store.  The two 16-row blocks of a strip group run on one XCD
// (blockIdx remap): the second reads the strips from that XCD's L2.
// =====================================================================================
constexpr int GEN_Q = 32;   // float4 groups of 4 k-steps per lane (K = 512)

// (parameters in order of first use: all but `logits` / `rec` arrive preloaded in SGPRs)
// REC: also the per-strip top-2 records (qtx_kernels.h launch_generator_mfma); without it the
// kernel is what it was before the records existed
template <bool REC>
__global__ __launch_bounds__(1024) void k_generator_mfma(const float* Wm, int V, int M,
                                                         const float* bias, const float* x,
                                                         long ldx, const float* ln_a,
                                                         const float* ln_b, float* logits,
                                                         float* rec) {
  __shared__ __attribute__((aligned(16))) float X[16][514];   // stride 514: conflict-free reads
  __shared__ __attribute__((aligned(16))) v4f part[3][4][64];  // quarters 1..3: [strip][lane]
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int fr = lane & 15, fg = lane >> 4;
  const int sw = wave & 3, qq = wave >> 2;          // strip within the group, k-quarter
  // blockIdx -> (strip group g, row block rb): hw = 8 (nrb (g / 8) + rb) + g % 8, so the
  // row blocks of group g share hw % 8 (one XCD under round-robin placement)
  const unsigned nrb = (unsigned)(M + 15) >> 4, hw = blockIdx.x;   // (unsigned: a shorter division)
  const int rb = (int)((hw >> 3) % nrb), g = (int)(((hw >> 3) / nrb) * 8 + (hw & 7));
  const int nstrip = (V + 15) / 16, strip = g * 4 + sw;
  if (g * 4 >= nstrip) return;                     // whole block (uniform)
  const int m0 = rb * 16;
  const int vcol = strip * 16 + fr;
  QTX_STAMP(0);
  // 1. the quarter strip's B operands, all in flight before anything else (the row and the
  //    LayerNorm parameters first — the order of the skinny GEMMs — gained 0.02 ms per decode
  //    here, less than the A/B's bar: DESIGN.md §5, round 8)
  constexpr int QQ = GEN_Q / 4;
  const unsigned wo = 16u * (unsigned)((min(strip, nstrip - 1) * GEN_Q + QQ * qq) * 64 + lane);
  float4 wq[QQ];
#pragma unroll
  for (int q = 0; q < QQ; ++q) wq[q] = ld_at(reinterpret_cast<const float4*>(Wm), wo + 1024u * q);
  const float bv = ld_at(bias, 4u * min(vcol, V - 1));
  // 2. row `wave` of the block, LayerNorm in the canonical order, into LDS
  float xv[1][2][4];
  {
    const int m = min(m0 + wave, M - 1);
#pragma unroll
    for (int c = 0; c < 2; ++c) {
      const float4 t = ld_at(reinterpret_cast<const float4*>(x), 4u * (unsigned)(m * (int)ldx + 4 * (lane + 64 * c)));
      xv[0][c][0] = t.x; xv[0][c][1] = t.y; xv[0][c][2] = t.z; xv[0][c][3] = t.w;
    }
  }
  if (ln_a) ln_rows512<1>(xv, ln_a, ln_b, lane);
#pragma unroll
  for (int c = 0; c < 2; ++c) {
    float* d = &X[wave][4 * (lane + 64 * c)];
    *reinterpret_cast<float2*>(d) = make_float2(xv[0][c][0], xv[0][c][1]);
    *reinterpret_cast<float2*>(d + 2) = make_float2(xv[0][c][2], xv[0][c][3]);
  }
  __syncthreads();
  QTX_STAMP(1);
  // 3. the quarter's k-ordered chain: step s = 4 (QQ qq + q) + e uses A = X[fr][4s + fg],
  //    B = wq[q][e]
  v4f acc = {0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
  for (int q = 0; q < QQ; ++q) {
    const float b4[4] = {wq[q].x, wq[q].y, wq[q].z, wq[q].w};
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const float a = X[fr][4 * (4 * (QQ * qq + q) + e) + fg];
      acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a, b4[e], acc, 0, 0, 0);
    }
  }
  if (qq) part[qq - 1][sw][lane] = acc;
  __syncthreads();
  QTX_STAMP(2);
  if constexpr (!REC) {
    if (qq || vcol >= V) return;
    const v4f p1 = part[0][sw][lane], p2 = part[1][sw][lane], p3 = part[2][sw][lane];
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const int m = m0 + 4 * fg + e;
      if (m < M) st_at(logits, 4u * (unsigned)(m * V + vcol), ((acc[e] + p1[e]) + (p2[e] + p3[e])) + bv);
    }
    QTX_STAMP(3);
    return;
  }
  if (qq) return;
  const v4f p1 = part[0][sw][lane], p2 = part[1][sw][lane], p3 = part[2][sw][lane];
  const bool vok = vcol < V;
  float y[4];
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    const int m = m0 + 4 * fg + e;
    y[e] = ((acc[e] + p1[e]) + (p2[e] + p3[e])) + bv;
    if (vok && m < M) st_at(logits, 4u * (unsigned)(m * V + vcol), y[e]);
  }
  QTX_STAMP(3);
  // 4. the strip's top-2 record of each row (launch_skinny_tok finishes the reduction): the
  //    16 columns of row 4 fg + e are the 16 lanes of DPP row fg — no cross-wave step
  if (strip >= nstrip) return;                            // (wave-uniform)
  float m1[4], m2[4];
  int i1[4], fl[4];
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    m1[e] = row16_max(vok ? fmaxf(-3.0e38f, y[e]) : -3.0e38f);
    fl[e] = vok ? ((y[e] < __builtin_inff() ? 0 : 1) | (y[e] > -__builtin_inff() ? 2 : 0)) : 0;
  }
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    i1[e] = row16_min_i32(vok && y[e] == m1[e] ? vcol : 0x7fffffff);
    fl[e] = row16_or_i32(fl[e]);
  }
#pragma unroll
  for (int e = 0; e < 4; ++e)
    m2[e] = row16_max(vok && vcol != i1[e] ? fmaxf(-3.0e38f, y[e]) : -3.0e38f);
  if (fr == 0) {
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const int m = m0 + 4 * fg + e;
      if (m < M)
        st_at(reinterpret_cast<float4*>(rec), 16u * (unsigned)(m * nstrip + strip),
              make_float4(m1[e], m2[e], __int_as_float(i1[e]), __int_as_float(fl[e])));
    }
  }
}

hipError_t launch_generator_mfma(const float* x, long ldx, int M, const float* ln_a,
                                 const float* ln_b, const float* Wm, const float* b, int V,
                                 float* logits, hipStream_t st, float* rec) {
  if (M <= 0) return hipSuccess;
  if ((long)M * V >= (1L << 30) || (long)M * ldx >= (1L << 30)) return hipErrorInvalidValue;   // 32-bit offsets
  const int ngroup = (V + 63) / 64, nrb = (M + 15) / 16;
  const unsigned grid = 8u * nrb * ((ngroup + 7) / 8);
  if (rec)
    k_generator_mfma<true><<<dim3(grid), dim3(1024), 0, st>>>(Wm, V, M, b, x, ldx, ln_a, ln_b, logits, rec);
  else
    k_generator_mfma<false><<<dim3(grid), dim3(1024), 0, st>>>(Wm, V, M, b, x, ldx, ln_a, ln_b, logits, rec);
  return hipGetLastError();
}

// W [V][512] -> the MFMA-ordered strips of k_generator_mfma: out[((c * 32 + q) * 64 + l) * 4 + e]
// = W[16 c + (l & 15)][4 (4 q + e) + (l >> 4)] (0 past V).  One thread per float4.
__global__ void k_pack_gen(const float* W, int V, float* out) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  const int nstrip = (V + 15) / 16;
  if (i >= (long)nstrip * GEN_Q * 64) return;
  const int l = (int)(i % 64), q = (int)((i / 64) % GEN_Q), c = (int)(i / (64 * GEN_Q));
  const int v = 16 * c + (l & 15);
  float4 o;
  float* op = reinterpret_cast<float*>(&o);
#pragma unroll
  for (int e = 0; e < 4; ++e) op[e] = v < V ? W[(long)v * 512 + 4 * (4 * q + e) + (l >> 4)] : 0.0f;
  reinterpret_cast<float4*>(out)[i] = o;
}
hipError_t launch_pack_gen(const float* W, int V, float* out, hipStream_t st) {
  const long n = (long)((V + 15) / 16) * GEN_Q * 64;
  k_pack_gen<<<dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st>>>(W, V, out);
  return hipGetLastError();
}

#ifdef QTX_STAMPS   // diagnostic builds only: the generator launched bare (tools/stamp_bench.py)
extern "C" int qtx_debug_generator(const float* x, int M, const float* lna, const float* lnb,
                                   const float* Wt, const float* b, int V, float* logits,
                                   void* st) {
  return (int)launch_generator_mfma(x, 512, M, lna, lnb, Wt, b, V, logits, (hipStream_t)st);
}
#endif

__global__ void k_transpose(const float* in, int R, int Cc, float* out) {
  __shared__ float t[32][33];
  const int c0 = blockIdx.x * 32, r0 = blockIdx.y * 32, tx = threadIdx.x, ty = threadIdx.y;
  for (int i = ty; i < 32; i += 8)
    if (r0 + i < R && c0 + tx < Cc) t[i][tx] = in[(long)(r0 + i) * Cc + c0 + tx];
  __syncthreads();
  for (int i = ty; i < 32; i += 8)
    if (c0 + i < Cc && r0 + tx < R) out[(long)(c0 + i) * R + r0 + tx] = t[tx][i];
}
hipError_t launch_transpose(const float* in, int R, int Cc, float* out, hipStream_t st) {
  k_transpose<<<dim3((Cc + 31) / 32, (R + 31) / 32), dim3(32, 8), 0, st>>>(in, R, Cc, out);
  return hipGetLastError();
}

// =====================================================================================
// k_argmax_embed: one 1024-thread workgroup per row.  The row of logits stays in
// registers (8 per thread, all loads in flight at once).  The token is the first argmax
// of logp = (x - max) - lse (generator.py:15 log_softmax, torch.max's first-index rule).
// lse only matters when another logit lies within a few ulps of the maximum: with
// lse = logf(sum) <= logf(V) < 16, (x - max) < -ARG_DELTA rounds below -lse, so only
// values above max - ARG_DELTA can tie it.  Fast path (block-uniform): exactly one such
// value — it is the maximum and the token.  Otherwise the exponentials go through LDS
// for the canonical lane-split denominator (wave 0) and the first argmax of logp decides.
// A non-finite row (any NaN or +inf, or only -inf) is all-NaN under torch's log_softmax,
// and torch.max of it is index 0: that row's token is 0 (oracle log_softmax_argmax).
// Then the block writes the next decoder input (embedding + PE of the token).
// =====================================================================================
constexpr int ARG_T = 1024, ARG_NV = 8;
static_assert(ARG_MAXV == ARG_T * ARG_NV, "the row of logits in the workgroup's registers");
constexpr float ARG_DELTA = 4.0e-6f;   // >= 2 ulp(16): covers every V <= ARG_MAXV

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

// host_s1: the position + 1 when the host knows it (then no read of *step and no step
// advance: nothing of a decode whose every step knows its position reads the counter);
// 0: read *step and advance it (the last workgroup to arrive)
// (parameters in order of first use: those up to ids_bs arrive preloaded in SGPRs)
__global__ __launch_bounds__(1024) void k_argmax_embed(const float* logits, int V, int host_s1,
                                                       int* step, const float* pe,
                                                       const float* lut, int max_pos,
                                                       long ids_bs, int64_t* ids,
                                                       unsigned* arrive, float* xnext) {
  __shared__ float Ev[ARG_MAXV];
  __shared__ float redf[16], lse_s;
  __shared__ int redi[16], redc[16], redb[16];
  const int m = blockIdx.x, tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  QTX_STAMP(0);
  const unsigned xo = 4u * (unsigned)(m * V);
  float t[ARG_NV];
#pragma unroll
  for (int i = 0; i < ARG_NV; ++i) t[i] = ld_at(logits, xo + 4u * min(tid + ARG_T * i, V - 1));   // clamped
  // (the logits go out first: their addresses need preloaded arguments only, the position
  // may be a scalar load of the device counter)
  __builtin_amdgcn_sched_barrier(0);
  const int s = host_s1 > 0 ? host_s1 - 1 : *step;
  float4 pe_row = make_float4(0.0f, 0.0f, 0.0f, 0.0f);   // position s+1 is known up front
  if (tid < 128) pe_row = ld_at(reinterpret_cast<const float4*>(pe), 16u * (unsigned)(min(s + 1, max_pos - 1) * 128 + tid));
  QTX_STAMP(1);
  // max: order-free; every wave reduces the 16 wave maxima itself (no second barrier);
  // with it the non-finite test: bit 0 = a NaN or +inf, bit 1 = a value above -inf
  float lm = -3.0e38f;
  bool nonfin = false, fin = false;
#pragma unroll
  for (int i = 0; i < ARG_NV; ++i)
    if (tid + ARG_T * i < V) {
      lm = fmaxf(lm, t[i]);
      nonfin |= !(t[i] < __builtin_inff());
      fin |= t[i] > -__builtin_inff();
    }
  lm = wave_max(lm);
  const int flags = (__ballot(nonfin) ? 1 : 0) | (__ballot(fin) ? 2 : 0);
  if (lane == 0) { redf[w] = lm; redb[w] = flags; }
  __syncthreads();
  const float mx = wave_max(lane < 16 ? redf[lane] : -3.0e38f);
  // candidates for the first argmax of logp, and the first index of the maximum
  int cnt = 0, bi = 0x7fffffff;
#pragma unroll
  for (int i = 0; i < ARG_NV; ++i) {
    const int v = tid + ARG_T * i;
    if (v < V) {
      cnt += t[i] > mx - ARG_DELTA ? 1 : 0;
      if (t[i] == mx && v < bi) bi = v;
    }
  }
  cnt = wave_sum_i32(cnt);
  bi = wave_min_i32(bi);
  if (lane == 0) { redc[w] = cnt; redi[w] = bi; }
  __syncthreads();
  cnt = wave_sum_i32(lane < 16 ? redc[lane] : 0);
  int id = wave_min_i32(lane < 16 ? redi[lane] : 0x7fffffff);
  const bool bad = __ballot(lane < 16 && (redb[lane] & 1)) != 0ull ||
                   __ballot(lane < 16 && (redb[lane] & 2)) == 0ull;
  QTX_STAMP(2);
  if (bad) {
    id = 0;                                // torch.max of an all-NaN log_softmax row
  } else if (cnt != 1) {   // near-tie: the exact log-softmax decides (block-uniform)
    // e_v = qexp(x_v - max) into LDS for the ordered sum
#pragma unroll
    for (int i = 0; i < ARG_NV; ++i) {
      const int v = tid + ARG_T * i;
      if (v < V) Ev[v] = qexp(t[i] - mx);
    }
    __syncthreads();
    // canonical denominator: lane l sums e[l], e[l+64], ... in order (one wave), then tree
    if (w == 0) {
      float ls = 0.0f;
#pragma unroll 8
      for (int v = lane; v < V; v += 64) ls = ls + Ev[v];
      ls = wave_sum(ls);
      if (lane == 0) lse_s = logf(ls);
    }
    __syncthreads();
    const float lse = lse_s;
    // first argmax of logp = (x - max) - lse (torch.max tie rule)
    float best = -3.0e38f;
    int bj = 0x7fffffff;
#pragma unroll
    for (int i = 0; i < ARG_NV; ++i) {
      const int v = tid + ARG_T * i;
      if (v < V) {
        const float lp = (t[i] - mx) - lse;
        if (lp > best) { best = lp; bj = v; }
      }
    }
    // the maximum, then the smallest index holding it: per wave, then over the 16 waves
    const float wb = wave_max(best);
    const int wi = wave_min_i32(best == wb ? bj : 0x7fffffff);
    __syncthreads();                       // (redf / redi are reused)
    if (lane == 0) { redf[w] = wb; redi[w] = wi; }
    __syncthreads();
    const float gv = lane < 16 ? redf[lane] : -3.0e38f;
    const float gb = wave_max(gv);
    id = wave_min_i32(lane < 16 && gv == gb ? redi[lane] : 0x7fffffff);
    id = min(id, V - 1);                   // keeps the embedding gather in bounds, whatever
  }
  if (tid == 0 && s >= 0 && s + 1 < ids_bs) ids[m * ids_bs + s + 1] = id;   // bounded (stale position)
  QTX_STAMP(4);
  // next decoder input: tgt_embed(id) at position s + 1 (embeddings.py:12-13)
  if (tid < 128) {
    const float sc = 0x1.6a09e6p+4f;
    const float4 e = ld_at(reinterpret_cast<const float4*>(lut), 16u * (unsigned)(id * 128 + tid));
    const float4 q = pe_row;
    st_at(reinterpret_cast<float4*>(xnext), 16u * (unsigned)(m * 128 + tid),
          make_float4(e.x * sc + q.x, e.y * sc + q.y, e.z * sc + q.z, e.w * sc + q.w));
  }
  QTX_STAMP(5);
  // every workgroup has read *step above; the last one to arrive advances it
  if (host_s1 == 0 && tid == 0) {
    const unsigned tk = atomicAdd(arrive, 1u);
    if (tk == gridDim.x - 1) {
      *step = s + 1;
      *arrive = 0u;
    }
  }
}

hipError_t launch_argmax_embed(const float* logits, int M, int V, int64_t* ids, long ids_bs,
                               int* step, unsigned* arrive, const float* lut, const float* pe,
                               int max_pos, float* xnext, hipStream_t st, int host_s1) {
  if (M <= 0) return hipSuccess;
  if (V > ARG_MAXV || host_s1 < 0 || (long)M * V >= (1L << 30)) return hipErrorInvalidValue;
  k_argmax_embed<<<dim3(M), dim3(ARG_T), 0, st>>>(logits, V, host_s1, step, pe, lut, max_pos,
                                                  ids_bs, ids, arrive, xnext);
  return hipGetLastError();
}

// =====================================================================================
// k_skinny_wide_tok: the decode tail folded into layer 0's LN+QKV launch (steps after the
// first of a plain decode whose positions the host knows).  k_skinny_wide<RB, 8, A_LN, 0>
// with another source of its rows: the wave that owns row m finishes the vocabulary
// reduction the generator began (k_generator_mfma's per-strip records: <= 8 per lane, merged
// lane-locally, then over the wave — max / top-2 is order-free), decides the token exactly as
// k_argmax_embed does, gathers its embedding and forms x = e * sqrt(512) + pe, the row the
// A_LN prologue would have loaded.  The near-tie path is k_argmax_embed's canonical
// lane-split sum with one wave holding the whole row (lane l: logits l, l + 64, ... in order).
// Every column workgroup decides the same token from the same records; those of the first
// column block store x (the residual of layer 0's O-projection) and the id.  The records'
// and the PE row's addresses come from preloaded arguments; the weights follow them.
// =====================================================================================
struct TkLead {
  uint64_t rec, pe_row; int M, V; uint64_t W; int ldw, N; uint64_t sw, lut;
};
struct TkTail {
  const float* ln_a; const float* ln_b; const float* bias; const float* logits;
  float* out; float* xres; int64_t* ids; long ids_bs; int pos, ldo;
};
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
// the first argmax of logp = (x - mx) - lse over one row of logits, one wave
__device__ __forceinline__ int tok_exact(const float* row, int V, float mx, int lane) {
  float ls = 0.0f;
  for (int v = lane; v < V; v += 64) ls = ls + qexp(row[v] - mx);
  ls = wave_sum(ls);
  const float lse = logf(ls);
  float best = -3.0e38f;
  int bj = 0x7fffffff;
  for (int v = lane; v < V; v += 64) {
    const float lp = (row[v] - mx) - lse;
    if (lp > best) { best = lp; bj = v; }
  }
  const float wb = wave_max(best);
  return wave_min_i32(best == wb ? bj : 0x7fffffff);
}

template <int RB>
__global__ __launch_bounds__(256) void k_skinny_wide_tok(QTX_KA_PARAMS, TkTail kt) {
  const TkLead l = __builtin_bit_cast(TkLead, QTX_KA_VALS);
  constexpr int K = 512, NS = K / 64, LDA = K + 16, RPW = RB / 4;
  constexpr int NR = ARG_MAXV / 16 / 64;   // records per lane
  static_assert(RB == 4 || RB == 8, "one or two rows per wave");
  __shared__ __attribute__((aligned(16))) uint8_t As[16 * LDA];
  __shared__ float sas[16];
  __shared__ v4i tail[4][4 * RB];
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int fr = lane & 15, fg = lane >> 4;
  const int n0 = blockIdx.x * 64 + 16 * wave, m0 = blockIdx.y * RB;
  const int M = l.M, V = l.V, nstrip = (V + 15) >> 4;
  // 1. the rows' records (lane: strips lane, lane + 64, ...; clamped, masked below) and the
  //    PE row of the position
  float4 rc[RPW][NR], pe[2];
#pragma unroll
  for (int j = 0; j < RPW; ++j) {
    const int m = min(m0 + wave + 4 * j, M - 1);
#pragma unroll
    for (int i = 0; i < NR; ++i)
      rc[j][i] = ld_at(ka_ptr<const float4>(l.rec), 16u * (unsigned)(m * nstrip + min(lane + 64 * i, nstrip - 1)));
  }
#pragma unroll
  for (int c = 0; c < 2; ++c) pe[c] = ld_at(ka_ptr<const float4>(l.pe_row), 16u * (unsigned)(lane + 64 * c));
  // 2. this lane's W fragments (all of K) and the epilogue operands (N % 64 == 0: in range)
  const int col = n0 + fr;
  uint4 wf[NS];
#pragma unroll
  for (int s = 0; s < NS; ++s)
    wf[s] = ld_at(ka_ptr<const uint4>(l.W), (unsigned)(col * l.ldw + 64 * s + 16 * fg));
  const float swc = ld_at(ka_ptr<const float>(l.sw), 4u * col);
  __builtin_amdgcn_sched_barrier(0);   // as in k_skinny: trailing arguments from here on
  const float bc = ld_at(kt.bias, 4u * col);
  float ga[2][4], gb[2][4];
  ln_params512(kt.ln_a, kt.ln_b, lane, ga, gb);
  // 3. the token of each row and its input row x
  float v[RPW][2][4];
  int ids[RPW];
#pragma unroll
  for (int j = 0; j < RPW; ++j) {
    const int m = min(m0 + wave + 4 * j, M - 1);
    TokRec t{-3.0e38f, -3.0e38f, 0x7fffffff, 0};
#pragma unroll
    for (int i = 0; i < NR; ++i) {
      const bool in = lane + 64 * i < nstrip;
      tok_merge(t, in ? rc[j][i].x : -3.0e38f, in ? rc[j][i].y : -3.0e38f,
                in ? __float_as_int(rc[j][i].z) : 0x7fffffff, in ? __float_as_int(rc[j][i].w) : 0);
    }
    tok_merge_dpp<0xB1>(t);
    tok_merge_dpp<0x4E>(t);
    tok_merge_dpp<0x141>(t);
    tok_merge_dpp<0x140>(t);
    TokRec w{lane_f(t.m1, 0), lane_f(t.m2, 0), __builtin_amdgcn_readlane(t.i1, 0),
             __builtin_amdgcn_readlane(t.fl, 0)};
#pragma unroll
    for (int q = 16; q < 64; q += 16)
      tok_merge(w, lane_f(t.m1, q), lane_f(t.m2, q), __builtin_amdgcn_readlane(t.i1, q),
                __builtin_amdgcn_readlane(t.fl, q));
    int id;
    if ((w.fl & 1) || !(w.fl & 2)) {
      id = 0;                              // torch.max of an all-NaN log_softmax row
    } else if (!(w.m2 > w.m1 - ARG_DELTA) && w.i1 != 0x7fffffff) {
      id = w.i1;                           // exactly one value above max - ARG_DELTA
    } else {                               // near-tie: the exact log-softmax decides
      id = tok_exact(kt.logits + (long)m * V, V, w.m1, lane);
    }
    ids[j] = max(min(id, V - 1), 0);       // keeps the embedding gather in bounds, whatever
  }
  // next decoder input: tgt_embed(id) at the position (every load in flight before its use)
  float4 em[RPW][2];
#pragma unroll
  for (int j = 0; j < RPW; ++j)
#pragma unroll
    for (int c = 0; c < 2; ++c)
      em[j][c] = ld_at(ka_ptr<const float4>(l.lut), 16u * (unsigned)(ids[j] * 128 + lane + 64 * c));
#pragma unroll
  for (int j = 0; j < RPW; ++j) {
    const int r = wave + 4 * j, m = min(m0 + r, M - 1);
    const float sc = 0x1.6a09e6p+4f;
    const bool st = blockIdx.x == 0 && m0 + r < M;
#pragma unroll
    for (int c = 0; c < 2; ++c) {
      const float4 e = em[j][c];
      const float4 x = make_float4(e.x * sc + pe[c].x, e.y * sc + pe[c].y, e.z * sc + pe[c].z,
                                   e.w * sc + pe[c].w);
      v[j][c][0] = x.x; v[j][c][1] = x.y; v[j][c][2] = x.z; v[j][c][3] = x.w;
      if (st) st_at(reinterpret_cast<float4*>(kt.xres), 16u * (unsigned)(m * 128 + lane + 64 * c), x);
    }
    if (st && lane == 0 && kt.pos < kt.ids_bs) kt.ids[m * kt.ids_bs + kt.pos] = ids[j];
  }
  // 4. LayerNorm + per-token quantization into LDS, as the A_LN prologue
  {
    uint32_t q[RPW][2];
    float sc[RPW];
    ln_rows512<RPW>(v, ga, gb);
    quant_rows512<RPW, true>(v, q, sc);
#pragma unroll
    for (int j = 0; j < RPW; ++j) {
      const int r = wave + 4 * j;
      const bool ok = m0 + r < M;
      uint32_t* dst = reinterpret_cast<uint32_t*>(As + r * LDA);
      dst[lane] = ok ? q[j][0] : 0u;
      dst[lane + 64] = ok ? q[j][1] : 0u;
      if (lane == 0) sas[r] = ok ? sc[j] : 0.0f;
    }
  }
  __syncthreads();
  // 5. MFMA over all of K and the epilogue of k_skinny_wide (flags 0)
  v4i acc = v4i{0, 0, 0, 0};
#pragma unroll
  for (int s = 0; s < NS; ++s) {
    const v4i afr = *reinterpret_cast<const v4i*>(As + fr * LDA + 64 * s + 16 * fg);
    acc = __builtin_amdgcn_mfma_i32_16x16x64_i8(afr, __builtin_bit_cast(v4i, wf[s]), acc, 0, 0, 0);
  }
  if (fg < RPW) tail[wave][16 * fg + fr] = acc;
  __builtin_amdgcn_wave_barrier();      // as in k_skinny_wide
#pragma unroll
  for (int j = 0; j < RPW; ++j) {
    const int vv = reinterpret_cast<const int*>(&tail[wave][16 * j + fr])[fg];
    const int r = fg + 4 * j, row = m0 + r;
    const float y = ((float)vv * sas[r]) * swc + bc;
    if (row < M) st_at(kt.out, 4u * (unsigned)(row * kt.ldo + col), y);
  }
}

hipError_t launch_skinny_tok(const SkinnyArgs& g, const TokArgs& t, hipStream_t st) {
  if (g.M <= 0) return hipSuccess;
  const long lim = 1L << 30;   // 32-bit byte offsets, as launch_skinny
  if (g.K != 512 || g.N % 64 || g.flags || g.ldw != 512 || t.V < 1 || t.V > ARG_MAXV ||
      t.pos < 1 || (long)g.M * t.V >= lim || (long)g.M * g.ldo >= lim || (long)g.N * g.ldw >= lim)
    return hipErrorInvalidValue;
  TkLead l{};
  l.rec = ka_int(t.rec); l.pe_row = ka_int(t.pe + (long)std::min(t.pos, t.max_pos - 1) * 512);
  l.M = g.M; l.V = t.V; l.W = ka_int(g.W); l.ldw = (int)g.ldw; l.N = g.N;
  l.sw = ka_int(g.sw); l.lut = ka_int(t.lut);
  const TkTail kt{g.ln_a, g.ln_b, g.bias, t.logits, g.out, t.xres, t.ids, t.ids_bs, t.pos, (int)g.ldo};
  const KaLead ka = ka_pack(l);
  // rows per workgroup as skinny_mode's N-split LayerNorm GEMMs
  if (g.M >= 96)
    k_skinny_wide_tok<8><<<dim3(g.N / 64, (g.M + 7) / 8), 256, 0, st>>>(QTX_KA_ARGS(ka), kt);
  else
    k_skinny_wide_tok<4><<<dim3(g.N / 64, (g.M + 3) / 4), 256, 0, st>>>(QTX_KA_ARGS(ka), kt);
  return hipGetLastError();
}

// =====================================================================================
// k_top2_embed: k_argmax_embed's scored form (the campaign's torch.topk(prob, 2) of the
// step, parallelized_inject_onnx_transformer.py:718-740).  Same workgroup shape, loads and
// position / arrival-counter contract; it always evaluates the canonical log-softmax
// (k_argmax_embed's near-tie branch, with the denominator's log taken by qlog: the values
// go out to the caller) and selects the two best entries of logp under "larger logp, then
// smaller index" (include/qtx.h: scored decode): per thread, per wave, then over the 16
// waves.  Row m writes ids[m * ids_bs + s + 1] = top 1, entry (m * (ids_bs - 1) + s) of
// top_ids / top_logp [.., 2], and the next decoder input tgt_embed(top 1) at position s + 1,
// bit-identical to k_argmax_embed's.  A non-finite row: ids (0, 1), both values NaN.
// Limits as k_argmax_embed: V <= ARG_MAXV, M * V < 2^30; and V >= 2.
// (parameters in order of first use: those up to ids_bs arrive preloaded in SGPRs)
// =====================================================================================
__global__ __launch_bounds__(1024) void k_top2_embed(const float* logits, int V, int host_s1,
                                                     int* step, const float* pe,
                                                     const float* lut, int max_pos,
                                                     long ids_bs, int64_t* ids,
                                                     int64_t* top_ids, float* top_logp,
                                                     unsigned* arrive, float* xnext) {
  __shared__ float Ev[ARG_MAXV];
  __shared__ float redf[16], lse_s, rv1[16], rv2[16];
  __shared__ int redb[16], ri1[16], ri2[16];
  const int m = blockIdx.x, tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const unsigned xo = 4u * (unsigned)(m * V);
  float t[ARG_NV];
#pragma unroll
  for (int i = 0; i < ARG_NV; ++i) t[i] = ld_at(logits, xo + 4u * min(tid + ARG_T * i, V - 1));   // clamped
  __builtin_amdgcn_sched_barrier(0);
  const int s = host_s1 > 0 ? host_s1 - 1 : *step;
  float4 pe_row = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
  if (tid < 128) pe_row = ld_at(reinterpret_cast<const float4*>(pe), 16u * (unsigned)(min(s + 1, max_pos - 1) * 128 + tid));
  // max and the non-finite test, as k_argmax_embed
  float lm = -3.0e38f;
  bool nonfin = false, fin = false;
#pragma unroll
  for (int i = 0; i < ARG_NV; ++i)
    if (tid + ARG_T * i < V) {
      lm = fmaxf(lm, t[i]);
      nonfin |= !(t[i] < __builtin_inff());
      fin |= t[i] > -__builtin_inff();
    }
  lm = wave_max(lm);
  const int flags = (__ballot(nonfin) ? 1 : 0) | (__ballot(fin) ? 2 : 0);
  if (lane == 0) { redf[w] = lm; redb[w] = flags; }
  __syncthreads();
  const float mx = wave_max(lane < 16 ? redf[lane] : -3.0e38f);
  const bool bad = __ballot(lane < 16 && (redb[lane] & 1)) != 0ull ||
                   __ballot(lane < 16 && (redb[lane] & 2)) == 0ull;
  Top2 top;
  if (bad) {                               // an all-NaN log_softmax row (block-uniform)
    top.i1 = 0; top.i2 = 1;
    top.v1 = top.v2 = __builtin_nanf("");
  } else {
    // e_v = qexp(x_v - max) into LDS for the ordered sum
#pragma unroll
    for (int i = 0; i < ARG_NV; ++i) {
      const int v = tid + ARG_T * i;
      if (v < V) Ev[v] = qexp(t[i] - mx);
    }
    __syncthreads();
    // canonical denominator: lane l sums e[l], e[l+64], ... in order (one wave), then tree
    if (w == 0) {
      float ls = 0.0f;
#pragma unroll 8
      for (int v = lane; v < V; v += 64) ls = ls + Ev[v];
      ls = wave_sum(ls);
      if (lane == 0) lse_s = qlog(ls);
    }
    __syncthreads();
    const float lse = lse_s;
    // the two best of logp = (x - max) - lse: this thread's (ascending indices), the wave's
#pragma unroll
    for (int i = 0; i < ARG_NV; ++i) {
      const int v = tid + ARG_T * i;
      if (v < V) top.add((t[i] - mx) - lse, v);
    }
    wave_top2(top);
    if (lane == 0) { rv1[w] = top.v1; ri1[w] = top.i1; rv2[w] = top.v2; ri2[w] = top.i2; }
    __syncthreads();
    // the 16 waves' pairs: every wave merges them itself
    top = Top2{};
    if (lane < 16) { top.v1 = rv1[lane]; top.i1 = ri1[lane]; top.v2 = rv2[lane]; top.i2 = ri2[lane]; }
    wave_top2(top);
  }
  const int id = min(max(top.i1, 0), V - 1);   // keeps the embedding gather in bounds, whatever
  if (tid == 0 && s >= 0 && s + 1 < ids_bs) {  // bounded (stale position)
    ids[m * ids_bs + s + 1] = id;
    const long e = 2 * (m * (ids_bs - 1) + s);
    top_ids[e] = id; top_ids[e + 1] = top.i2;
    top_logp[e] = top.v1; top_logp[e + 1] = top.v2;
  }
  // next decoder input: tgt_embed(id) at position s + 1 (embeddings.py:12-13)
  if (tid < 128) {
    const float sc = 0x1.6a09e6p+4f;
    const float4 e = ld_at(reinterpret_cast<const float4*>(lut), 16u * (unsigned)(id * 128 + tid));
    const float4 q = pe_row;
    st_at(reinterpret_cast<float4*>(xnext), 16u * (unsigned)(m * 128 + tid),
          make_float4(e.x * sc + q.x, e.y * sc + q.y, e.z * sc + q.z, e.w * sc + q.w));
  }
  // every workgroup has read *step above; the last one to arrive advances it
  if (host_s1 == 0 && tid == 0) {
    const unsigned tk = atomicAdd(arrive, 1u);
    if (tk == gridDim.x - 1) {
      *step = s + 1;
      *arrive = 0u;
    }
  }
}

hipError_t launch_top2_embed(const float* logits, int M, int V, int64_t* ids, long ids_bs,
                             int64_t* top_ids, float* top_logp, int* step, unsigned* arrive,
                             const float* lut, const float* pe, int max_pos, float* xnext,
                             hipStream_t st, int host_s1) {
  if (M <= 0) return hipSuccess;
  if (V < 2 || V > ARG_MAXV || host_s1 < 0 || (long)M * V >= (1L << 30)) return hipErrorInvalidValue;
  k_top2_embed<<<dim3(M), dim3(ARG_T), 0, st>>>(logits, V, host_s1, step, pe, lut, max_pos,
                                                ids_bs, ids, top_ids, top_logp, arrive, xnext);
  return hipGetLastError();
}

// =====================================================================================
// The decoder-fault decode's small kernels (qtx_greedy_decode_dfault, qtx_api.hip): one lane
// per sentence.  Scalars lead the parameter lists (preloaded); every offset is bounded on
// the host (B * ids_bs < 2^30) and every position write checks its column.
//   rec_ids int64 / rec_logp float [B][2][2]: [b][0] the golden, [b][1] the faulty top 2 of
//   the corrupted step.
// =====================================================================================
// k_dfault_gold: rec[b][0][:] = entry (b, step) of top_ids / top_logp [B][top_bs][2] — the
// golden pair, kept before the faulty one replaces the entry
__global__ __launch_bounds__(64) void k_dfault_gold(int B, int step, int top_bs,
                                                    const int64_t* top_ids, const float* top_logp,
                                                    int64_t* rec_ids, float* rec_logp) {
  const int b = blockIdx.x * 64 + threadIdx.x;
  if (b >= B || step >= top_bs) return;
  const int e = 2 * (b * top_bs + step);
  rec_ids[4 * b] = top_ids[e]; rec_ids[4 * b + 1] = top_ids[e + 1];
  rec_logp[4 * b] = top_logp[e]; rec_logp[4 * b + 1] = top_logp[e + 1];
}

hipError_t launch_dfault_gold(const int64_t* top_ids, const float* top_logp, long top_bs,
                              int step, int B, int64_t* rec_ids, float* rec_logp,
                              hipStream_t st) {
  if (B <= 0) return hipSuccess;
  if (step < 0 || step >= top_bs || (long)B * top_bs >= (1L << 29)) return hipErrorInvalidValue;
  k_dfault_gold<<<dim3((B + 63) / 64), dim3(64), 0, st>>>(B, step, (int)top_bs, top_ids, top_logp,
                                                         rec_ids, rec_logp);
  return hipGetLastError();
}

// k_dfault_tail: the faulty pair rec[b][1][:] goes out — its winner to ids[b][step + 1], the
// pair to entry (b, step) of top_ids / top_logp [B][ids_bs - 1][2], and changed[b] = (the
// golden winner != the faulty one).  ids, top_ids / top_logp, changed: each may be null.
__global__ __launch_bounds__(64) void k_dfault_tail(int B, int step, int ids_bs,
                                                    const int64_t* rec_ids, const float* rec_logp,
                                                    int64_t* ids, int64_t* top_ids,
                                                    float* top_logp, int* changed) {
  const int b = blockIdx.x * 64 + threadIdx.x;
  if (b >= B) return;
  const int64_t f0 = rec_ids[4 * b + 2], f1 = rec_ids[4 * b + 3];
  if (ids && step + 1 < ids_bs) ids[b * ids_bs + step + 1] = f0;
  if (top_ids && step < ids_bs - 1) {
    const int e = 2 * (b * (ids_bs - 1) + step);
    top_ids[e] = f0; top_ids[e + 1] = f1;
    top_logp[e] = rec_logp[4 * b + 2]; top_logp[e + 1] = rec_logp[4 * b + 3];
  }
  if (changed) changed[b] = rec_ids[4 * b] != f0 ? 1 : 0;
}

hipError_t launch_dfault_tail(const int64_t* rec_ids, const float* rec_logp, int B, int step,
                              long ids_bs, int64_t* ids, int64_t* top_ids, float* top_logp,
                              int* changed, hipStream_t st) {
  if (B <= 0) return hipSuccess;
  if (step < 0 || step + 1 >= ids_bs || (long)B * ids_bs >= (1L << 29) || !top_ids != !top_logp)
    return hipErrorInvalidValue;
  k_dfault_tail<<<dim3((B + 63) / 64), dim3(64), 0, st>>>(B, step, (int)ids_bs, rec_ids, rec_logp,
                                                         ids, top_ids, top_logp, changed);
  return hipGetLastError();
}

// k_causal_mask: mask [T][T] uint8, keep[i][j] = j <= i (the faulty pass's target mask)
__global__ __launch_bounds__(256) void k_causal_mask(int T, uint8_t* mask) {
  const int e = blockIdx.x * 256 + threadIdx.x;
  if (e >= T * T) return;
  mask[e] = e % T <= e / T ? 1 : 0;
}

hipError_t launch_causal_mask(uint8_t* mask, int T, hipStream_t st) {
  if (T <= 0) return hipSuccess;
  if (T > 512) return hipErrorInvalidValue;
  k_causal_mask<<<dim3((T * T + 255) / 256), dim3(256), 0, st>>>(T, mask);
  return hipGetLastError();
}

// k_set_steps: the decode's position counters set to `value`, the arrival counters to 0:
// step [4] (the unfused step) and the G sub-batches' gsteps [G][4] (lane g + 1)
__global__ __launch_bounds__(64) void k_set_steps(int G, int value, int* step, int* gsteps) {
  const int l = threadIdx.x;
  if (l > G) return;
  int* s = l == 0 ? step : gsteps + 4 * (l - 1);
  s[0] = value;
  s[1] = 0;
}

hipError_t launch_set_steps(int* step, int* gsteps, int G, int value, hipStream_t st) {
  if (G < 0 || G > 63 || value < 0) return hipErrorInvalidValue;
  k_set_steps<<<dim3(1), dim3(64), 0, st>>>(G, value, step, gsteps);
  return hipGetLastError();
}

// k_cache_upset: one stored bit of the decode's K/V caches flipped (qtx_greedy_decode_kvfault,
// include/qtx.h qtx_cache_upset): bit `bit` of the code bytes c0 and c1 (c1: a second copy of
// the same cell, e.g. the cross values' 4-key groups next to their row-major rows) or of the
// float32 scale word s; each may be null.  The caller bounds every address on the host.
__global__ __launch_bounds__(64) void k_cache_upset(int bit, uint8_t* c0, uint8_t* c1,
                                                    uint32_t* s) {
  if (threadIdx.x != 0) return;
  if (c0) *c0 = (uint8_t)(*c0 ^ (1u << bit));
  if (c1) *c1 = (uint8_t)(*c1 ^ (1u << bit));
  if (s) *s = *s ^ (1u << bit);
}

hipError_t launch_cache_upset(int8_t* c0, int8_t* c1, float* s, int bit, hipStream_t st) {
  if (bit < 0 || bit > ((c0 || c1) ? 7 : 31) || ((c0 || c1) && s) || (!c0 && !c1 && !s))
    return hipErrorInvalidValue;
  k_cache_upset<<<dim3(1), dim3(64), 0, st>>>(bit, reinterpret_cast<uint8_t*>(c0),
                                             reinterpret_cast<uint8_t*>(c1),
                                             reinterpret_cast<uint32_t*>(s));
  return hipGetLastError();
}


// =====================================================================================
// Beam search (include/qtx.h, beam search; qtx_api.hip beam_prologue / beam_steps /
// qtx_beam_decode).  Rows r = b * K + k are the K hypotheses of sentence b.  Scalars lead the
// parameter lists (preloaded); every offset is bounded on the host (launch_beam_select:
// B * K * V < 2^30, V < 2^21, B * K < 2^21) and every position write checks its column.
// =====================================================================================
// The candidate (value, flat) as one 64-bit key whose unsigned order is the selection's total
// order "larger value, then smaller flat": the value's monotone image in the high word, ~flat
// in the low word.  Key 0 is the empty slot: below every candidate (-inf maps to 0x007fffff).
// The image orders +0.0 above -0.0, which the order on values takes as equal.  The search never
// forms a -0.0 (it needs (-0) + (-0), and the scores start at +0.0); a caller of the per-op
// entry who passes a -0.0 score gets it ranked just below +0.0 and returned unchanged.
__device__ __forceinline__ uint32_t beam_fkey(float v) {
  const uint32_t b = __float_as_uint(v);
  return b ^ ((b >> 31) ? 0xffffffffu : 0x80000000u);
}
__device__ __forceinline__ float beam_fval(uint32_t k) {
  return __uint_as_float(k ^ ((k >> 31) ? 0x80000000u : 0xffffffffu));
}
__device__ __forceinline__ unsigned long long wave_max_u64(unsigned long long v) {
#pragma unroll
  for (int off = 1; off < 64; off <<= 1) {
    const unsigned long long o = __shfl_xor(v, off, 64);
    v = o > v ? o : v;
  }
  return v;
}

// k_beam_select: one 1024-thread workgroup per sentence; the tail of the beam step, fused and
// unfused (no LDS-resident vocabulary: the logits are read from global memory; V < 2^21 for the
// 32-bit embedding offsets).  Waves 0 .. K-1 form their row's log-softmax terms (row_lse,
// qtx_common.h); then every thread scans its stripe of the K * V candidates
//   live row k:     (fl32(score[k] + logp[k][v]), k * V + v), a non-finite value taken as -inf
//   finished row k: the single candidate (score[k], k * V + pad)
// keeping its best KB keys in registers, and K rounds of a workgroup maximum (the winner
// removed each round) give the K best in order.  Slot j takes the j-th: parent = flat / V,
// token = flat % V, score = value, finished = parent finished or token == eos, length = s + 1
// unless the parent was finished; back-pointers (parent, token) of step s; the next decoder
// input tgt_embed(token) at position s + 1.  step[0]: the position s (read, then advanced by
// the last workgroup to arrive), step[1]: arrival counter, step[2]: accumulator of the rows
// still live, step[3]: their count after this step (what the host reads for the early exit).
constexpr int BEAM_T = 1024;
template <int KB>
__global__ __launch_bounds__(BEAM_T) void k_beam_select(int V, int K, int eos, int pad,
                                                        int max_len, int max_pos,
                                                        const float* logits, int* step,
                                                        float* score, int* fin, int* len,
                                                        int* parent, int* bp_par, int* bp_tok,
                                                        const float* lut, const float* pe,
                                                        float* xnext) {
  __shared__ float s_mx[BEAM_MAXK], s_lse[BEAM_MAXK], s_score[BEAM_MAXK];
  __shared__ int s_bad[BEAM_MAXK], s_fin[BEAM_MAXK], s_len[BEAM_MAXK];
  __shared__ unsigned long long red[2][BEAM_T / 64], win[BEAM_MAXK];
  const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int R = gridDim.x * K;
  const int s = *step;
  if (tid < K) {
    s_score[tid] = score[b * K + tid];
    s_fin[tid] = fin[b * K + tid];
    s_len[tid] = len[b * K + tid];
  }
  if (w < K) {
    float mx, lse;
    bool bad;
    row_lse(logits + (size_t)(b * K + w) * V, V, lane, mx, lse, bad);
    if (lane == 0) { s_mx[w] = mx; s_lse[w] = lse; s_bad[w] = bad ? 1 : 0; }
  }
  __syncthreads();
  unsigned long long keys[KB];
#pragma unroll
  for (int i = 0; i < KB; ++i) keys[i] = 0ull;
  auto offer = [&](float val, int flat) {
    if (!(fabsf(val) < __builtin_inff())) val = -__builtin_inff();   // NaN, +-inf
    const unsigned long long key =
        ((unsigned long long)beam_fkey(val) << 32) | (unsigned long long)(~(uint32_t)flat);
    if (key > keys[KB - 1]) {
      keys[KB - 1] = key;
#pragma unroll
      for (int i = KB - 1; i > 0; --i)
        if (keys[i] > keys[i - 1]) {
          const unsigned long long t = keys[i]; keys[i] = keys[i - 1]; keys[i - 1] = t;
        }
    }
  };
  for (int k = 0; k < K; ++k) {
    const float sc = s_score[k];
    if (s_fin[k]) {                          // (block-uniform)
      if (tid == 0) offer(sc, k * V + pad);
      continue;
    }
    const float* x = logits + (size_t)(b * K + k) * V;
    const float mx = s_mx[k], lse = s_lse[k];
    const bool bad = s_bad[k] != 0;
    for (int v = tid; v < V; v += BEAM_T)
      offer(bad ? -__builtin_inff() : sc + ((x[v] - mx) - lse), k * V + v);
  }
  for (int j = 0; j < K; ++j) {
    const unsigned long long h = wave_max_u64(keys[0]);
    if (lane == 0) red[j & 1][w] = h;
    __syncthreads();
    unsigned long long g = 0ull;
#pragma unroll
    for (int i = 0; i < BEAM_T / 64; ++i) {
      const unsigned long long o = red[j & 1][i];
      g = o > g ? o : g;
    }
    if (keys[0] == g && g != 0ull) {         // the winner's owner drops it (keys are distinct)
#pragma unroll
      for (int i = 0; i + 1 < KB; ++i) keys[i] = keys[i + 1];
      keys[KB - 1] = 0ull;
    }
    if (tid == 0) win[j] = g;
  }
  __syncthreads();
  if (tid == 0) {
    int live = 0;
    for (int j = 0; j < K; ++j) {
      const unsigned long long g = win[j];
      const uint32_t flat = ~(uint32_t)g;
      const int p = min((int)(flat / (uint32_t)V), K - 1), tok = (int)(flat % (uint32_t)V);
      const int r = b * K + j;
      const int pf = s_fin[p], nf = (pf || tok == eos) ? 1 : 0;
      parent[r] = p;
      score[r] = beam_fval((uint32_t)(g >> 32));
      fin[r] = nf;
      len[r] = pf ? s_len[p] : s + 1;
      live += nf ? 0 : 1;
      if (s >= 0 && s + 1 < max_len) {       // bounded (stale position)
        bp_par[s * R + r] = p;
        bp_tok[s * R + r] = tok;
      }
    }
    // the rows still live, then the arrival: the last workgroup publishes the sum, advances
    // the position (every workgroup has read it above) and re-arms both counters
    atomicAdd(step + 2, live);
    __threadfence();
    const unsigned tk = atomicAdd(reinterpret_cast<unsigned*>(step + 1), 1u);
    if (tk == gridDim.x - 1) {
      __threadfence();
      step[3] = atomicExch(step + 2, 0);
      step[0] = s + 1;
      step[1] = 0;
    }
  }
  // next decoder inputs: tgt_embed(token) at position s + 1 (embeddings.py:12-13), 128 threads
  // per slot
  const int j = tid >> 7, q = tid & 127;
  if (j < K) {
    const int tok = (int)((~(uint32_t)win[j]) % (uint32_t)V);
    const float sc = 0x1.6a09e6p+4f;
    const float4 e = ld_at(reinterpret_cast<const float4*>(lut), 16u * (unsigned)(tok * 128 + q));
    const float4 pr = ld_at(reinterpret_cast<const float4*>(pe),
                            16u * (unsigned)(max(min(s + 1, max_pos - 1), 0) * 128 + q));
    st_at(reinterpret_cast<float4*>(xnext), 16u * (unsigned)((b * K + j) * 128 + q),
          make_float4(e.x * sc + pr.x, e.y * sc + pr.y, e.z * sc + pr.z, e.w * sc + pr.w));
  }
}

hipError_t launch_beam_select(const float* logits, int B, int K, int V, int eos, int pad,
                              int max_len, int* step, float* score, int* fin, int* len,
                              int* parent, int* bp_par, int* bp_tok, const float* lut,
                              const float* pe, int max_pos, float* xnext, hipStream_t st) {
  if (B <= 0) return hipSuccess;
  if (K < 1 || K > BEAM_MAXK || K > V || eos < 0 || eos >= V || pad < 0 || pad >= V ||
      max_len < 1 || max_pos < 1 || (long)B * K * V >= (1L << 30) ||
      (long)B * K * max_len >= (1L << 30) ||
      V >= (1 << 21) || (long)B * K >= (1L << 21))   // 16 * (row * 128 + q) in 32 bits
    return hipErrorInvalidValue;
#define QTX_BEAM_SEL(KB)                                                                      \
  k_beam_select<KB><<<dim3(B), dim3(BEAM_T), 0, st>>>(V, K, eos, pad, max_len, max_pos,       \
                                                      logits, step, score, fin, len, parent, \
                                                      bp_par, bp_tok, lut, pe, xnext)
  if (K == 1) QTX_BEAM_SEL(1);
  else if (K == 2) QTX_BEAM_SEL(2);
  else if (K <= 4) QTX_BEAM_SEL(4);
  else QTX_BEAM_SEL(8);
#undef QTX_BEAM_SEL
  return hipGetLastError();
}

// k_beam_reorder: every layer's self K/V caches of slot j become those of its parent, in
// place, one launch for all layers.  A row's cache is four contiguous regions (qtx_beam.h
// BeamGeom); the same byte offset in all K regions of a sentence is owned by ONE thread, which
// loads its K chunks and then stores them by parent — no two threads touch the same byte, so
// there is no barrier and no second copy of the caches.  Only the valid prefix moves: positions
// 0 .. n-1 with n = step[0] (the select has advanced it to the count of cached positions).
// Workgroup (c, b, l) = blockIdx.x = (l * B + b) * nblk + c; chunk index c * 256 + tid runs
// over the K, V, K-scale and V-scale chunks of (l, b).  l_* : layer strides.
__global__ __launch_bounds__(256) void k_beam_reorder(int K, int max_len, int grouped, int B,
                                                      int nblk, long k_ls, long v_ls, long s_ls,
                                                      const int* step, const int* parent,
                                                      int8_t* kc, int8_t* vc, float* skc,
                                                      float* svc) {
  const int c = blockIdx.x % nblk, lb = blockIdx.x / nblk, b = lb % B, l = lb / B;
  const BeamGeom g{max_len, grouped};
  const int n = g.clamp(*step);
  const long i = (long)c * 256 + threadIdx.x;
  int p[BEAM_MAXK];
  bool ident = true;
#pragma unroll
  for (int j = 0; j < BEAM_MAXK; ++j) {
    p[j] = j < K ? min(max(parent[b * K + min(j, K - 1)], 0), K - 1) : j;
    ident &= p[j] == j;
  }
  if (ident) return;
  const BeamGeom::Chunk ck = g.locate(n, i);
  if (ck.region == BEAM_NONE) return;
  const size_t r0 = (size_t)b * K;
  if (ck.region == BEAM_K || ck.region == BEAM_V) {
    const bool isk = ck.region == BEAM_K;
    const size_t row = isk ? g.k_row() : g.v_row();
    uint8_t* base = reinterpret_cast<uint8_t*>(isk ? kc : vc) + (size_t)l * (isk ? k_ls : v_ls) +
                    r0 * row + (size_t)ck.off;
    uint4 ch[BEAM_MAXK];
#pragma unroll
    for (int j = 0; j < BEAM_MAXK; ++j)
      if (j < K) ch[j] = *reinterpret_cast<const uint4*>(base + j * row);
#pragma unroll
    for (int j = 0; j < BEAM_MAXK; ++j)
      if (j < K && p[j] != j) {
        uint4 v = ch[0];
#pragma unroll
        for (int q = 1; q < BEAM_MAXK; ++q)
          if (p[j] == q) v = ch[q];
        *reinterpret_cast<uint4*>(base + j * row) = v;
      }
    return;
  }
  float* base = (ck.region == BEAM_SK ? skc : svc) + (size_t)l * s_ls + r0 * g.s_row() + ck.off;
  float ch[BEAM_MAXK];
#pragma unroll
  for (int j = 0; j < BEAM_MAXK; ++j)
    if (j < K) ch[j] = base[j * g.s_row()];
#pragma unroll
  for (int j = 0; j < BEAM_MAXK; ++j)
    if (j < K && p[j] != j) {
      float v = ch[0];
#pragma unroll
      for (int q = 1; q < BEAM_MAXK; ++q)
        if (p[j] == q) v = ch[q];
      base[j * g.s_row()] = v;
    }
}

hipError_t launch_beam_reorder(int8_t* kc, int8_t* vc, float* skc, float* svc, int B, int K,
                               int max_len, int L, long k_ls, long v_ls, long s_ls, int grouped,
                               const int* step, const int* parent, hipStream_t st) {
  if (B <= 0 || L <= 0 || K == 1) return hipSuccess;   // one hypothesis: nothing to permute
  const BeamGeom g{max_len, grouped ? 1 : 0};
  if (K < 1 || K > BEAM_MAXK || max_len < 1 || max_len > 512 ||
      k_ls < (long)B * K * g.k_row() || v_ls < (long)B * K * g.v_row() ||
      s_ls < (long)B * K * g.s_row() || (k_ls | v_ls) % 16 != 0 ||
      (reinterpret_cast<uintptr_t>(kc) | reinterpret_cast<uintptr_t>(vc)) % 16 != 0)
    return hipErrorInvalidValue;
  const long nblk = (g.chunks(max_len) + 255) / 256;
  if (nblk * B * L >= (1L << 31)) return hipErrorInvalidValue;
  k_beam_reorder<<<dim3((unsigned)(nblk * B * L)), dim3(256), 0, st>>>(
      K, max_len, g.grouped, B, (int)nblk, k_ls, v_ls, s_ls, step, parent, kc, vc, skc, svc);
  return hipGetLastError();
}

// k_beam_rep: region r of out (n elements) = region r / K of in: the cross K/V, their scales
// and the source mask replicated from the B sentences to the B * K hypotheses, once per decode.
template <class T>
__global__ __launch_bounds__(256) void k_beam_rep(int K, long n, const T* in, T* out) {
  const long i = (long)blockIdx.y * 256 + threadIdx.x;
  const size_t r = blockIdx.x;
  if (i < n) out[r * n + i] = in[(r / K) * n + i];
}

hipError_t launch_beam_rep(const void* in, void* out, int B, int K, long bytes, hipStream_t st) {
  if (B <= 0 || bytes <= 0) return hipSuccess;
  if (K < 1 || bytes >= (1L << 30)) return hipErrorInvalidValue;
  const bool v16 = bytes % 16 == 0 && ((reinterpret_cast<uintptr_t>(in) | reinterpret_cast<uintptr_t>(out)) & 15) == 0;
  const long n = v16 ? bytes / 16 : bytes;
  const dim3 grid((unsigned)(B * K), (unsigned)((n + 255) / 256));
  if (v16)
    k_beam_rep<uint4><<<grid, dim3(256), 0, st>>>(K, n, static_cast<const uint4*>(in), static_cast<uint4*>(out));
  else
    k_beam_rep<uint8_t><<<grid, dim3(256), 0, st>>>(K, n, static_cast<const uint8_t*>(in), static_cast<uint8_t*>(out));
  return hipGetLastError();
}

// k_beam_init: the search state before step 0 — score 0 on slot 0 and -inf on the others, no
// row finished, length 0 — and the four step words zeroed.
__global__ __launch_bounds__(256) void k_beam_init(int R, int K, float* score, int* fin, int* len,
                                                   int* parent, int* step) {
  const int r = blockIdx.x * 256 + threadIdx.x;
  if (r < 4) step[r] = 0;
  if (r >= R) return;
  score[r] = r % K == 0 ? 0.0f : -__builtin_inff();
  fin[r] = 0; len[r] = 0; parent[r] = r % K;
}

hipError_t launch_beam_init(int B, int K, float* score, int* fin, int* len, int* parent,
                            int* step, hipStream_t st) {
  if (B <= 0 || K < 1) return hipErrorInvalidValue;
  const int R = B * K;
  k_beam_init<<<dim3((R + 255) / 256), dim3(256), 0, st>>>(R, K, score, fin, len, parent, step);
  return hipGetLastError();
}

// k_beam_backtrack: the histories from the back-pointers of the nsteps steps that ran: row r
// of out [R][max_len] = start, then the tokens along slot r's ancestry, then pad.
__global__ __launch_bounds__(64) void k_beam_backtrack(int R, int K, int max_len, int nsteps,
                                                       long long start, long long pad,
                                                       const int* bp_par, const int* bp_tok,
                                                       int64_t* out) {
  const int r = blockIdx.x * 64 + threadIdx.x;
  if (r >= R) return;
  int64_t* o = out + (size_t)r * max_len;
  o[0] = start;
  for (int t = nsteps + 1; t < max_len; ++t) o[t] = pad;
  int cur = r;
  for (int t = nsteps - 1; t >= 0; --t) {
    o[t + 1] = bp_tok[t * R + cur];
    cur = (cur / K) * K + min(max(bp_par[t * R + cur], 0), K - 1);
  }
}

hipError_t launch_beam_backtrack(const int* bp_par, const int* bp_tok, int B, int K, int max_len,
                                 int nsteps, long long start, long long pad, int64_t* out,
                                 hipStream_t st) {
  if (B <= 0) return hipSuccess;
  if (K < 1 || max_len < 1 || nsteps < 0 || nsteps > max_len - 1 ||
      (long)B * K * max_len >= (1L << 30))
    return hipErrorInvalidValue;
  const int R = B * K;
  k_beam_backtrack<<<dim3((R + 63) / 64), dim3(64), 0, st>>>(R, K, max_len, nsteps, start, pad,
                                                            bp_par, bp_tok, out);
  return hipGetLastError();
}

}  // namespace qtx

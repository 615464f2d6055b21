// qtx_decode_beam.hip — the beam search past 128 keys without moving a cache (gfx950, wave64).
//
//   k_dec_attn_beam   the fused step's self-attention for beam rows, 1 to 512 keys: every cached
//                     position of a hypothesis is read from the cache row of the slot that wrote
//                     it, through a per-row ancestry table
//   k_beam_ancestry   the table permuted by the step's parents: the step's tail in place of
//                     k_beam_reorder (qtx_decode.hip), bytes per position instead of cache rows
//   k_beam_anc_init   the table before step 0: every position the row's own slot
//
// Arguments, cache layouts, canonical order and results of k_dec_attn_long<true>
// (qtx_decode_long.hip): on the caches gathered through the table the two agree bit for bit.
#include "qtx_common.h"
#include "qtx_decode_ka.h"
#include "qtx_kernels.h"

namespace qtx {

// =====================================================================================
// k_dec_attn_beam: grid (R, 8), 256 threads, R = B * K rows, row r = b * K + k.  The split of
// k_dec_attn_long: wave w scores the 128-key block [128 w, 128 w + 128) on
// v_mfma_i32_16x16x64_i8 (key fragments loaded straight into the B layout), the maximum meets
// across waves in LDS, every wave forms the denominator in the lane-split order from E[512],
// wave c runs PV chain c and wave 0 sums (c0 + c1) + (c2 + c3).  What differs is where a cached
// row comes from: position j of row r lies in the cache row of slot anc[r][j] of the same
// sentence, cache row b * K + anc[r][j].
//   table   anc[r][0 .. kv_bs) is the same for the row's 8 heads and 4 waves.  Its bytes are
//           loaded with the step's q / k / v rows and the position (two byte loads per thread,
//           no address depends on the position), clamped to K - 1 and stored in LDS; the one
//           barrier behind them is what the table costs ahead of the key loads.  A stale or
//           uninitialised table therefore gives wrong numbers, never an address outside the
//           sentence's K cache rows (the position clamps are k_dec_attn_long's).
//   keys    the lane that loads key j reads slot A[j] from LDS and forms its own base: the same
//           16-byte non-temporal loads, 32-bit offsets inside the sentence's K rows (at most
//           8 * 512 * 512 bytes).  The scales skc / svc go through the same slot.
//   values  a value dword holds four positions of one dim, and their slots may differ.  The
//           four slots of a group are one aligned LDS dword (lane g of the wave reads group
//           4 g + w's, v_readlane hands it to the scalar unit).  In the group that holds the
//           position itself the bytes from the position on are dead — the new v byte is patched
//           in from registers and later keys have PS == 0 — so they take the slot of the byte
//           before them and do not make the group mixed.  A wave whose live groups all agree
//           (hypotheses keep long stretches of one slot) issues one dword load per group, as
//           k_dec_attn_long does.  Otherwise it walks its 64-key chunks: the four groups of a
//           chunk load the dword of each byte's slot (16 loads, the same address where slots
//           repeat) and the lane's dword is assembled byte by byte, byte q from slot
//           A[4 g + q] (v_bfi_b32 byte selects); chunk G + 1's loads are issued before chunk G
//           is assembled, so the loads of consecutive chunks overlap.  Both branches are
//           wave-uniform.
//   append  row `step` of the row's OWN slot (cache row r), in the K row and the grouped V
//           byte: the table says so already (k_beam_anc_init; k_beam_ancestry moves the entry
//           with its prefix after the select).
// Registers (-Rpass-analysis=kernel-resource-usage, the build's flags): 166 VGPRs, 14 AGPRs,
// no scratch and no spill (two waves per SIMD against k_dec_attn_long's four: the 32 dwords of
// the mixed path's two chunks in flight); LDS 5776 bytes.
// =====================================================================================
struct DaBeamTail { DaTail t; const uint8_t* anc; int K; };

__global__ __launch_bounds__(256) void k_dec_attn_beam(QTX_KA_PARAMS, DaBeamTail bt) {
  const DecAttnArgs a = da_args<true>(QTX_KA_VALS, bt.t);
  __shared__ __attribute__((aligned(16))) float E[DEC_LONG_MAXK];    // qexp(score - max), 0 past Sk
  __shared__ __attribute__((aligned(16))) float PS[DEC_LONG_MAXK];   // RN(P_j * s_v[j]), 0 past Sk
  __shared__ float part[4][64];                                  // the chains' partial sums
  __shared__ __attribute__((aligned(16))) int8_t qs[128];        // q and new k codes
  __shared__ __attribute__((aligned(16))) uint8_t A[DEC_LONG_MAXK];   // the row's slots, clamped
  __shared__ float wmax[4];
  const int b = blockIdx.x, h = blockIdx.y;
  const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63;
  const int fr = lane & 15, fg = lane >> 4;    // MFMA fragment: column (key) fr, byte chunk fg
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
  const float q_own = yr[h * 64 + lane];
  const float k_own = yr[512 + h * 64 + lane];
  const float v_own = yr[1024 + h * 64 + lane];
  const uint8_t* const ar = bt.anc + (long)b * kvn;
  const int t = threadIdx.x;
  const uint8_t a0 = ar[min(t, kvn - 1)], a1 = ar[min(t + 256, kvn - 1)];
  __builtin_amdgcn_sched_barrier(0);
  // clamped: a stale position (a counter not reset) must not index past the cache
  const int step = a.host_step1 > 0 ? a.host_step1 - 1 : min(max(*a.step, 0), kvn - 1);
  A[t] = (uint8_t)min((int)a0, K - 1);         // (entries past kv_bs - 1: the last one's copy)
  A[t + 256] = (uint8_t)min((int)a1, K - 1);
  __syncthreads();

  // phase 0b: this wave's key block, scales and value dwords through the table
  const int nrows = step + 1;                          // rows loaded: 1 .. min(kv_bs, 512)
  const int r0 = 128 * w;                              // this wave's key block
  const int nw = min(max(nrows - r0, 0), 128);         // its live rows (0: the wave scores nothing)
  const long kvb = (long)b0 * kvn;                     // the sentence's first position
  const int G4 = (kvn + 3) >> 2;                       // value groups per cache row
  const int glast = (nrows - 1) >> 2;                  // the last loaded 4-key value group
  const int8_t* const kbase = a.kc + kvb * 512 + h * 64;
  const int8_t* const vbase = a.vc + (long)b0 * G4 * 2048 + h * 256;
  uint4 kr[8];
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    kr[i] = make_uint4(0, 0, 0, 0);
    if (16 * i < nw) {                                 // wave-uniform
      const int j = min(r0 + 16 * i + fr, nrows - 1);
      const unsigned koff = (unsigned)(((int)A[j] * kvn + j) * 512 + 16 * fg);
      kr[i] = __builtin_bit_cast(uint4, __builtin_nontemporal_load(reinterpret_cast<const v4i*>(kbase + koff)));
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
  const float own3[3] = {q_own, k_own, v_own};
  int code[3];
  quant_one_n<3>(own3, am, code);
  const float sq = am[0], sk = am[1], sv = am[2];
  const int8_t kq = (int8_t)code[1], vq = (int8_t)code[2];
  if (w == 0) {
    const long row = (long)b * kvn + step;      // the append: the row's own slot
    a.kc[row * 512 + h * 64 + lane] = kq;
    a.vc[(((long)b * G4 + (step >> 2)) * 512 + h * 64 + lane) * 4 + (step & 3)] = vq;
    if (h == 0 && lane == 0) { a.skc[row] = sk; a.svc[row] = sv; }
    qs[lane] = (int8_t)code[0];
    qs[64 + lane] = kq;
  }
  if (r0 + lane == step) { sk0 = sk; sv0 = sv; }          // the new scales in the lane that
  if (r0 + lane + 64 == step) { sk1 = sk; sv1 = sv; }     // scores the key
  __syncthreads();

  // phase 2: operand fragments (A: the q codes' chunk fg in every row), the new key patched in
  const v4i qf = *reinterpret_cast<const v4i*>(qs + 16 * fg);
  {
    const uint4 kn = *reinterpret_cast<const uint4*>(qs + 64 + 16 * fg);
    const bool own = w == (step >> 7) && fr == (step & 15);
#pragma unroll
    for (int i = 0; i < 8; ++i)
      if (i == ((step >> 4) & 7) && own) kr[i] = kn;
  }
  const int Sk = nrows;

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
    for (int t4 = 1; t4 < 4; ++t4) dot = fg == t4 ? sacc[4 * u + t4][0] : dot;
    live[u] = r0 + lane + 64 * u < Sk;
    const float s = (((float)dot * sq) * (u ? sk1 : sk0)) * 0.125f;
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
  // key order, the new v byte in place of the cached one
  {
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
    if (64 * G < Sk) {                                 // wave-uniform (vg loaded)
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
      const float amx = wave_max(fabsf(ctx));
      if (lane == 0) a.pmax[(long)h * a.B + b] = amx;
    }
  }
}

// a: the self form (kv_new) with 1 .. 512 rows to load; anc [B][kv_bs]; B = sentences * K rows
hipError_t launch_dec_attn_beam(const DecAttnArgs& a, const uint8_t* anc, int K, int B, hipStream_t st) {
  if (B <= 0) return hipSuccess;
  if (!a.ctx || a.B != B || !anc || !a.kv_new || !a.kc || !a.vc || !a.skc || !a.svc || !a.y)
    return hipErrorInvalidValue;
  if (a.ldy < 0 || a.ldy >= (1L << 31)) return hipErrorInvalidValue;   // 32-bit in the lead block
  if (a.kv_bs <= 0 || a.kv_bs > DEC_LONG_MAXK || a.host_step1 < 0 || a.host_step1 > a.kv_bs ||
      (a.host_step1 == 0 && !a.step) || (long)B * 512 >= (1L << 29))
    return hipErrorInvalidValue;
  if (K < 1 || K > BEAM_MAXK || B % K != 0) return hipErrorInvalidValue;
  if (a.dk != 64) return launch_dec_attn_beam_hd(a, anc, K, B, st);   // head widths 32 / 128
  const KaLead l = da_lead<true>(a);
  const DaBeamTail t{{a.step, a.mask, a.ctx, a.pmax, a.B}, anc, K};
  k_dec_attn_beam<<<dim3(B, 8), dim3(256), 0, st>>>(QTX_KA_ARGS(l), t);
  return hipGetLastError();
}

// =====================================================================================
// k_beam_ancestry: anc'[b K + k][j] = anc[b K + parent[k]][j] for j < n, in place, n = step[0]
// (the select has advanced it to the count of cached positions).  k_beam_reorder's rule on
// bytes: thread (b, j) owns offset j of the sentence's K table rows (AncGeom::owner), loads its
// K bytes and then stores them by parent — no byte has two owners, so no barrier and any parent
// vector (shared parents, cycles) works; an identity vector returns at once.  Grid
// (ceil(max_len / 256), B).
// =====================================================================================
__global__ __launch_bounds__(256) void k_beam_ancestry(int K, int max_len, const int* step,
                                                       const int* parent, uint8_t* anc) {
  const int b = blockIdx.y;
  const AncGeom g{max_len};
  int p[BEAM_MAXK];
  bool ident = true;
#pragma unroll
  for (int j = 0; j < BEAM_MAXK; ++j) {
    p[j] = j < K ? min(max(parent[b * K + min(j, K - 1)], 0), K - 1) : j;
    ident &= p[j] == j;
  }
  if (ident) return;
  const long off = g.owner(*step, (long)blockIdx.x * 256 + threadIdx.x);
  if (off < 0) return;
  uint8_t* base = anc + (size_t)b * K * max_len + off;
  uint8_t ch[BEAM_MAXK];
#pragma unroll
  for (int j = 0; j < BEAM_MAXK; ++j)
    if (j < K) ch[j] = base[(size_t)j * max_len];
#pragma unroll
  for (int j = 0; j < BEAM_MAXK; ++j)
    if (j < K && p[j] != j) {
      uint8_t v = ch[0];
#pragma unroll
      for (int q = 1; q < BEAM_MAXK; ++q)
        if (p[j] == q) v = ch[q];
      base[(size_t)j * max_len] = v;
    }
}

hipError_t launch_beam_ancestry(uint8_t* anc, int B, int K, int max_len, const int* step,
                                const int* parent, hipStream_t st) {
  if (B <= 0 || K == 1) return hipSuccess;   // one hypothesis: nothing to permute
  if (!anc || !step || !parent || K < 1 || K > BEAM_MAXK || max_len < 1 ||
      max_len > DEC_LONG_MAXK || B > 65535)
    return hipErrorInvalidValue;
  k_beam_ancestry<<<dim3((unsigned)((max_len + 255) / 256), (unsigned)B), dim3(256), 0, st>>>(
      K, max_len, step, parent, anc);
  return hipGetLastError();
}

// k_beam_anc_init: anc[b K + k][j] = k for every j < max_len.  The entry at the position a step
// appends is then right before the permute, and the entries past the prefix are valid slots.
__global__ __launch_bounds__(256) void k_beam_anc_init(int K, int max_len, long n, uint8_t* anc) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i < n) anc[i] = (uint8_t)((i / max_len) % K);
}

hipError_t launch_beam_anc_init(uint8_t* anc, int B, int K, int max_len, hipStream_t st) {
  if (B <= 0) return hipSuccess;
  if (!anc || K < 1 || K > BEAM_MAXK || max_len < 1 || max_len > DEC_LONG_MAXK)
    return hipErrorInvalidValue;
  const long n = (long)B * K * max_len;
  if ((n + 255) / 256 >= (1L << 31)) return hipErrorInvalidValue;
  k_beam_anc_init<<<dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st>>>(K, max_len, n, anc);
  return hipGetLastError();
}

}  // namespace qtx

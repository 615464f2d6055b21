// qtx_decode_wide.hip — the fused decode step's tails for vocabularies of up to WIDE_MAXV =
// 65536 words (gfx950, wave64).
//
//   k_tok_wide   plain decode: log_softmax + first argmax + next-token embedding + step advance
//                from the generator's per-strip records (k_generator_mfma<true>)
//   k_top2_wide  scored decode: the two best (id, logp) of the row as well
//
// k_argmax_embed / k_top2_embed (qtx_decode.hip) keep a row of logits in one workgroup's
// registers and its exponentials in LDS, which ends at 8192 words.  A row of 65536 logits is
// 256 KB: it fits neither, but it is L2-resident (the generator has just written it), so these
// kernels stream it.  One 1024-thread workgroup per row, as the narrow kernels; outputs, the
// position / arrival-counter contract and every float step are theirs, bit for bit
// (oracle/qtx_oracle.py log_softmax_argmax).
#include "qtx_common.h"
#include "qtx_kernels.h"
#include "qtx_tail.h"

namespace qtx {

constexpr int WIDE_T = 1024, WIDE_NW = WIDE_T / 64;
constexpr int WIDE_CH = 4096;            // exponentials per ring slot
constexpr int WIDE_PROD = WIDE_T - 64;   // producer threads (waves 1 .. 15)
constexpr int WIDE_PK = (WIDE_CH + WIDE_PROD - 1) / WIDE_PROD;   // elements per producer, at most
constexpr int WIDE_NR = WIDE_MAXV / 16 / WIDE_T;                 // records per thread, at most
static_assert(WIDE_CH % 64 == 0, "a chunk border falls between two rounds of the 64 lanes");
static_assert(WIDE_NR * 16 * WIDE_T == WIDE_MAXV, "every record of a row in the workgroup's registers");

// =====================================================================================
// wide_row_sum: the canonical log-softmax denominator of one row, sum_v qexp(x_v - mx), in the
// order of row_sum_lanesplit: lane l of ONE wave adds e[l], e[l + 64], ... sequentially from
// 0.0, then wave_sum.  A lane's chain cannot be split between waves (fp32 addition is not
// associative), so the 1024 threads cannot each sum a part: what can be spread is everything
// but the chain's additions.
//   producers  waves 1 .. 15 fill ring slot c & 1 with the exponentials of chunk c (WIDE_CH
//              consecutive elements; 0.0 past V: x + 0 == x for the x >= 0 summed here): thread
//              p takes elements p, p + 960, ... of the chunk — at most WIDE_PK = 5 clamped loads,
//              all in flight before the first qexp; consecutive threads store consecutive dwords.
//   consumer   wave 0 extends its 64 register accumulators over chunk c - 1 in index order: lane
//              l reads ring[l + 64 k], k = 0 .. 63 (consecutive lanes, consecutive dwords: no
//              bank conflict).  The accumulators live across the chunk borders, so the chain is
//              bit for bit the one long chain; WIDE_CH % 64 == 0 keeps element v in lane v % 64.
// One barrier per chunk: in round c the producers write slot c & 1 while the consumer reads slot
// (c - 1) & 1, and the barrier that ends the round orders both against round c + 1.
// Expected cycles per chunk (from instruction counts; not measured): a producer wave spends
// about 20 VALU per element (the subtraction, qexp's 17, the select) on 4.27 elements, ~340
// issue cycles; four waves share a SIMD (three beside the consumer), so ~1400 (~1000) cycles
// per chunk and SIMD, plus one L2 latency that the other waves' arithmetic covers.  The consumer
// spends 64 dependent v_add_f32, ~8 cycles each with the wait for its operand, ~500 cycles, and
// its 64 ds_read_b32 are independent of the chain.  By these counts the producers set the pace: a
// row of 65536 is 16 chunks, ~23k cycles.  (Measured for the whole of k_top2_wide, three passes, at
// V = 32768 and 32 rows: 19.8 us per launch, profiles/wide_vocab_ab.md; the passes not separately.)
// Every thread of the workgroup calls it (uniform trip count); the sum is valid in wave 0.
// =====================================================================================
__device__ __forceinline__ float wide_row_sum(const float* logits, unsigned xo, int V, float mx,
                                              float (*ring)[WIDE_CH], int tid) {
  const int w = __builtin_amdgcn_readfirstlane(tid >> 6), lane = tid & 63;
  const int nch = (V + WIDE_CH - 1) / WIDE_CH;
  float acc = 0.0f;
  for (int c = 0; c <= nch; ++c) {
    if (w != 0) {
      if (c < nch) {
        const int v0 = c * WIDE_CH + (tid - 64);
        float x[WIDE_PK];
#pragma unroll
        for (int k = 0; k < WIDE_PK; ++k)
          x[k] = ld_at(logits, xo + 4u * (unsigned)min(v0 + WIDE_PROD * k, V - 1));   // clamped
        float* slot = ring[c & 1];
#pragma unroll
        for (int k = 0; k < WIDE_PK; ++k) {
          const int i = (tid - 64) + WIDE_PROD * k;
          if (i < WIDE_CH) slot[i] = v0 + WIDE_PROD * k < V ? qexp(x[k] - mx) : 0.0f;
        }
      }
    } else if (c >= 1) {
      const float* slot = ring[(c - 1) & 1];
#pragma unroll 16
      for (int k = 0; k < WIDE_CH / 64; ++k) acc = acc + slot[lane + 64 * k];
    }
    __syncthreads();
  }
  return wave_sum(acc);
}

// The end both tails share: the next decoder input tgt_embed(id) at position s + 1
// (embeddings.py:12-13), then the counter: every workgroup has read *step, the last one to
// arrive advances it.
__device__ __forceinline__ void wide_finish(int m, int tid, int id, int s, int host_s1, float4 pe_row,
                                            const float* lut, int* step, unsigned* arrive,
                                            float* xnext) {
  if (tid < 128) {
    const float sc = 0x1.6a09e6p+4f;
    const float4 e = ld_at(reinterpret_cast<const float4*>(lut), 16u * (unsigned)(id * 128 + tid));
    const float4 q = pe_row;
    st_at(reinterpret_cast<float4*>(xnext), 16u * (unsigned)(m * 128 + tid),
          make_float4(e.x * sc + q.x, e.y * sc + q.y, e.z * sc + q.z, e.w * sc + q.w));
  }
  if (host_s1 == 0 && tid == 0) {
    const unsigned tk = atomicAdd(arrive, 1u);
    if (tk == gridDim.x - 1) {
      *step = s + 1;
      *arrive = 0u;
    }
  }
}

// =====================================================================================
// k_tok_wide: the token of k_argmax_embed without a pass over the logits.  The generator has
// reduced every 16-column strip to a record {m1, m2, i1, flags}; the row's ceil(V / 16) <= 4096
// records are at most WIDE_NR = 4 float4 per thread, all loads in flight at once.  They merge
// per thread, over the wave by DPP and over the 16 waves through LDS (the merge is commutative
// and associative: any order gives the row's record), and the decision is k_skinny_wide_tok's:
// a non-finite row gives 0; one value above max - ARG_DELTA is the token; otherwise the exact
// log-softmax decides — wide_row_sum, logf, then the first argmax of (x - max) - lse over the
// streamed logits (thread t: elements t, t + 1024, ... in ascending order, eight loads in flight).
// host_s1 / step / arrive / ids / xnext: as k_argmax_embed.  1 <= V <= WIDE_MAXV, M * V < 2^30.
// (parameters in order of first use: those up to ids_bs arrive preloaded in SGPRs)
// =====================================================================================
__global__ __launch_bounds__(1024) void k_tok_wide(const float* rec, int V, int host_s1, int* step,
                                                   const float* pe, const float* lut, int max_pos,
                                                   long ids_bs, int64_t* ids, const float* logits,
                                                   unsigned* arrive, float* xnext) {
  __shared__ __attribute__((aligned(16))) float ring[2][WIDE_CH];
  __shared__ float r_m1[64], r_m2[64], redf[WIDE_NW], lse_s;
  __shared__ int r_i1[64], r_fl[64], redi[WIDE_NW];
  const int m = blockIdx.x, tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int nstrip = (V + 15) >> 4;
  float4 rc[WIDE_NR];
#pragma unroll
  for (int i = 0; i < WIDE_NR; ++i)   // clamped, masked below
    rc[i] = ld_at(reinterpret_cast<const float4*>(rec), 16u * (unsigned)(m * nstrip + min(tid + WIDE_T * i, nstrip - 1)));
  __builtin_amdgcn_sched_barrier(0);
  const int s = host_s1 > 0 ? host_s1 - 1 : *step;
  float4 pe_row = make_float4(0.0f, 0.0f, 0.0f, 0.0f);   // position s+1 is known up front
  if (tid < 128) pe_row = ld_at(reinterpret_cast<const float4*>(pe), 16u * (unsigned)(min(s + 1, max_pos - 1) * 128 + tid));
  TokRec t{-3.0e38f, -3.0e38f, 0x7fffffff, 0};
#pragma unroll
  for (int i = 0; i < WIDE_NR; ++i) {
    const bool in = tid + WIDE_T * i < nstrip;
    tok_merge(t, in ? rc[i].x : -3.0e38f, in ? rc[i].y : -3.0e38f,
              in ? __float_as_int(rc[i].z) : 0x7fffffff, in ? __float_as_int(rc[i].w) : 0);
  }
  tok_merge_dpp<0xB1>(t);
  tok_merge_dpp<0x4E>(t);
  tok_merge_dpp<0x141>(t);
  tok_merge_dpp<0x140>(t);
  if ((lane & 15) == 0) {   // the records of the wave's four DPP rows: 64 per workgroup
    const int j = 4 * w + (lane >> 4);
    r_m1[j] = t.m1; r_m2[j] = t.m2; r_i1[j] = t.i1; r_fl[j] = t.fl;
  }
  __syncthreads();
  // every wave merges the 64 itself (one per lane): no second barrier on the common path
  t = TokRec{r_m1[lane], r_m2[lane], r_i1[lane], r_fl[lane]};
  tok_merge_dpp<0xB1>(t);
  tok_merge_dpp<0x4E>(t);
  tok_merge_dpp<0x141>(t);
  tok_merge_dpp<0x140>(t);
  TokRec g{lane_f(t.m1, 0), lane_f(t.m2, 0), __builtin_amdgcn_readlane(t.i1, 0),
           __builtin_amdgcn_readlane(t.fl, 0)};
#pragma unroll
  for (int q = 16; q < 64; q += 16)
    tok_merge(g, lane_f(t.m1, q), lane_f(t.m2, q), __builtin_amdgcn_readlane(t.i1, q),
              __builtin_amdgcn_readlane(t.fl, q));
  int id;
  if ((g.fl & 1) || !(g.fl & 2)) {
    id = 0;                                // torch.max of an all-NaN log_softmax row
  } else if (!(g.m2 > g.m1 - ARG_DELTA) && g.i1 != 0x7fffffff) {
    id = g.i1;                             // exactly one value above max - ARG_DELTA
  } else {                                 // near-tie: the exact log-softmax decides (block-uniform)
    const unsigned xo = 4u * (unsigned)(m * V);
    const float mx = g.m1;
    const float den = wide_row_sum(logits, xo, V, mx, ring, tid);
    if (tid == 0) lse_s = logf(den);
    __syncthreads();
    const float lse = lse_s;
    // first argmax of logp = (x - max) - lse (torch.max tie rule): this thread's, ascending
    float best = -3.0e38f;
    int bj = 0x7fffffff;
    for (int i0 = 0; i0 < V; i0 += 8 * WIDE_T) {
      float x[8];
#pragma unroll
      for (int j = 0; j < 8; ++j) x[j] = ld_at(logits, xo + 4u * (unsigned)min(i0 + WIDE_T * j + tid, V - 1));
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const int v = i0 + WIDE_T * j + tid;
        const float lp = (x[j] - mx) - lse;
        if (v < V && lp > best) { best = lp; bj = v; }
      }
    }
    // the maximum, then the smallest index holding it: per wave, then over the 16 waves
    const float wb = wave_max(best);
    const int wi = wave_min_i32(best == wb ? bj : 0x7fffffff);
    if (lane == 0) { redf[w] = wb; redi[w] = wi; }
    __syncthreads();
    const float gv = lane < WIDE_NW ? redf[lane] : -3.0e38f;
    const float gb = wave_max(gv);
    id = wave_min_i32(lane < WIDE_NW && gv == gb ? redi[lane] : 0x7fffffff);
  }
  id = max(min(id, V - 1), 0);             // keeps the embedding gather in bounds, whatever
  if (tid == 0 && s >= 0 && s + 1 < ids_bs) ids[m * ids_bs + s + 1] = id;   // bounded (stale position)
  wide_finish(m, tid, id, s, host_s1, pe_row, lut, step, arrive, xnext);
}

hipError_t launch_tok_wide(const float* rec, const float* logits, int M, int V, int64_t* ids,
                           long ids_bs, int* step, unsigned* arrive, const float* lut,
                           const float* pe, int max_pos, float* xnext, hipStream_t st, int host_s1) {
  if (M <= 0) return hipSuccess;
  if (V < 1 || V > WIDE_MAXV || host_s1 < 0 || (long)M * V >= (1L << 30)) return hipErrorInvalidValue;
  k_tok_wide<<<dim3(M), dim3(WIDE_T), 0, st>>>(rec, V, host_s1, step, pe, lut, max_pos, ids_bs, ids,
                                               logits, arrive, xnext);
  return hipGetLastError();
}

// =====================================================================================
// k_top2_wide: k_top2_embed for a streamed row — three passes over the logits (thread t:
// elements t, t + 1024, ..., eight loads in flight), the second and third from L2:
//   1  the maximum and the non-finite flags (order-free: per wave, then the 16 waves)
//   2  the denominator, wide_row_sum; its log by qlog (the values go out to the caller)
//   3  the two best of logp = (x - max) - lse under "larger logp, then smaller index": per
//      thread in ascending index order (Top2::add), wave_top2, then the 16 waves' pairs
// A non-finite row: ids (0, 1), both values NaN.  Outputs and the position contract as
// k_top2_embed.  2 <= V <= WIDE_MAXV, M * V < 2^30.
// (parameters in order of first use: those up to ids_bs arrive preloaded in SGPRs)
// =====================================================================================
__global__ __launch_bounds__(1024) void k_top2_wide(const float* logits, int V, int host_s1,
                                                    int* step, const float* pe, const float* lut,
                                                    int max_pos, long ids_bs, int64_t* ids,
                                                    int64_t* top_ids, float* top_logp,
                                                    unsigned* arrive, float* xnext) {
  __shared__ __attribute__((aligned(16))) float ring[2][WIDE_CH];
  __shared__ float redf[WIDE_NW], lse_s, rv1[WIDE_NW], rv2[WIDE_NW];
  __shared__ int redb[WIDE_NW], ri1[WIDE_NW], ri2[WIDE_NW];
  const int m = blockIdx.x, tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const unsigned xo = 4u * (unsigned)(m * V);
  float lm = -3.0e38f;
  bool nonfin = false, fin = false;
  float4 pe_row = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
  int s = 0;
  for (int i0 = 0; i0 < V; i0 += 8 * WIDE_T) {
    float x[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) x[j] = ld_at(logits, xo + 4u * (unsigned)min(i0 + WIDE_T * j + tid, V - 1));
    if (i0 == 0) {   // (behind the first loads, as k_top2_embed: the position may be a load of the counter)
      __builtin_amdgcn_sched_barrier(0);
      s = host_s1 > 0 ? host_s1 - 1 : *step;
      if (tid < 128) pe_row = ld_at(reinterpret_cast<const float4*>(pe), 16u * (unsigned)(min(s + 1, max_pos - 1) * 128 + tid));
    }
#pragma unroll
    for (int j = 0; j < 8; ++j)
      if (i0 + WIDE_T * j + tid < V) {
        lm = fmaxf(lm, x[j]);
        nonfin |= !(x[j] < __builtin_inff());
        fin |= x[j] > -__builtin_inff();
      }
  }
  lm = wave_max(lm);
  const int flags = (__ballot(nonfin) ? 1 : 0) | (__ballot(fin) ? 2 : 0);
  if (lane == 0) { redf[w] = lm; redb[w] = flags; }
  __syncthreads();
  const float mx = wave_max(lane < WIDE_NW ? redf[lane] : -3.0e38f);
  const bool bad = __ballot(lane < WIDE_NW && (redb[lane] & 1)) != 0ull ||
                   __ballot(lane < WIDE_NW && (redb[lane] & 2)) == 0ull;
  Top2 top;
  if (bad) {                               // an all-NaN log_softmax row (block-uniform)
    top.i1 = 0; top.i2 = 1;
    top.v1 = top.v2 = __builtin_nanf("");
  } else {
    const float den = wide_row_sum(logits, xo, V, mx, ring, tid);
    if (tid == 0) lse_s = qlog(den);
    __syncthreads();
    const float lse = lse_s;
    for (int i0 = 0; i0 < V; i0 += 8 * WIDE_T) {
      float x[8];
#pragma unroll
      for (int j = 0; j < 8; ++j) x[j] = ld_at(logits, xo + 4u * (unsigned)min(i0 + WIDE_T * j + tid, V - 1));
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const int v = i0 + WIDE_T * j + tid;
        if (v < V) top.add((x[j] - mx) - lse, v);
      }
    }
    wave_top2(top);
    if (lane == 0) { rv1[w] = top.v1; ri1[w] = top.i1; rv2[w] = top.v2; ri2[w] = top.i2; }
    __syncthreads();
    // the 16 waves' pairs: every wave merges them itself
    top = Top2{};
    if (lane < WIDE_NW) { top.v1 = rv1[lane]; top.i1 = ri1[lane]; top.v2 = rv2[lane]; top.i2 = ri2[lane]; }
    wave_top2(top);
  }
  const int id = min(max(top.i1, 0), V - 1);   // keeps the embedding gather in bounds, whatever
  if (tid == 0 && s >= 0 && s + 1 < ids_bs) {  // bounded (stale position)
    ids[m * ids_bs + s + 1] = id;
    const long e = 2 * (m * (ids_bs - 1) + s);
    top_ids[e] = id; top_ids[e + 1] = top.i2;
    top_logp[e] = top.v1; top_logp[e + 1] = top.v2;
  }
  wide_finish(m, tid, id, s, host_s1, pe_row, lut, step, arrive, xnext);
}

hipError_t launch_top2_wide(const float* logits, int M, int V, int64_t* ids, long ids_bs,
                            int64_t* top_ids, float* top_logp, int* step, unsigned* arrive,
                            const float* lut, const float* pe, int max_pos, float* xnext,
                            hipStream_t st, int host_s1) {
  if (M <= 0) return hipSuccess;
  if (V < 2 || V > WIDE_MAXV || host_s1 < 0 || (long)M * V >= (1L << 30)) return hipErrorInvalidValue;
  k_top2_wide<<<dim3(M), dim3(WIDE_T), 0, st>>>(logits, V, host_s1, step, pe, lut, max_pos, ids_bs,
                                                ids, top_ids, top_logp, arrive, xnext);
  return hipGetLastError();
}

}  // namespace qtx

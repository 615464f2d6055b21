// qtx_carve.h — the workspace carving that has no GPU in it: the bump allocator, the stack
// scratch, the cross K/V, and the workspaces of the greedy, decoder-fault, kvfault and beam
// decodes and of the target scoring, each with its size function.  Plain C++ over qtx_config
// and sizes: the drivers (qtx_api.hip, qtx_fault.hip, qtx_search.hip) carve the callers'
// workspaces with it, and tools/beam_host_check.cpp and tools/carve_host_check.cpp run it
// under the host sanitizers.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <algorithm>
#include <vector>

#include "../../include/qtx.h"
#include "qtx_beam.h"

namespace qtx {

inline size_t align_up(size_t x, size_t a = 256) { return (x + a - 1) / a * a; }

// bump allocator over a caller-provided (or model-owned) device region
struct Arena {
  uint8_t* base = nullptr;
  size_t cap = 0, used = 0;
  template <class T>
  T* take(size_t n) {
    const size_t off = align_up(used);
    used = off + n * sizeof(T);
    return base ? reinterpret_cast<T*>(base + off) : nullptr;
  }
};

// scratch for one stack pass over M rows (fp32 residual stream + quant buffers)
struct Scratch {
  float* x;      // [M, D] residual stream
  int8_t* a8;    // [M, max(D, F)] activation ints (max K)
  float* sa;     // [M]
  float* y;      // [M, max(3D, F)] GEMM output
  int8_t* q8;    // [M, D]   q8, k8, v8 contiguous ([3][M][D]) with sq, sk, sv ([3][M]):
  float* sq;     // [M]      the row GEMM writes the three quantized projections in one
  int8_t* k8;    // [M, D]   launch (tile stride M*D / M)
  float* sk;
  int8_t* v8;    // [M, D]
  float* sv;
  float* ctx;    // [M, D]
  int8_t* h8;    // [M, F]  quantized FFN hidden
  float* sh;     // [M]
  float* pmax;   // [F/512, M] FFN1 per-tile row maxima
  unsigned* status = nullptr;   // the call's status word (call_status_begin)
};

inline Scratch carve_scratch(Arena& ar, const qtx_config& c, long M) {
  const int D = c.d_model, F = c.d_ff;
  const int Y = 3 * D > F ? 3 * D : F;
  Scratch s;
  s.x = ar.take<float>(M * D);
  // the inputs of every linear, K = D or F wide (d_ff 256: D is the wider);
  // + 1 row: KP row pairs of an odd M
  s.a8 = ar.take<int8_t>((M + 1) * (D > F ? D : F));
  s.sa = ar.take<float>(M);
  s.y = ar.take<float>(M * Y);
  s.q8 = ar.take<int8_t>(3 * M * D); s.k8 = s.q8 + M * D; s.v8 = s.k8 + M * D;
  s.sq = ar.take<float>(3 * M); s.sk = s.sq + M; s.sv = s.sk + M;
  s.ctx = ar.take<float>(M * D);
  s.h8 = ar.take<int8_t>((M + 1) * F);
  s.sh = ar.take<float>(M);
  s.pmax = ar.take<float>((F / 512 + 1) * M);
  return s;
}

// decoder-specific scratch: quantized memory + cross K/V for all layers
struct CrossKV {
  int8_t* am8;  // [B*S, D] quantized memory (per token, layer independent)
  float* sam;
  std::vector<int8_t*> k8, v8;
  std::vector<float*> sk, sv;
  float* y;     // [B*S, 2D]
};

// rows_only: the per-layer K/V rows alone (am8 / sam / y null) — cross K/V that are copied
// from another CrossKV, never projected into (beam hypotheses, scoring's replicated rows)
inline CrossKV carve_cross(Arena& ar, const qtx_config& c, long Ms, bool rows_only = false) {
  const int D = c.d_model;
  CrossKV x;
  x.am8 = rows_only ? nullptr : ar.take<int8_t>(Ms * D);
  x.sam = rows_only ? nullptr : ar.take<float>(Ms);
  x.y = rows_only ? nullptr : ar.take<float>(Ms * 2 * D);
  // k8 / v8 of every layer contiguous (tile t = 2 l + {0: K, 1: V} at t * Ms * D), and
  // sk / sv likewise (t * Ms): the layout of one row GEMM's per-512-column-tile outputs
  int8_t* kv = ar.take<int8_t>(2L * c.n_layers * Ms * D);
  float* sc = ar.take<float>(2L * c.n_layers * Ms);
  for (int l = 0; l < c.n_layers; ++l) {
    x.k8.push_back(kv ? kv + 2L * l * Ms * D : nullptr);
    x.v8.push_back(kv ? kv + (2L * l + 1) * Ms * D : nullptr);
    x.sk.push_back(sc ? sc + 2L * l * Ms : nullptr);
    x.sv.push_back(sc ? sc + (2L * l + 1) * Ms : nullptr);
  }
  return x;
}

// The beam step's tail (k_beam_select + k_beam_reorder) in place of the argmax / top-2 tail:
// the search state, and every layer's self K/V caches as one allocation each (layer strides)
struct BeamTail {
  BeamState st;
  int K = 1, eos = 0, pad = 0;
  int8_t *kc0 = nullptr, *vc0 = nullptr;
  float *skc0 = nullptr, *svc0 = nullptr;
  long k_ls = 0, v_ls = 0, s_ls = 0;
  bool grouped = true;   // V in the fused step's 4-key groups (else [max_len][512])
};

// The fused decode runs the batch as up to QTX_MAX_GROUPS independent sub-batches, each a
// graph on its own stream (qtx_greedy_decode).
constexpr int QTX_MAX_GROUPS = 4;

// G sub-batch groups of Bg rows (the last one may be shorter); qtx_api.hip decode_groups
// chooses G, split_groups clamps it so that no group is empty.
struct Groups {
  int G, Bg;
  int b0(int i) const { return i * Bg; }
  int rows(int i, int B) const { return std::min(B, (i + 1) * Bg) - i * Bg; }
};
inline Groups split_groups(int B, int G) {
  G = std::max(1, std::min(std::min(G, QTX_MAX_GROUPS), B));
  const int Bg = (B + G - 1) / G;
  return Groups{(B + Bg - 1) / Bg, Bg};   // no empty group
}

// greedy decode workspace: encoder scratch, decoder step scratch (M=B), cross K/V,
// self K/V caches [L][B][max_len][D], memory, logits, step counter
struct GreedyWS {
  Scratch enc, dec;
  CrossKV cross;
  std::vector<int8_t*> cvg;   // the cross values in k_dec_attn's 4-key groups, per layer
  std::vector<int8_t*> kc, vc;   // self K [B][max_len][D]; V in 4-key groups (fused step) or
                                 // [B][max_len][D] (unfused step)
  std::vector<float*> skc, svc;
  float* memory;
  float* xo;
  float* logits;
  float* rec;         // [B][ceil(V/16)][4] the generator's per-strip top-2 records (folded tail)
  int* step;          // [0] = decode position, [1] = argmax arrival counter
  float* pmax_a;      // [8][B]    per-head absmax of the attention context (A_F32Q input)
  float* pmax_f;      // [F/16][B] per-column-tile absmax of FFN1's output
  // fused-decode sub-batches: step scratch (grp[0] = dec) and step counters, 4 ints each
  std::vector<Scratch> grp;
  int* gsteps;
  int64_t* ids;       // [B][max_len] the decode writes here; copied out to the caller's ids
  uint8_t* mask;      // [B][S] staged copy of the caller's src_mask
  // scored decode only (else null): [B][max_len-1][2] the two best ids / log-probs of every
  // step; copied out to the caller's top_ids / top_logp
  int64_t* top_ids = nullptr;
  float* top_logp = nullptr;
  // the decoder-fault decode (qtx_greedy_decode_dfault): its tail is never folded into the
  // next step's first launch (a step may follow the faulty pass, not a generator launch)
  bool no_fold = false;
  // beam search (qtx_beam_decode): the step's rows are B * beam hypotheses and its tail is the
  // selection + cache reorder; the tail is never folded; the next input comes from the select
  const BeamTail* beam = nullptr;
};

// scored: the scores follow everything else, so the plain layout (and size) is a prefix
inline GreedyWS carve_greedy(Arena& ar, const qtx_config& c, const Groups& gr, int B, int S,
                             int max_len, bool scored = false) {
  GreedyWS g;
  const int D = c.d_model;
  g.enc = carve_scratch(ar, c, (long)B * S);
  g.dec = carve_scratch(ar, c, B);
  g.cross = carve_cross(ar, c, (long)B * S);
  // the cross values regrouped once per decode (layer stride: B * ceil(S/4) * 4 * D bytes)
  int8_t* cvg = ar.take<int8_t>((size_t)c.n_layers * B * ((S + 3) & ~3) * D);
  for (int l = 0; l < c.n_layers; ++l) {
    g.cvg.push_back(cvg ? cvg + (size_t)l * B * ((S + 3) & ~3) * D : nullptr);
    g.kc.push_back(ar.take<int8_t>((size_t)B * max_len * D));
    g.skc.push_back(ar.take<float>((size_t)B * max_len));
    g.vc.push_back(ar.take<int8_t>((size_t)B * ((max_len + 3) & ~3) * D));
    g.svc.push_back(ar.take<float>((size_t)B * max_len));
  }
  g.memory = ar.take<float>((size_t)B * S * D);
  g.xo = ar.take<float>((size_t)B * D);
  g.logits = ar.take<float>((size_t)B * c.tgt_vocab);
  g.step = ar.take<int>(4);
  g.pmax_a = ar.take<float>((size_t)8 * B);
  g.pmax_f = ar.take<float>((size_t)(c.d_ff / 16) * B);
  g.grp.push_back(g.dec);
  for (int i = 1; i < gr.G; ++i) g.grp.push_back(carve_scratch(ar, c, gr.Bg));
  g.gsteps = ar.take<int>(4 * QTX_MAX_GROUPS);
  g.ids = ar.take<int64_t>((size_t)B * max_len);
  g.mask = ar.take<uint8_t>((size_t)B * S);
  g.rec = ar.take<float>((size_t)B * ((c.tgt_vocab + 15) / 16) * 4);
  if (scored) {
    g.top_ids = ar.take<int64_t>((size_t)B * (max_len - 1) * 2);
    g.top_logp = ar.take<float>((size_t)B * (max_len - 1) * 2);
  }
  return g;
}

// The workspace of sub-batch i (rows b0 ..): every per-sentence buffer offset by b0.
inline GreedyWS group_view(const GreedyWS& g, const qtx_config& c, int i, int b0, int S,
                           int max_len) {
  const long D = c.d_model;
  GreedyWS v = g;
  v.dec = g.grp[i];
  for (int l = 0; l < c.n_layers; ++l) {
    v.kc[l] += b0 * max_len * D; v.vc[l] += b0 * ((max_len + 3) & ~3) * D;
    v.skc[l] += b0 * max_len; v.svc[l] += b0 * max_len;
    v.cross.k8[l] += b0 * S * D; v.cross.v8[l] += b0 * S * D;
    v.cvg[l] += b0 * ((S + 3) & ~3) * D;
    v.cross.sk[l] += b0 * S; v.cross.sv[l] += b0 * S;
  }
  v.logits += (long)b0 * c.tgt_vocab;
  v.rec += (long)b0 * ((c.tgt_vocab + 15) / 16) * 4;
  v.pmax_a += (long)8 * b0;               // each sub-batch: its own [P][rows] block
  v.pmax_f += (long)(c.d_ff / 16) * b0;
  v.step = g.gsteps + 4 * i;
  if (g.top_ids) {
    v.top_ids += (long)b0 * (max_len - 1) * 2;
    v.top_logp += (long)b0 * (max_len - 1) * 2;
  }
  return v;
}
inline size_t greedy_ws(const qtx_config& c, const Groups& gr, int B, int S, int max_len,
                        bool scored = false) {
  Arena ar;
  carve_greedy(ar, c, gr, B, S, max_len, scored);
  return align_up(ar.used);
}

// The beam decode's workspace: encoder scratch and cross K/V for the B sentences; everything
// per row for the R = B * beam hypotheses (the step's GreedyWS, whose rows they are), the self
// K/V caches of all layers as one allocation each (k_beam_reorder's layer strides), the search
// state.
struct BeamWS {
  GreedyWS g;
  BeamTail tail;
  CrossKV cross_b;      // the B sentences' cross K/V (replicated into g.cross)
  int8_t* cvg_b;        // their regrouped cross values, all layers (fused step)
  uint8_t* mask_b;      // [B][S] staged copy of the caller's src_mask (g.mask: [R][S])
};

inline BeamWS carve_beam(Arena& ar, const qtx_config& c, int B, int K, int S, int max_len) {
  BeamWS w;
  GreedyWS& g = w.g;
  const size_t D = c.d_model, L = c.n_layers, R = (size_t)B * K;
  const size_t S4 = (S + 3) & ~3, ML4 = (max_len + 3) & ~3;
  g.enc = carve_scratch(ar, c, (long)B * S);
  g.dec = carve_scratch(ar, c, (long)R);
  w.cross_b = carve_cross(ar, c, (long)B * S);
  w.cvg_b = ar.take<int8_t>(L * B * S4 * D);
  g.cross = carve_cross(ar, c, (long)(R * S), true);   // the hypotheses' cross K/V
  int8_t* cvg = ar.take<int8_t>(L * R * S4 * D);
  w.tail.k_ls = (long)(R * max_len * D);
  w.tail.v_ls = (long)(R * ML4 * D);
  w.tail.s_ls = (long)(R * max_len);
  w.tail.kc0 = ar.take<int8_t>(L * w.tail.k_ls);
  w.tail.vc0 = ar.take<int8_t>(L * w.tail.v_ls);
  w.tail.skc0 = ar.take<float>(L * w.tail.s_ls);
  w.tail.svc0 = ar.take<float>(L * w.tail.s_ls);
  for (size_t l = 0; l < L; ++l) {
    g.cvg.push_back(cvg ? cvg + l * R * S4 * D : nullptr);
    g.kc.push_back(w.tail.kc0 ? w.tail.kc0 + l * w.tail.k_ls : nullptr);
    g.vc.push_back(w.tail.vc0 ? w.tail.vc0 + l * w.tail.v_ls : nullptr);
    g.skc.push_back(w.tail.skc0 ? w.tail.skc0 + l * w.tail.s_ls : nullptr);
    g.svc.push_back(w.tail.svc0 ? w.tail.svc0 + l * w.tail.s_ls : nullptr);
  }
  g.memory = ar.take<float>((size_t)B * S * D);
  g.xo = ar.take<float>(R * D);
  g.logits = ar.take<float>(R * c.tgt_vocab);
  g.step = ar.take<int>(4);
  g.pmax_a = ar.take<float>(8 * R);
  g.pmax_f = ar.take<float>((size_t)(c.d_ff / 16) * R);
  g.grp.push_back(g.dec);
  g.gsteps = nullptr; g.ids = nullptr; g.rec = nullptr;
  g.mask = ar.take<uint8_t>(R * S);
  w.mask_b = ar.take<uint8_t>((size_t)B * S);
  w.tail.st = carve_beam_state(ar, B, K, max_len);
  w.tail.K = K;
  return w;
}

inline size_t beam_ws(const qtx_config& c, int B, int K, int S, int max_len) {
  Arena ar;
  carve_beam(ar, c, B, K, S, max_len);
  return align_up(ar.used);
}

// The decoder-fault decode's workspace (qtx_greedy_decode_dfault): the scored decode's (a
// prefix, so the captured steps see the same buffers in the plain and the scored form), then the faulty pass's scratch, the record, and the
// golden copies a resume returns.
struct DfaultWS {
  GreedyWS g;
  Scratch fs;           // the faulty full-prefix pass, B * (max_len - 1) rows
  CrossKV fx;           // its cross K/V when the fault sits in a memory K/V projection
  float* fout;          // [B * (max_len - 1), D] its output
  float* flogits;       // [B, V] the generator on each sentence's last row
  uint8_t* tmask;       // [T, T] causal mask
  int64_t* rec_ids;     // [B, 2, 2]
  float* rec_logp;
  int* changed;         // [B]
  int64_t* gold_ids;    // [B, max_len]          the golden decode, as far as it is known
  int64_t* gold_top_ids;   // [B, max_len-1, 2]  (qtx_model::DfaultHdr)
  float* gold_top_logp;
  int64_t* stamp;       // [2] the header's nonce (resume compares it with the host table's)
};

inline DfaultWS carve_dfault(Arena& ar, const qtx_config& c, const Groups& gr, int B, int S,
                             int max_len) {
  DfaultWS w;
  const size_t D = c.d_model, Tm = max_len > 1 ? max_len - 1 : 1;
  w.g = carve_greedy(ar, c, gr, B, S, max_len, true);
  w.g.no_fold = true;
  w.fs = carve_scratch(ar, c, (long)(B * Tm));
  w.fx = carve_cross(ar, c, (long)B * S);
  w.fout = ar.take<float>(B * Tm * D);
  w.flogits = ar.take<float>((size_t)B * c.tgt_vocab);
  w.tmask = ar.take<uint8_t>(Tm * Tm);
  w.rec_ids = ar.take<int64_t>((size_t)B * 4);
  w.rec_logp = ar.take<float>((size_t)B * 4);
  w.changed = ar.take<int>((size_t)B);
  w.gold_ids = ar.take<int64_t>((size_t)B * max_len);
  w.gold_top_ids = ar.take<int64_t>(B * Tm * 2);
  w.gold_top_logp = ar.take<float>(B * Tm * 2);
  w.stamp = ar.take<int64_t>(2);
  return w;
}

inline size_t dfault_ws(const qtx_config& c, const Groups& gr, int B, int S, int max_len) {
  Arena ar;
  carve_dfault(ar, c, gr, B, S, max_len);
  return align_up(ar.used);
}

// The workspace of the KV-cached decode's own faults (qtx_greedy_decode_kvfault): the scored
// decode's (a prefix, as DfaultWS) and the record.
struct KvfaultWS {
  GreedyWS g;
  int64_t* rec_ids;     // [B, 2, 2]
  float* rec_logp;
};

inline KvfaultWS carve_kvfault(Arena& ar, const qtx_config& c, const Groups& gr, int B, int S,
                               int max_len) {
  KvfaultWS w;
  w.g = carve_greedy(ar, c, gr, B, S, max_len, true);
  w.g.no_fold = true;
  w.rec_ids = ar.take<int64_t>((size_t)B * 4);
  w.rec_logp = ar.take<float>((size_t)B * 4);
  return w;
}

inline size_t kvfault_ws(const qtx_config& c, const Groups& gr, int B, int S, int max_len) {
  Arena ar;
  carve_kvfault(ar, c, gr, B, S, max_len);
  return align_up(ar.used);
}

// The trials decode's workspace (qtx_greedy_decode_kvtrials): the kvfault decode's (a prefix),
// then the per-row fault table, the rows' trial steps, and the eager step's top 2.
struct KvtrialsWS {
  KvfaultWS k;
  int* tab;             // [B][10] words: one RowFault (qtx_kernels.h) per row
  int* tstep;           // [B] the row's trial step, -1: none
  int64_t* pair_ids;    // [B, 2, 2]: [:, 1, :] the top 2 of the eager faulty step
  float* pair_logp;
};

inline KvtrialsWS carve_kvtrials(Arena& ar, const qtx_config& c, const Groups& gr, int B, int S,
                                 int max_len) {
  KvtrialsWS w;
  w.k = carve_kvfault(ar, c, gr, B, S, max_len);
  w.tab = ar.take<int>((size_t)B * 10);
  w.tstep = ar.take<int>((size_t)B);
  w.pair_ids = ar.take<int64_t>((size_t)B * 4);
  w.pair_logp = ar.take<float>((size_t)B * 4);
  return w;
}

inline size_t kvtrials_ws(const qtx_config& c, const Groups& gr, int B, int S, int max_len) {
  Arena ar;
  carve_kvtrials(ar, c, gr, B, S, max_len);
  return align_up(ar.used);
}

// The encoder trials decode's workspace (qtx_greedy_decode_enctrials): the scored greedy
// decode's (a prefix), then the per-token-row fault table.
struct EnctrialsWS {
  GreedyWS g;
  int* tab;             // [B * S][10] words: one RowFault (qtx_kernels.h) per token row
};

inline EnctrialsWS carve_enctrials(Arena& ar, const qtx_config& c, const Groups& gr, int B, int S,
                                   int max_len) {
  EnctrialsWS w;
  w.g = carve_greedy(ar, c, gr, B, S, max_len, true);
  w.tab = ar.take<int>((size_t)B * S * 10);
  return w;
}

inline size_t enctrials_ws(const qtx_config& c, const Groups& gr, int B, int S, int max_len) {
  Arena ar;
  carve_enctrials(ar, c, gr, B, S, max_len);
  return align_up(ar.used);
}

// Teacher-forced target scoring (qtx_score_targets).  One generator chunk's logits at the model-level call: at most 64 MiB, there only to bound
// the workspace whatever R * T is.  Larger chunks measured faster all the way to one launch
// (cfg2's shape, 2272 rows, V = 4444: generator + tail 1.043 / 0.371 / 0.235 / 0.204 ms with
// chunks of 64 / 256 / 928 / all rows, profiles/score_bench.md).
constexpr size_t SCORE_CHUNK_BYTES = (size_t)64 << 20;

// what the model-level call reserves for a chunk's logits
inline size_t score_logits_bytes(int V, long M) {
  const size_t rows = std::max((size_t)16, (SCORE_CHUNK_BYTES / (4 * (size_t)V)) & ~(size_t)15);
  return std::min(rows, ((size_t)M + 15) & ~(size_t)15) * (size_t)V * 4;
}

struct ScoreWS {
  Scratch enc, dec;     // B * S source rows; R * T target rows
  CrossKV cross;        // the B sentences' golden cross K/V
  CrossKV fcross;       // a faulty trial's own copy (encoder fault, CK / CV fault)
  CrossKV rcross;       // tgt_per_src > 1: the golden ones replicated to the R rows
  float* memory;        // [B * S, D] golden
  float* fmemory;       // an encoder-fault trial's
  uint8_t* rmask;       // [R, S] the source mask per row (tgt_per_src > 1)
  uint8_t* tmask;       // [R, T, T] (pad < 0: [T, T])
  float* out;           // [R * T, D] the decoder's output
  float* logits;        // one chunk
  size_t logits_bytes;
};

inline ScoreWS carve_score(Arena& ar, const qtx_config& c, long B, long S, long L, long K, long nf) {
  ScoreWS w;
  const size_t D = c.d_model, R = (size_t)(B * K), T = (size_t)(L - 1);
  const size_t Ms = (size_t)(B * S);
  w.enc = carve_scratch(ar, c, (long)Ms);
  w.dec = carve_scratch(ar, c, (long)(R * T));
  w.cross = carve_cross(ar, c, (long)Ms);
  w.memory = ar.take<float>(Ms * D);
  w.fmemory = nullptr;
  if (nf > 0) {
    w.fcross = carve_cross(ar, c, (long)Ms);
    w.fmemory = ar.take<float>(Ms * D);
  }
  w.rmask = nullptr;
  if (K > 1) {
    w.rcross = carve_cross(ar, c, (long)(R * S), true);
    w.rmask = ar.take<uint8_t>(R * S);
  }
  w.tmask = ar.take<uint8_t>(R * T * T);
  w.out = ar.take<float>(R * T * D);
  w.logits_bytes = score_logits_bytes(c.tgt_vocab, (long)(R * T));
  w.logits = ar.take<float>(w.logits_bytes / 4);
  return w;
}

inline size_t score_ws(const qtx_config& c, long B, long S, long L, long K, long nf) {
  Arena ar;
  carve_score(ar, c, B, S, L, K, nf);
  return align_up(ar.used);
}

}  // namespace qtx

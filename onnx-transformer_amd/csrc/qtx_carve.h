// qtx_carve.h — the workspace carving that has no GPU in it: the bump allocator, the stack
// scratch, the cross K/V, the decode workspace and the beam decode's carve_beam.  Plain C++
// over qtx_config and sizes; qtx_api.hip carves the callers' workspaces with it and
// tools/beam_host_check.cpp runs carve_beam under the host sanitizers.
#pragma once
#include <stddef.h>
#include <stdint.h>

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

inline CrossKV carve_cross(Arena& ar, const qtx_config& c, long Ms) {
  const int D = c.d_model;
  CrossKV x;
  x.am8 = ar.take<int8_t>(Ms * D);
  x.sam = ar.take<float>(Ms);
  x.y = ar.take<float>(Ms * 2 * D);
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
  // the hypotheses' cross K/V: the layout of carve_cross (tile 2 l + {0: K, 1: V})
  g.cross.am8 = nullptr; g.cross.sam = nullptr; g.cross.y = nullptr;
  int8_t* kv = ar.take<int8_t>(2 * L * R * S * D);
  float* sc = ar.take<float>(2 * L * R * S);
  int8_t* cvg = ar.take<int8_t>(L * R * S4 * D);
  w.tail.k_ls = (long)(R * max_len * D);
  w.tail.v_ls = (long)(R * ML4 * D);
  w.tail.s_ls = (long)(R * max_len);
  w.tail.kc0 = ar.take<int8_t>(L * w.tail.k_ls);
  w.tail.vc0 = ar.take<int8_t>(L * w.tail.v_ls);
  w.tail.skc0 = ar.take<float>(L * w.tail.s_ls);
  w.tail.svc0 = ar.take<float>(L * w.tail.s_ls);
  for (size_t l = 0; l < L; ++l) {
    g.cross.k8.push_back(kv ? kv + 2 * l * R * S * D : nullptr);
    g.cross.v8.push_back(kv ? kv + (2 * l + 1) * R * S * D : nullptr);
    g.cross.sk.push_back(sc ? sc + 2 * l * R * S : nullptr);
    g.cross.sv.push_back(sc ? sc + (2 * l + 1) * R * S : nullptr);
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

}  // namespace qtx

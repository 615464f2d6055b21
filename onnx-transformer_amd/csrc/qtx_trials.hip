// qtx_trials.hip — the trials decode of the C-ABI (include/qtx.h): one KV-cached scored decode
// that carries one independent kvfault trial per sentence (qtx_greedy_decode_kvtrials), and the
// per-op entry of its GEMM (qtx_linear_i8_rowfaults).  Built from the kvfault decode's parts
// (qtx_fault.hip) and the row-fault GEMM (qtx_rowfault.hip); the workspace is carved by
// qtx_carve.h.  Host code only.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <string>
#include <vector>

#include "qtx_host.h"

namespace qtx {

static_assert(sizeof(RowFault) == 10 * sizeof(int), "KvtrialsWS::tab carves 10 words per row");

// One row's trial as the schedule uses it: the step fault in B = 1 coordinates, or where the
// upset lands in the whole batch's caches.  what 0 (or a step the decode never runs): golden.
struct RowTrial {
  int what = 0, step = -1;
  qtx_fault f{};
  UpsetAt at{};
  int bit = 0;
};

// The refusal of row b, with the row in its text.
int named(int rc, int b) {
  if (rc == QTX_OK) return rc;
  const std::string msg = qtx_last_error();
  return fail(rc, "trial row %d: %s", b, msg.c_str());
}

// A linear step fault (B = 1 coordinates: its token row is 0) as its row's table entry, in the
// coordinates of the GEMM that computes its MatMul (fault_for at M = 1).  Attention targets and
// a WEIGHT16 window that misses row 0 leave the entry empty.
RowFault rowfault_of(const qtx_fault* f, int step, const qtx_config& c) {
  RowFault r{};
  static const GemmId gids[] = {G_QKV, G_O, G_FFN1, G_FFN2, G_CQ, G_CO};
  for (GemmId gid : gids) {
    const FaultArgs fa = fault_for(f, 1, f->layer, gid, 1, c);
    if (fa.kind == FK_NONE) continue;
    if (fa.kind == FK_WEIGHT && !(fa.lo <= 0 && 0 < fa.hi)) return r;
    r.step = step; r.layer = f->layer; r.gemm = gid; r.kind = fa.kind; r.bit = fa.bit;
    r.col = (int)fa.col; r.wrow = fa.kind == FK_WEIGHT ? (int)fa.row : 0;
    r.lo = (int)fa.lo; r.hi = (int)fa.hi; r.value = fa.value;
    return r;
  }
  return r;
}

// linear() at M = B on the row-fault GEMM: every row with the table entry of its own trial
int rf_linear(const QLin& L, const int8_t* a8, const float* sa, int M, int flags, const float* res,
              float* out, long ldo, const RowFault* tab, int t, int l, GemmId gid, hipStream_t st) {
  GemmArgs g{};
  g.A = a8; g.lda = L.K; g.sa = sa;
  g.W = L.w8(); g.ldw = L.K; g.sw = L.s; g.bias = L.b;
  g.out = out; g.ldo = ldo; g.res = res; g.ldr = ldo;
  g.M = M; g.N = L.N; g.K = L.K; g.flags = flags;
  HIPCHK(launch_gemm_rowfault(g, tab, t, l, gid, st));
  return QTX_OK;
}

// Step `t` of the KV-cached decode, eager, on the whole batch, every row with the step fault of
// its own trial (rows whose trial is not a step fault at t: none).  kvfault_step (qtx_fault.hip)
// with the row-fault GEMM in place of linear(.., fa), and one recomputation of the affected
// (sentence, head) per attention-target trial; the step's logits land in g.logits.
int kvtrials_step(const qtx_model* m, GreedyWS& g, int B, int S, int max_len, int t,
                  const std::vector<RowTrial>& rows, const RowFault* tab, bool fused,
                  hipStream_t st) {
  const qtx_config& c = m->cfg;
  const int D = c.d_model, F = c.d_ff;
  Scratch& s = g.dec;
  HIPCHK(launch_set_steps(g.step, g.gsteps, 0, t, st));
  HIPCHK(launch_embed(g.ids + t, max_len, B, 1, nullptr, t, m->tgt_lut, c.tgt_vocab, m->pe,
                      c.max_len, s.x, D, st));
  // the attention-target trials of this step in layer l, each with af.b = its row; a WEIGHT16
  // window that misses the step's only query row has no effect
  auto attn_faults = [&](int l, bool cross) {
    std::vector<AttnFault> v;
    for (int b = 0; b < B; ++b) {
      const RowTrial& r = rows[b];
      AttnFault af{};
      if (r.what != 1 || r.step != t || !attn_fault_for(&r.f, 1, l, cross, 1, cross ? S : t + 1, af))
        continue;
      if (af.row0 > 0 || af.row0 + af.nrows <= 0) continue;
      af.row0 = 0; af.nrows = 1; af.b = b;
      v.push_back(af);
    }
    return v;
  };
  // the one query row of sentence af.b with the caches as the fused step keeps them
  auto fused_attn_fault = [&](const AttnFault& af, int l, bool cross) -> int {
    RC(quant(s.y, cross ? D : 3 * D, B, D, s.q8, s.sq, st));   // the query codes k_dec_attn formed
    const long krows = cross ? S : max_len;
    AttnArgs a{};
    a.q = s.q8; a.q_bs = D; a.q_ld = D; a.sq = s.sq; a.sq_bs = 1;
    a.k = cross ? g.cross.k8[l] : g.kc[l]; a.k_bs = krows * D; a.k_ld = D;
    a.sk = cross ? g.cross.sk[l] : g.skc[l]; a.sk_bs = krows;
    a.v = cross ? g.cvg[l] : g.vc[l];
    a.sv = cross ? g.cross.sv[l] : g.svc[l]; a.sv_bs = krows;
    if (cross) { a.mask = g.mask; a.m_bs = S; a.m_is = 0; }
    a.ctx = s.ctx; a.c_bs = D; a.c_ld = D;
    a.B = B; a.H = c.n_heads; a.Sq = 1; a.Sk = cross ? S : t + 1; a.dec = 1;
    HIPCHK(launch_dec_attn_fault(a, af, (int)((krows + 3) / 4), st));
    return QTX_OK;
  };
  for (int l = 0; l < c.n_layers; ++l) {
    const DecLayer& L = m->dec[l];
    auto lin = [&](const QLin& q, const int8_t* a8, const float* sa, int flags, const float* res,
                   float* out, long ldo, GemmId gid) {
      return rf_linear(q, a8, sa, B, flags, res, out, ldo, tab, t, l, gid, st);
    };
    const std::vector<AttnFault> self_f = attn_faults(l, false), cross_f = attn_faults(l, true);
    RC(ln_quant(s.x, B, L.ln[0], D, s.a8, s.sa, st));
    RC(lin(L.qkv, s.a8, s.sa, 0, nullptr, s.y, 3 * D, G_QKV));
    if (fused) {
      HIPCHK(launch_dec_attn(dec_attn_self(g, l, B, max_len, t + 1), B, st));
      for (const AttnFault& af : self_f) RC(fused_attn_fault(af, l, false));
    } else {
      RC(cached_self_attn_unfused(g, l, B, max_len, t, nullptr, st));
      AttnArgs a = attn_args(s, B, 1, t + 1, max_len);   // as cached_self_attn_unfused ran it
      a.k = g.kc[l]; a.sk = g.skc[l]; a.v = g.vc[l]; a.sv = g.svc[l];
      a.dec = 1;
      for (const AttnFault& af : self_f) HIPCHK(launch_attn_fault_rows(a, af, st));
    }
    RC(quant(s.ctx, D, B, D, s.a8, s.sa, st));
    RC(lin(L.o, s.a8, s.sa, EPI_RESIDUAL, s.x, s.x, D, G_O));
    RC(ln_quant(s.x, B, L.ln[1], D, s.a8, s.sa, st));
    RC(lin(L.cq, s.a8, s.sa, 0, nullptr, s.y, D, G_CQ));
    if (fused) {
      HIPCHK(launch_dec_attn(dec_attn_cross(g, l, B, S, g.mask), B, st));
      for (const AttnFault& af : cross_f) RC(fused_attn_fault(af, l, true));
    } else {                                             // cross_attn_block's attention
      RC(quant(s.y, D, B, D, s.q8, s.sq, st));
      AttnArgs a = attn_args(s, B, 1, S, S);
      a.k = g.cross.k8[l]; a.sk = g.cross.sk[l]; a.v = g.cross.v8[l]; a.sv = g.cross.sv[l];
      a.mask = g.mask; a.m_bs = S; a.m_is = 0;
      a.dec = 1;
      HIPCHK(launch_attention(a, st));
      for (const AttnFault& af : cross_f) HIPCHK(launch_attn_fault_rows(a, af, st));
    }
    RC(quant(s.ctx, D, B, D, s.a8, s.sa, st));
    RC(lin(L.co, s.a8, s.sa, EPI_RESIDUAL, s.x, s.x, D, G_CO));
    // ffn_block
    RC(ln_quant(s.x, B, L.ln[2], D, s.a8, s.sa, st));
    RC(lin(L.w1, s.a8, s.sa, EPI_RELU, nullptr, s.y, F, G_FFN1));
    RC(quant(s.y, F, B, F, s.a8, s.sa, st));
    RC(lin(L.w2, s.a8, s.sa, EPI_RESIDUAL, s.x, s.x, D, G_FFN2));
  }
  RC(ln_out(s.x, B, m->dec_norm, D, g.xo, st));
  HIPCHK(launch_generator_mfma(g.xo, D, B, nullptr, nullptr, m->gen_wt, m->gen_b, c.tgt_vocab,
                               g.logits, st));
  return QTX_OK;
}

}  // namespace qtx

using namespace qtx;

extern "C" {

size_t qtx_greedy_kvtrials_workspace_size(const qtx_model* m, int32_t B, int32_t S,
                                          int32_t max_len) {
  if (!m || B <= 0 || S <= 0 || max_len < 1) return 0;
  return kvtrials_ws(m->cfg, decode_groups(B), B, S, max_len);
}

int32_t qtx_greedy_decode_kvtrials(const qtx_model* m, const int64_t* src, const uint8_t* src_mask,
                                   int32_t B, int32_t S, int32_t max_len, int64_t start,
                                   int64_t* ids, int64_t* top_ids, float* top_logp,
                                   int64_t* rec_ids, float* rec_logp, void* ws, size_t ws_bytes,
                                   const qtx_kv_trial* trials, void* stream) {
  if (!m || !src || !src_mask || !ids || !ws || !trials) return fail(QTX_E_INVALID, "null argument");
  RC(check_pairs(top_ids, top_logp, rec_ids, rec_logp));
  const qtx_config& c = m->cfg;
  RC(check_decode_shape(c, B, S, max_len));
  RC(check_below_2_30(c, B, max_len));
  // per row, what the stand-alone call refuses before it looks at its workspace
  for (int b = 0; b < B; ++b) {
    const qtx_kv_trial& tr = trials[b];
    if (tr.what < 0 || tr.what > 2) return fail(QTX_E_INVALID, "trial row %d: what %d", b, tr.what);
    if (tr.what == 0) continue;
    if (tr.step < 0) return fail(QTX_E_INVALID, "trial row %d: step %d", b, tr.step);
    if (tr.what != 1) continue;
    if (tr.fault.kind == QTX_FAULT_NONE || tr.fault.module != 1)
      return fail(QTX_E_INVALID, "trial row %d: a step fault is one decoder fault (module 1)", b);
    RC(named(check_fault_bits(c), b));
    if (tr.fault.linear == QTX_LIN_CK || tr.fault.linear == QTX_LIN_CV)
      return fail(QTX_E_UNSUPPORTED, "trial row %d: a memory K/V projection fault is not a trial "
                                     "of this entry (qtx_greedy_decode_kvfault takes it)", b);
  }
  RC(refuse_dbg_tail("kvtrials decode"));
  RC(check_top2_vocab(c));
  const Groups gr = decode_groups(B);
  RC(check_workspace(ws_bytes, kvtrials_ws(c, gr, B, S, max_len)));
  const int last = max_len - 1;          // steps 0 .. last-1
  const bool fused = greedy_fused(c, S, max_len);
  // carved before the frame begins, as the kvfault decode: the upsets are validated against the
  // carved caches, and only a call that will run forgets the workspace's header
  Arena ar = ws_arena(ws, ws_bytes);
  KvtrialsWS w = carve_kvtrials(ar, c, gr, B, S, max_len);
  GreedyWS& g = w.k.g;
  RowFault* tab = reinterpret_cast<RowFault*>(w.tab);
  std::vector<RowTrial> rows((size_t)B);
  std::vector<RowFault> htab((size_t)B, RowFault{});
  std::vector<int> htstep((size_t)B, -1), steps;
  for (int b = 0; b < B; ++b) {
    const qtx_kv_trial& tr = trials[b];
    if (tr.what == 0 || tr.step >= last) continue;   // never applied: coordinates not checked
    RowTrial& r = rows[b];
    if (tr.what == 1) {
      RC(named(kvfault_check_fault(m, &tr.fault, 1, S, tr.step), b));
      r.f = tr.fault;
      htab[b] = rowfault_of(&r.f, tr.step, c);
    } else {
      // the sentence's own coordinates first (the stand-alone B = 1 call's), then the batch's
      RC(named(kvfault_upset_at(c, g, &tr.upset, 1, S, max_len, tr.step, fused, nullptr), b));
      qtx_cache_upset u = tr.upset;
      u.row += (int64_t)b * (u.cache < 2 ? max_len : S);
      RC(named(kvfault_upset_at(c, g, &u, B, S, max_len, tr.step, fused, &r.at), b));
      r.bit = u.bit;
    }
    r.what = tr.what; r.step = tr.step;
    htstep[b] = tr.step;
    steps.push_back(tr.step);
  }
  std::sort(steps.begin(), steps.end());
  steps.erase(std::unique(steps.begin(), steps.end()), steps.end());
  hipStream_t st = (hipStream_t)stream;
  CallFrame fr;
  RC(frame_begin(m, ws, ws_bytes, st, true, &fr));
  g.enc.status = fr.status;
  // the table and the rows' steps, once, before the first launch (the host vectors outlive
  // the copies: the stream is waited for here, where nothing of this call is queued yet)
  HIPCHK(hipMemcpyAsync(tab, htab.data(), (size_t)B * sizeof(RowFault), hipMemcpyHostToDevice, st));
  HIPCHK(hipMemcpyAsync(w.tstep, htstep.data(), (size_t)B * sizeof(int), hipMemcpyHostToDevice, st));
  HIPCHK(hipStreamSynchronize(st));
  const bool rec = rec_ids != nullptr;
  if (rec) {   // rows without an applied trial keep zeros
    HIPCHK(hipMemsetAsync(w.k.rec_ids, 0, (size_t)B * 4 * sizeof(int64_t), st));
    HIPCHK(hipMemsetAsync(w.k.rec_logp, 0, (size_t)B * 4 * sizeof(float), st));
  }
  const int V = c.tgt_vocab;
  // the top 2 of step t, which just ran, into rec[b, which, :] of the rows whose trial is at t
  auto record = [&](int t, int which) -> int {
    HIPCHK(launch_trial_record(g.top_ids, g.top_logp, last, t, B, w.tstep, which, w.k.rec_ids,
                               w.k.rec_logp, st));
    return QTX_OK;
  };
  HIPCHK(hipMemcpyAsync(g.mask, src_mask, (size_t)B * S, hipMemcpyDeviceToDevice, st));
  RC(greedy_prologue(m, g, src, B, S, max_len, start, nullptr, fused, st));
  int cur = 0;   // the next step to run
  for (int t : steps) {
    // golden up to the step; with a record, the step itself once before anything is applied
    RC(dfault_steps(m, g, B, S, max_len, cur, rec ? t + 1 : t, st));
    if (rec) RC(record(t, 0));
    bool step_fault = false;
    for (int b = 0; b < B; ++b) {
      const RowTrial& r = rows[b];
      if (r.step != t) continue;
      if (r.what == 2) HIPCHK(launch_cache_upset(r.at.c0, r.at.c1, r.at.s, r.bit, st));
      step_fault |= r.what == 1;
    }
    if (step_fault) {
      RC(kvtrials_step(m, g, B, S, max_len, t, rows, tab, fused, st));
      // every row's token and entry t from this run: as after_faulty_step's scored form
      RC(record_top2(g.logits, B, V, w.pair_ids, w.pair_logp, 1, st));
      HIPCHK(launch_dfault_tail(w.pair_ids, w.pair_logp, B, t, max_len, g.ids, g.top_ids,
                                g.top_logp, nullptr, st));
    } else {
      RC(dfault_steps(m, g, B, S, max_len, t, t + 1, st));
    }
    if (rec) RC(record(t, 1));
    cur = t + 1;
  }
  RC(dfault_steps(m, g, B, S, max_len, cur, last, st));
  RC(copy_out(g.ids, g.top_ids, g.top_logp, B, max_len, ids, top_ids, top_logp, st));
  return copy_out_record(w.k.rec_ids, w.k.rec_logp, B, rec_ids, rec_logp, st);
}

int32_t qtx_linear_i8_rowfaults(const int8_t* A, const float* sa, const int8_t* W, const float* sw,
                                const float* bias, int32_t M, int32_t N, int32_t K, int32_t flags,
                                const float* res, float* out, const qtx_fault* rows, void* stream) {
  if (!A || !sa || !W || !sw || !bias || !out || !rows) return fail(QTX_E_INVALID, "null argument");
  if ((flags & EPI_RESIDUAL) && !res) return fail(QTX_E_INVALID, "residual flag without res");
  if (M <= 0 || N <= 0) return QTX_OK;
  if (K <= 0 || K % 64) return fail(QTX_E_UNSUPPORTED, "K=%d not a multiple of 64", K);
  if (!aligned16(A) || !aligned16(W)) return fail(QTX_E_INVALID, "A and W must be 16-byte aligned");
  std::vector<RowFault> htab((size_t)M, RowFault{});
  for (int r = 0; r < M; ++r) {
    const qtx_fault& f = rows[r];
    RowFault& e = htab[r];
    const bool win = f.kind == QTX_FAULT_INPUT16 || f.kind == QTX_FAULT_WEIGHT16;
    auto bad = [&](const char* what) { return fail(QTX_E_INVALID, "row %d: fault %s", r, what); };
    if (win && (f.win_len < 1 || f.win_len > 16 || f.win_start < 0)) return bad("window");
    switch (f.kind) {
      case QTX_FAULT_NONE: continue;
      case QTX_FAULT_INPUT: case QTX_FAULT_INPUT16:
        if (f.row != 0 || f.col < 0 || f.col >= K || f.bit < 0 || f.bit > 7) return bad("index");
        if (win && f.win_start + f.win_len > N) return bad("window");
        e.kind = FK_INPUT; e.col = (int)f.col; e.bit = f.bit;
        e.lo = win ? (int)f.win_start : 0; e.hi = win ? e.lo + f.win_len : N;
        break;
      case QTX_FAULT_WEIGHT: case QTX_FAULT_WEIGHT16:
        if (f.row < 0 || f.row >= N || f.col < 0 || f.col >= K || f.bit < 0 || f.bit > 7)
          return bad("index");
        if (win && f.win_start > 0) continue;   // the window misses row 0: no effect
        e.kind = FK_WEIGHT; e.wrow = (int)f.row; e.col = (int)f.col; e.bit = f.bit;
        break;
      case QTX_FAULT_OUTPUT:
        if (f.row != 0 || f.col < 0 || f.col >= N) return bad("index");
        e.kind = FK_OUTPUT; e.col = (int)f.col; e.value = f.value;
        break;
      default: return bad("kind");
    }
  }
  GemmArgs g{};
  g.A = A; g.lda = K; g.sa = sa; g.W = W; g.ldw = K; g.sw = sw; g.bias = bias;
  g.out = out; g.ldo = N; g.res = res; g.ldr = N;
  g.M = M; g.N = N; g.K = K; g.flags = flags;
  // a test entry: the table lives in memory of its own for the length of the call
  hipStream_t st = (hipStream_t)stream;
  RowFault* tab = nullptr;
  HIPCHK(hipMalloc(&tab, (size_t)M * sizeof(RowFault)));
  hipError_t e = hipMemcpy(tab, htab.data(), (size_t)M * sizeof(RowFault), hipMemcpyHostToDevice);
  if (e == hipSuccess) e = launch_gemm_rowfault(g, tab, 0, 0, 0, st);
  if (e == hipSuccess) e = hipStreamSynchronize(st);
  (void)hipFree(tab);
  HIPCHK(e);
  return QTX_OK;
}

}  // extern "C"

// qtx_fault.hip — the fault decodes of the C-ABI (include/qtx.h): the KV-cached greedy decode
// with one decoder fault and its resume (qtx_greedy_decode_dfault, qtx_greedy_dfault_resume),
// and the faults of the KV-cached decode itself (qtx_greedy_decode_kvfault).  Built from the
// stacks and steps of qtx_api.hip; the workspaces are carved by qtx_carve.h.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <mutex>
#include <vector>

#include "qtx_host.h"

namespace qtx {

// KV-cached steps t0 .. t1-1 from ids[:, t0], with the decode's path selection: the unfused
// step; the fused step launched eagerly at host positions (QTX_NO_GRAPH); or the fused step
// captured at the device counter's position — graphs of QTX_GRAPH_STEPS (default 8) steps and
// of one step, so that any range is a few replays and a sweep over fault steps captures
// nothing new.  A range never crosses the fault step: the caller splits there.
int dfault_steps(const qtx_model* m, GreedyWS& g, int B, int S, int max_len, int t0, int t1,
                 hipStream_t st) {
  if (t0 >= t1) return QTX_OK;
  const qtx_config& c = m->cfg;
  const bool fused = greedy_fused(c, S, max_len);
  const Groups gr = decode_groups(B);
  HIPCHK(launch_set_steps(g.step, g.gsteps, fused ? gr.G : 0, t0, st));
  if (!fused) {
    for (int t = t0; t < t1; ++t) RC(greedy_step_unfused(m, g, B, S, max_len, g.ids, g.mask, st));
    return QTX_OK;
  }
  std::vector<GreedyWS> gv = group_views(g, c, gr, S, max_len);
  for (int i = 0; i < gr.G; ++i)   // the first decoder input: tgt_embed(ids[:, t0]) at t0
    HIPCHK(launch_embed(g.ids + (long)gr.b0(i) * max_len + t0, max_len, gr.rows(i, B), 1, nullptr,
                        t0, m->tgt_lut, c.tgt_vocab, m->pe, c.max_len, gv[i].dec.x, c.d_model, st));
  // this entry's own graphs
  StepRequest rq = step_request(m, gv, gr, B, S, max_len,
                                g.top_ids ? StepForm::DfaultScored : StepForm::Dfault);
  const int big = graph_chunk();
  const int nbig = big > 1 ? (t1 - t0) / big : 0, none = (t1 - t0) - nbig * big;
  if (nbig) rq.plan.push_back({big, nbig, t0});
  if (none) rq.plan.push_back({1, none, t0 + nbig * big});
  return run_steps(m, rq, st);
}

// The faulty full-prefix decoder pass of step `step` over the whole batch (the fault's row
// indexes its [B * T] tokens, T = step + 1) and the generator on each sentence's last row:
// flogits [B, V].  The body of qtx_decoder_forward_fault on this call's workspace; the
// cached cross K/V are read, never written (a memory K/V fault gets its own copy).
int dfault_pass(const qtx_model* m, DfaultWS& w, int B, int S, int max_len, const qtx_fault* f,
                int step, hipStream_t st) {
  const qtx_config& c = m->cfg;
  const int D = c.d_model, T = step + 1;
  GreedyWS& g = w.g;
  // the scratch was carved for the longest prefix: the three projections and their scales lie
  // M = B * T rows apart, as the row GEMM writes them (carve_scratch)
  Scratch s = w.fs;
  const long M = (long)B * T;
  s.k8 = s.q8 + M * D; s.v8 = s.k8 + M * D;
  s.sk = s.sq + M; s.sv = s.sk + M;
  HIPCHK(launch_embed(g.ids, max_len, B, T, nullptr, 0, m->tgt_lut, c.tgt_vocab, m->pe, c.max_len,
                      s.x, (long)T * D, st));
  HIPCHK(launch_causal_mask(w.tmask, T, st));
  const bool own_kv = ckv_fault(m, f, B * S);
  if (own_kv) RC(cross_kv(m, g.memory, B * S, w.fx, st, f));
  RC(decoder_body(m, s, own_kv ? w.fx : g.cross, g.mask, w.tmask, 0, B, T, S, w.fout, f, st));
  HIPCHK(launch_generator_mfma(w.fout + (long)(T - 1) * D, (long)T * D, B, nullptr, nullptr,
                               m->gen_wt, m->gen_b, c.tgt_vocab, w.flogits, st));
  return QTX_OK;
}

// The top 2 of these logits [B, V] into rec[:, which, :] (0: the golden, 1: the faulty pair).
int record_top2(const float* logits, int B, int V, int64_t* rec_ids, float* rec_logp, int which,
                hipStream_t st) {
  HIPCHK(launch_logsoftmax_top2(logits, B, V, nullptr, 0, nullptr, 0, rec_ids + 2 * which,
                                rec_logp + 2 * which, 2, st));
  return QTX_OK;
}

// After the faulty step `step`, before the cached steps above it: the scored form takes the
// faulty pair rec[:, 1, :] as the step's entry and token; the plain form applies the plain
// tail's rule (qtx_generator without log-probabilities) to the faulty logits.
int after_faulty_step(GreedyWS& g, const float* logits, const int64_t* rec_ids,
                      const float* rec_logp, int B, int V, int step, int max_len, bool scored,
                      hipStream_t st) {
  if (scored)
    HIPCHK(launch_dfault_tail(rec_ids, rec_logp, B, step, max_len, g.ids, g.top_ids, g.top_logp,
                              nullptr, st));
  else
    HIPCHK(launch_logsoftmax_argmax(logits, B, V, nullptr, g.ids, max_len, nullptr, step + 1, st));
  return QTX_OK;
}

void dfault_store(const qtx_model* m, const void* ws, const qtx_model::DfaultHdr& h) {
  qtx_model* mm = const_cast<qtx_model*>(m);
  std::lock_guard<std::mutex> lk(mm->mu);
  mm->dfault[ws] = h;
}

int dfault_args(const qtx_model* m, int B, int S, int max_len, const qtx_fault* f, int fault_step) {
  const qtx_config& c = m->cfg;
  RC(check_decode_shape(c, B, S, max_len));
  RC(check_below_2_30(c, B, max_len));
  if (!f || f->kind == QTX_FAULT_NONE || f->module != 1)
    return fail(QTX_E_INVALID, "the decoder-fault decode takes one decoder fault (encoder "
                               "faults: qtx_greedy_decode_fault / _scored)");
  if (fault_step < 0) return fail(QTX_E_INVALID, "fault_step %d", fault_step);
  RC(check_fault_bits(c));
  return refuse_dbg_tail("decoder-fault decode");
}

}  // namespace qtx

using namespace qtx;

extern "C" {

size_t qtx_greedy_dfault_workspace_size(const qtx_model* m, int32_t B, int32_t S,
                                        int32_t max_len) {
  if (!m || B <= 0 || S <= 0 || max_len < 1) return 0;
  return dfault_ws(m->cfg, decode_groups(B), B, S, max_len);
}

int32_t qtx_greedy_decode_dfault(const qtx_model* m, const int64_t* src, const uint8_t* src_mask,
                                 int32_t B, int32_t S, int32_t max_len, int64_t start,
                                 int64_t* ids, int64_t* top_ids, float* top_logp,
                                 int64_t* rec_ids, float* rec_logp, void* ws, size_t ws_bytes,
                                 const qtx_fault* f, int32_t fault_step, void* stream) {
  if (!m || !src || !src_mask || !ids || !ws) return fail(QTX_E_INVALID, "null argument");
  const bool scored = top_ids || top_logp;
  RC(check_pairs(top_ids, top_logp, rec_ids, rec_logp));
  RC(dfault_args(m, B, S, max_len, f, fault_step));
  const qtx_config& c = m->cfg;
  if (scored || rec_ids) RC(check_top2_vocab(c));
  const Groups gr = decode_groups(B);
  RC(check_workspace(ws_bytes, dfault_ws(c, gr, B, S, max_len)));
  const int last = max_len - 1;             // steps 0 .. last-1
  const bool applied = fault_step < last;   // else the fault's step is never run: golden
  if (applied) RC(check_fault(m, f, 1, B, fault_step + 1, S));
  hipStream_t st = (hipStream_t)stream;
  CallFrame fr;                             // (no header while the workspace is rewritten)
  RC(frame_begin(m, ws, ws_bytes, st, true, &fr));
  DfaultWS w = carve_dfault(fr.ar, c, gr, B, S, max_len);
  GreedyWS& g = w.g;
  g.enc.status = fr.status;
  if (!scored) g.top_ids = nullptr, g.top_logp = nullptr;   // the plain step and its tail
  auto keep_gold = [&]() -> int {   // what is golden so far, for later resumes
    return copy_out(g.ids, g.top_ids, g.top_logp, B, max_len, w.gold_ids, w.gold_top_ids,
                    w.gold_top_logp, st);
  };
  HIPCHK(hipMemcpyAsync(g.mask, src_mask, (size_t)B * S, hipMemcpyDeviceToDevice, st));
  RC(greedy_prologue(m, g, src, B, S, max_len, start, nullptr, greedy_fused(c, S, max_len), st));
  RC(dfault_steps(m, g, B, S, max_len, 0, applied ? fault_step + 1 : last, st));
  if (applied) {
    const int V = c.tgt_vocab;
    if (scored) {          // the cached step's top 2 is the golden record (the campaign's out_2)
      RC(keep_gold());
      HIPCHK(launch_dfault_gold(g.top_ids, g.top_logp, last, fault_step, B, w.rec_ids, w.rec_logp, st));
    } else if (rec_ids) {  // plain form: from the cached step's logits
      RC(record_top2(g.logits, B, V, w.rec_ids, w.rec_logp, 0, st));
    }
    RC(dfault_pass(m, w, B, S, max_len, f, fault_step, st));
    if (scored || rec_ids) RC(record_top2(w.flogits, B, V, w.rec_ids, w.rec_logp, 1, st));
    RC(after_faulty_step(g, w.flogits, w.rec_ids, w.rec_logp, B, V, fault_step, max_len, scored, st));
    RC(dfault_steps(m, g, B, S, max_len, fault_step + 1, last, st));
  } else if (scored && last > 0) {
    RC(keep_gold());
  }
  RC(copy_out(g.ids, g.top_ids, g.top_logp, B, max_len, ids, top_ids, top_logp, st));
  if (applied) RC(copy_out_record(w.rec_ids, w.rec_logp, B, rec_ids, rec_logp, st));
  if (scored && last > 0) {
    static std::atomic<long long> next_nonce{1};
    const long long nonce = (long long)(m->serial << 40) ^ next_nonce.fetch_add(1);
    HIPCHK(launch_fill_col(w.stamp, 1, 1, nonce, st));
    dfault_store(m, ws, qtx_model::DfaultHdr{B, S, max_len, applied ? fault_step : last - 1,
                                             !applied, ws_bytes, nonce});
  }
  return QTX_OK;
}

int32_t qtx_greedy_dfault_resume(const qtx_model* m, int32_t B, int32_t S, int32_t max_len,
                                 int64_t* ids, int64_t* top_ids, float* top_logp,
                                 int64_t* rec_ids, float* rec_logp, void* ws, size_t ws_bytes,
                                 const qtx_fault* f, int32_t fault_step, int32_t* changed_host,
                                 void* stream) {
  if (!m || !ids || !top_ids || !top_logp || !ws || !rec_ids != !rec_logp)
    return fail(QTX_E_INVALID, "null argument");
  RC(dfault_args(m, B, S, max_len, f, fault_step));
  const qtx_config& c = m->cfg;
  RC(check_top2_vocab(c));
  const Groups gr = decode_groups(B);
  RC(check_workspace(ws_bytes, dfault_ws(c, gr, B, S, max_len)));
  qtx_model::DfaultHdr h{};
  {
    qtx_model* mm = const_cast<qtx_model*>(m);
    std::lock_guard<std::mutex> lk(mm->mu);
    auto it = mm->dfault.find(ws);
    if (it == mm->dfault.end())
      return fail(QTX_E_INVALID, "resume: the workspace holds no scored decoder-fault decode of this model");
    h = it->second;
  }
  if (h.B != B || h.S != S || h.L != max_len)
    return fail(QTX_E_INVALID, "resume: the workspace was filled for B=%d S=%d max_len=%d", h.B, h.S, h.L);
  if (fault_step > h.n)
    return fail(QTX_E_INVALID, "resume: fault_step %d above the golden prefix's last step %d",
                fault_step, h.n);
  RC(check_fault(m, f, 1, B, fault_step + 1, S));
  hipStream_t st = (hipStream_t)stream;
  Arena ar = ws_arena(ws, ws_bytes);   // no frame_begin: the header stays until the stamp check
  DfaultWS w = carve_dfault(ar, c, gr, B, S, max_len);
  GreedyWS& g = w.g;
  long long stamp = 0;   // the memory must still be what the header describes
  HIPCHK(hipMemcpyAsync(&stamp, w.stamp, sizeof stamp, hipMemcpyDeviceToHost, st));
  HIPCHK(hipStreamSynchronize(st));
  if (stamp != h.nonce) {
    dfault_forget(m, ws);
    return fail(QTX_E_INVALID, "resume: the workspace was overwritten since its decode");
  }
  const int last = max_len - 1;
  HIPCHK(launch_dfault_gold(w.gold_top_ids, w.gold_top_logp, last, fault_step, B, w.rec_ids,
                            w.rec_logp, st));
  RC(dfault_pass(m, w, B, S, max_len, f, fault_step, st));
  RC(record_top2(w.flogits, B, c.tgt_vocab, w.rec_ids, w.rec_logp, 1, st));
  HIPCHK(launch_dfault_tail(w.rec_ids, w.rec_logp, B, fault_step, max_len, nullptr, nullptr,
                            nullptr, w.changed, st));
  // the one synchronising copy: whether any sentence's token changed decides what runs next
  std::vector<int32_t> changed((size_t)B);
  HIPCHK(hipMemcpyAsync(changed.data(), w.changed, (size_t)B * sizeof(int32_t), hipMemcpyDeviceToHost, st));
  HIPCHK(hipStreamSynchronize(st));
  bool any = false;
  for (int b = 0; b < B; ++b) any |= changed[b] != 0;
  if (changed_host) std::copy(changed.begin(), changed.end(), changed_host);
  if (!any && h.gold_full) {   // a masked fault: the golden decode with the faulty entry
    RC(copy_out(w.gold_ids, w.gold_top_ids, w.gold_top_logp, B, max_len, ids, top_ids, top_logp, st));
    HIPCHK(launch_dfault_tail(w.rec_ids, w.rec_logp, B, fault_step, max_len, nullptr, top_ids,
                              top_logp, nullptr, st));
  } else {                     // the steps above fault_step again, from the faulty tokens
    dfault_forget(m, ws);
    RC(after_faulty_step(g, w.flogits, w.rec_ids, w.rec_logp, B, c.tgt_vocab, fault_step, max_len, true, st));
    RC(dfault_steps(m, g, B, S, max_len, fault_step + 1, last, st));
    RC(copy_out(g.ids, g.top_ids, g.top_logp, B, max_len, ids, top_ids, top_logp, st));
    h.n = fault_step;
    dfault_store(m, ws, h);
  }
  return copy_out_record(w.rec_ids, w.rec_logp, B, rec_ids, rec_logp, st);
}

}  // extern "C"

// =======================================================================================
// Faults of the KV-cached decode itself: one step fault or one cache upset
// (include/qtx.h: qtx_greedy_decode_kvfault)
// =======================================================================================
namespace qtx {

// A step fault's coordinates against the step's own MatMuls: one token row and one query row
// per sentence, Sk = step + 1 self keys or S cross keys (include/qtx.h).
int kvfault_check_fault(const qtx_model* m, const qtx_fault* f, int B, int S, int step) {
  if ((f->linear == QTX_LIN_CK || f->linear == QTX_LIN_CV) && step != 0)
    return fail(QTX_E_INVALID, "a memory K/V projection fault belongs to step 0 (step %d)", step);
  return check_fault(m, f, 1, B, 1, S, step + 1, 1L << 30);
}

// Where an upset lands: the code byte(s) or the scale word, as offsets checked against the
// caches' extents here, on the host (UpsetAt: qtx_host.h).
int kvfault_upset_at(const qtx_config& c, GreedyWS& g, const qtx_cache_upset* u, int B, int S,
                     int max_len, int step, bool fused, UpsetAt* at) {
  const long D = c.d_model;
  if (u->cache < 0 || u->cache > 3) return fail(QTX_E_INVALID, "upset cache %d", u->cache);
  if (u->layer < 0 || u->layer >= c.n_layers) return fail(QTX_E_INVALID, "upset layer %d", u->layer);
  if (u->field != 0 && u->field != 1) return fail(QTX_E_INVALID, "upset field %d", u->field);
  const bool self = u->cache < 2, is_v = u->cache & 1;
  const long per = self ? max_len : S;            // rows per sentence
  if (u->row < 0 || u->row >= (long)B * per)
    return fail(QTX_E_INVALID, "upset row %ld outside [0, %ld)", (long)u->row, (long)B * per);
  const long b = u->row / per, j = u->row % per;
  if (self && j >= step)
    return fail(QTX_E_INVALID, "upset of self-cache position %ld at step %d: not written yet", j, step);
  if (u->field == 0 ? (u->bit < 0 || u->bit > 7) : !((u->bit >= 0 && u->bit <= 22) || u->bit == 31))
    return fail(QTX_E_INVALID, "upset bit %d (codes: 0..7; scales: 0..22 and 31)", u->bit);
  if (u->col < 0 || u->col >= (u->field == 0 ? D : 1))
    return fail(QTX_E_INVALID, "upset col %d", u->col);
  if (!at) return QTX_OK;
  const int l = u->layer;
  *at = UpsetAt{nullptr, nullptr, nullptr};
  if (u->field == 1) {
    float* sc = self ? (is_v ? g.svc[l] : g.skc[l]) : (is_v ? g.cross.sv[l] : g.cross.sk[l]);
    at->s = sc + u->row;
    return QTX_OK;
  }
  const long rm = u->row * D + u->col;                                   // row-major
  const long G4 = (per + 3) / 4;
  const long grp = ((b * G4 + j / 4) * D + u->col) * 4 + j % 4;          // 4-key groups
  if (rm >= (long)B * per * D || grp >= (long)B * G4 * 4 * D) return fail(QTX_E_INVALID, "upset offset");
  if (!is_v) at->c0 = (self ? g.kc[l] : g.cross.k8[l]) + rm;
  else if (self) at->c0 = g.vc[l] + (fused ? grp : rm);                  // one layout per path
  else {
    at->c0 = g.cross.v8[l] + rm;                                         // every copy a step reads
    if (fused) at->c1 = g.cvg[l] + grp;
  }
  return QTX_OK;
}

// Step `t` of the KV-cached decode with fault f, eager, on the whole batch: the decoder input
// is tgt_embed(ids[:, t]); every layer's cache row t is (re)written from this run; the step's
// logits land in g.logits.  Built from pieces that agree bit for bit with the fused step's
// kernels: the FaultArgs-aware linear() at M = B, the row quantizers, and — on the fused
// workspace, whose values lie in 4-key groups — k_dec_attn itself for the attention.
int kvfault_step(const qtx_model* m, GreedyWS& g, int B, int S, int max_len, int t,
                 const qtx_fault* f, bool fused, hipStream_t st) {
  const qtx_config& c = m->cfg;
  const int D = c.d_model;
  Scratch& s = g.dec;
  HIPCHK(launch_set_steps(g.step, g.gsteps, 0, t, st));
  HIPCHK(launch_embed(g.ids + t, max_len, B, 1, nullptr, t, m->tgt_lut, c.tgt_vocab, m->pe,
                      c.max_len, s.x, D, st));
  // the one query row of sentence af.b with the caches as the fused step keeps them
  auto fused_attn_fault = [&](const AttnFault& af, int l, bool cross) -> int {
    RC(quant(s.y, cross ? D : 3 * D, B, D, s.q8, s.sq, st));   // the query codes k_dec_attn formed
    const long rows = cross ? S : max_len;
    AttnArgs a{};
    a.q = s.q8; a.q_bs = D; a.q_ld = D; a.sq = s.sq; a.sq_bs = 1;
    a.k = cross ? g.cross.k8[l] : g.kc[l]; a.k_bs = rows * D; a.k_ld = D;
    a.sk = cross ? g.cross.sk[l] : g.skc[l]; a.sk_bs = rows;
    a.v = cross ? g.cvg[l] : g.vc[l];
    a.sv = cross ? g.cross.sv[l] : g.svc[l]; a.sv_bs = rows;
    if (cross) { a.mask = g.mask; a.m_bs = S; a.m_is = 0; }
    a.ctx = s.ctx; a.c_bs = D; a.c_ld = D;
    a.B = B; a.H = c.n_heads; a.Sq = 1; a.Sk = cross ? S : t + 1; a.dec = 1;
    HIPCHK(launch_dec_attn_fault(a, af, (int)((rows + 3) / 4), st));
    return QTX_OK;
  };
  for (int l = 0; l < c.n_layers; ++l) {
    const DecLayer& L = m->dec[l];
    auto fa = [&](GemmId gid) { return fault_for(f, 1, l, gid, B, c); };
    // an attention WEIGHT16 window that misses the step's only query row has no effect
    AttnFault af_self{}, af_cross{};
    auto hits = [](AttnFault& af) {
      if (af.row0 > 0 || af.row0 + af.nrows <= 0) return false;
      af.row0 = 0; af.nrows = 1;
      return true;
    };
    const bool self_f = attn_fault_for(f, 1, l, false, 1, t + 1, af_self) && hits(af_self);
    const bool cross_f = attn_fault_for(f, 1, l, true, 1, S, af_cross) && hits(af_cross);
    RC(ln_quant(s.x, B, L.ln[0], D, s.a8, s.sa, st));
    RC(linear(c, L.qkv, s.a8, s.sa, B, 0, nullptr, s.y, 3 * D, st, fa(G_QKV)));
    if (fused) {
      HIPCHK(launch_dec_attn(dec_attn_self(g, l, B, max_len, t + 1), B, st));
      if (self_f) RC(fused_attn_fault(af_self, l, false));
    } else {
      RC(cached_self_attn_unfused(g, l, B, max_len, t, self_f ? &af_self : nullptr, st));
    }
    RC(quant(s.ctx, D, B, D, s.a8, s.sa, st));
    RC(linear(c, L.o, s.a8, s.sa, B, EPI_RESIDUAL, s.x, s.x, D, st, fa(G_O)));
    if (fused) {
      RC(ln_quant(s.x, B, L.ln[1], D, s.a8, s.sa, st));
      RC(linear(c, L.cq, s.a8, s.sa, B, 0, nullptr, s.y, D, st, fa(G_CQ)));
      HIPCHK(launch_dec_attn(dec_attn_cross(g, l, B, S, g.mask), B, st));
      if (cross_f) RC(fused_attn_fault(af_cross, l, true));
      RC(quant(s.ctx, D, B, D, s.a8, s.sa, st));
      RC(linear(c, L.co, s.a8, s.sa, B, EPI_RESIDUAL, s.x, s.x, D, st, fa(G_CO)));
    } else {
      RC(cross_attn_block(m, L, l, s, g.cross, B, 1, S, g.mask, st, fa(G_CQ), fa(G_CO),
                          cross_f ? &af_cross : nullptr));
    }
    RC(ffn_block(c, L.w1, L.w2, L.ln[2], s, B, st, fa(G_FFN1), fa(G_FFN2)));
  }
  RC(ln_out(s.x, B, m->dec_norm, D, g.xo, st));
  HIPCHK(launch_generator_mfma(g.xo, D, B, nullptr, nullptr, m->gen_wt, m->gen_b, c.tgt_vocab,
                               g.logits, st));
  return QTX_OK;
}

}  // namespace qtx

extern "C" {

size_t qtx_greedy_kvfault_workspace_size(const qtx_model* m, int32_t B, int32_t S,
                                         int32_t max_len) {
  if (!m || B <= 0 || S <= 0 || max_len < 1) return 0;
  return kvfault_ws(m->cfg, decode_groups(B), B, S, max_len);
}

int32_t qtx_greedy_decode_kvfault(const qtx_model* m, const int64_t* src, const uint8_t* src_mask,
                                  int32_t B, int32_t S, int32_t max_len, int64_t start,
                                  int64_t* ids, int64_t* top_ids, float* top_logp,
                                  int64_t* rec_ids, float* rec_logp, void* ws, size_t ws_bytes,
                                  const qtx_fault* f, const qtx_cache_upset* u, int32_t step,
                                  void* stream) {
  if (!m || !src || !src_mask || !ids || !ws) return fail(QTX_E_INVALID, "null argument");
  const bool scored = top_ids || top_logp;
  RC(check_pairs(top_ids, top_logp, rec_ids, rec_logp));
  if (!f == !u) return fail(QTX_E_INVALID, "exactly one of fault / upset");
  const qtx_config& c = m->cfg;
  RC(check_decode_shape(c, B, S, max_len));
  RC(check_below_2_30(c, B, max_len));
  if (f && (f->kind == QTX_FAULT_NONE || f->module != 1))
    return fail(QTX_E_INVALID, "a step fault is one decoder fault (module 1)");
  if (step < 0) return fail(QTX_E_INVALID, "step %d", step);
  if (f) RC(check_fault_bits(c));
  RC(refuse_dbg_tail("kvfault decode"));
  if (scored || rec_ids) RC(check_top2_vocab(c));
  const Groups gr = decode_groups(B);
  RC(check_workspace(ws_bytes, kvfault_ws(c, gr, B, S, max_len)));
  const int last = max_len - 1;          // steps 0 .. last-1
  const bool applied = step < last;      // else nothing runs at or after `step`: golden
  const bool fused = greedy_fused(c, S, max_len);
  // carved before the frame begins: the upset is validated against the carved caches, and only
  // a call that will run forgets the workspace's header (frame_begin)
  Arena ar = ws_arena(ws, ws_bytes);
  KvfaultWS w = carve_kvfault(ar, c, gr, B, S, max_len);
  GreedyWS& g = w.g;
  UpsetAt at{};
  if (applied && f) RC(kvfault_check_fault(m, f, B, S, step));
  if (applied && u) RC(kvfault_upset_at(c, g, u, B, S, max_len, step, fused, &at));
  hipStream_t st = (hipStream_t)stream;
  CallFrame fr;
  RC(frame_begin(m, ws, ws_bytes, st, true, &fr));
  g.enc.status = fr.status;
  if (!scored) g.top_ids = nullptr, g.top_logp = nullptr;   // the plain step and its tail
  const int V = c.tgt_vocab;
  const bool rec = applied && rec_ids;
  // the top 2 of the step that just ran, into rec[:, which, :]
  auto record = [&](int which) -> int {
    if (!scored) return record_top2(g.logits, B, V, w.rec_ids, w.rec_logp, which, st);
    HIPCHK(launch_dfault_gold(g.top_ids, g.top_logp, last, step, B, w.rec_ids + 2 * which,
                              w.rec_logp + 2 * which, st));
    return QTX_OK;
  };
  // cached steps t0 .. last-1; with a record, step t0's top 2 is the faulty pair
  auto run_from = [&](int t0) -> int {
    if (rec) {
      RC(dfault_steps(m, g, B, S, max_len, t0, t0 + 1, st));
      RC(record(1));
      ++t0;
    }
    return dfault_steps(m, g, B, S, max_len, t0, last, st);
  };
  HIPCHK(hipMemcpyAsync(g.mask, src_mask, (size_t)B * S, hipMemcpyDeviceToDevice, st));
  RC(greedy_prologue(m, g, src, B, S, max_len, start, nullptr, fused, st));
  if (!applied) {
    RC(dfault_steps(m, g, B, S, max_len, 0, last, st));
  } else {
    // golden up to the step; with a record, the step itself once on the golden caches
    RC(dfault_steps(m, g, B, S, max_len, 0, rec ? step + 1 : step, st));
    if (rec) RC(record(0));
    if (u) {
      HIPCHK(launch_cache_upset(at.c0, at.c1, at.s, u->bit, st));
      RC(run_from(step));
    } else if (f->linear == QTX_LIN_CK || f->linear == QTX_LIN_CV) {
      // the one-time memory K/V projection again, with the fault: it serves every step
      RC(cross_kv(m, g.memory, B * S, g.cross, st, f));
      if (fused) RC(regroup_cross_values(c, g.cross, B, S, g.cvg[0], st));
      RC(run_from(0));
    } else {
      RC(kvfault_step(m, g, B, S, max_len, step, f, fused, st));
      if (scored || rec) RC(record_top2(g.logits, B, V, w.rec_ids, w.rec_logp, 1, st));
      RC(after_faulty_step(g, g.logits, w.rec_ids, w.rec_logp, B, V, step, max_len, scored, st));
      RC(dfault_steps(m, g, B, S, max_len, step + 1, last, st));
    }
  }
  RC(copy_out(g.ids, g.top_ids, g.top_logp, B, max_len, ids, top_ids, top_logp, st));
  return applied ? copy_out_record(w.rec_ids, w.rec_logp, B, rec_ids, rec_logp, st) : QTX_OK;
}

}  // extern "C"

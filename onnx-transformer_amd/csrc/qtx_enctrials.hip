// qtx_enctrials.hip — the C-ABI of include/qtx_enctrials.h: the scored greedy decode that carries
// one encoder-side fault trial per sentence (qtx_greedy_decode_enctrials: an encoder fault, or a
// fault of the one-time memory K/V projection), and the per-op entry of its GEMM, the table-aware
// row-complete GEMM (qtx_gemm.hip, k_gemm_row's FAULT = 2 form; launch_gemm_row_tab), which
// gives every token row of an M = B * S launch the fault of its own sentence's trial.
// Host code only.
#include <hip/hip_runtime.h>

#include <vector>

#include "../../include/qtx_enctrials.h"
#include "qtx_host.h"

namespace qtx {

static_assert(sizeof(RowFault) == 10 * sizeof(int), "EnctrialsWS::tab carves 10 words per token row");

namespace {

// The launches of the whole call that some trial names: [layer][GemmId] counts, and per layer
// the attention-target trials (af.b = the trial's sentence).
struct TrialPlan {
  std::vector<std::vector<int>> hits;
  std::vector<std::vector<AttnFault>> attn;
  bool ckv = false;
  const RowFault* tab = nullptr;
  const RowFault* for_launch(int l, GemmId gid) const { return hits[l][gid] ? tab : nullptr; }
};

// the row-complete chain's launches (row_quant / row_res_ln / row_ffn1 of qtx_api.hip, row-major
// operands) through the table form; a launch no trial names takes the no-fault instance
int tab_quant(const QLin& L, const int8_t* a8, const float* sa, int M, int8_t* out8, float* os,
              const TrialPlan& p, int l, GemmId gid, hipStream_t st) {
  RowGemmArgs g = rowgemm(L, a8, sa, M, RE_QUANT, false);
  g.out8 = out8; g.ldo8 = 512; g.o8_ts = (long)M * 512; g.os = os; g.os_ts = M;
  HIPCHK(launch_gemm_row_tab(g, p.for_launch(l, gid), l, gid, st));
  return QTX_OK;
}
int tab_res_ln(const QLin& L, const int8_t* a8, const float* sa, int M, float* x,
               const float* const* ln, int8_t* lnq, float* lns, float* lnout, const TrialPlan& p,
               int l, GemmId gid, hipStream_t st) {
  RowGemmArgs g = rowgemm(L, a8, sa, M, RE_RES_LN, false);
  g.res = x; g.xout = x; g.ln_a = ln[0]; g.ln_b = ln[1];
  g.lnq = lnq; g.lns = lns; g.lnout = lnout;
  HIPCHK(launch_gemm_row_tab(g, p.for_launch(l, gid), l, gid, st));
  return QTX_OK;
}
int tab_ffn1(const qtx_config& c, const QLin& L, const int8_t* a8, const float* sa, int M,
             Scratch& s, const TrialPlan& p, int l, hipStream_t st) {
  RowGemmArgs g = rowgemm(L, a8, sa, M, RE_RELU_PMAX, false);
  g.pmax_out = s.pmax;
  HIPCHK(launch_gemm_row_tab(g, p.for_launch(l, G_FFN1), l, G_FFN1, st));
  g.epi = RE_RELU_QUANT_PMAX;
  g.pmax_in = s.pmax; g.pmax_n = c.d_ff / 512;
  g.out8 = s.h8; g.ldo8 = c.d_ff; g.os = s.sh;
  HIPCHK(launch_gemm_row_tab(g, p.for_launch(l, G_FFN1), l, G_FFN1, st));
  return QTX_OK;
}
// linear() of the generic chain: the row-fault GEMM where a trial names the launch
int tab_linear(const qtx_config& c, const QLin& L, const int8_t* a8, const float* sa, int M,
               int flags, const float* res, float* out, long ldo, const TrialPlan& p, int l,
               GemmId gid, hipStream_t st) {
  if (!p.hits[l][gid]) return linear(c, L, a8, sa, M, flags, res, out, ldo, st);
  return rf_linear(L, a8, sa, M, flags, res, out, ldo, p.tab, 0, l, gid, st);
}

// encoder_run on the fault chain's layout (row-major, kp = false) with the trials' table: s.x
// holds the embedded sources, out [B * S, D] the memory
int enctrials_encoder(const qtx_model* m, const uint8_t* mask, int B, int S, float* out, Scratch& s,
                      const TrialPlan& p, hipStream_t st) {
  const qtx_config& c = m->cfg;
  const int D = c.d_model, F = c.d_ff, M = B * S, NL = c.n_layers;
  const bool rows = row_path(c);
  if (rows) RC(ln_quant(s.x, M, m->enc[0].ln[0], D, s.a8, s.sa, st));
  for (int l = 0; l < NL; ++l) {
    const EncLayer& L = m->enc[l];
    AttnArgs a = attn_args(s, B, S, S, S);
    a.mask = mask; a.m_bs = S; a.m_is = 0;
    a.c_ld = D;
    // the golden attention, then the affected (sentence, head) rows of each attention trial
    auto attention_trials = [&]() -> int {
      HIPCHK(launch_attention(a, st));
      for (const AttnFault& af : p.attn[l]) HIPCHK(launch_attn_fault_rows(a, af, st));
      return quant(s.ctx, D, M, D, s.a8, s.sa, st);
    };
    if (!rows) {   // self_attn_block + ffn_block
      RC(ln_quant(s.x, M, L.ln[0], D, s.a8, s.sa, st));
      RC(tab_linear(c, L.qkv, s.a8, s.sa, M, 0, nullptr, s.y, 3 * D, p, l, G_QKV, st));
      RC(quant(s.y, 3 * D, M, D, s.q8, s.sq, st));
      RC(quant(s.y + D, 3 * D, M, D, s.k8, s.sk, st));
      RC(quant(s.y + 2 * D, 3 * D, M, D, s.v8, s.sv, st));
      RC(attention_trials());
      RC(tab_linear(c, L.o, s.a8, s.sa, M, EPI_RESIDUAL, s.x, s.x, D, p, l, G_O, st));
      RC(ln_quant(s.x, M, L.ln[1], D, s.a8, s.sa, st));
      RC(tab_linear(c, L.w1, s.a8, s.sa, M, EPI_RELU, nullptr, s.y, F, p, l, G_FFN1, st));
      RC(quant(s.y, F, M, F, s.a8, s.sa, st));
      RC(tab_linear(c, L.w2, s.a8, s.sa, M, EPI_RESIDUAL, s.x, s.x, D, p, l, G_FFN2, st));
      continue;
    }
    RC(tab_quant(L.qkv, s.a8, s.sa, M, s.q8, s.sq, p, l, G_QKV, st));
    if (p.attn[l].empty()) RC(attention_quant(a, nullptr, M, D, s, false, st));
    else RC(attention_trials());
    RC(tab_res_ln(L.o, s.a8, s.sa, M, s.x, L.ln[1], s.a8, s.sa, nullptr, p, l, G_O, st));
    RC(tab_ffn1(c, L.w1, s.a8, s.sa, M, s, p, l, st));
    if (l + 1 < NL)
      RC(tab_res_ln(L.w2, s.h8, s.sh, M, s.x, m->enc[l + 1].ln[0], s.a8, s.sa, nullptr, p, l, G_FFN2, st));
    else
      RC(tab_res_ln(L.w2, s.h8, s.sh, M, s.x, m->enc_norm, nullptr, nullptr, out, p, l, G_FFN2, st));
  }
  if (!rows) RC(ln_out(s.x, M, m->enc_norm, D, out, st));
  return QTX_OK;
}

// cross_kv's per-layer loop with the CK / CV trials' table
int enctrials_cross_kv(const qtx_model* m, const float* memory, int Ms, CrossKV& x,
                       const TrialPlan& p, hipStream_t st) {
  const qtx_config& c = m->cfg;
  const int D = c.d_model;
  RC(quant(memory, D, Ms, D, x.am8, x.sam, st));
  for (int l = 0; l < c.n_layers; ++l) {
    if (row_path(c)) {
      RC(tab_quant(m->dec[l].ckv, x.am8, x.sam, Ms, x.k8[l], x.sk[l], p, l, G_CKV, st));
      continue;
    }
    RC(tab_linear(c, m->dec[l].ckv, x.am8, x.sam, Ms, 0, nullptr, x.y, 2 * D, p, l, G_CKV, st));
    RC(quant(x.y, 2 * D, Ms, D, x.k8[l], x.sk[l], st));
    RC(quant(x.y + D, 2 * D, Ms, D, x.v8[l], x.sv[l], st));
  }
  return QTX_OK;
}

// Sentence b's fault (B = 1 coordinates, validated) into the plan and the host table [B * S]
void add_trial(const qtx_fault& f, int b, int S, const qtx_config& c, TrialPlan& p,
               std::vector<RowFault>& htab) {
  AttnFault af{};
  if (f.module == 0 && attn_fault_for(&f, 0, f.layer, false, S, S, af)) {
    af.b = b;
    p.attn[f.layer].push_back(af);
    return;
  }
  static const GemmId enc_gids[] = {G_QKV, G_O, G_FFN1, G_FFN2}, dec_gids[] = {G_CKV};
  const GemmId* gids = f.module == 0 ? enc_gids : dec_gids;
  for (int k = 0, n = f.module == 0 ? 4 : 1; k < n; ++k) {
    const GemmId gid = gids[k];
    const FaultArgs fa = fault_for(&f, f.module, f.layer, gid, S, c);
    if (fa.kind == FK_NONE) continue;
    RowFault r{};
    r.step = 0; r.layer = f.layer; r.gemm = gid; r.kind = fa.kind; r.bit = fa.bit;
    r.col = (int)fa.col; r.value = fa.value;
    if (fa.kind == FK_WEIGHT) {          // every row of the sentence inside the window
      r.wrow = (int)fa.row;
      for (long i = fa.lo; i < fa.hi; ++i) htab[(size_t)b * S + i] = r;
    } else {
      r.lo = (int)fa.lo; r.hi = (int)fa.hi;
      htab[(size_t)b * S + fa.row] = r;
    }
    p.hits[f.layer][gid]++;
    p.ckv |= gid == G_CKV;
    return;
  }
}

}  // namespace
}  // namespace qtx

using namespace qtx;

static_assert(sizeof(qtx_row_fault) == sizeof(RowFault), "qtx_row_fault is RowFault, word for word");

extern "C" {

size_t qtx_greedy_enctrials_workspace_size(const qtx_model* m, int32_t B, int32_t S,
                                           int32_t max_len) {
  if (!m || B <= 0 || S <= 0 || max_len < 1) return 0;
  return enctrials_ws(m->cfg, decode_groups(B), B, S, max_len);
}

int32_t qtx_greedy_decode_enctrials(const qtx_model* m, const int64_t* src, const uint8_t* src_mask,
                                    int32_t B, int32_t S, int32_t max_len, int64_t start,
                                    int64_t* ids, int64_t* top_ids, float* top_logp, void* ws,
                                    size_t ws_bytes, const qtx_fault* faults, void* stream) {
  if (!m || !src || !src_mask || !ids || !ws || !faults || (max_len > 1 && (!top_ids || !top_logp)))
    return fail(QTX_E_INVALID, "null argument");
  const qtx_config& c = m->cfg;
  RC(check_decode_shape(c, B, S, max_len));
  RC(check_below_2_30(c, B, max_len));
  // per row, what the stand-alone B = 1 call refuses
  for (int b = 0; b < B; ++b) {
    const qtx_fault& f = faults[b];
    if (f.kind == QTX_FAULT_NONE) continue;
    if (f.module == 1) {
      if (f.linear != QTX_LIN_CK && f.linear != QTX_LIN_CV)
        return fail(QTX_E_UNSUPPORTED, "trial row %d: a decoder fault other than a memory K/V "
                                       "projection fault is not a trial of this entry "
                                       "(qtx_greedy_decode_kvtrials takes it)", b);
      RC(named(kvfault_check_fault(m, &f, 1, S, 0), b));
    } else {
      RC(named(check_fault(m, &f, 0, 1, S, 0), b));
    }
  }
  RC(refuse_dbg_tail("enctrials decode"));
  RC(check_top2_vocab(c));
  const Groups gr = decode_groups(B);
  RC(check_workspace(ws_bytes, enctrials_ws(c, gr, B, S, max_len)));
  TrialPlan plan;
  plan.hits.assign((size_t)c.n_layers, std::vector<int>(G_CO + 1, 0));
  plan.attn.resize((size_t)c.n_layers);
  std::vector<RowFault> htab((size_t)B * S, RowFault{});
  for (int b = 0; b < B; ++b)
    if (faults[b].kind != QTX_FAULT_NONE) add_trial(faults[b], b, S, c, plan, htab);
  hipStream_t st = (hipStream_t)stream;
  CallFrame fr;
  RC(frame_begin(m, ws, ws_bytes, st, true, &fr));
  EnctrialsWS w = carve_enctrials(fr.ar, c, gr, B, S, max_len);
  GreedyWS& g = w.g;
  g.enc.status = fr.status;
  plan.tab = reinterpret_cast<const RowFault*>(w.tab);
  // the table, once, before the first launch (the host vector outlives the copy: the stream is
  // waited for here, where nothing of this call is queued yet)
  HIPCHK(hipMemcpyAsync(w.tab, htab.data(), htab.size() * sizeof(RowFault), hipMemcpyHostToDevice, st));
  HIPCHK(hipStreamSynchronize(st));
  HIPCHK(hipMemcpyAsync(g.mask, src_mask, (size_t)B * S, hipMemcpyDeviceToDevice, st));
  // encode_src with the trials: embed, the encoder, the cross K/V of every layer
  const bool fused = greedy_fused(c, S, max_len);
  HIPCHK(launch_embed(src, S, B, S, nullptr, 0, m->src_lut, c.src_vocab, m->pe, c.max_len, g.enc.x,
                      (long)S * c.d_model, st));
  RC(enctrials_encoder(m, g.mask, B, S, g.memory, g.enc, plan, st));
  if (plan.ckv) RC(enctrials_cross_kv(m, g.memory, B * S, g.cross, plan, st));
  else RC(cross_kv(m, g.memory, B * S, g.cross, st));
  if (fused) RC(regroup_cross_values(c, g.cross, B, S, g.cvg[0], st));
  // ids[:, 0] = start and the step counters (greedy_prologue), then the golden scored steps
  HIPCHK(launch_fill_col(g.ids, max_len, B, start, st));
  HIPCHK(launch_zero(g.step, 16, st));
  RC(greedy_steps(m, g, B, S, max_len, st));
  return copy_out(g.ids, g.top_ids, g.top_logp, B, max_len, ids, top_ids, top_logp, st);
}

int32_t qtx_linear_rows_faults(const qtx_row_gemm* a, const qtx_row_fault* tab, int32_t layer,
                               int32_t gemm, void* stream) {
  RowGemmArgs g{};
  RC(row_gemm_args(a, &g));
  if (g.kp != 0 || g.ksplit > 1)
    return fail(QTX_E_UNSUPPORTED, "rows GEMM with a fault table: kp 0 and no K split (kp=%d ksplit=%d)",
                g.kp, g.ksplit);
  hipStream_t st = (hipStream_t)stream;
  if (!tab || g.M <= 0)
    return launched(launch_gemm_row(g, st), "rows GEMM: N=%d K=%d epi=%d", g.N, g.K, g.epi);
  // the kernel trusts every entry's indices: bound them here, whichever launch they name
  std::vector<RowFault> htab((size_t)g.M);
  for (int r = 0; r < g.M; ++r) {
    const qtx_row_fault& f = tab[r];
    auto bad = [&](const char* what) { return fail(QTX_E_INVALID, "table row %d: fault %s", r, what); };
    if (f.kind < FK_NONE || f.kind > FK_OUTPUT) return bad("kind");
    if (f.kind == FK_INPUT || f.kind == FK_WEIGHT) {
      if (f.bit < 0 || f.bit > 7) return bad("bit");
      if (f.col < 0 || f.col >= g.K) return bad("col");
    }
    if (f.kind == FK_INPUT && (f.lo < 0 || f.lo > f.hi || f.hi > g.N)) return bad("window");
    if (f.kind == FK_WEIGHT && (f.wrow < 0 || f.wrow >= g.N)) return bad("wrow");
    if (f.kind == FK_OUTPUT && (f.col < 0 || f.col >= g.N)) return bad("col");
    RowFault& e = htab[r];
    e.step = 0; e.layer = f.layer; e.gemm = f.gemm; e.kind = f.kind; e.bit = f.bit; e.col = f.col;
    e.wrow = f.wrow; e.lo = f.lo; e.hi = f.hi; e.value = f.value;
  }
  // the table lives in memory of its own for the length of the call
  RowFault* dtab = nullptr;
  HIPCHK(hipMalloc(&dtab, htab.size() * sizeof(RowFault)));
  hipError_t e = hipMemcpy(dtab, htab.data(), htab.size() * sizeof(RowFault), hipMemcpyHostToDevice);
  if (e == hipSuccess) e = launch_gemm_row_tab(g, dtab, layer, gemm, st);
  if (e == hipSuccess) e = hipStreamSynchronize(st);
  (void)hipFree(dtab);
  return launched(e, "rows GEMM with a fault table: N=%d K=%d epi=%d", g.N, g.K, g.epi);
}

}  // extern "C"

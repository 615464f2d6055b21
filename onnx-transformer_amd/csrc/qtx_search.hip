// qtx_search.hip — the beam-search decode with EOS stop (qtx_beam_decode) and the
// teacher-forced target scoring (qtx_score_targets) of the C-ABI (include/qtx.h), with their
// per-op entries.  Both run the encoder once on the B sentences and replicate its cross K/V to
// their rows; the workspaces are carved by qtx_carve.h.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <vector>

#include "qtx_host.h"

namespace qtx {

// The cross K/V of the B sentences in src replicated to K rows each in dst: region r of dst =
// region r / K of src.  vg_src non-null: the values in k_dec_attn's 4-key groups (all layers,
// B * ceil(S / 4) * 4 * D bytes each) into vg_dst[l] in place of the row-major v8.
int replicate_cross(const qtx_config& c, const CrossKV& src, CrossKV& dst, int B, int K, int S,
                    const int8_t* vg_src, const std::vector<int8_t*>& vg_dst, hipStream_t st) {
  const long D = c.d_model, S4 = (S + 3) & ~3;
  for (int l = 0; l < c.n_layers; ++l) {
    HIPCHK(launch_beam_rep(src.k8[l], dst.k8[l], B, K, S * D, st));
    if (vg_src)
      HIPCHK(launch_beam_rep(vg_src + (size_t)l * B * S4 * D, vg_dst[l], B, K, S4 * D, st));
    else
      HIPCHK(launch_beam_rep(src.v8[l], dst.v8[l], B, K, S * D, st));
    HIPCHK(launch_beam_rep(src.sk[l], dst.sk[l], B, K, S * 4L, st));
    HIPCHK(launch_beam_rep(src.sv[l], dst.sv[l], B, K, S * 4L, st));
  }
  return QTX_OK;
}

// What precedes the steps: the encoder and the cross K/V GEMM once on the B sentences, their
// results replicated to the B * K hypotheses, the search state and the first decoder input.
int beam_prologue(const qtx_model* m, BeamWS& w, const int64_t* src, int B, int K, int S,
                  int64_t start, bool fused, hipStream_t st) {
  const qtx_config& c = m->cfg;
  GreedyWS& g = w.g;
  RC(encode_src(m, g, src, w.mask_b, B, S, w.cross_b, fused ? w.cvg_b : nullptr, nullptr, st));
  RC(replicate_cross(c, w.cross_b, g.cross, B, K, S, fused ? w.cvg_b : nullptr, g.cvg, st));
  HIPCHK(launch_beam_rep(w.mask_b, g.mask, B, K, S, st));
  const BeamState& bs = w.tail.st;
  HIPCHK(launch_beam_init(B, K, bs.score, bs.fin, bs.len, bs.parent, g.step, st));
  HIPCHK(launch_fill_col(bs.ids0, 1, B * K, start, st));
  HIPCHK(launch_embed(bs.ids0, 1, B * K, 1, nullptr, 0, m->tgt_lut, c.tgt_vocab, m->pe, c.max_len,
                      g.dec.x, c.d_model, st));
  return QTX_OK;
}

// n more beam steps at the device counter's position, with dfault_steps' path selection: the
// unfused step or eager fused steps (QTX_NO_GRAPH), else captured graphs — one of `big` steps
// when n == big, else n replays of the one-step graph.  One group: no sub-batches.
int beam_steps(const qtx_model* m, BeamWS& w, int R, int S, int max_len, int n, int big,
               bool fused, hipStream_t st) {
  GreedyWS& g = w.g;
  if (!fused) {
    for (int t = 0; t < n; ++t) RC(greedy_step_unfused(m, g, R, S, max_len, nullptr, g.mask, st));
    return QTX_OK;
  }
  // the beam step's own graphs: the select's eos / pad are baked into the captured launch
  const BeamTail& bt = w.tail;
  std::vector<GreedyWS> gv{g};   // one group: the R rows themselves (ids null, anchor g.step)
  StepRequest rq = step_request(m, gv, Groups{1, R}, R, S, max_len, StepForm::Beam);
  rq.key.beam_k = bt.K; rq.key.eos = bt.eos; rq.key.pad = bt.pad;
  const int per = n == big ? big : 1;
  rq.plan = {{per, n / per, -1}};
  return run_steps(m, rq, st);
}

}  // namespace qtx

using namespace qtx;

extern "C" {

size_t qtx_beam_workspace_size(const qtx_model* m, int32_t B, int32_t S, int32_t max_len,
                               int32_t beam) {
  if (!m || B <= 0 || S <= 0 || max_len < 1 || beam < 1 || beam > BEAM_MAXK) return 0;
  return beam_ws(m->cfg, B, beam, S, max_len);
}

int32_t qtx_beam_decode(const qtx_model* m, const int64_t* src, const uint8_t* src_mask,
                        int32_t B, int32_t S, int32_t max_len, int32_t beam, int64_t start,
                        int64_t eos, int64_t pad, int32_t early_exit, int64_t* hyp_ids,
                        float* hyp_score, int32_t* hyp_len, int32_t* steps_run, void* ws,
                        size_t ws_bytes, void* stream) {
  if (!m || !src || !src_mask || !hyp_ids || !hyp_score || !hyp_len || !ws)
    return fail(QTX_E_INVALID, "null argument");
  const qtx_config& c = m->cfg;
  RC(check_decode_shape(c, B, S, max_len));
  if (const int lim = beam_limits(B, beam, c.tgt_vocab, start, eos, pad); lim != QTX_OK)
    return fail(lim, "beam decode: 1 <= beam <= 8, beam <= tgt_vocab, start / eos / pad inside "
                     "the vocabulary, eos != pad, B * beam * tgt_vocab < 2^30 (beam=%d eos=%lld "
                     "pad=%lld)", beam, (long long)eos, (long long)pad);
  if ((long)B * beam * max_len * c.d_model >= (1L << 30))
    return fail(QTX_E_UNSUPPORTED, "beam decode: B * beam * max_len * d_model must be below 2^30");
  RC(refuse_dbg_tail("beam decode"));
  RC(check_workspace(ws_bytes, beam_ws(c, B, beam, S, max_len)));
  hipStream_t st = (hipStream_t)stream;
  CallFrame fr;
  RC(frame_begin(m, ws, ws_bytes, st, true, &fr));
  BeamWS w = carve_beam(fr.ar, c, B, beam, S, max_len);
  w.tail.eos = (int)eos; w.tail.pad = (int)pad;
  const int R = B * beam;
  // every config decodes: the fused step where the greedy decode of R rows would take it
  const bool fused = greedy_fused(c, S, max_len);
  w.tail.grouped = fused;
  w.g.beam = &w.tail;
  w.g.enc.status = fr.status;
  HIPCHK(hipMemcpyAsync(w.mask_b, src_mask, (size_t)B * S, hipMemcpyDeviceToDevice, st));
  RC(beam_prologue(m, w, src, B, beam, S, start, fused, st));
  // the steps in chunks of QTX_GRAPH_STEPS (default 8); with early_exit the rows still live
  // are read back after each chunk (one 4-byte synchronising copy) and the decode stops at 0
  const int total = max_len - 1, big = graph_chunk();
  int run = 0;
  while (run < total) {
    const int n = std::min(big, total - run);
    RC(beam_steps(m, w, R, S, max_len, n, big, fused, st));
    run += n;
    if (early_exit && run < total) {
      int live = 1;
      HIPCHK(hipMemcpyAsync(&live, w.g.step + 3, sizeof(int), hipMemcpyDeviceToHost, st));
      HIPCHK(hipStreamSynchronize(st));
      if (live == 0) break;
    }
  }
  const BeamState& bs = w.tail.st;
  HIPCHK(launch_beam_backtrack(bs.bp_par, bs.bp_tok, B, beam, max_len, run, start, pad, hyp_ids, st));
  HIPCHK(hipMemcpyAsync(hyp_score, bs.score, (size_t)R * sizeof(float), hipMemcpyDeviceToDevice, st));
  HIPCHK(hipMemcpyAsync(hyp_len, bs.len, (size_t)R * sizeof(int), hipMemcpyDeviceToDevice, st));
  if (steps_run) *steps_run = run;
  return QTX_OK;
}

int32_t qtx_beam_select(const qtx_model* m, const float* logits, int32_t B, int32_t beam,
                        int64_t eos, int64_t pad, int32_t max_len, int32_t* step_dev,
                        float* score, int32_t* fin, int32_t* len, int32_t* parent,
                        int32_t* bp_par, int32_t* bp_tok, float* x_next, void* stream) {
  if (!m || !logits || !step_dev || !score || !fin || !len || !parent || !bp_par || !bp_tok ||
      !x_next)
    return fail(QTX_E_INVALID, "null argument");
  if (max_len < 1 || max_len > 512) return fail(QTX_E_INVALID, "max_len %d", max_len);
  if (const int lim = beam_limits(B, beam, m->cfg.tgt_vocab, 0, eos, pad); lim != QTX_OK)
    return fail(lim, "beam select: beam %d, eos %lld, pad %lld, tgt_vocab %d", beam,
                (long long)eos, (long long)pad, m->cfg.tgt_vocab);
  HIPCHK(launch_beam_select(logits, B, beam, m->cfg.tgt_vocab, (int)eos, (int)pad, max_len,
                            step_dev, score, fin, len, parent, bp_par, bp_tok, m->tgt_lut, m->pe,
                            m->cfg.max_len, x_next, (hipStream_t)stream));
  return QTX_OK;
}

int32_t qtx_beam_reorder(int8_t* kc, int8_t* vc, float* skc, float* svc, int32_t B, int32_t beam,
                         int32_t max_len, int32_t n_layers, int64_t k_ls, int64_t v_ls,
                         int64_t s_ls, int32_t v_grouped, const int32_t* step_dev,
                         const int32_t* parent, void* stream) {
  if (!kc || !vc || !skc || !svc || !step_dev || !parent) return fail(QTX_E_INVALID, "null argument");
  if (B <= 0 || beam < 1 || beam > BEAM_MAXK || max_len < 1 || max_len > 512 || n_layers < 1)
    return fail(QTX_E_INVALID, "bad shape B=%d beam=%d max_len=%d layers=%d", B, beam, max_len,
                n_layers);
  const BeamGeom g{max_len, v_grouped ? 1 : 0};
  if (k_ls < (int64_t)B * beam * g.k_row() || v_ls < (int64_t)B * beam * g.v_row() ||
      s_ls < (int64_t)B * beam * g.s_row() || k_ls % 16 || v_ls % 16 || !aligned16(kc) ||
      !aligned16(vc))
    return fail(QTX_E_INVALID, "beam reorder: layer strides below B * beam rows, or codes not "
                               "16-byte aligned");
  HIPCHK(launch_beam_reorder(kc, vc, skc, svc, B, beam, max_len, n_layers, k_ls, v_ls, s_ls,
                             g.grouped, step_dev, parent, (hipStream_t)stream));
  return QTX_OK;
}

}  // extern "C"

// =======================================================================================
// Teacher-forced target scoring (include/qtx.h: qtx_score_targets)
// =======================================================================================
namespace qtx {

// Rows of logits per generator launch that `bytes` of workspace hold: a multiple of 16 (the
// generator's row block) with chunk * V below 2^30 (its 32-bit offsets), at most M; 0 when
// not even 16 rows fit.
int score_chunk(size_t bytes, int V, long M) {
  size_t rows = bytes / (4 * (size_t)V);
  rows = std::min(rows, (size_t)(((1L << 30) - 1) / V)) & ~(size_t)15;
  if (rows < 16) return 0;
  return (int)std::min(rows, (size_t)M);
}

// The generator on x [M, D] (the final LayerNorm already applied) in chunks of `chunk` rows,
// each followed by k_lsm_score on the chunk's logits; label of row g: y[(g / y_t) * y_l + g % y_t].
int score_rows_run(const qtx_model* m, const float* x, long M, const int64_t* y, int y_t, int y_l,
                   float* tok_logp, int* rank, int64_t* top_ids, float* top_logp, float* logits,
                   int chunk, hipStream_t st) {
  const qtx_config& c = m->cfg;
  for (long r0 = 0; r0 < M; r0 += chunk) {
    const int n = (int)std::min((long)chunk, M - r0);
    HIPCHK(launch_generator_mfma(x + r0 * c.d_model, c.d_model, n, nullptr, nullptr, m->gen_wt,
                                 m->gen_b, c.tgt_vocab, logits, st));
    HIPCHK(launch_lsm_score(logits, n, c.tgt_vocab, y, r0, y_t, y_l, tok_logp, rank, top_ids,
                            top_logp, st));
  }
  return QTX_OK;
}

}  // namespace qtx

extern "C" {

size_t qtx_score_workspace_size(const qtx_model* m, int32_t B, int32_t S, int32_t L,
                                int32_t tgt_per_src, int32_t n_faults) {
  if (!m || B <= 0 || S <= 0 || L < 2 || tgt_per_src < 1 || n_faults < 0) return 0;
  return score_ws(m->cfg, B, S, L, tgt_per_src, n_faults);
}

int32_t qtx_score_targets(const qtx_model* m, const int64_t* src, const uint8_t* src_mask,
                          int32_t B, int32_t S, const int64_t* tgt, int32_t L,
                          int32_t tgt_per_src, int64_t pad, const qtx_fault* faults,
                          int32_t n_faults, float* tok_logp, int32_t* rank, int64_t* top_ids,
                          float* top_logp, void* ws, size_t ws_bytes, void* stream) {
  if (!m || !src || !src_mask || !tgt || !tok_logp || !rank || !ws)
    return fail(QTX_E_INVALID, "null argument");
  RC(check_top_pair(top_ids, top_logp));
  const qtx_config& c = m->cfg;
  const int K = tgt_per_src, T = L - 1;
  if (bad_decode_shape(c, B, S, T) || K < 1)
    return fail(QTX_E_INVALID, "bad shape B=%d S=%d L=%d tgt_per_src=%d", B, S, L, K);
  RC(check_top2_vocab(c));
  if (n_faults < 0 || (n_faults > 0 && !faults))
    return fail(QTX_E_INVALID, "n_faults %d without a fault array", n_faults);
  const long Rl = (long)B * K;
  if (Rl * T * c.d_model >= (1L << 30))
    return fail(QTX_E_UNSUPPORTED, "target scoring: B * tgt_per_src * (L - 1) * d_model must be "
                                   "below 2^30");
  if (n_faults > 0) {
    RC(check_fault_bits(c));
    if (K != 1) return fail(QTX_E_UNSUPPORTED, "fault trials need tgt_per_src == 1 (%d)", K);
    for (int n = 0; n < n_faults; ++n) {
      const qtx_fault* f = faults + n;
      if (f->kind == QTX_FAULT_NONE) return fail(QTX_E_INVALID, "fault %d: kind NONE", n);
      if (f->module == 0) RC(check_fault(m, f, 0, B, S, 0));
      else if (f->module == 1) RC(check_fault(m, f, 1, B, T, S));
      else return fail(QTX_E_INVALID, "fault %d: module %d", n, f->module);
    }
  }
  RC(check_workspace(ws_bytes, score_ws(c, B, S, L, K, n_faults)));
  hipStream_t st = (hipStream_t)stream;
  CallFrame fr;
  RC(frame_begin(m, ws, ws_bytes, st, true, &fr));
  ScoreWS w = carve_score(fr.ar, c, B, S, L, K, n_faults);
  w.enc.status = fr.status;
  const int D = c.d_model, R = (int)Rl, Ms = B * S;
  const long M = (long)R * T;
  auto embed_src = [&]() -> int {
    HIPCHK(launch_embed(src, S, B, S, nullptr, 0, m->src_lut, c.src_vocab, m->pe, c.max_len,
                        w.enc.x, (long)S * D, st));
    return QTX_OK;
  };
  // the golden encoder pass and cross K/V, once on the B sentences (greedy_prologue's)
  RC(embed_src());
  RC(encoder_run(m, w.enc.x, src_mask, B, S, w.memory, w.enc, st, nullptr));
  RC(cross_kv(m, w.memory, Ms, w.cross, st));
  const CrossKV* gx = &w.cross;
  const uint8_t* rmask = src_mask;
  if (K > 1) {   // row r reads the cross K/V and the source mask of sentence r / K
    RC(replicate_cross(c, w.cross, w.rcross, B, K, S, nullptr, {}, st));
    HIPCHK(launch_beam_rep(src_mask, w.rmask, B, K, S, st));
    gx = &w.rcross;
    rmask = w.rmask;
  }
  long tm_bs = 0;
  if (pad >= 0) {
    HIPCHK(launch_std_mask(tgt, R, L, pad, w.tmask, st));
    tm_bs = (long)T * T;
  } else {
    HIPCHK(launch_causal_mask(w.tmask, T, st));
  }
  for (int n = 0; n <= n_faults; ++n) {   // trial 0 golden, trial n: faults[n - 1]
    const qtx_fault* f = n ? faults + n - 1 : nullptr;
    const CrossKV* x = gx;
    if (f && f->module == 0) {   // the encoder and the cross K/V again, into the trial's own buffers
      RC(embed_src());
      RC(encoder_run(m, w.enc.x, src_mask, B, S, w.fmemory, w.enc, st, f));
      RC(cross_kv(m, w.fmemory, Ms, w.fcross, st));
      x = &w.fcross;
      f = nullptr;
    } else if (ckv_fault(m, f, Ms)) {   // a memory K / V projection fault: its own cross copy
      RC(cross_kv(m, w.memory, Ms, w.fcross, st, f));
      x = &w.fcross;
    }
    HIPCHK(launch_embed(tgt, L, R, T, nullptr, 0, m->tgt_lut, c.tgt_vocab, m->pe, c.max_len,
                        w.dec.x, (long)T * D, st));
    RC(decoder_body(m, w.dec, *x, rmask, w.tmask, tm_bs, R, T, S, w.out, f, st));
    const long o = (long)n * M;
    RC(score_rows_run(m, w.out, M, tgt + 1, T, L, tok_logp + o, rank + o,
                      top_ids ? top_ids + 2 * o : nullptr, top_logp ? top_logp + 2 * o : nullptr,
                      w.logits, score_chunk(w.logits_bytes, c.tgt_vocab, M), st));
  }
  return QTX_OK;
}

int32_t qtx_score_logits(const float* logits, const int64_t* y, int32_t M, int32_t V,
                         float* tok_logp, int32_t* rank, int64_t* top_ids, float* top_logp,
                         void* stream) {
  if (!logits || !y || !tok_logp || !rank) return fail(QTX_E_INVALID, "null argument");
  RC(check_top_pair(top_ids, top_logp));
  if (V < 2) return fail(QTX_E_INVALID, "scoring needs V >= 2 (%d)", V);
  if (M <= 0) return QTX_OK;
  HIPCHK(launch_lsm_score(logits, M, V, y, 0, 1, 1, tok_logp, rank, top_ids, top_logp,
                          (hipStream_t)stream));
  return QTX_OK;
}

int32_t qtx_score_rows(const qtx_model* m, const float* x, int32_t M, const int64_t* y,
                       float* tok_logp, int32_t* rank, int64_t* top_ids, float* top_logp,
                       void* ws, size_t ws_bytes, void* stream) {
  if (!m || !x || !y || !tok_logp || !rank || !ws) return fail(QTX_E_INVALID, "null argument");
  RC(check_top_pair(top_ids, top_logp));
  const int V = m->cfg.tgt_vocab;
  if (V < 2) return fail(QTX_E_INVALID, "scoring needs tgt_vocab >= 2 (%d)", V);
  if (M <= 0) return QTX_OK;
  if ((long)M * m->cfg.d_model >= (1L << 30))
    return fail(QTX_E_UNSUPPORTED, "score rows: M * d_model must be below 2^30");
  const int chunk = score_chunk(ws_bytes, V, M);
  if (!chunk) return fail(QTX_E_WORKSPACE, "ws holds fewer than 16 rows of logits");
  return score_rows_run(m, x, M, y, 1, 1, tok_logp, rank, top_ids, top_logp, (float*)ws, chunk,
                        (hipStream_t)stream);
}

}  // extern "C"

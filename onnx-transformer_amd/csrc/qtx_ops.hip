// qtx_ops.hip — the per-op and debug entry points of the C-ABI (include/qtx.h): one kernel
// launcher each, behind the argument checks that keep its vector loads and stores in bounds.
#include <hip/hip_runtime.h>

#include <cstdarg>
#include <cstdio>
#include <mutex>

#include "qtx_host.h"

namespace qtx {

// A launcher's result as the entry's: hipErrorInvalidValue is the launchers' "shape not
// supported" (QTX_E_UNSUPPORTED with the entry's own text), any other failure a HIP error.
__attribute__((format(printf, 2, 3))) int launched(hipError_t e, const char* fmt, ...) {
  if (e == hipSuccess) return QTX_OK;
  if (e != hipErrorInvalidValue) return fail(QTX_E_HIP, "launch: %s", hipGetErrorString(e));
  char buf[512];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof(buf), fmt, ap);
  va_end(ap);
  return fail(QTX_E_UNSUPPORTED, "%s", buf);
}

// Dense attention operands: q [B, Sq, D], k / v [B, Sk, D] with their per-token scales,
// D = 64 H, ctx [B, Sq, D]
AttnArgs dense_attn_args(const int8_t* q, const float* sq, const int8_t* k, const float* sk,
                         const int8_t* v, const float* sv, const uint8_t* mask, long m_bs,
                         long m_is, int B, int H, int Sq, int Sk, float* ctx, int dec) {
  const long D = (long)H * 64;
  AttnArgs a{};
  a.q = q; a.q_bs = Sq * D; a.q_ld = D; a.sq = sq; a.sq_bs = Sq;
  a.k = k; a.k_bs = Sk * D; a.k_ld = D; a.sk = sk; a.sk_bs = Sk;
  a.v = v; a.v_bs = Sk * D; a.v_ld = D; a.sv = sv; a.sv_bs = Sk;
  a.mask = mask; a.m_bs = m_bs; a.m_is = m_is;
  a.ctx = ctx; a.c_bs = Sq * D; a.c_ld = D;
  a.B = B; a.H = H; a.Sq = Sq; a.Sk = Sk;
  a.dec = dec != 0;
  return a;
}

// qtx_row_gemm as the kernels' RowGemmArgs, with every argument rule of qtx_linear_rows
int row_gemm_args(const qtx_row_gemm* a, RowGemmArgs* g) {
  if (!a || !a->A || !a->sa || !a->W || !a->sw || !a->bias) return fail(QTX_E_INVALID, "null argument");
  g->A = a->A; g->lda = a->K; g->sa = a->sa; g->W = a->W; g->ldw = a->K; g->sw = a->sw;
  g->bias = a->bias; g->M = a->M; g->N = a->N; g->K = a->K; g->epi = a->epi;
  g->out8 = a->out8; g->ldo8 = a->ldo8; g->o8_ts = a->o8_ts; g->os = a->os; g->os_ts = a->os_ts;
  g->res = a->res; g->xout = a->xout; g->ln_a = a->ln_a; g->ln_b = a->ln_b;
  g->lnq = a->lnq; g->lns = a->lns; g->lnout = a->lnout;
  g->pmax_out = a->pmax_out; g->pmax_in = a->pmax_in; g->pmax_n = a->pmax_n; g->kp = a->kp;
  g->status = reinterpret_cast<unsigned*>(a->status);
  g->part = a->part; g->ksplit = a->ksplit;
  if (g->ksplit > 1 && (g->epi != RE_RES_LN || g->kp != 1 || !g->part || (g->ksplit & (g->ksplit - 1)) ||
                       g->ksplit > 8))
    return fail(QTX_E_INVALID, "ksplit %d: epi 1 with kp 1, a power of two <= 8, and part", g->ksplit);
  if (g->ksplit > 1 && (g->K % 64 || (g->K / 64) % (4 * g->ksplit)))   // launch_gemm_row's split
    return fail(QTX_E_INVALID, "ksplit %d needs K / 64 a multiple of 4 * ksplit (K=%d)", g->ksplit, g->K);
  const bool ok = (g->epi == RE_QUANT && g->out8 && g->os) ||
                  (g->epi == RE_RES_LN && g->res && g->xout && g->ln_a && g->ln_b &&
                   (g->lnq ? g->lns != nullptr : g->lnout != nullptr)) ||
                  (g->epi == RE_RELU_PMAX && g->pmax_out) ||
                  (g->epi == RE_RELU_QUANT_PMAX && g->out8 && g->os &&
                   (g->kp == 3 || g->kp == 5 ? g->pmax_out != nullptr : (g->pmax_in && g->pmax_n > 0)));
  if (!ok) return fail(QTX_E_INVALID, "operands missing for epi %d", g->epi);
  // A, W and out8 move in 16-byte vectors (k_gemm_row: plain stores; the WS kernels: buffer
  // stores through a descriptor of M * ldo8 bytes), so their bases and the out8 strides must
  // be multiples of 16 and a row must hold its tile — checked here, before any launch
  if (!aligned16(g->A) || !aligned16(g->W))
    return fail(QTX_E_INVALID, "A / W must be 16-byte aligned");
  if (g->epi == RE_QUANT || g->epi == RE_RELU_QUANT_PMAX) {
    const long row = g->epi == RE_QUANT ? 512 : g->N;
    if (!aligned16(g->out8) || g->ldo8 < row || g->ldo8 % 16 || (g->kp && g->epi != RE_QUANT && g->ldo8 % 64))
      return fail(QTX_E_INVALID, "out8 must be 16-byte aligned with ldo8 %% 16 == 0 (KP: %% 64) "
                                 "and ldo8 >= %ld (ldo8=%ld)", row, (long)g->ldo8);
    if (g->epi == RE_QUANT && (g->o8_ts % 16 || g->o8_ts < 0 || g->os_ts < 0))
      return fail(QTX_E_INVALID, "o8_ts must be a non-negative multiple of 16, os_ts >= 0 "
                                 "(o8_ts=%ld os_ts=%ld)", (long)g->o8_ts, (long)g->os_ts);
  }
  return QTX_OK;
}

}  // namespace qtx

using namespace qtx;

extern "C" {

int32_t qtx_embed(const qtx_model* m, int32_t which, const int64_t* ids, int32_t B, int32_t T,
                  int32_t pos0, float* out, void* stream) {
  if (!m || !ids || !out) return fail(QTX_E_INVALID, "null argument");
  if (pos0 < 0 || pos0 + T > m->cfg.max_len)
    return fail(QTX_E_INVALID, "positions exceed max_len %d", m->cfg.max_len);
  const float* lut = which ? m->tgt_lut : m->src_lut;
  const int vocab = which ? m->cfg.tgt_vocab : m->cfg.src_vocab;
  HIPCHK(launch_embed(ids, T, B, T, nullptr, pos0, lut, vocab, m->pe, m->cfg.max_len, out,
                      (long)T * m->cfg.d_model, (hipStream_t)stream));
  return QTX_OK;
}

int32_t qtx_generator(const qtx_model* m, const float* x, int32_t M, float* logp,
                      int64_t* ids, void* ws, size_t ws_bytes, void* stream) {
  if (!m || !x || !ws) return fail(QTX_E_INVALID, "null argument");
  const int V = m->cfg.tgt_vocab;
  if (ws_bytes < (size_t)M * V * sizeof(float)) return fail(QTX_E_WORKSPACE, "ws too small");
  hipStream_t st = (hipStream_t)stream;
  float* logits = (float*)ws;   // the raw logits stay in ws[0 .. M*V) for the caller
  HIPCHK(launch_generator_mfma(x, m->cfg.d_model, M, nullptr, nullptr, m->gen_wt, m->gen_b, V,
                               logits, st));
  HIPCHK(launch_logsoftmax_argmax(logits, M, V, logp, ids, 1, nullptr, 0, st));
  return QTX_OK;
}

int32_t qtx_generator_top2(const qtx_model* m, const float* x, int32_t M, int64_t* top_ids,
                           float* top_logp, void* ws, size_t ws_bytes, void* stream) {
  if (!m || !x || !top_ids || !top_logp || !ws) return fail(QTX_E_INVALID, "null argument");
  const int V = m->cfg.tgt_vocab;
  RC(check_top2_vocab(m->cfg));
  if (M <= 0) return QTX_OK;
  if (ws_bytes < (size_t)M * V * sizeof(float)) return fail(QTX_E_WORKSPACE, "ws too small");
  hipStream_t st = (hipStream_t)stream;
  float* logits = (float*)ws;   // the raw logits stay in ws[0 .. M*V) for the caller
  HIPCHK(launch_generator_mfma(x, m->cfg.d_model, M, nullptr, nullptr, m->gen_wt, m->gen_b, V,
                               logits, st));
  HIPCHK(launch_logsoftmax_top2(logits, M, V, nullptr, 0, nullptr, 0, top_ids, top_logp, 1, st));
  return QTX_OK;
}

// ---- per-op entry points ---------------------------------------------------------------
int32_t qtx_row_quant(const float* x, int32_t rows, int32_t D, float qmax, int8_t* q,
                      float* s, void* stream) {
  if (!x || !q || !s) return fail(QTX_E_INVALID, "null argument");
  RowArgs a = rows_quant(x, D, rows, D, q, s);
  a.qmax = qmax;
  return launched(launch_rows(a, (hipStream_t)stream), "D=%d unsupported", D);
}

int32_t qtx_layernorm_quant(const float* x, const float* a, const float* b, int32_t rows,
                            int32_t D, float* y, int8_t* q, float* s, void* stream) {
  if (!x || !a || !b || (!y && !q)) return fail(QTX_E_INVALID, "null argument");
  RowArgs r{};
  r.x = x; r.ldx = D; r.rows = rows; r.D = D; r.ln_a = a; r.ln_b = b;
  r.yout = y; r.ldy = D; r.q = q; r.ldq = D; r.s = s; r.qmax = 127.0f;
  r.rpb = rows > 0 ? rows : 1;
  return launched(launch_rows(r, (hipStream_t)stream), "D=%d unsupported", D);
}

int32_t qtx_linear_i8(const int8_t* A, const float* sa, const void* W, const float* sw,
                      const float* bias, int32_t M, int32_t N, int32_t K, int32_t weight_bits,
                      int32_t flags, const float* res, float* out, void* stream) {
  if (!A || !sa || !W || !sw || !bias || !out) return fail(QTX_E_INVALID, "null argument");
  if ((flags & EPI_RESIDUAL) && !res) return fail(QTX_E_INVALID, "residual flag without res");
  if (K % 64) return fail(QTX_E_UNSUPPORTED, "K=%d not a multiple of 64", K);
  GemmArgs g{};
  g.A = A; g.lda = K; g.sa = sa; g.W = (const int8_t*)W;
  g.ldw = weight_bits == 8 ? K : K / 2; g.sw = sw; g.bias = bias;
  g.out = out; g.ldo = N; g.res = res; g.ldr = N;
  g.M = M; g.N = N; g.K = K; g.flags = flags;
  return launched(launch_gemm(g, weight_bits, (hipStream_t)stream), "weight_bits=%d", weight_bits);
}

int32_t qtx_linear_rows(const qtx_row_gemm* a, void* stream) {
  RowGemmArgs g{};
  RC(row_gemm_args(a, &g));
  return launched(g.kp == 3 || g.kp == 5 ? launch_gemm_wsx(g, (hipStream_t)stream)
                       : g.kp == 2 || g.kp == 4 ? launch_gemm_ws(g, (hipStream_t)stream)
                                   : launch_gemm_row(g, (hipStream_t)stream),
                  "rows GEMM: N=%d K=%d epi=%d kp=%d", g.N, g.K, g.epi, g.kp);
}

int32_t qtx_pack_w_kp(const int8_t* W, int32_t N, int32_t K, int8_t* out, void* stream) {
  if (!W || !out) return fail(QTX_E_INVALID, "null argument");
  return launched(launch_pack_w_kp(W, N, K, out, (hipStream_t)stream), "pack_w_kp N=%d K=%d", N, K);
}

int32_t qtx_ffn_rows(const qtx_ffn_args* a, void* stream) {
  if (!a || !a->A || !a->sa || !a->wf || !a->sw1 || !a->b1 || !a->sw2 || !a->b2 || !a->x ||
      !a->ln_a || !a->ln_b || (a->lnq ? !a->lns : !a->lnout))
    return fail(QTX_E_INVALID, "null argument");
  FfnArgs g{};
  g.A = a->A; g.sa = a->sa; g.wf = a->wf; g.sw1 = a->sw1; g.b1 = a->b1; g.sw2 = a->sw2;
  g.b2 = a->b2; g.x = a->x; g.ln_a = a->ln_a; g.ln_b = a->ln_b; g.lnq = a->lnq;
  g.lns = a->lns; g.lnout = a->lnout; g.M = a->M; g.F = a->F;
  return launched(launch_ffn_fused(g, (hipStream_t)stream), "ffn_rows: F=%d", a->F);
}

int32_t qtx_pack_ffn(const int8_t* W1, const int8_t* W2, int32_t F, int8_t* out, void* stream) {
  if (!W1 || !W2 || !out) return fail(QTX_E_INVALID, "null argument");
  return launched(launch_pack_ffn(W1, W2, F, out, (hipStream_t)stream), "pack_ffn F=%d", F);
}

int32_t qtx_pack_w_ws(const int8_t* W, int32_t N, int32_t K, int8_t* out, void* stream) {
  if (!W || !out) return fail(QTX_E_INVALID, "null argument");
  return launched(launch_pack_w_ws(W, N, K, out, (hipStream_t)stream), "pack_w_ws N=%d K=%d", N, K);
}

int32_t qtx_skinny_linear(int32_t amode, const int8_t* A, const float* sa, const float* X,
                          int64_t ldx, const float* ln_a, const float* ln_b,
                          const float* pmax_in, int32_t pmax_n, const void* W, const float* sw,
                          const float* bias, int32_t M, int32_t N, int32_t K,
                          int32_t weight_bits, int32_t flags, const float* res, float* out,
                          float* pmax_out, void* stream) {
  if (!W || !sw || !bias || !out) return fail(QTX_E_INVALID, "null argument");
  if ((amode == A_I8 && (!A || !sa)) || (amode == A_LN && (!X || !ln_a || !ln_b)) ||
      (amode == A_F32Q && (!X || !pmax_in || pmax_n <= 0 || pmax_n > 128)) ||
      (amode == A_F32R && !X) || amode < 0 || amode > 3)
    return fail(QTX_E_INVALID, "operands missing for amode %d", amode);
  if (((flags & EPI_RESIDUAL) && !res) || ((flags & EPI_ROWMAX) && !pmax_out))
    return fail(QTX_E_INVALID, "flags need res / pmax_out");
  // the A / X rows and the W fragments are read in 16-byte vectors (8-byte for 4-bit W)
  if (!aligned16(W) || (amode == A_I8 ? !aligned16(A) : (!aligned16(X) || ldx < K || ldx % 4)))
    return fail(QTX_E_INVALID, "skinny: A / X / W must be 16-byte aligned, ldx %% 4 == 0 and "
                               "ldx >= K (ldx=%ld)", (long)ldx);
  SkinnyArgs g{};
  g.amode = amode; g.A = A; g.sa = sa; g.X = X; g.ldx = ldx; g.ln_a = ln_a; g.ln_b = ln_b;
  g.pmax_in = pmax_in; g.pmax_n = pmax_n;
  g.W = (const int8_t*)W; g.ldw = weight_bits == 8 ? K : K / 2;
  g.sw = sw; g.bias = bias; g.out = out; g.ldo = N; g.res = res; g.ldr = N;
  g.pmax_out = pmax_out; g.M = M; g.N = N; g.K = K; g.flags = flags;
  return launched(launch_skinny(g, weight_bits, (hipStream_t)stream),
                  "skinny: N=%d K=%d amode=%d bits=%d", N, K, amode, weight_bits);
}

int32_t qtx_decode_attention(int32_t kv_new, const float* y, int64_t ldy, int8_t* kc,
                             int8_t* vc, float* skc, float* svc, int32_t kv_bs,
                             const int32_t* step_dev, int32_t S, const uint8_t* mask,
                             int32_t B, float* ctx, float* pmax, void* stream) {
  if (!y || !kc || !vc || !skc || !svc || !ctx || !pmax)
    return fail(QTX_E_INVALID, "null argument");
  if (kv_new ? (!step_dev || kv_bs <= 0 || kv_bs > 128)
             : (!mask || S <= 0 || S > 128 || S > kv_bs))
    return fail(QTX_E_INVALID, "decode attention: bad step/mask/S/kv_bs");
  // y rows and the cached key / value rows are read in 16-byte vectors
  if (!aligned16(y) || !aligned16(kc) || !aligned16(vc) || ldy % 4 || ldy < (kv_new ? 1536 : 512))
    return fail(QTX_E_INVALID, "decode attention: y / kc / vc must be 16-byte aligned, "
                               "ldy %% 4 == 0 and ldy >= the row width (ldy=%ld)", (long)ldy);
  DecAttnArgs a{};
  a.y = y; a.ldy = ldy; a.kc = kc; a.vc = vc; a.skc = skc; a.svc = svc; a.kv_bs = kv_bs;
  a.step = step_dev; a.S = S; a.mask = mask; a.kv_new = kv_new;
  a.ctx = ctx; a.pmax = pmax; a.B = B;
  HIPCHK(launch_dec_attn(a, B, (hipStream_t)stream));
  return QTX_OK;
}

int32_t qtx_debug_graph_stats(const qtx_model* m, int32_t* entries, int64_t* captures) {
  if (!m || !entries || !captures) return fail(QTX_E_INVALID, "null argument");
  qtx_model* mm = const_cast<qtx_model*>(m);
  std::lock_guard<std::mutex> lock(mm->mu);
  *entries = (int32_t)mm->sg.entries();
  *captures = mm->sg.captures();
  return QTX_OK;
}

int32_t qtx_debug_nop(void* stream) {
  HIPCHK(launch_nop((hipStream_t)stream));
  return QTX_OK;
}

int32_t qtx_decode_generator(const qtx_model* m, const float* x, int32_t M, float* logits,
                             float* rec, void* stream) {
  if (!m || !x || !logits) return fail(QTX_E_INVALID, "null argument");
  if (M <= 0) return QTX_OK;
  if (!aligned16(x) || (rec && !aligned16(rec)))
    return fail(QTX_E_INVALID, "x / rec must be 16-byte aligned");
  return launched(launch_generator_mfma(x, m->cfg.d_model, M, m->dec_norm[0], m->dec_norm[1],
                                             m->gen_wt, m->gen_b, m->cfg.tgt_vocab, logits,
                                             (hipStream_t)stream, rec),
                  "M * tgt_vocab >= 2^30");
}

int32_t qtx_decode_argmax_embed(const qtx_model* m, const float* logits, int32_t M,
                                int64_t* ids, int64_t ids_bs, int32_t* step_dev,
                                float* x_next, void* stream) {
  if (!m || !logits || !ids || !step_dev || !x_next) return fail(QTX_E_INVALID, "null argument");
  if (M <= 0) return QTX_OK;
  const qtx_config& c = m->cfg;
  return launched(launch_argmax_embed(logits, M, c.tgt_vocab, ids, ids_bs, step_dev,
                                           reinterpret_cast<unsigned*>(step_dev + 1),
                                           m->tgt_lut, m->pe, c.max_len, x_next,
                                           (hipStream_t)stream),
                  "tgt_vocab %d", c.tgt_vocab);
}

int32_t qtx_decode_top2_embed(const qtx_model* m, const float* logits, int32_t M, int64_t* ids,
                              int64_t ids_bs, int64_t* top_ids, float* top_logp,
                              int32_t* step_dev, float* x_next, void* stream) {
  if (!m || !logits || !ids || !top_ids || !top_logp || !step_dev || !x_next)
    return fail(QTX_E_INVALID, "null argument");
  const qtx_config& c = m->cfg;
  RC(check_top2_vocab(c));
  if (M <= 0) return QTX_OK;
  return launched(launch_top2_embed(logits, M, c.tgt_vocab, ids, ids_bs, top_ids, top_logp,
                                         step_dev, reinterpret_cast<unsigned*>(step_dev + 1),
                                         m->tgt_lut, m->pe, c.max_len, x_next,
                                         (hipStream_t)stream),
                  "tgt_vocab %d", c.tgt_vocab);
}

int32_t qtx_pack_int4(const int8_t* q, int32_t N, int32_t K, uint8_t* packed, void* stream) {
  if (!q || !packed || K % 2) return fail(QTX_E_INVALID, "bad argument");
  HIPCHK(launch_pack_int4(q, N, K, packed, (hipStream_t)stream));
  return QTX_OK;
}

int32_t qtx_attention_trace(const int8_t* q, const float* sq, const int8_t* k, const float* sk,
                            const int8_t* v, const float* sv, const uint8_t* mask, int64_t m_bs,
                            int64_t m_is, int32_t B, int32_t H, int32_t Sq, int32_t Sk,
                            float* ctx, float* qk_acc, float* p_codes, int32_t dec, void* stream) {
  if (!q || !sq || !k || !sk || !v || !sv || !ctx) return fail(QTX_E_INVALID, "null argument");
  if (Sk <= 0 || Sk > 512 || Sq <= 0 || B <= 0 || H <= 0)
    return fail(QTX_E_UNSUPPORTED, "Sk=%d (max 512) Sq=%d B=%d H=%d", Sk, Sq, B, H);
  const AttnArgs a = dense_attn_args(q, sq, k, sk, v, sv, mask, m_bs, m_is, B, H, Sq, Sk, ctx, dec);
  HIPCHK(launch_attn_trace(a, qk_acc, p_codes, (hipStream_t)stream));
  return QTX_OK;
}

int32_t qtx_attention_i8_quant(const int8_t* q, const float* sq, const int8_t* k,
                               const float* sk, const int8_t* v, const float* sv,
                               const uint8_t* key_mask, int32_t B, int32_t S, int8_t* ctx8,
                               float* sctx, void* stream) {
  if (!q || !sq || !k || !sk || !v || !sv || !ctx8 || !sctx) return fail(QTX_E_INVALID, "null argument");
  if (B <= 0 || S <= 0 || S > 128) return fail(QTX_E_UNSUPPORTED, "S=%d (1..128)", S);
  const AttnArgs a = dense_attn_args(q, sq, k, sk, v, sv, key_mask, S, 0, B, 8, S, S, nullptr, 0);
  HIPCHK(launch_attention_encq(a, ctx8, sctx, (hipStream_t)stream, true));
  return QTX_OK;
}

int32_t qtx_attention_i8(const int8_t* q, const float* sq, const int8_t* k, const float* sk,
                         const int8_t* v, const float* sv, const uint8_t* mask, int64_t m_bs,
                         int64_t m_is, int32_t B, int32_t H, int32_t Sq, int32_t Sk,
                         float* ctx, int32_t dec, void* stream) {
  if (!q || !sq || !k || !sk || !v || !sv || !ctx) return fail(QTX_E_INVALID, "null argument");
  if (Sk <= 0 || Sk > 512 || Sq <= 0) return fail(QTX_E_UNSUPPORTED, "Sk=%d (max 512)", Sk);
  const AttnArgs a = dense_attn_args(q, sq, k, sk, v, sv, mask, m_bs, m_is, B, H, Sq, Sk, ctx, dec);
  HIPCHK(launch_attention(a, (hipStream_t)stream));
  return QTX_OK;
}

}  // extern "C"

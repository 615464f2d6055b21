// qtx_api.hip — the stacks and the greedy decode of the C-ABI (include/qtx.h): the building
// blocks over the kernels' launchers (qtx_kernels.h), the fault mapping, the encoder and decoder
// stacks, the fused and unfused KV-cached decode steps, and the encoder / decoder / greedy
// entry points.  The other drivers (qtx_fault.hip, qtx_search.hip) are built from these.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <mutex>
#include <vector>

#include "qtx_host.h"

namespace qtx {

// ---- building blocks ------------------------------------------------------------------
RowArgs rows_quant(const float* x, long ldx, int rows, int D, int8_t* q, float* s) {
  RowArgs a{};
  a.x = x; a.ldx = ldx; a.rows = rows; a.D = D;
  a.q = q; a.ldq = D; a.s = s; a.qmax = 127.0f;
  a.rpb = rows > 0 ? rows : 1; a.dst_bstride = 0; a.dst_off = 0;
  return a;
}

int ln_quant(const float* x, int rows, const float* const* ln, int D, int8_t* q, float* s,
             hipStream_t st, bool kp) {
  RowArgs a = rows_quant(x, D, rows, D, q, s);
  a.ln_a = ln[0]; a.ln_b = ln[1]; a.kp = kp;
  HIPCHK(launch_rows(a, st));
  return QTX_OK;
}

int ln_out(const float* x, int rows, const float* const* ln, int D, float* y, hipStream_t st) {
  RowArgs a{};
  a.x = x; a.ldx = D; a.rows = rows; a.D = D; a.ln_a = ln[0]; a.ln_b = ln[1];
  a.yout = y; a.ldy = D; a.rpb = rows > 0 ? rows : 1;
  HIPCHK(launch_rows(a, st));
  return QTX_OK;
}

int quant(const float* x, long ldx, int rows, int D, int8_t* q, float* s, hipStream_t st,
          bool kp) {
  RowArgs a = rows_quant(x, ldx, rows, D, q, s);
  a.kp = kp;
  HIPCHK(launch_rows(a, st));
  return QTX_OK;
}

int linear(const qtx_config& c, const QLin& L, const int8_t* a8, const float* sa, int M,
           int flags, const float* res, float* out, long ldo, hipStream_t st,
           const FaultArgs& fa) {
  GemmArgs g{};
  g.fault = fa;
  g.A = a8; g.lda = L.K; g.sa = sa;
  const int wb = L.q8 ? 8 : c.weight_bits;
  g.W = L.w8(); g.ldw = wb == 8 ? L.K : L.K / 2; g.sw = L.s; g.bias = L.b;
  g.out = out; g.ldo = ldo; g.res = res; g.ldr = ldo;
  g.M = M; g.N = L.N; g.K = L.K; g.flags = flags;
  HIPCHK(launch_gemm(g, wb, st));
  return QTX_OK;
}

// Row-complete GEMM (k_gemm_row) for 8-bit weights: epilogues of whole 512-wide rows.
bool row_path(const qtx_config& c) {   // (4-bit models: on the unpacked int8 weights)
  return c.d_ff % 512 == 0 && !knobs().no_rowgemm;
}
// kp: A (a8) in the KP layout and W from L.qkp; the int8 lnq / FFN-hidden outputs are
// then written KP as well (RE_QUANT's q8 stays row-major: attention reads it).
// With kp, a K = 512 GEMM over many rows runs weight-stationary (kp = 2, W from L.qws):
// each workgroup keeps a 512-column slice of W on chip (qtx_wsgemm.hip); below ws_min_m
// rows the per-workgroup W load is not amortized and the row GEMM is faster.
// Measured (tools/enc_small.py, the greedy decode's encoder): at M = 2304 (B = 32, S = 72)
// the Q/K/V and FFN1 launches on the weight-stationary kernel took the encoder 0.83 ->
// 0.73 ms (the row GEMM's 128-row tiles give 18 workgroups).  The O-projection's residual +
// LayerNorm epilogue runs weight-stationary only between ws_res_min_m and ws_res_max_m
// (above it the KP row GEMM is faster).  QTX_WS_MIN_M / QTX_WS_RES_MIN_M / _MAX_M: A/B.
long ws_min_m() { return knobs().ws_min_m; }
bool ws_res_ok(long M) { return M >= knobs().ws_res_min_m && M < knobs().ws_res_max_m; }
RowGemmArgs rowgemm(const QLin& L, const int8_t* a8, const float* sa, int M, int epi,
                    bool kp = false) {
  RowGemmArgs g{};
  const bool ws = kp && L.qws && L.K == 512 &&
                  (epi == RE_RES_LN ? ws_res_ok(M) : M >= ws_min_m());
  // Q/K/V on the 32x32x32 MFMA kernel (diagnostic build, QTX_WS32)
  const bool ws32 = ws && epi == RE_QUANT && L.qws32 && knobs().ws32;
  g.A = a8; g.lda = L.K; g.sa = sa; g.W = ws32 ? L.qws32 : ws ? L.qws : kp ? L.qkp : L.w8();
  g.ldw = L.K;
  g.sw = L.s; g.bias = L.b;
  g.M = M; g.N = L.N; g.K = L.K; g.epi = epi; g.kp = ws32 ? 4 : ws ? 2 : kp;
  return g;
}
hipError_t launch_row_gemm_any(const RowGemmArgs& g, hipStream_t st) {
  return g.kp == 2 || g.kp == 4 ? launch_gemm_ws(g, st) : launch_gemm_row(g, st);
}
// out = per-token quantized (a8 . W^T) per 512-wide tile into out8 + t*M*512, os + t*M
int row_quant(const QLin& L, const int8_t* a8, const float* sa, int M, int8_t* out8,
              float* os, hipStream_t st, const FaultArgs& fa = FaultArgs{}, bool kp = false,
              void* zero = nullptr, long zero16 = 0) {
  RowGemmArgs g = rowgemm(L, a8, sa, M, RE_QUANT, kp);
  g.fault = fa;
  g.zero = zero; g.zero16 = zero16;   // a side job (launch_gemm_ws), else a zeroing kernel
  g.out8 = out8; g.ldo8 = 512; g.o8_ts = (long)M * 512; g.os = os; g.os_ts = M;
  HIPCHK(launch_row_gemm_any(g, st));
  return QTX_OK;
}
// x += a8 . W^T, then LayerNorm(x) (ln) quantized into (lnq, lns) or fp32 into lnout
// part: scratch for split-K partials (>= 4 * M * 2 KB; the FFN2 call sites pass the fp32
// GEMM scratch, free by then).  A KP row GEMM over at most 64 row tiles (FFN2 at the decode
// encoder's M = 2304: 18 workgroups, 43.9 us) runs K split 4 ways + a row-wise epilogue.
int row_res_ln(const QLin& L, const int8_t* a8, const float* sa, int M, float* x,
               const float* const* ln, int8_t* lnq, float* lns, float* lnout, hipStream_t st,
               const FaultArgs& fa = FaultArgs{}, bool kp = false, float* part = nullptr) {
  RowGemmArgs g = rowgemm(L, a8, sa, M, RE_RES_LN, kp);
  g.fault = fa;
  g.res = x; g.xout = x; g.ln_a = ln[0]; g.ln_b = ln[1];
  g.lnq = lnq; g.lns = lns; g.lnout = lnout;
  if (part && g.kp == 1 && fa.kind == FK_NONE && (M + 127) / 128 <= 64 && L.K % 2048 == 0 &&
      !knobs().no_splitk) {
    g.part = reinterpret_cast<int32_t*>(part);
    g.ksplit = 4;
  }
  HIPCHK(launch_row_gemm_any(g, st));
  return QTX_OK;
}
// FFN1: relu(a8 . W1^T) quantized per token over all d_ff columns, two passes (row
// maxima, then recompute + quantize: cheaper than the fp32 hidden's round trip)
// FFN1 in one weight-stationary pass with the row maxima exchanged between the column
// slices' workgroups inside the launch (k_gemm_wsx); QTX_NO_WSX=1: the two passes
bool wsx_on() { return !knobs().no_wsx; }
// Whether row_ffn1 takes the one-pass FFN1 (k_gemm_wsx / wsy) with its exchange scratch in
// s.y: then the layer's Q/K/V launch can zero that scratch as a side job (encoder_run).
bool ffn1_onepass(const QLin& L, int M, bool kp, const FaultArgs& fa) {
  return rowgemm(L, nullptr, nullptr, M, RE_RELU_PMAX, kp).kp == 2 && L.N == 2048 &&
         fa.kind == FK_NONE && wsx_on();
}
long ffn1_scratch16(int M) { return (4L * 32 * ((M + 31) / 32) + 2) / 2; }   // 16-B chunks
int row_ffn1(const qtx_config& c, const QLin& L, const int8_t* a8, const float* sa, int M,
             Scratch& s, hipStream_t st,
             const FaultArgs& fa = FaultArgs{}, bool kp = false, unsigned* status = nullptr,
             bool prezeroed = false) {
  RowGemmArgs g = rowgemm(L, a8, sa, M, RE_RELU_PMAX, kp);
  if (g.kp == 2 && L.N == 2048 && fa.kind == FK_NONE && wsx_on()) {
    g.epi = RE_RELU_QUANT_PMAX;
    g.prezeroed = prezeroed;
    if (L.qws32 && knobs().ws32) { g.W = L.qws32; g.kp = 5; }   // k_gemm_wsy32
    g.pmax_out = s.y;                // granules + ticket: <= 32 * M + 2048 bytes of the (unused) fp32 GEMM scratch
    g.out8 = s.h8; g.ldo8 = c.d_ff; g.os = s.sh;
    g.status = status;               // the model's status word: a timeout becomes an error
    HIPCHK(launch_gemm_wsx(g, st));
    return QTX_OK;
  }
  g.fault = fa;
  g.pmax_out = s.pmax;
  HIPCHK(launch_row_gemm_any(g, st));
  g.epi = RE_RELU_QUANT_PMAX;
  g.pmax_in = s.pmax; g.pmax_n = c.d_ff / 512;
  g.out8 = s.h8; g.ldo8 = c.d_ff; g.os = s.sh;
  HIPCHK(launch_row_gemm_any(g, st));
  return QTX_OK;
}

AttnArgs attn_args(const Scratch& s, int B, int Sq, int Sk, long kbs_rows) {
  AttnArgs a{};
  const int D = 512;
  a.q = s.q8; a.q_bs = (long)Sq * D; a.q_ld = D; a.sq = s.sq; a.sq_bs = Sq;
  a.k = s.k8; a.k_bs = kbs_rows * D; a.k_ld = D; a.sk = s.sk; a.sk_bs = kbs_rows;
  a.v = s.v8; a.v_bs = kbs_rows * D; a.v_ld = D; a.sv = s.sv; a.sv_bs = kbs_rows;
  a.ctx = s.ctx; a.c_bs = (long)Sq * D; a.c_ld = D;
  a.B = B; a.H = 8; a.Sq = Sq; a.Sk = Sk;
  return a;
}

// Self-attention sublayer: x += O(attn(LN(x)))   (sublayer_connection.py:15-17,
// attention.py:39-67).  Q/K/V come out of ONE N=3D GEMM and are quantized per token.
// fqkv / fo / af: a fault of a fault-injection run in the Q/K/V GEMM, the O projection or
// the attention MatMuls (fault_for, attn_fault_for), as on the row-GEMM chain.
int self_attn_block(const qtx_config& c, const QLin& qkv, const QLin& o,
                    const float* const* ln, Scratch& s, int B, int S, const uint8_t* mask,
                    long m_bs, long m_is, bool dec, hipStream_t st,
                    const FaultArgs& fqkv = FaultArgs{}, const FaultArgs& fo = FaultArgs{},
                    const AttnFault* af = nullptr) {
  const int D = c.d_model, M = B * S;
  RC(ln_quant(s.x, M, ln, D, s.a8, s.sa, st));
  RC(linear(c, qkv, s.a8, s.sa, M, 0, nullptr, s.y, 3 * D, st, fqkv));
  RC(quant(s.y, 3 * D, M, D, s.q8, s.sq, st));
  RC(quant(s.y + D, 3 * D, M, D, s.k8, s.sk, st));
  RC(quant(s.y + 2 * D, 3 * D, M, D, s.v8, s.sv, st));
  AttnArgs a = attn_args(s, B, S, S, S);
  a.mask = mask; a.m_bs = m_bs; a.m_is = m_is;
  a.dec = dec;
  HIPCHK(launch_attention(a, st));
  if (af) HIPCHK(launch_attn_fault_rows(a, *af, st));   // the faulty rows recomputed
  RC(quant(s.ctx, D, M, D, s.a8, s.sa, st));
  RC(linear(c, o, s.a8, s.sa, M, EPI_RESIDUAL, s.x, s.x, D, st, fo));
  return QTX_OK;
}

// FFN sublayer: x += w_2(relu(w_1(LN(x))))   (position_feed_forward.py:11-12)
int ffn_block(const qtx_config& c, const QLin& w1, const QLin& w2, const float* const* ln,
              Scratch& s, int M, hipStream_t st, const FaultArgs& f1, const FaultArgs& f2) {
  const int D = c.d_model, F = c.d_ff;
  RC(ln_quant(s.x, M, ln, D, s.a8, s.sa, st));
  RC(linear(c, w1, s.a8, s.sa, M, EPI_RELU, nullptr, s.y, F, st, f1));
  RC(quant(s.y, F, M, F, s.a8, s.sa, st));
  RC(linear(c, w2, s.a8, s.sa, M, EPI_RESIDUAL, s.x, s.x, D, st, f2));
  return QTX_OK;
}


// ---- fault injection (qtx_fault, include/qtx.h) -------------------------------------
// The fault in the coordinates of the GEMM that computes its reference MatMul (GemmId,
// qtx_host.h), with that linear's column offset in it.
FaultArgs fault_for(const qtx_fault* f, int module, int layer, GemmId gid, int M,
                    const qtx_config& c) {
  FaultArgs fa{};
  if (!f || f->kind == QTX_FAULT_NONE || f->module != module || f->layer != layer) return fa;
  const int lin = f->linear;
  long off = 0, nlin = c.d_model;
  switch (gid) {
    case G_QKV: if (lin < QTX_LIN_Q || lin > QTX_LIN_V) return fa; off = (long)lin * c.d_model; break;
    case G_CKV: if (lin != QTX_LIN_CK && lin != QTX_LIN_CV) return fa;
                off = (long)(lin - QTX_LIN_CK) * c.d_model; break;
    case G_O: if (lin != QTX_LIN_O) return fa; break;
    case G_FFN1: if (lin != QTX_LIN_FFN1) return fa; nlin = c.d_ff; break;
    case G_FFN2: if (lin != QTX_LIN_FFN2) return fa; break;
    case G_CQ: if (lin != QTX_LIN_CQ) return fa; break;
    case G_CO: if (lin != QTX_LIN_CO) return fa; break;
  }
  fa.bit = f->bit;
  switch (f->kind) {
    case QTX_FAULT_INPUT: case QTX_FAULT_INPUT16:
      fa.kind = FK_INPUT; fa.row = f->row; fa.col = f->col;
      fa.lo = off + (f->kind == QTX_FAULT_INPUT16 ? f->win_start : 0);
      fa.hi = f->kind == QTX_FAULT_INPUT16 ? fa.lo + f->win_len : off + nlin;
      break;
    case QTX_FAULT_WEIGHT: case QTX_FAULT_WEIGHT16:
      fa.kind = FK_WEIGHT; fa.row = off + f->row; fa.col = f->col;
      fa.lo = f->kind == QTX_FAULT_WEIGHT16 ? f->win_start : 0;
      fa.hi = f->kind == QTX_FAULT_WEIGHT16 ? fa.lo + f->win_len : M;
      break;
    case QTX_FAULT_OUTPUT:
      fa.kind = FK_OUTPUT; fa.row = f->row; fa.col = off + f->col; fa.value = f->value;
      break;
  }
  return fa;
}

// The fault as an AttnFault if it targets this layer's self (cross = false) or cross
// attention MatMuls (see qtx.h for the index conventions).
bool attn_fault_for(const qtx_fault* f, int module, int layer, bool cross, int Sq, int Sk,
                    AttnFault& af) {
  if (!f || f->kind == QTX_FAULT_NONE || f->module != module || f->layer != layer) return false;
  const int lin = f->linear;
  bool qk;
  if (!cross && (lin == QTX_LIN_QK || lin == QTX_LIN_PV)) qk = lin == QTX_LIN_QK;
  else if (cross && (lin == QTX_LIN_CQK || lin == QTX_LIN_CPV)) qk = lin == QTX_LIN_CQK;
  else return false;
  const bool in = f->kind == QTX_FAULT_INPUT || f->kind == QTX_FAULT_INPUT16;
  const bool win = f->kind == QTX_FAULT_INPUT16 || f->kind == QTX_FAULT_WEIGHT16;
  af = AttnFault{};
  af.bit = f->bit;
  af.value = f->value;
  const long row = f->row, col = f->col;
  if (f->kind == QTX_FAULT_OUTPUT) {
    af.kind = qk ? AF_QK_OUTPUT : AF_PV_OUTPUT;
    af.b = row / Sq; af.i = row % Sq;
    if (qk) { af.h = col / Sk; af.j = col % Sk; } else { af.h = col / 64; af.d = col % 64; }
    af.row0 = af.i; af.nrows = 1;
    return true;
  }
  if (in) {
    af.kind = qk ? AF_QK_INPUT : AF_PV_INPUT;
    af.b = row / Sq; af.i = row % Sq;
    if (qk) { af.h = col / 64; af.d = col % 64; } else { af.h = col / Sk; af.j = col % Sk; }
    af.lo = win ? (int)f->win_start : 0;
    af.hi = win ? (int)(f->win_start + f->win_len) : (qk ? Sk : 64);
    af.row0 = af.i; af.nrows = 1;
  } else {
    af.kind = qk ? AF_QK_WEIGHT : AF_PV_WEIGHT;
    af.b = row / Sk; af.j = row % Sk; af.h = col / 64; af.d = col % 64;
    af.lo = win ? (int)f->win_start : 0;
    af.hi = win ? (int)(f->win_start + f->win_len) : Sq;
    af.row0 = af.lo; af.nrows = af.hi - af.lo;
  }
  return true;
}

// attention with an optional fault: fp32 context (+ the faulty rows recomputed), then the
// per-token quantization of the O-projection input
int attention_fault(const AttnArgs& a, const AttnFault& af, int M, int D, Scratch& s,
                    hipStream_t st) {
  HIPCHK(launch_attention(a, st));
  HIPCHK(launch_attn_fault_rows(a, af, st));
  RC(quant(s.ctx, D, M, D, s.a8, s.sa, st));
  return QTX_OK;
}

// A stack's self-attention with the context quantized per token into s.a8 / s.sa: the
// all-heads kernel that quantizes in its epilogue where it takes the shape, else the fp32
// context + a quantization kernel; af: the attention with that fault.
int attention_quant(const AttnArgs& a, const AttnFault* af, int M, int D, Scratch& s, bool kp,
                    hipStream_t st) {
  if (af) return attention_fault(a, *af, M, D, s, st);
  const hipError_t ea = knobs().no_attn_encq ? hipErrorNotSupported
                                             : launch_attention_encq(a, s.a8, s.sa, st, false, kp);
  if (ea != hipErrorNotSupported) {
    HIPCHK(ea);
    return QTX_OK;
  }
  HIPCHK(launch_attention(a, st));
  return quant(s.ctx, D, M, D, s.a8, s.sa, st, kp);
}

// Validates a fault against the shapes of its target MatMul (M token rows of the module,
// Ms memory rows for the decoder's cross K/V); returns QTX_OK or an error code.
int check_fault(const qtx_model* m, const qtx_fault* f, int module, long B, long Sq, long Ss,
                long self_keys, long w_window) {
  if (!f || f->kind == QTX_FAULT_NONE) return QTX_OK;
  const qtx_config& c = m->cfg;
  const long M = B * Sq, Ms = B * Ss;
  RC(check_fault_bits(c));
  if (f->kind < 0 || f->kind > QTX_FAULT_OUTPUT) return fail(QTX_E_INVALID, "fault kind %d", f->kind);
  if (f->module != module) return fail(QTX_E_INVALID, "fault module %d", f->module);
  if (f->layer < 0 || f->layer >= c.n_layers) return fail(QTX_E_INVALID, "fault layer %d", f->layer);
  const int lin = f->linear;
  const bool in_kind = f->kind == QTX_FAULT_INPUT || f->kind == QTX_FAULT_INPUT16;
  const bool w_kind = f->kind == QTX_FAULT_WEIGHT || f->kind == QTX_FAULT_WEIGHT16;
  const bool win = f->kind == QTX_FAULT_INPUT16 || f->kind == QTX_FAULT_WEIGHT16;
  if ((in_kind || w_kind) && (f->bit < 0 || f->bit > 7)) return fail(QTX_E_INVALID, "fault bit %d", f->bit);
  auto bad_idx = [&](long r, long nr, long cc, long nc) {
    return fail(QTX_E_INVALID, "fault index (%ld, %ld) outside [%ld, %ld]", r, cc, nr, nc);
  };
  const long row = f->row, col = f->col;
  const bool attn_self = lin == QTX_LIN_QK || lin == QTX_LIN_PV;
  const bool attn_cross = lin == QTX_LIN_CQK || lin == QTX_LIN_CPV;
  if (attn_self || attn_cross) {
    if (attn_cross && module != 1) return fail(QTX_E_INVALID, "fault linear %d", lin);
    const long sq = Sq, sk = attn_cross ? Ss : self_keys ? self_keys : Sq, H = c.n_heads;
    if (sk > 512) return fail(QTX_E_UNSUPPORTED, "attention fault with %ld keys", sk);
    const bool qk = lin == QTX_LIN_QK || lin == QTX_LIN_CQK;
    long nr, nc, wmax;
    if (f->kind == QTX_FAULT_OUTPUT) { nr = B * sq; nc = qk ? H * sk : H * 64; wmax = 0; }
    else if (in_kind) { nr = B * sq; nc = qk ? H * 64 : H * sk; wmax = qk ? sk : 64; }
    else { nr = B * sk; nc = H * 64; wmax = w_window ? w_window : sq; }
    if (row < 0 || row >= nr || col < 0 || col >= nc) return bad_idx(row, nr, col, nc);
    if (win && (f->win_len < 1 || f->win_len > 16 || f->win_start < 0 || f->win_start + f->win_len > wmax))
      return fail(QTX_E_INVALID, "fault window [%ld, +%d) outside %ld", (long)f->win_start, f->win_len, wmax);
    return QTX_OK;
  }
  const bool enc_ok = lin == QTX_LIN_Q || lin == QTX_LIN_K || lin == QTX_LIN_V || lin == QTX_LIN_O ||
                      lin == QTX_LIN_FFN1 || lin == QTX_LIN_FFN2;
  const bool dec_ok = enc_ok || (lin >= QTX_LIN_CQ && lin <= QTX_LIN_CO);
  if (!(module == 0 ? enc_ok : dec_ok)) return fail(QTX_E_INVALID, "fault linear %d", lin);
  const long rows = (lin == QTX_LIN_CK || lin == QTX_LIN_CV) ? Ms : M;
  const long K = lin == QTX_LIN_FFN2 ? c.d_ff : c.d_model;
  const long N = lin == QTX_LIN_FFN1 ? c.d_ff : c.d_model;
  if (in_kind && (row < 0 || row >= rows || col < 0 || col >= K)) return bad_idx(row, rows, col, K);
  if (w_kind && (row < 0 || row >= N || col < 0 || col >= K)) return bad_idx(row, N, col, K);
  if (f->kind == QTX_FAULT_OUTPUT && (row < 0 || row >= rows || col < 0 || col >= N))
    return bad_idx(row, rows, col, N);
  if (f->kind == QTX_FAULT_INPUT16 &&
      (f->win_len < 1 || f->win_len > 16 || f->win_start < 0 || f->win_start + f->win_len > N))
    return fail(QTX_E_INVALID, "INPUT16 window");
  if (f->kind == QTX_FAULT_WEIGHT16 &&
      (f->win_len < 1 || f->win_len > 16 || f->win_start < 0 || f->win_start + f->win_len > rows))
    return fail(QTX_E_INVALID, "WEIGHT16 window");
  return QTX_OK;
}

// The fused FFN launch (qtx_ffn.hip) replaces the one-pass FFN1 + the FFN2 row GEMM on the
// KP path from ffn_fused_min_m rows (QTX_FFN_FUSED_MIN_M; QTX_NO_FFN_FUSED: never): one
// workgroup per 128 rows, so below ~1 block per CU the split launches use the chip better.
bool ffn_fused_ok(const EncLayer& L, long M, bool kp) {
  return kp && L.ffn && !knobs().no_ffn_fused && M >= knobs().ffn_fused_min_m;
}

int encoder_run(const qtx_model* m, const float* x, const uint8_t* mask, int B, int S,
                float* out, Scratch& s, hipStream_t st, const qtx_fault* f,
                hipEvent_t after_first) {
  const qtx_config& c = m->cfg;
  const int D = c.d_model, M = B * S;
  if (x != s.x) HIPCHK(hipMemcpyAsync(s.x, x, (size_t)M * D * 4, hipMemcpyDeviceToDevice, st));
  if (!row_path(c)) {
    for (int l = 0; l < c.n_layers; ++l) {
      const EncLayer& L = m->enc[l];
      auto fa = [&](GemmId gid) { return fault_for(f, 0, l, gid, M, c); };
      AttnFault af;
      const bool attn_f = attn_fault_for(f, 0, l, false, S, S, af);
      RC(self_attn_block(c, L.qkv, L.o, L.ln[0], s, B, S, mask, S, 0, false, st, fa(G_QKV),
                         fa(G_O), attn_f ? &af : nullptr));
      RC(ffn_block(c, L.w1, L.w2, L.ln[1], s, M, st, fa(G_FFN1), fa(G_FFN2)));
    }
    RC(ln_out(s.x, M, m->enc_norm, D, out, st));
    return QTX_OK;
  }
  // Every LayerNorm + per-token quantization after the first is fused into the epilogue of
  // the GEMM that produces the residual it normalizes (O-proj, FFN2); Q/K/V and the FFN
  // hidden are quantized in their GEMM's epilogue; the last FFN2 applies the final norm.
  // KP: the int8 activations between the kernels (LN output, attention context, FFN
  // hidden) live in the KP layout the row GEMM's 64-byte-step DMA reads as full lines
  // (qtx_common.h kp_off); the fault variants keep the row-major layout.
  const int NL = c.n_layers;
  const bool kp = (f == nullptr || f->kind == QTX_FAULT_NONE) && m->enc[0].qkv.qkp &&
                  !knobs().no_kp;
  RC(ln_quant(s.x, M, m->enc[0].ln[0], D, s.a8, s.sa, st, kp));
  for (int l = 0; l < NL; ++l) {
    const EncLayer& L = m->enc[l];
    auto fa = [&](GemmId gid) { return fault_for(f, 0, l, gid, M, c); };
    // the FFN1 below in one pass: its exchange scratch (in s.y, which nothing between here
    // and it writes) zeroed by the Q/K/V launch instead of a kernel of its own
    const bool zero_ffn1 = kp && !ffn_fused_ok(L, M, kp) && ffn1_onepass(L.w1, M, kp, fa(G_FFN1));
    RC(row_quant(L.qkv, s.a8, s.sa, M, s.q8, s.sq, st, fa(G_QKV), kp,
                 zero_ffn1 ? s.y : nullptr, zero_ffn1 ? ffn1_scratch16(M) : 0));
    if (l == 0 && after_first) HIPCHK(hipEventRecord(after_first, st));
    AttnArgs a = attn_args(s, B, S, S, S);
    a.mask = mask; a.m_bs = S; a.m_is = 0;
    a.c_ld = D;
    AttnFault af;
    RC(attention_quant(a, attn_fault_for(f, 0, l, false, S, S, af) ? &af : nullptr, M, D, s, kp, st));
    RC(row_res_ln(L.o, s.a8, s.sa, M, s.x, L.ln[1], s.a8, s.sa, nullptr, st, fa(G_O), kp));
    if (ffn_fused_ok(L, M, kp)) {
      // the FFN sublayer in one launch (k_ffn_fused): the hidden stays on chip; each
      // workgroup reads its rows of a8 / sa before it writes them (the next LN's codes)
      FfnArgs g{};
      g.A = s.a8; g.sa = s.sa; g.wf = L.ffn;
      g.sw1 = L.w1.s; g.b1 = L.w1.b; g.sw2 = L.w2.s; g.b2 = L.w2.b;
      g.x = s.x; g.M = M; g.F = c.d_ff;
      if (l + 1 < NL) {
        g.ln_a = m->enc[l + 1].ln[0][0]; g.ln_b = m->enc[l + 1].ln[0][1];
        g.lnq = s.a8; g.lns = s.sa;
      } else {
        g.ln_a = m->enc_norm[0]; g.ln_b = m->enc_norm[1]; g.lnout = out;
      }
      HIPCHK(launch_ffn_fused(g, st));
      continue;
    }
    RC(row_ffn1(c, L.w1, s.a8, s.sa, M, s, st, fa(G_FFN1), kp, s.status, zero_ffn1));
    if (l + 1 < NL)
      RC(row_res_ln(L.w2, s.h8, s.sh, M, s.x, m->enc[l + 1].ln[0], s.a8, s.sa, nullptr, st,
                    fa(G_FFN2), kp, s.y));
    else
      RC(row_res_ln(L.w2, s.h8, s.sh, M, s.x, m->enc_norm, nullptr, nullptr, out, st,
                    fa(G_FFN2), kp, s.y));
  }
  return QTX_OK;
}

// Encoder sub-batch pipelining: a batch of >= 256 sentences runs as two halves on two
// streams, the second half one kernel behind, so the HBM-bound epilogues (residual +
// LayerNorm) of one half overlap the MFMA / VALU-bound kernels (attention, FFN) of the
// other on different CUs.  Results are identical (rows are independent).
// (not with the one-pass FFN1, which makes the layer's kernels MFMA / exchange-bound rather
// than HBM-bound: the split measured no gain before it, 2.07 vs 2.05 ms)
bool enc_split(int B) { return B >= 256 && !knobs().enc_nosplit && !wsx_on(); }

size_t enc_ws(const qtx_config& c, int B, int S) {
  Arena ar;
  carve_scratch(ar, c, (long)B * S);
  if (enc_split(B)) {
    Arena a2;
    carve_scratch(a2, c, (long)(B / 2) * S);
    carve_scratch(a2, c, (long)(B - B / 2) * S);
    ar.used = std::max(ar.used, a2.used);
  }
  return align_up(ar.used);
}

// (CrossKV / carve_cross, quantized memory + cross K/V for all layers: qtx_carve.h)

bool ckv_fault(const qtx_model* m, const qtx_fault* f, int Ms) {
  bool hit = false;
  for (int l = 0; l < m->cfg.n_layers; ++l)
    hit |= fault_for(f, 1, l, G_CKV, Ms, m->cfg).kind != FK_NONE;
  return hit;
}

// memory -> per-layer cross K/V (get_quantized_model.py:160-168: K/V outputs quantized)
int cross_kv(const qtx_model* m, const float* memory, int Ms, CrossKV& x, hipStream_t st,
             const qtx_fault* f) {
  const qtx_config& c = m->cfg;
  const int D = c.d_model;
  RC(quant(memory, D, Ms, D, x.am8, x.sam, st));
  if (row_path(c) && D == 512 && !ckv_fault(m, f, Ms)) {
    // every layer's K and V in ONE row GEMM (N = n_layers * 2 * 512): its 512-column tiles
    // are the layers' K / V, each quantized per token in the epilogue exactly as the
    // per-layer launches below (decode prologue: 6 launches of 36 workgroups -> one of 216)
    RC(row_quant(m->ckv_all, x.am8, x.sam, Ms, x.k8[0], x.sk[0], st));
    return QTX_OK;
  }
  for (int l = 0; l < c.n_layers; ++l) {
    if (row_path(c)) {     // K and V tiles quantized in the GEMM epilogue
      RC(row_quant(m->dec[l].ckv, x.am8, x.sam, Ms, x.k8[l], x.sk[l], st,
                   fault_for(f, 1, l, G_CKV, Ms, c)));
      continue;
    }
    RC(linear(c, m->dec[l].ckv, x.am8, x.sam, Ms, 0, nullptr, x.y, 2 * D, st,
              fault_for(f, 1, l, G_CKV, Ms, c)));
    RC(quant(x.y, 2 * D, Ms, D, x.k8[l], x.sk[l], st));
    RC(quant(x.y + D, 2 * D, Ms, D, x.v8[l], x.sv[l], st));
  }
  return QTX_OK;
}

// Cross-attention sublayer: x += O(attn(LN(x) -> Q, memory -> K/V)), decoder.py:32
int cross_attn_block(const qtx_model* m, const DecLayer& L, int l, Scratch& s,
                     const CrossKV& x, int B, int T, int S, const uint8_t* src_mask,
                     hipStream_t st, const FaultArgs& fcq, const FaultArgs& fco,
                     const AttnFault* af) {
  const qtx_config& c = m->cfg;
  const int D = c.d_model, M = B * T;
  RC(ln_quant(s.x, M, L.ln[1], D, s.a8, s.sa, st));
  RC(linear(c, L.cq, s.a8, s.sa, M, 0, nullptr, s.y, D, st, fcq));
  RC(quant(s.y, D, M, D, s.q8, s.sq, st));
  AttnArgs a = attn_args(s, B, T, S, S);
  a.k = x.k8[l]; a.sk = x.sk[l]; a.v = x.v8[l]; a.sv = x.sv[l];
  a.mask = src_mask; a.m_bs = S; a.m_is = 0;
  a.dec = 1;
  HIPCHK(launch_attention(a, st));
  if (af) HIPCHK(launch_attn_fault_rows(a, *af, st));
  RC(quant(s.ctx, D, M, D, s.a8, s.sa, st));
  RC(linear(c, L.co, s.a8, s.sa, M, EPI_RESIDUAL, s.x, s.x, D, st, fco));
  return QTX_OK;
}

size_t dec_ws(const qtx_config& c, int B, int T, int S) {
  Arena ar;
  carve_scratch(ar, c, (long)B * T);
  carve_cross(ar, c, (long)B * S);
  return align_up(ar.used);
}

// (GreedyWS, the greedy decode workspace with carve_greedy / group_view, and BeamTail, the
// beam step's tail: qtx_carve.h)

// Sub-batch split of the fused decode.  Sentences are independent (per-token quantization:
// no value depends on another sentence), and one sub-batch's step is a chain of ~50
// latency-bound kernels that each occupy a fraction of the 256 CUs.  G sub-batch graphs
// on G streams (ms per decode, profiles/r03_concurrency.md): B = 32: 14.5 / 21.0 for
// G = 1 / 2; B = 256: 34.9 / 35.8; B = 512: 59.0 / 51.9 — two chains of 256 rows overlap
// as well as two processes of 256 sentences each (50.6), two of 128 or 16 do not gain.
// Default G = 2 from B = 512, else 1; QTX_DECODE_GROUPS overrides it (experiments).
Groups decode_groups(int B) {   // (Groups / split_groups, no empty group: qtx_carve.h)
  return split_groups(B, knobs().decode_groups > 0 ? knobs().decode_groups : B >= 512 ? 2 : 1);
}

// ---- fused decode step (M = B rows, keys <= 128) ----------------------------------------
// Its kernels exist for the flagship shapes only: the skinny GEMM takes K = 512 or 2048
// (FFN2: K = d_ff; launch_skinny) and the argmax / top-2 tails a vocabulary of at most
// ARG_MAXV.  Every other config qtx_model_create accepts decodes with the unfused step,
// whose kernels have no such limit (greedy_run decides before anything is captured).
bool fused_step_ok(const qtx_config& c) {
  return (c.d_ff == 512 || c.d_ff == 2048) && c.tgt_vocab <= ARG_MAXV;
}

SkinnyArgs skinny(int wbits, const QLin& L, int M, int amode, int flags, float* out, long ldo) {
  SkinnyArgs s{};
  // wbits 8 on a 4-bit model: its unpacked int8 copy
  s.amode = amode; s.W = wbits == 8 ? L.w8() : L.q; s.ldw = wbits == 8 ? L.K : L.K / 2;
  s.sw = L.s; s.bias = L.b;
  s.out = out; s.ldo = ldo; s.M = M; s.N = L.N; s.K = L.K; s.flags = flags;
  return s;
}

DecAttnArgs dec_attn_self(const GreedyWS& g, int l, int B, int max_len, int host_step1) {
  DecAttnArgs at{};
  at.y = g.dec.y; at.ldy = 3 * 512; at.kv_new = 1; at.step = g.step;
  at.kc = g.kc[l]; at.vc = g.vc[l]; at.skc = g.skc[l]; at.svc = g.svc[l]; at.kv_bs = max_len;
  at.ctx = g.dec.ctx; at.B = B; at.host_step1 = host_step1;
  return at;
}
DecAttnArgs dec_attn_cross(const GreedyWS& g, int l, int B, int S, const uint8_t* src_mask) {
  DecAttnArgs at{};
  at.y = g.dec.y; at.ldy = 512; at.kv_new = 0; at.S = S; at.mask = src_mask;
  at.kc = g.cross.k8[l]; at.vc = g.cvg[l]; at.skc = g.cross.sk[l]; at.svc = g.cross.sv[l];
  at.kv_bs = S; at.ctx = g.dec.ctx; at.B = B;
  return at;
}

// The beam step's tail on the step's R = B * beam rows: the selection (scores, parents, tokens,
// next inputs, position + 1, rows still live), then the caches of every layer by parent.
int beam_tail(const qtx_model* m, GreedyWS& g, int R, int max_len, hipStream_t st) {
  const qtx_config& c = m->cfg;
  const BeamTail& b = *g.beam;
  HIPCHK(launch_beam_select(g.logits, R / b.K, b.K, c.tgt_vocab, b.eos, b.pad, max_len, g.step,
                            b.st.score, b.st.fin, b.st.len, b.st.parent, b.st.bp_par,
                            b.st.bp_tok, m->tgt_lut, m->pe, c.max_len, g.dec.x, st));
  HIPCHK(launch_beam_reorder(b.kc0, b.vc0, b.skc0, b.svc0, R / b.K, b.K, max_len, c.n_layers,
                             b.k_ls, b.v_ls, b.s_ls, b.grouped ? 1 : 0, g.step, b.st.parent, st));
  return QTX_OK;
}

// One KV-cached decoder step for every sentence, 8 kernels per layer + 2:
//   [LN+QKV] [self-attn] [O+res] [LN+Qc] [cross-attn] [Oc+res] [LN+FFN1+relu] [FFN2+res]
//   [final LN + generator] [log_softmax/argmax + next embedding + step++]
// Reads the position from g.step (device), so it can be captured once and replayed.
// t_host: the step's position when the caller knows it at launch or capture time (the
// whole decode in one graph, or eager launches), else -1
int greedy_step_fused(const qtx_model* m, GreedyWS& g, int B, int S, int max_len,
                      int64_t* ids, const uint8_t* src_mask, hipStream_t st, int t_host) {
  const qtx_config& c = m->cfg;
  const int D = c.d_model, F = c.d_ff;
  const int wb = m->dec[0].qkv.q8 && !knobs().int4_packed ? 8 : c.weight_bits;
  // the FFN hidden quantized once by its own kernel (instead of in every FFN2 workgroup's
  // prologue from FFN1's partial maxima) from 96 rows on: measured faster there despite the
  // extra launch (profiles/r05_rb_sweep.md), slower at B = 32
  const bool ffn_qkernel = knobs().ffn_qkernel || B >= 96;
  const bool fused_ln = !knobs().split_ln;
  // O / Oc form the context's per-token maximum from the rows they load (A_F32R) instead of
  // the attention's per-head maxima (QTX_ATTN_PMAX=1: the per-head maxima, A_F32Q)
  const bool own_max = !knobs().attn_pmax;
  // likewise FFN2 forms the hidden's per-token maximum itself (QTX_FFN_PMAX=1: from FFN1's
  // per-tile maxima, FFN1 with the maxima epilogue)
  const bool ffn_own = !knobs().ffn_pmax;
  // the position from the host (self-attention, argmax + embedding; the device counter then
  // neither read nor advanced) or from the device counter (QTX_DEVICE_STEP, or a step replayed
  // at several positions)
  const bool host_pos = t_host >= 0 && !knobs().device_step;
  // The tail folded into the next step's first launch (plain decode, int8 kernels, positions
  // from the host; QTX_NO_TAIL_FOLD: never): the generator also writes per-strip top-2 records,
  // and from step 1 on layer 0's LN+QKV launch decides the previous step's token from them,
  // embeds it and stores ids / x itself (launch_skinny_tok) — a step is then 49 launches.
  // Only the last step still ends with the argmax kernel.
  const bool fold = !knobs().no_tail_fold && host_pos && !g.top_ids && wb == 8 && fused_ln &&
                    !knobs().ablate && !knobs().dbg_tail && !g.no_fold && !g.beam;
  Scratch& s = g.dec;
  // Timing experiments only (wrong results): QTX_ABLATE=<bitmask> drops kernel classes
  // from the step (replaced by an empty kernel with QTX_ABLATE_NOP=1) to measure what
  // each costs inside the real graph.  1 LN, 2 QKV/Qc, 4 self-attn, 8 cross-attn,
  // 16 O/Oc, 32 FFN1, 64 h-quant, 128 FFN2, 256 tail.
  const int abl = knobs().ablate;           // always 0 outside the QTX_DIAG build
  const bool abl_nop = knobs().ablate_nop;
#define QTX_RUN_(bit, stmt)                    \
  do {                                         \
    if (abl & (bit)) {                         \
      if (abl_nop) HIPCHK(launch_nop(st));     \
    } else {                                   \
      stmt;                                    \
    }                                          \
  } while (0)
#define QTX_RUN(bit, launch) QTX_RUN_(bit, HIPCHK(launch))
#define QTX_RUNRC(bit, expr) QTX_RUN_(bit, RC(expr))
  // out = epilogue(quant(LN(x)) . W^T): the LayerNorm + per-token quant is recomputed in
  // the prologue of every GEMM workgroup (4 rows each, A_LN) — cheaper than its own kernel
  // launch; QTX_SPLIT_LN=1 restores the separate LN kernel (timing experiments).
  auto ln_linear = [&](const QLin& W, const float* const* ln, int flags, float* out,
                       long ldo, int bit) -> int {
    SkinnyArgs k = skinny(wb, W, B, fused_ln ? A_LN : A_I8, flags, out, ldo);
    if (flags & EPI_ROWMAX) k.pmax_out = g.pmax_f;
    if (fused_ln) {
      k.X = s.x; k.ldx = D; k.ln_a = ln[0]; k.ln_b = ln[1];
    } else {
      QTX_RUNRC(1, ln_quant(s.x, B, ln, D, s.a8, s.sa, st));
      k.A = s.a8; k.sa = s.sa;
    }
    QTX_RUN(bit, launch_skinny(k, wb, st));
    return QTX_OK;
  };
  for (int l = 0; l < c.n_layers; ++l) {
    const DecLayer& L = m->dec[l];
    SkinnyArgs a;
    if (fold && l == 0 && t_host >= 1) {
      SkinnyArgs k = skinny(wb, L.qkv, B, A_LN, 0, s.y, 3 * D);
      k.ln_a = L.ln[0][0]; k.ln_b = L.ln[0][1];
      TokArgs tk{};
      tk.rec = g.rec; tk.logits = g.logits; tk.V = c.tgt_vocab; tk.lut = m->tgt_lut;
      tk.pe = m->pe; tk.max_pos = c.max_len; tk.pos = t_host; tk.ids = ids; tk.ids_bs = max_len;
      tk.xres = s.x;
      HIPCHK(launch_skinny_tok(k, tk, st));
    } else {
      RC(ln_linear(L.qkv, L.ln[0], 0, s.y, 3 * D, 2));
    }
    DecAttnArgs at = dec_attn_self(g, l, B, max_len, host_pos ? t_host + 1 : 0);
    at.pmax = own_max ? nullptr : g.pmax_a;
    QTX_RUN(4, launch_dec_attn(at, B, st));
    a = skinny(wb, L.o, B, own_max ? A_F32R : A_F32Q, EPI_RESIDUAL, s.x, D);   // quantizes ctx per token
    a.X = s.ctx; a.ldx = D; a.pmax_in = g.pmax_a; a.pmax_n = 8; a.res = s.x; a.ldr = D;
    QTX_RUN(16, launch_skinny(a, wb, st));
    RC(ln_linear(L.cq, L.ln[1], 0, s.y, D, 2));
    at = dec_attn_cross(g, l, B, S, src_mask);
    at.pmax = own_max ? nullptr : g.pmax_a;
    QTX_RUN(8, launch_dec_attn(at, B, st));
    a = skinny(wb, L.co, B, own_max ? A_F32R : A_F32Q, EPI_RESIDUAL, s.x, D);
    a.X = s.ctx; a.ldx = D; a.pmax_in = g.pmax_a; a.pmax_n = 8; a.res = s.x; a.ldr = D;
    QTX_RUN(16, launch_skinny(a, wb, st));
    if (!ffn_qkernel) {   // FFN2 quantizes h itself (from its rows, or FFN1's per-tile maxima)
      RC(ln_linear(L.w1, L.ln[2], ffn_own ? EPI_RELU : EPI_RELU | EPI_ROWMAX, s.y, F, 32));
      a = skinny(wb, L.w2, B, ffn_own ? A_F32R : A_F32Q, EPI_RESIDUAL, s.x, D);
      a.X = s.y; a.ldx = F; a.pmax_in = g.pmax_f; a.pmax_n = F / 16; a.res = s.x; a.ldr = D;
      QTX_RUN(128, launch_skinny(a, wb, st));
    } else {              // one wave per row quantizes h (quant_linear.py:30-43), then FFN2
      RC(ln_linear(L.w1, L.ln[2], EPI_RELU, s.y, F, 32));
      if (F == 2048 && !knobs().hquant_rows)   // one 4-wave workgroup per row
        QTX_RUN(64, launch_quant_h2048(s.y, F, B, s.a8, s.sa, st));
      else
        QTX_RUNRC(64, quant(s.y, F, B, F, s.a8, s.sa, st));
      a = skinny(wb, L.w2, B, A_I8, EPI_RESIDUAL, s.x, D);
      a.A = s.a8; a.sa = s.sa; a.res = s.x; a.ldr = D;
      QTX_RUN(128, launch_skinny(a, wb, st));
    }
  }
  if (knobs().dbg_tail) {   // bisection aid (QTX_DIAG build): reference-shaped tail kernels
    RC(ln_out(s.x, B, m->dec_norm, D, g.xo, st));
    HIPCHK(launch_generator(g.xo, D, B, m->gen_w, m->gen_b, c.tgt_vocab, g.logits, st));
    HIPCHK(launch_logsoftmax_argmax(g.logits, B, c.tgt_vocab, nullptr, ids, max_len, g.step,
                                    1, st));
    HIPCHK(launch_step_inc(g.step, st));
    HIPCHK(launch_embed(ids, max_len, B, 1, g.step, 0, m->tgt_lut, c.tgt_vocab, m->pe,
                        c.max_len, s.x, D, st));
    return QTX_OK;
  }
  QTX_RUN(256, launch_generator_mfma(s.x, D, B, m->dec_norm[0], m->dec_norm[1], m->gen_wt,
                                     m->gen_b, c.tgt_vocab, g.logits, st, fold ? g.rec : nullptr));
  if (fold && t_host + 2 < max_len) return QTX_OK;   // the next step's first launch is the tail
  if (g.beam) return beam_tail(m, g, B, max_len, st);
  if (g.top_ids)   // scored decode: the tail that also writes the step's two best (id, logp)
    QTX_RUN(256, launch_top2_embed(g.logits, B, c.tgt_vocab, ids, max_len, g.top_ids, g.top_logp,
                                   g.step, reinterpret_cast<unsigned*>(g.step + 1), m->tgt_lut,
                                   m->pe, c.max_len, s.x, st, host_pos ? t_host + 1 : 0));
  else
    QTX_RUN(256, launch_argmax_embed(g.logits, B, c.tgt_vocab, ids, max_len, g.step,
                                     reinterpret_cast<unsigned*>(g.step + 1), m->tgt_lut, m->pe,
                                     c.max_len, s.x, st, host_pos ? t_host + 1 : 0));
  return QTX_OK;
#undef QTX_RUN_
#undef QTX_RUN
#undef QTX_RUNRC
}

int cached_self_attn_unfused(GreedyWS& g, int l, int B, int max_len, int t, const AttnFault* af,
                             hipStream_t st) {
  const int D = 512;
  Scratch& s = g.dec;
  RC(quant(s.y, 3 * D, B, D, s.q8, s.sq, st));
  RowArgs kr = rows_quant(s.y + D, 3 * D, B, D, g.kc[l], g.skc[l]);
  RowArgs vr = rows_quant(s.y + 2 * D, 3 * D, B, D, g.vc[l], g.svc[l]);
  kr.rpb = vr.rpb = 1; kr.dst_bstride = vr.dst_bstride = max_len;
  if (t >= 0) kr.dst_off = vr.dst_off = t;
  else kr.dst_off_dev = vr.dst_off_dev = g.step;
  HIPCHK(launch_rows(kr, st));
  HIPCHK(launch_rows(vr, st));
  AttnArgs a = attn_args(s, B, 1, t >= 0 ? t + 1 : 0, max_len);
  a.k = g.kc[l]; a.sk = g.skc[l]; a.v = g.vc[l]; a.sv = g.svc[l];
  if (t < 0) { a.sk_dev = g.step; a.sk_add = 1; }
  a.dec = 1;
  HIPCHK(launch_attention(a, st));
  if (af) HIPCHK(launch_attn_fault_rows(a, *af, st));
  return QTX_OK;
}

// The reference-shaped unfused step (any key count up to 512).
int greedy_step_unfused(const qtx_model* m, GreedyWS& g, int B, int S, int max_len,
                        int64_t* ids, const uint8_t* src_mask, hipStream_t st) {
  const qtx_config& c = m->cfg;
  const int D = c.d_model;
  Scratch& s = g.dec;
  if (!g.beam)   // (the beam step's input row comes from the previous step's select)
    HIPCHK(launch_embed(ids, max_len, B, 1, g.step, 0, m->tgt_lut, c.tgt_vocab, m->pe,
                        c.max_len, s.x, D, st));
  for (int l = 0; l < c.n_layers; ++l) {
    const DecLayer& L = m->dec[l];
    RC(ln_quant(s.x, B, L.ln[0], D, s.a8, s.sa, st));
    RC(linear(c, L.qkv, s.a8, s.sa, B, 0, nullptr, s.y, 3 * D, st));
    RC(cached_self_attn_unfused(g, l, B, max_len, -1, nullptr, st));
    RC(quant(s.ctx, D, B, D, s.a8, s.sa, st));
    RC(linear(c, L.o, s.a8, s.sa, B, EPI_RESIDUAL, s.x, s.x, D, st));
    RC(cross_attn_block(m, L, l, s, g.cross, B, 1, S, src_mask, st));
    RC(ffn_block(c, L.w1, L.w2, L.ln[2], s, B, st));
  }
  RC(ln_out(s.x, B, m->dec_norm, D, g.xo, st));
  HIPCHK(launch_generator(g.xo, D, B, m->gen_w, m->gen_b, c.tgt_vocab, g.logits, st));
  if (g.beam) return beam_tail(m, g, B, max_len, st);   // (it advances the position itself)
  if (g.top_ids)
    HIPCHK(launch_logsoftmax_top2(g.logits, B, c.tgt_vocab, ids, max_len, g.step, 1, g.top_ids,
                                  g.top_logp, max_len - 1, st));
  else
    HIPCHK(launch_logsoftmax_argmax(g.logits, B, c.tgt_vocab, nullptr, ids, max_len, g.step, 1,
                                    st));
  HIPCHK(launch_step_inc(g.step, st));
  return QTX_OK;
}


// The decoder stack over M = B * T rows: s.x holds the embedded targets, x the cross K/V
// (cross_kv); out [M, D] = the final LayerNorm's output.  f: one optional fault.
int decoder_body(const qtx_model* m, Scratch& s, const CrossKV& x, const uint8_t* src_mask,
                 const uint8_t* tgt_mask, long tm_bs, int B, int T, int S, float* out,
                 const qtx_fault* f, hipStream_t st) {
  const qtx_config& c = m->cfg;
  const int D = c.d_model, M = B * T;
  if (!row_path(c)) {
    for (int l = 0; l < c.n_layers; ++l) {
      const DecLayer& L = m->dec[l];
      auto fa = [&](GemmId gid) { return fault_for(f, 1, l, gid, M, c); };
      AttnFault af;
      const bool self_f = attn_fault_for(f, 1, l, false, T, T, af);
      RC(self_attn_block(c, L.qkv, L.o, L.ln[0], s, B, T, tgt_mask, tm_bs, T, true, st,
                         fa(G_QKV), fa(G_O), self_f ? &af : nullptr));
      const bool cross_f = attn_fault_for(f, 1, l, true, T, S, af);
      RC(cross_attn_block(m, L, l, s, x, B, T, S, src_mask, st, fa(G_CQ), fa(G_CO),
                          cross_f ? &af : nullptr));
      RC(ffn_block(c, L.w1, L.w2, L.ln[2], s, M, st, fa(G_FFN1), fa(G_FFN2)));
    }
    RC(ln_out(s.x, M, m->dec_norm, D, out, st));
    return QTX_OK;
  }
  // LayerNorm + quant of each sublayer's input fused into the previous residual GEMM
  // (as encoder_run); the last FFN2 applies the final decoder norm
  const int NL = c.n_layers;
  RC(ln_quant(s.x, M, m->dec[0].ln[0], D, s.a8, s.sa, st));
  for (int l = 0; l < NL; ++l) {
    const DecLayer& L = m->dec[l];
    auto fa = [&](GemmId gid) { return fault_for(f, 1, l, gid, M, c); };
    RC(row_quant(L.qkv, s.a8, s.sa, M, s.q8, s.sq, st, fa(G_QKV)));
    AttnArgs a = attn_args(s, B, T, T, T);
    a.mask = tgt_mask; a.m_bs = tm_bs; a.m_is = T;
    a.c_ld = D;
    a.dec = 1;
    AttnFault af;
    RC(attention_quant(a, attn_fault_for(f, 1, l, false, T, T, af) ? &af : nullptr, M, D, s, false, st));
    RC(row_res_ln(L.o, s.a8, s.sa, M, s.x, L.ln[1], s.a8, s.sa, nullptr, st, fa(G_O)));
    RC(row_quant(L.cq, s.a8, s.sa, M, s.q8, s.sq, st, fa(G_CQ)));
    a = attn_args(s, B, T, S, S);
    a.k = x.k8[l]; a.sk = x.sk[l]; a.v = x.v8[l]; a.sv = x.sv[l];
    a.mask = src_mask; a.m_bs = S; a.m_is = 0;
    a.dec = 1;
    if (attn_fault_for(f, 1, l, true, T, S, af)) {
      RC(attention_fault(a, af, M, D, s, st));
    } else {
      HIPCHK(launch_attention(a, st));
      RC(quant(s.ctx, D, M, D, s.a8, s.sa, st));
    }
    RC(row_res_ln(L.co, s.a8, s.sa, M, s.x, L.ln[2], s.a8, s.sa, nullptr, st, fa(G_CO)));
    RC(row_ffn1(c, L.w1, s.a8, s.sa, M, s, st, fa(G_FFN1)));
    if (l + 1 < NL)
      RC(row_res_ln(L.w2, s.h8, s.sh, M, s.x, m->dec[l + 1].ln[0], s.a8, s.sa, nullptr, st, fa(G_FFN2)));
    else
      RC(row_res_ln(L.w2, s.h8, s.sh, M, s.x, m->dec_norm, nullptr, nullptr, out, st, fa(G_FFN2)));
  }
  return QTX_OK;
}

// whether the decode runs the fused step (else the unfused one)
bool greedy_fused(const qtx_config& c, int S, int max_len) {
  return S <= 128 && max_len <= 128 && fused_step_ok(c) && !knobs().unfused;
}

int regroup_cross_values(const qtx_config& c, const CrossKV& x, int B, int S, int8_t* cvg,
                         hipStream_t st) {
  const long v_ls = c.n_layers > 1 ? (long)(x.v8[1] - x.v8[0]) : 0;
  HIPCHK(launch_vgroup4(x.v8[0], v_ls, c.n_layers, B, S, cvg,
                        (long)B * ((S + 3) & ~3) * c.d_model, st));
  return QTX_OK;
}

// The encode step of every decode, on the B sentences: memory = encode(src_embed(src), mask),
// the cross K/V of every layer into x and, for the fused step (cvg non-null), the cross
// values in k_dec_attn's 4-key groups.
// (captured into a hipGraph with the steps' replay — QTX_PRE_GRAPH in round 3 — it
// measured no faster: 14.34 vs 14.31 ms per B = 32 decode; the host's enqueue of these
// launches runs ahead of the GPU)
int encode_src(const qtx_model* m, GreedyWS& g, const int64_t* src, const uint8_t* mask, int B,
               int S, CrossKV& x, int8_t* cvg, const qtx_fault* f, hipStream_t st) {
  const qtx_config& c = m->cfg;
  HIPCHK(launch_embed(src, S, B, S, nullptr, 0, m->src_lut, c.src_vocab, m->pe, c.max_len,
                      g.enc.x, (long)S * c.d_model, st));
  RC(encoder_run(m, g.enc.x, mask, B, S, g.memory, g.enc, st, f));
  RC(cross_kv(m, g.memory, B * S, x, st));
  if (cvg) RC(regroup_cross_values(c, x, B, S, cvg, st));
  return QTX_OK;
}

// What precedes the steps: the encode step in place, ids[:, 0] and the step counters.
int greedy_prologue(const qtx_model* m, GreedyWS& g, const int64_t* src, int B, int S,
                    int max_len, int64_t start, const qtx_fault* f, bool fused, hipStream_t st) {
  RC(encode_src(m, g, src, g.mask, B, S, g.cross, fused ? g.cvg[0] : nullptr, f, st));
  // ids[:, 0] = start ; step[0] = position 0, step[1] = arrival counter
  HIPCHK(launch_fill_col(g.ids, max_len, B, start, st));
  HIPCHK(launch_zero(g.step, 16, st));
  return QTX_OK;
}

// The fused steps of a request through the model's step-graph runner, serialised per model
// with the model's device current (the runner creates streams and events).
int run_steps(const qtx_model* m, const StepRequest& rq, hipStream_t st) {
  qtx_model* mm = const_cast<qtx_model*>(m);
  std::lock_guard<std::mutex> lock(mm->mu);
  DeviceGuard dg(mm->device);
  return mm->sg.run(rq, st);
}

StepRequest step_request(const qtx_model* m, std::vector<GreedyWS>& gv, const Groups& gr, int B,
                         int S, int max_len, StepForm form) {
  StepRequest rq;
  rq.key.rows = B; rq.key.S = S; rq.key.max_len = max_len;
  rq.key.groups = gr.G;
  rq.key.anchor = gv[0].step;   // the step counters baked into the capture
  rq.key.form = form;
  rq.step = [m, &gv, gr, B, S, max_len](int i, hipStream_t s, int t) {
    GreedyWS& g = gv[i];   // (ids and mask: the parent's, not offset by group_view)
    return greedy_step_fused(m, g, gr.rows(i, B), S, max_len,
                             g.ids ? g.ids + (long)gr.b0(i) * max_len : nullptr,
                             g.mask + (long)gr.b0(i) * S, s, t);
  };
  return rq;
}

// The steps of a greedy decode after its prologue, with the decode's path selection (the plain
// or, with g.top_ids, the scored step).
int greedy_steps(const qtx_model* m, GreedyWS& g, int B, int S, int max_len, hipStream_t st) {
  const qtx_config& c = m->cfg;
  const bool fused = greedy_fused(c, S, max_len);
  if (!fused) {
    for (int t = 0; t + 1 < max_len; ++t) RC(greedy_step_unfused(m, g, B, S, max_len, g.ids, g.mask, st));
    return QTX_OK;
  }
  // sub-batches: each has its own step scratch and step counter; the first decoder input
  // is tgt_embed(ys[:, 0]) at position 0, later ones come from the previous step's argmax
  const Groups gr = decode_groups(B);
  std::vector<GreedyWS> gv = group_views(g, c, gr, S, max_len);
  HIPCHK(hipMemsetAsync(g.gsteps, 0, sizeof(int) * 4 * QTX_MAX_GROUPS, st));
  for (int i = 0; i < gr.G; ++i)
    HIPCHK(launch_embed(g.ids + (long)gr.b0(i) * max_len, max_len, gr.rows(i, B), 1, gv[i].step,
                        0, m->tgt_lut, c.tgt_vocab, m->pe, c.max_len, gv[i].dec.x, c.d_model, st));
  if (max_len <= 1) return QTX_OK;
  // steps per graph: the whole decode in one graph by default (one graph launch); must
  // divide max_len-1 (the step position is read from device memory, so replays chain)
  int per_graph = max_len - 1;
  if (const int v = knobs().graph_steps; v > 0 && (max_len - 1) % v == 0) per_graph = v;
  // the scored step: its own entry
  StepRequest rq = step_request(m, gv, gr, B, S, max_len, g.top_ids ? StepForm::Scored : StepForm::Plain);
  // a graph of the whole decode is replayed once per decode from position 0: each captured
  // step knows its position (a shorter graph replays at several)
  rq.key.host_pos = per_graph == max_len - 1;
  rq.key.joint = gr.G > 1 && knobs().group_graph;
  rq.plan = {{per_graph, (max_len - 1) / per_graph, 0}};
  rq.timed = knobs().time_graph;
  return run_steps(m, rq, st);
}

int greedy_run(const qtx_model* m, GreedyWS& g, const int64_t* src, int B, int S, int max_len,
               int64_t start, const qtx_fault* f, hipStream_t st) {
  RC(greedy_prologue(m, g, src, B, S, max_len, start, f, greedy_fused(m->cfg, S, max_len), st));
  return greedy_steps(m, g, B, S, max_len, st);
}

}  // namespace qtx

using namespace qtx;

extern "C" {

size_t qtx_encoder_workspace_size(const qtx_model* m, int32_t B, int32_t S) {
  return m ? enc_ws(m->cfg, B, S) : 0;
}
size_t qtx_decoder_workspace_size(const qtx_model* m, int32_t B, int32_t T, int32_t S) {
  return m ? dec_ws(m->cfg, B, T, S) : 0;
}
size_t qtx_greedy_workspace_size(const qtx_model* m, int32_t B, int32_t S, int32_t max_len) {
  return m ? greedy_ws(m->cfg, decode_groups(B), B, S, max_len) : 0;
}
size_t qtx_greedy_scored_workspace_size(const qtx_model* m, int32_t B, int32_t S,
                                        int32_t max_len) {
  return m && max_len >= 1 ? greedy_ws(m->cfg, decode_groups(B), B, S, max_len, true) : 0;
}

int32_t qtx_encoder_forward_fault(const qtx_model* m, const float* x, const uint8_t* src_mask,
                                  int32_t B, int32_t S, float* out, void* ws, size_t ws_bytes,
                                  const qtx_fault* f, void* stream) {
  if (!m || !x || !src_mask || !out || !ws) return fail(QTX_E_INVALID, "null argument");
  if (B <= 0 || S <= 0 || S > 512) return fail(QTX_E_INVALID, "bad shape B=%d S=%d", B, S);
  RC(check_workspace(ws_bytes, enc_ws(m->cfg, B, S)));
  RC(check_fault(m, f, 0, B, S, 0));
  hipStream_t st = (hipStream_t)stream;
  CallFrame fr;
  RC(frame_begin(m, ws, ws_bytes, st, true, &fr));
  if (!enc_split(B) || (f && f->kind != QTX_FAULT_NONE)) {
    Scratch s = carve_scratch(fr.ar, m->cfg, (long)B * S);
    s.status = fr.status;
    return encoder_run(m, x, src_mask, B, S, out, s, st, f);
  }
  // The model's second stream and its three events are shared by every caller: the lock
  // is held across the whole record / wait sequence, so two threads' fork, lag and join
  // records cannot interleave (a wait always pairs with its own call's record).
  qtx_model* mm = const_cast<qtx_model*>(m);
  std::lock_guard<std::mutex> lk(mm->mu);
  DeviceGuard dg(mm->device);
  if (!mm->estream) {
    HIPCHK(hipStreamCreateWithFlags(&mm->estream, hipStreamNonBlocking));
    HIPCHK(hipEventCreateWithFlags(&mm->ev_fork, hipEventDisableTiming));
    HIPCHK(hipEventCreateWithFlags(&mm->ev_lag, hipEventDisableTiming));
    HIPCHK(hipEventCreateWithFlags(&mm->ev_join, hipEventDisableTiming));
  }
  const int B0 = B / 2, B1 = B - B0;
  const long D = m->cfg.d_model;
  Scratch s0 = carve_scratch(fr.ar, m->cfg, (long)B0 * S);
  Scratch s1 = carve_scratch(fr.ar, m->cfg, (long)B1 * S);
  s0.status = s1.status = fr.status;
  // half 1 starts when half 0's first layer has passed its QKV GEMM (ev_lag)
  HIPCHK(hipEventRecord(mm->ev_fork, st));
  HIPCHK(hipStreamWaitEvent(mm->estream, mm->ev_fork, 0));
  RC(encoder_run(m, x, src_mask, B0, S, out, s0, st, nullptr, mm->ev_lag));
  HIPCHK(hipStreamWaitEvent(mm->estream, mm->ev_lag, 0));
  RC(encoder_run(m, x + (long)B0 * S * D, src_mask + (long)B0 * S, B1, S, out + (long)B0 * S * D,
                 s1, mm->estream, nullptr));
  HIPCHK(hipEventRecord(mm->ev_join, mm->estream));
  HIPCHK(hipStreamWaitEvent(st, mm->ev_join, 0));
  return QTX_OK;
}

int32_t qtx_encoder_forward(const qtx_model* m, const float* x, const uint8_t* src_mask,
                            int32_t B, int32_t S, float* out, void* ws, size_t ws_bytes,
                            void* stream) {
  return qtx_encoder_forward_fault(m, x, src_mask, B, S, out, ws, ws_bytes, nullptr, stream);
}

int32_t qtx_decoder_forward_fault(const qtx_model* m, const float* y, const float* memory,
                                  const uint8_t* src_mask, const uint8_t* tgt_mask,
                                  int32_t tgt_mask_batched, int32_t B, int32_t T, int32_t S,
                                  float* out, void* ws, size_t ws_bytes, const qtx_fault* f,
                                  void* stream) {
  if (!m || !y || !memory || !src_mask || !tgt_mask || !out || !ws)
    return fail(QTX_E_INVALID, "null argument");
  // the rule of every decoder-side entry: at most 512 positions and no more than the
  // positional table holds (y = tgt_embed(ys) exists for no longer target)
  if (bad_decode_shape(m->cfg, B, S, T))
    return fail(QTX_E_INVALID, "bad shape B=%d T=%d S=%d (table %d)", B, T, S, m->cfg.max_len);
  RC(check_workspace(ws_bytes, dec_ws(m->cfg, B, T, S)));
  RC(check_fault(m, f, 1, B, T, S));
  hipStream_t st = (hipStream_t)stream;
  const qtx_config& c = m->cfg;
  const int D = c.d_model, M = B * T;
  CallFrame fr;   // no status word: frame_begin
  RC(frame_begin(m, ws, ws_bytes, st, false, &fr));
  Scratch s = carve_scratch(fr.ar, c, M);
  CrossKV x = carve_cross(fr.ar, c, (long)B * S);
  RC(cross_kv(m, memory, B * S, x, st, f));
  HIPCHK(hipMemcpyAsync(s.x, y, (size_t)M * D * 4, hipMemcpyDeviceToDevice, st));
  return decoder_body(m, s, x, src_mask, tgt_mask, tgt_mask_batched ? (long)T * T : 0, B, T, S, out,
                      f, st);
}

int32_t qtx_decoder_forward(const qtx_model* m, const float* y, const float* memory,
                            const uint8_t* src_mask, const uint8_t* tgt_mask,
                            int32_t tgt_mask_batched, int32_t B, int32_t T, int32_t S,
                            float* out, void* ws, size_t ws_bytes, void* stream) {
  return qtx_decoder_forward_fault(m, y, memory, src_mask, tgt_mask, tgt_mask_batched, B, T, S,
                                   out, ws, ws_bytes, nullptr, stream);
}

// the plain (scored = false: top_ids / top_logp unused) and the scored greedy decode
static int32_t greedy_decode(const qtx_model* m, const int64_t* src, const uint8_t* src_mask,
                             int32_t B, int32_t S, int32_t max_len, int64_t start, int64_t* ids,
                             bool scored, int64_t* top_ids, float* top_logp, void* ws,
                             size_t ws_bytes, const qtx_fault* f, void* stream) {
  if (!m || !src || !src_mask || !ids || !ws ||
      (scored && max_len > 1 && (!top_ids || !top_logp)))   // (max_len 1: no step, no entry)
    return fail(QTX_E_INVALID, "null argument");
  const qtx_config& c = m->cfg;
  RC(check_decode_shape(c, B, S, max_len));
  if (scored) RC(check_top2_vocab(c));
  if (scored) RC(refuse_dbg_tail("scored decode"));
  const Groups gr = decode_groups(B);
  RC(check_workspace(ws_bytes, greedy_ws(c, gr, B, S, max_len, scored)));
  if (f && f->kind != QTX_FAULT_NONE && f->module != 0)
    return fail(QTX_E_UNSUPPORTED, "greedy decode takes encoder faults (decoder faults: "
                                   "qtx_decoder_forward_fault on the step's prefix)");
  RC(check_fault(m, f, 0, B, S, 0));
  hipStream_t st = (hipStream_t)stream;
  CallFrame fr;
  RC(frame_begin(m, ws, ws_bytes, st, true, &fr));
  GreedyWS g = carve_greedy(fr.ar, c, gr, B, S, max_len, scored);
  g.enc.status = fr.status;
  // the decode reads the workspace's copy of src_mask and writes the workspace's ids
  // (the captured graphs then depend on the workspace only); ids go out at the end
  HIPCHK(hipMemcpyAsync(g.mask, src_mask, (size_t)B * S, hipMemcpyDeviceToDevice, st));
  RC(greedy_run(m, g, src, B, S, max_len, start, f, st));
  return copy_out(g.ids, g.top_ids, g.top_logp, B, max_len, ids, scored ? top_ids : nullptr,
                  top_logp, st);
}

int32_t qtx_greedy_decode_fault(const qtx_model* m, const int64_t* src,
                                const uint8_t* src_mask, int32_t B, int32_t S, int32_t max_len,
                                int64_t start, int64_t* ids, void* ws, size_t ws_bytes,
                                const qtx_fault* f, void* stream) {
  return greedy_decode(m, src, src_mask, B, S, max_len, start, ids, false, nullptr, nullptr, ws,
                       ws_bytes, f, stream);
}

int32_t qtx_greedy_decode_scored(const qtx_model* m, const int64_t* src,
                                 const uint8_t* src_mask, int32_t B, int32_t S, int32_t max_len,
                                 int64_t start, int64_t* ids, int64_t* top_ids, float* top_logp,
                                 void* ws, size_t ws_bytes, const qtx_fault* f, void* stream) {
  return greedy_decode(m, src, src_mask, B, S, max_len, start, ids, true, top_ids, top_logp, ws,
                       ws_bytes, f, stream);
}

int32_t qtx_greedy_decode(const qtx_model* m, const int64_t* src, const uint8_t* src_mask,
                          int32_t B, int32_t S, int32_t max_len, int64_t start, int64_t* ids,
                          void* ws, size_t ws_bytes, void* stream) {
  return qtx_greedy_decode_fault(m, src, src_mask, B, S, max_len, start, ids, ws, ws_bytes,
                                 nullptr, stream);
}

}  // extern "C"

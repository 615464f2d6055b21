/* qtx_enctrials.h — the table-aware row-complete GEMM of the encoder-side fault trials.
 *
 * The reference's campaign (parallelized_inject_onnx_transformer.py:536-860) draws its targets
 * from the encoder's and the memory K/V projections' MatMuls (input/encoder/matmul_*.json) as
 * well as the decoder's.  Those MatMuls run once per sentence, at M = B * S token rows, on the
 * row-complete int8 GEMM (qtx.h qtx_linear_rows).  Its fault form takes ONE fault per launch
 * (inject_utils/layers.py:48-84: one perturbed operand element or one replaced output); the
 * entry below takes a table with one entry per token row, so that every sentence of a batch can
 * carry a fault of its own.  Sentences never interact: every op is per token or per (sentence,
 * head) and the int32 accumulators are exact, so a row computed here equals, bit for bit, the
 * same row of the single-fault GEMM on that sentence alone.
 *
 * This header declares what qtx.h does not; it includes qtx.h and follows its conventions
 * (status codes, qtx_last_error, device pointers unless stated, streams as void*). */
#ifndef QTX_ENCTRIALS_H
#define QTX_ENCTRIALS_H

#include "qtx.h"

#ifdef __cplusplus
extern "C" {
#endif

/* One token row's entry, in the coordinates of the GEMM launch that computes its MatMul (the
 * linear's column offset inside a fused Q|K|V or K|V launch already added):
 *   kind 0  none
 *   kind 1  INPUT:  A[row, col] has bit `bit` flipped: acc[row, n] += (flip(a) - a) * W[n, col]
 *           for the output columns n in [lo, hi)
 *   kind 2  WEIGHT: W[wrow, col] has bit `bit` flipped as this row sees it:
 *           acc[row, wrow] += A[row, col] * (flip(w) - w).  A weight fault of a sentence is
 *           written into every token row of that sentence inside the fault's row window.
 *   kind 3  OUTPUT: the MatMul output (before bias, and before ReLU) at (row, col) is `value`
 * `row` is the entry's own index in the table.  An entry is applied only by the launch whose
 * (layer, gemm) it names; `step` is reserved (0). */
typedef struct {
  int32_t step, layer, gemm, kind;
  int32_t bit, col, wrow, lo, hi;
  float value;
} qtx_row_fault;

/* The row-complete GEMM of qtx.h, qtx_linear_rows, in its row-major form with a fault table: args->kp must be 0, 8-bit
 * weights, args->ksplit 0; every epilogue (epi 0..3) and every output exactly as qtx_linear_rows
 * documents them.  tab: HOST array [args->M], or NULL for no fault (then the launch is
 * qtx_linear_rows' own).  Output row m takes the corrections of tab[m] alone, and only if
 * tab[m].layer == layer and tab[m].gemm == gemm; the expressions and their order are the
 * single-fault row GEMM's: the exact int32 delta is added to the accumulator before the float
 * epilogue y = ((float(acc) * sa[m]) * sw[n]) + bias[n], an OUTPUT entry gives y = value +
 * bias[col] before the ReLU of epi 2 / 3.  For epi 2 followed by epi 3 (the two FFN1 passes) pass
 * the same table to both.
 * Refused with QTX_E_INVALID before anything is launched, the row named in the error text: a
 * kind outside 0..3, bit outside 0..7, col outside [0, K) (INPUT, WEIGHT) or [0, N) (OUTPUT),
 * wrow outside [0, N), a window outside 0 <= lo <= hi <= N — for every entry, whichever launch
 * it names.  QTX_E_UNSUPPORTED: kp != 0 or ksplit > 1.  Every other rule is qtx_linear_rows'.
 * With a table the call allocates device memory for it and synchronises the stream (a test and
 * campaign-building entry, not a hot path). */
int32_t qtx_linear_rows_faults(const qtx_row_gemm* args, const qtx_row_fault* tab, int32_t layer,
                               int32_t gemm, void* stream);

/* ---- one encoder-side fault trial per sentence in one scored greedy decode ----
 * The campaign (parallelized_inject_onnx_transformer.py:536-860) injects into the encoder's
 * MatMuls (input/encoder/matmul_*.json) and into the memory K/V projections of the decoder
 * (MatMul_{2L}, MatMul_{2L+1}) as it does into the decoder's own; both run once per sentence.
 * faults: HOST array [B].  faults[b].kind == QTX_FAULT_NONE: a golden row.  Otherwise one of
 *   module 0, any encoder target: linear Q K V O FFN1 FFN2 QK PV;
 *   module 1, linear QTX_LIN_CK or QTX_LIN_CV.
 * Row b of ids / top_ids / top_logp equals, bit for bit, the stand-alone B = 1 call on sentence b
 * alone (the same S, source row and mask row): for module 0 the scored greedy decode of qtx.h
 * with that fault, for CK / CV the scored kvfault decode of qtx.h with that fault at step 0.  So
 * the coordinates are that call's: linear INPUT* / OUTPUT row = token i in [0, S); linear WEIGHT*
 * row = out channel, a WEIGHT16 window over the sentence's own S rows; attention targets with
 * b = 0 and Sq = Sk = S; CK / CV rows = the sentence's S memory tokens.  A WEIGHT fault is seen
 * by its own sentence only; a fault on a padded token is legal (and mostly masked); a table of
 * all NONE is the golden scored decode.  Two faults in one sentence are not expressed here.
 * Scored form only: top_ids and top_logp are required (max_len > 1).  Writes exactly ids
 * [B, max_len], top_ids and top_logp [B, max_len-1, 2].
 * Schedule: the table is expanded on the host to one entry per token row [B * S] and uploaded
 * once into the workspace (the call waits for the stream once, for that upload); the encoder runs
 * row-major through the table-aware row GEMM (launches no trial names take the plain instance),
 * attention-target trials recompute their (sentence, head) rows after the golden attention; with
 * a CK / CV trial the cross K/V run layer by layer through the table form; then the scored steps
 * run exactly as in the scored greedy decode (same graphs and path selection).
 * Refused before anything is launched, the row named in the error text: faults NULL; per row
 * what the stand-alone call refuses for B = 1 (QTX_E_INVALID; QTX_E_UNSUPPORTED with 4-bit
 * weights); a module-1 fault other than CK / CV: QTX_E_UNSUPPORTED (the kvtrials decode of qtx.h
 * takes it); a short workspace: QTX_E_WORKSPACE.  B * tgt_vocab and B * max_len * d_model below
 * 2^30.  ws: qtx_greedy_enctrials_workspace_size bytes; a dfault resume header on it is dropped. */
size_t qtx_greedy_enctrials_workspace_size(const qtx_model* m, int32_t B, int32_t S,
                                           int32_t max_len);
int32_t qtx_greedy_decode_enctrials(const qtx_model* m, const int64_t* src, const uint8_t* src_mask,
                                    int32_t B, int32_t S, int32_t max_len, int64_t start,
                                    int64_t* ids, int64_t* top_ids, float* top_logp, void* ws,
                                    size_t ws_bytes, const qtx_fault* faults, void* stream);

#ifdef __cplusplus
}
#endif
#endif  /* QTX_ENCTRIALS_H */

/* qtx.h — C-ABI of libqtx.so, the MI355X (gfx950) W8A8 transformer inference path.
 *
 * This library replaces the ONNXRuntime-CPU execution of the reference's exported
 * encoder/decoder graphs (gebegebegebe/onnx-transformer).  Each entry point names the
 * reference interface it stands in for:
 *
 *   qtx_encoder_forward  <- ort.InferenceSession('encoder_fixed.onnx').run(None,
 *                           {global_in, global_in_1})       reference/onnx_reference_inference.py:625-626
 *                           / run_module("encoder", ...)     onnx_optimized_inference.py:297-304
 *   qtx_decoder_forward  <- InferenceSession('decoder_fixed.onnx').run(None, {global_in,
 *                           global_in_1, global_in_2, global_in_3})
 *                                                            reference/onnx_reference_inference.py:633-639
 *   qtx_greedy_decode    <- greedy_decode(model, src, src_mask, max_len, start_symbol)
 *                                                            reference/onnx_reference_inference.py:622-646
 *                                                            (batched form batch_output.py:659-673)
 *   qtx_embed            <- model.get_src_embed / get_tgt_embed  encoder_decoder.py:54-58
 *   qtx_generator        <- model.generator(x) + torch.max     generator.py:14-15,
 *                                                            reference/onnx_reference_inference.py:640-641
 *   qtx_greedy_decode_scored, qtx_generator_top2
 *                        <- the campaign's torch.topk(prob, 2, dim=1) of a step's generator
 *                           output           parallelized_inject_onnx_transformer.py:718-740
 *   qtx_score_targets, qtx_score_rows, qtx_score_logits
 *                        <- EncoderDecoder.forward on Batch.tgt / tgt_y + log_softmax
 *                           encoder_decoder.py:19-23, batch.py:17-30, generator.py:15
 *   qtx_row_quant        <- quantize_activation_per_token_absmax / quantize_weight_per_channel_absmax
 *                                                            quant_linear.py:30-43 / :5-17
 *   qtx_layernorm_quant  <- LayerNorm.forward (+ the next W8A8Linear's act quant)
 *                                                            layer_norm.py:12-15
 *   qtx_linear_i8        <- W8A8Linear.forward (int8 GEMM + dequant epilogue) quant_linear.py:111-119
 *   qtx_linear_rows      <- W8A8Linear.forward + the per-token quantizer / LayerNorm that
 *                           consumes its output (fused epilogues)        quant_linear.py:111-119
 *   qtx_attention_i8     <- MultiHeadedAttention.attention     attention.py:23-36
 *
 * Conventions: every pointer is a DEVICE pointer (HIP, gfx950) unless the
 * parameter says host; buffers are caller-owned; no entry point allocates device memory
 * except qtx_model_create; `stream` is a hipStream_t (0 = default stream); every function
 * returns 0 on success or a non-zero qtx_status, with a message in qtx_last_error().
 * Thread-compatible: one stream per thread; the model handle is read-only after creation.
 * Alignment: the kernels move rows in 16-byte vectors, so every device buffer must start
 * 16-byte aligned (any hipMalloc'd base does).  The entry points that take a stride
 * (qtx_linear_rows: ldo8 / o8_ts; qtx_skinny_linear: ldx; qtx_decode_attention: ldy) check
 * the base and the stride on the host and return QTX_E_INVALID before anything is launched.
 * 16 bytes is all any entry point needs, and any 16-byte aligned base is accepted: a view
 * into a larger allocation, a sub-allocated arena, a workspace at 16 (mod 256) (its carved
 * sub-buffers then sit at 16 (mod 256) too).  tests/test_gpu_bounds.py (ids align16) and
 * tests/test_gpu_min_align.py run every entry point that takes a device pointer with every
 * pointer at 16 (mod 256) against the oracle.
 * Extents are exact: a call writes nothing outside the output and scratch extents stated
 * here, and writes every element of them (tests/test_gpu_bounds.py).
 */
#ifndef QTX_H_
#define QTX_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef enum {
  QTX_OK = 0,
  QTX_E_INVALID = 1,   /* bad argument / shape (the reference raises on shape mismatch) */
  QTX_E_HIP = 2,       /* a HIP runtime error, message in qtx_last_error() */
  QTX_E_WORKSPACE = 3, /* workspace too small: see qtx_*_workspace_size */
  QTX_E_UNSUPPORTED = 4,
  QTX_E_DEVICE = 5     /* a kernel flagged an error it cannot repair in the calling
                        * thread's device status word on the model (k_gemm_wsx: FFN1 row-max
                        * exchange timed out, outputs invalid); reported (and cleared) by
                        * qtx_model_check — no later call clears it before that */
} qtx_status;

typedef struct qtx_model qtx_model;

/* make_model hyper-parameters (model.py:15-16).  d_model must be 512, d_ff a multiple of
 * 256 up to 2048, n_heads * 64 == d_model.  weight_bits: 8 (W8A8) or 4 (packed int4).
 * Every config qtx_model_create accepts runs every model-level call (tests/
 * test_gpu_model_configs.py; the kernel chain per config: DESIGN.md, supported shapes):
 * the row-GEMM encoder / decoder chain needs d_ff % 512 == 0, the fused decode step
 * d_ff 512 or 2048, tgt_vocab <= 8192 and S, max_len <= 128; any other config or length takes
 * the generic chain and the unfused step, with the same results.
 * max_len: the rows of the positional table.  Every decoder-side entry takes up to 512 target
 * positions and never more than the table holds (the same for S); 129 .. 512 positions run
 * the unfused step and the generic attention kernel (supported shapes;
 * tests/test_gpu_long_target.py). */
typedef struct {
  int32_t src_vocab, tgt_vocab, n_layers, d_model, d_ff, n_heads, max_len, weight_bits;
} qtx_config;

const char* qtx_last_error(void);
const char* qtx_version(void);

/* Number of float tensors qtx_model_create expects, and their names in order (the
 * reference state_dict keys; see qtx/weights.py:tensor_order).  names may be NULL. */
int32_t qtx_model_tensor_count(const qtx_config* cfg);

/* Build the device-resident quantized model from fp32 DEVICE tensors given in
 * tensor_order, plus the positional table pe [max_len, d_model].  Weights are quantized
 * per output channel on the device (quant_linear.py:5-17).  The inputs may be freed after
 * the call returns (it synchronizes `stream`). */
int32_t qtx_model_create(const qtx_config* cfg, const float* const* tensors,
                         int32_t n_tensors, const float* pe, void* stream, qtx_model** out);
int32_t qtx_model_destroy(qtx_model* m);
/* bytes of device memory owned by the model */
size_t qtx_model_device_bytes(const qtx_model* m);

/* Read-only views of the model's device tensors, for the op-by-op traced executor
 * (qtx/trace.py: the reference's node-by-node executor storing every intermediate by
 * name, onnx_optimized_inference.py:32-57).  module 0 = encoder, 1 = decoder; index in the
 * layer's weights.py:linear_names order (encoder 0..3 self_attn.linears, 4 w_1, 5 w_2;
 * decoder 0..3 self_attn, 4..7 src_attn, 8 w_1, 9 w_2).  q: int8 [N,K] (weight_bits 4:
 * packed [N,K/2]), s [N], b [N]: the per-channel quantized weight (quant_linear.py:5-17). */
int32_t qtx_model_linear(const qtx_model* m, int32_t module, int32_t layer, int32_t index,
                         const void** q, const float** s, const float** b, int32_t* N,
                         int32_t* K);
/* LayerNorm a_2 / b_2 [d_model]: sublayer index within the layer, or layer = -1 for the
 * stack's final norm (encoder.py:18, decoder.py:16). */
int32_t qtx_model_norm(const qtx_model* m, int32_t module, int32_t layer, int32_t sub,
                       const float** a, const float** b);

/* Workspace sizes (bytes) for the model-level calls. */
size_t qtx_encoder_workspace_size(const qtx_model* m, int32_t B, int32_t S);
size_t qtx_decoder_workspace_size(const qtx_model* m, int32_t B, int32_t T, int32_t S);
size_t qtx_greedy_workspace_size(const qtx_model* m, int32_t B, int32_t S, int32_t max_len);

/* Encoder graph: x [B,S,d] fp32 (= src_embed(src), "global_in"), src_mask [B,S] uint8
 * (nonzero = keep, "global_in_1" [B,1,S]) -> out [B,S,d] fp32 ("global_out"). */
int32_t qtx_encoder_forward(const qtx_model* m, const float* x, const uint8_t* src_mask,
                            int32_t B, int32_t S, float* out, void* ws, size_t ws_bytes,
                            void* stream);

/* Decoder graph: y [B,T,d] (= tgt_embed(ys), "global_in"), memory [B,S,d] ("global_in_1"),
 * src_mask [B,S] uint8 ("global_in_2"), tgt_mask uint8 [T,T] or [B,T,T]
 * (tgt_mask_batched = 0/1, "global_in_3") -> out [B,T,d] ("global_out").
 * T or S above 512 or above the positional table (cfg.max_len): QTX_E_INVALID, nothing
 * written.  Past 128 target positions the self-attention runs the generic kernel
 * (k_attention, up to 512 keys) under the [T,T] mask. */
int32_t qtx_decoder_forward(const qtx_model* m, const float* y, const float* memory,
                            const uint8_t* src_mask, const uint8_t* tgt_mask,
                            int32_t tgt_mask_batched, int32_t B, int32_t T, int32_t S,
                            float* out, void* ws, size_t ws_bytes, void* stream);

/* Whole greedy decode: src ids int64 [B,S], src_mask uint8 [B,S] -> ids int64 [B,max_len]
 * (ids[:,0] = start, then max_len-1 greedy steps with no EOS exit, like the reference).
 * KV-cached; results equal the reference's full-prefix recompute (causal invariance). */
int32_t qtx_greedy_decode(const qtx_model* m, const int64_t* src, const uint8_t* src_mask,
                          int32_t B, int32_t S, int32_t max_len, int64_t start, int64_t* ids,
                          void* ws, size_t ws_bytes, void* stream);

/* Synchronise `stream`, then report (and clear) the calling thread's device status word on
 * this model: QTX_OK, or QTX_E_DEVICE if a kernel of any of the thread's model-level calls on
 * it since its last check raised an error (the bits accumulate; nothing but this check clears
 * them).  Thread affinity: the word belongs to the thread that made the calls, so check from
 * that thread; a thread that made no encoder / greedy-decode call on the model gets QTX_OK.
 * A thread claims its word at its first encoder / greedy-decode call on the model and returns
 * it when it exits; at most 256 threads may hold one per model at a time — the call of a
 * further thread fails with QTX_E_UNSUPPORTED instead of sharing a word. */
int32_t qtx_model_check(const qtx_model* m, void* stream);

/* ---- fault injection (the reference's campaigns: inject_utils/layers.py:48-84,
 * onnx_optimized_inference.py:59-204, parallelized_inject_onnx_transformer.py:536-720) ----
 * One fault per run, at one QuantLinear MatMul of one module.  Targets use the reference's
 * ONNX MatMul numbering: encoder layer L MatMul_{8L+i}, i = QTX_LIN_Q/K/V/O/
 * FFN1/FFN2; decoder layer L MatMul_{12+12L+i} (self Q/K/V/O, cross Q/O, FFN) and the
 * memory K/V projections MatMul_{2L}, MatMul_{2L+1} (QTX_LIN_CK / QTX_LIN_CV).
 * Kinds (rows index the module's flattened [B*S] or [B*T] tokens; cross K/V: memory tokens):
 *   INPUT     bit `bit` of the int8 input q[row, col] flipped (every output column)
 *   WEIGHT    bit `bit` of the int8 weight q[row = out channel, col] flipped (every row)
 *   INPUT16   as INPUT, the output perturbation kept on columns win_start .. +win_len (<= 16)
 *   WEIGHT16  as WEIGHT, the perturbation kept on rows win_start .. +win_len (<= 16)
 *   OUTPUT    the MatMul output (before bias) at (row, col) replaced by `value`
 *             (RANDOM: a random float; RANDOM_BITFLIP: a bit-flipped golden value)
 * Attention MatMuls (QTX_LIN_QK / PV, decoder cross QTX_LIN_CQK / CPV; the reference's
 * "FirstMatMul" / "SecondMatMul" campaign targets) on one (sentence b, head h), Sq query
 * and Sk key rows per sentence:
 *   QK  INPUT*:  q element  row = b*Sq + i, col = h*64 + d   (INPUT16 window: keys)
 *       WEIGHT*: k element  row = b*Sk + j, col = h*64 + d   (WEIGHT16 window: query rows)
 *       OUTPUT:  QK^T value row = b*Sq + i, col = h*Sk + j   (before the / 8 and the mask)
 *   PV  INPUT*:  P*127 int  row = b*Sq + i, col = h*Sk + j   (INPUT16 window: head dims)
 *       WEIGHT*: v element  row = b*Sk + j, col = h*64 + d   (WEIGHT16 window: query rows)
 *       OUTPUT:  context    row = b*Sq + i, col = h*64 + d
 * Requires 8-bit weights (QTX_E_UNSUPPORTED otherwise); any d_ff. */
typedef enum {
  QTX_FAULT_NONE = 0, QTX_FAULT_INPUT = 1, QTX_FAULT_WEIGHT = 2, QTX_FAULT_INPUT16 = 3,
  QTX_FAULT_WEIGHT16 = 4, QTX_FAULT_OUTPUT = 5
} qtx_fault_kind;
typedef enum {
  QTX_LIN_Q = 0, QTX_LIN_K = 1, QTX_LIN_V = 2, QTX_LIN_QK = 3, QTX_LIN_PV = 4, QTX_LIN_O = 5,
  QTX_LIN_FFN1 = 6, QTX_LIN_FFN2 = 7, QTX_LIN_CQ = 8, QTX_LIN_CK = 9, QTX_LIN_CV = 10,
  QTX_LIN_CO = 11, QTX_LIN_CQK = 12, QTX_LIN_CPV = 13
} qtx_linear_id;
typedef struct {
  int32_t kind;      /* qtx_fault_kind */
  int32_t module;    /* 0 encoder, 1 decoder */
  int32_t layer;
  int32_t linear;    /* qtx_linear_id */
  int64_t row, col;  /* see the kinds above */
  int64_t win_start;
  int32_t win_len;
  int32_t bit;       /* 0..7 */
  float value;       /* OUTPUT */
  int32_t reserved;
} qtx_fault;

/* qtx_encoder_forward / qtx_decoder_forward / qtx_greedy_decode with one fault (host
 * pointer; NULL or kind NONE = golden run).  The greedy decode takes encoder faults. */
int32_t qtx_encoder_forward_fault(const qtx_model* m, const float* x, const uint8_t* src_mask,
                                  int32_t B, int32_t S, float* out, void* ws, size_t ws_bytes,
                                  const qtx_fault* fault, void* stream);
int32_t qtx_decoder_forward_fault(const qtx_model* m, const float* y, const float* memory,
                                  const uint8_t* src_mask, const uint8_t* tgt_mask,
                                  int32_t tgt_mask_batched, int32_t B, int32_t T, int32_t S,
                                  float* out, void* ws, size_t ws_bytes,
                                  const qtx_fault* fault, void* stream);
int32_t qtx_greedy_decode_fault(const qtx_model* m, const int64_t* src,
                                const uint8_t* src_mask, int32_t B, int32_t S, int32_t max_len,
                                int64_t start, int64_t* ids, void* ws, size_t ws_bytes,
                                const qtx_fault* fault, void* stream);

/* ---- scored decode: the two best tokens of every step and their log-probabilities ----
 * The reference's campaign prints torch.topk(prob, 2, dim=1) of the generator's output at the
 * step it corrupts (parallelized_inject_onnx_transformer.py:718-740, prob = generator.py:15's
 * log_softmax): the winner, the runner-up and their margin.  Semantics of every entry point
 * below, for one logits row x[0..V):
 *   logp  = the canonical log-softmax: z = x - max, lse = log(lane-split sum of qexp(z)),
 *           logp = z - lse, bit-identical to oracle/qtx_oracle.py:log_softmax_argmax(x)[0]
 *           (the log of the denominator is csrc/qtx_common.h:qlog, the oracle host's float32
 *           log restated operation by operation — not the platform logf).
 *   top 1 = the first index of the maximum logp: the rule of qtx_greedy_decode, so the token
 *           the plain decode picks (see the note below on rows the plain tail resolves by logf).
 *   top 2 = the first index of the maximum logp over v != top 1.
 *   The selection is on logp, not on the logits: two distinct logits can round to the same
 *   logp, and then the lower index wins.  "Larger logp, then smaller index" is a total order,
 *   so the pair does not depend on the order of the reduction.
 *   Values: logp[top 1], logp[top 2].  They always equal torch.topk(logp, 2).values; the
 *   indices equal torch.topk's wherever the two values (and the third best) are distinct —
 *   torch.topk does not promise the first index among equal values.
 *   A non-finite row (any NaN or +inf, or only -inf) has an all-NaN log-softmax under torch:
 *   ids (0, 1), both values NaN (the 0 is what the plain decode writes).
 *   V = tgt_vocab >= 2, else QTX_E_INVALID.
 * Note: qtx_greedy_decode's tail evaluates lse (with the platform's logf) only for rows with
 * two logits within 4e-6 of each other; on such a row a 1-ulp difference between logf and
 * qlog can move a logp collision, so top 1 may then differ from the plain decode's token.
 * On every other row the two agree by construction (the maximum logit is the unique winner).
 *
 * qtx_greedy_decode_fault plus top_ids int64 [B, max_len-1, 2] and top_logp float
 * [B, max_len-1, 2]: entry t describes the choice of ids[:, t+1], top_ids[:, :, 0] ==
 * ids[:, 1:].  fault: NULL or an encoder fault.  Same path selection as the plain decode
 * (fused step with graphs, eager, sub-batches, graphs of several steps, unfused step; the
 * scored step has its own captured graphs).  The fused step's tail (csrc/qtx_decode.hip
 * k_top2_embed) takes tgt_vocab <= 8192, as the plain one: a model with a larger vocabulary
 * decodes, plain and scored, with the unfused step, whose tail has no cap (the per-op
 * qtx_decode_argmax_embed / qtx_decode_top2_embed keep the cap).  B * tgt_vocab < 2^30.
 * Writes exactly ids [B, max_len], top_ids and top_logp [B, max_len-1, 2].
 * ws: qtx_greedy_scored_workspace_size bytes (qtx_greedy_workspace_size is unchanged).
 * QTX_E_UNSUPPORTED with the diagnostic QTX_DBG_TAIL switch. */
size_t qtx_greedy_scored_workspace_size(const qtx_model* m, int32_t B, int32_t S,
                                        int32_t max_len);
int32_t qtx_greedy_decode_scored(const qtx_model* m, const int64_t* src,
                                 const uint8_t* src_mask, int32_t B, int32_t S, int32_t max_len,
                                 int64_t start, int64_t* ids, int64_t* top_ids, float* top_logp,
                                 void* ws, size_t ws_bytes, const qtx_fault* fault, void* stream);

/* ---- KV-cached greedy decode with one DECODER fault, and its resume for sweeps ----
 * The campaign's trial (parallelized_inject_onnx_transformer.py:536-740) corrupts only the
 * decoder run of step i = fault_step (its target_inference_number - 1): that step's token and
 * nothing else directly.  So steps 0 .. i run KV-cached and golden; step i's cached run is the
 * campaign's golden run (its out_2) of the same prefix; the faulty token comes from ONE faulty
 * full-prefix decoder pass over ids[:, :i+1] (the fault's row indexes the whole batch's
 * [B * (i+1)] tokens; cross K/V rows: [B * S]) with the generator on each sentence's last
 * row; steps > i run KV-cached from the faulty token.  The caches are append-only: row i was
 * written from the golden input of step i, and the cached cross K/V stay golden.
 *
 * qtx_greedy_decode_dfault (:536-740): bit for bit the campaign loop's result.
 *   Scored form (top_ids and top_logp given): ids, and every step's top 2 under the scored
 *   decode's rules above; entry fault_step holds the faulty step's top 2.
 *   Plain form (top_ids == top_logp == NULL): ids only; the faulty step's token follows the
 *   plain rule (qtx_generator: first index of the maximum logp, platform logf), the cached
 *   steps the plain decode's tail.
 *   rec_ids int64 / rec_logp float [B, 2, 2] (both or neither; NULL allowed): [:, 0, :] the
 *   golden and [:, 1, :] the faulty top 2 of the corrupted step (:711-740).
 *   fault_step >= max_len - 1: the fault is never applied — a golden decode, rec_* untouched
 *   (the fault's coordinates are then not checked).
 *   Path selection as the plain and scored decode: unfused step; QTX_NO_GRAPH eager fused
 *   steps; else fused steps captured at the device counter's position as graphs of
 *   QTX_GRAPH_STEPS (default 8) steps and of one step, with graphs ending at the fault step;
 *   QTX_DECODE_GROUPS / two sub-batches from B = 512 (the faulty pass runs once over the whole
 *   batch after they join).  The tail is never folded into the next step's first launch here.
 *   Refused before anything is launched: fault NULL, kind NONE or module != 1, fault_step < 0,
 *   a coordinate outside the step's shapes (T = fault_step + 1): QTX_E_INVALID; 4-bit weights:
 *   QTX_E_UNSUPPORTED.  B * tgt_vocab and B * max_len * d_model below 2^30.
 *   Writes exactly ids, top_ids, top_logp, rec_ids, rec_logp.  ws:
 *   qtx_greedy_dfault_workspace_size bytes.
 *
 * qtx_greedy_dfault_resume (:536-740, one more trial on the same sentences): runs on a
 * workspace a SCORED qtx_greedy_decode_dfault or an earlier resume left, for the same
 * (m, B, S, max_len, src); scored outputs as above.  The library keeps a validity header per
 * workspace in a HOST-side table of the model, keyed by the workspace pointer: the shapes, the
 * highest step n up to which cache rows and ids are golden, and whether the workspace's second
 * copy of the golden ids / top 2 is complete (it is after a never-applied decode).  Header
 * missing or other shapes, or fault_step > n: QTX_E_INVALID.  Any other qtx call given that
 * workspace drops the header, and the header's nonce is also stamped into the workspace and
 * compared (one 8-byte copy) before a resume launches anything: memory that was overwritten
 * since is refused (QTX_E_INVALID) where the stamp shows it.  The caller must not write it.
 *   The faulty pass runs at fault_step from the golden prefix, the record is written, and the
 *   per-sentence "token changed" flags are copied to changed_host[B] (may be NULL) — one small
 *   synchronising copy.  No token changed and the golden copy complete: the outputs are the
 *   golden decode's with entry fault_step replaced by the faulty top 2; no step runs, n stays.
 *   Otherwise steps fault_step+1 .. run KV-cached from the faulty tokens, overwriting cache
 *   rows and ids above fault_step, and n becomes fault_step.  A sweep that visits its trials
 *   in DESCENDING step order therefore always finds its prefix golden. */
size_t qtx_greedy_dfault_workspace_size(const qtx_model* m, int32_t B, int32_t S,
                                        int32_t max_len);
int32_t qtx_greedy_decode_dfault(const qtx_model* m, const int64_t* src, const uint8_t* src_mask,
                                 int32_t B, int32_t S, int32_t max_len, int64_t start,
                                 int64_t* ids, int64_t* top_ids, float* top_logp,
                                 int64_t* rec_ids, float* rec_logp, void* ws, size_t ws_bytes,
                                 const qtx_fault* fault, int32_t fault_step, void* stream);
int32_t qtx_greedy_dfault_resume(const qtx_model* m, int32_t B, int32_t S, int32_t max_len,
                                 int64_t* ids, int64_t* top_ids, float* top_logp,
                                 int64_t* rec_ids, float* rec_logp, void* ws, size_t ws_bytes,
                                 const qtx_fault* fault, int32_t fault_step,
                                 int32_t* changed_host, void* stream);

/* ---- faults of the KV-cached decode itself: one step fault or one cache upset ----
 * qtx_greedy_decode_dfault follows the campaign's loop, which recomputes the whole prefix at
 * every step: its fault leaves no trace.  The engine here appends quantized K/V rows to a cache
 * and never recomputes them; this entry answers for that machine.  The reference has no such
 * memory: the contract is tests/kvfault_ref.py, a restatement of the oracle's KV-cached
 * DecodeState.step that takes one fault, plus an upset of its caches; results are equal bit for
 * bit.  Exactly one of fault / upset is given (HOST pointers).
 *
 * Step fault: one qtx_fault with module 1, at step i.  Steps 0 .. i-1 run golden; step i's
 * CACHED run is computed with the fault; steps i+1 .. run KV-cached from whatever step i left
 * in the caches and in ids.  So a fault on a K or V projection, or anywhere in a lower layer,
 * stays in the rows every later step reads.  Coordinates are those of the step's own MatMuls,
 * one row per sentence:
 *   Linear targets (Q K V O CQ CO FFN1 FFN2): rows index the step's [B] tokens (INPUT* / OUTPUT:
 *   row = b; WEIGHT*: row = out channel; the WEIGHT16 window runs over the [B] rows, the
 *   INPUT16 window over columns).
 *   Attention targets: the conventions above with Sq = 1 and Sk = i + 1 (self) or S (cross),
 *   e.g. QK WEIGHT: row = b*Sk + j, col = h*64 + d.  A WEIGHT16 window (over query rows) that
 *   does not contain row 0 is a fault without effect.  The cache keeps the golden code in every
 *   attention WEIGHT case: the fault corrupts the operand of that one MatMul in flight.
 *   QTX_LIN_CK / CV: applied to the one-time memory K/V projection before step 0 (rows
 *   [B * S]); the corrupted cross cache serves every step; step must be 0.
 *
 * Cache upset: one stored bit flips after step i-1 and before step i, and stays.
 *   cache  0 self K, 1 self V, 2 cross K, 3 cross V, of decoder layer `layer`
 *   row    self: b*max_len + j with 0 <= j < i (a row already written, so i >= 1);
 *          cross: b*S + j, any i >= 0
 *   field  0: bit `bit` (0..7) of the int8 code at column col (0 .. d_model-1);
 *          1: bit `bit` of the row's float32 scale, col = 0 — mantissa and sign only (bits
 *          0..22 and 31): an exponent flip can take the scores out of float range, and the
 *          decoder's non-finite rules are not pinned.
 *   Every copy a step reads is hit (the fused step reads the cross values from a regrouped
 *   copy).  Upsets do not depend on the weight width (4-bit models too); step faults need
 *   8-bit weights.
 *
 * Outputs as qtx_greedy_decode_dfault: the scored form (top_ids and top_logp given) or the
 * plain form (both NULL); rec_ids / rec_logp [B, 2, 2] (both or neither): the golden and the
 * faulty top 2 of step i, the golden pair from one golden cached run of step i on the golden
 * caches, made before the fault or the upset is applied (not run when no record is asked for).
 * step >= max_len - 1: nothing runs at or after it — a golden decode, rec_* untouched, the
 * coordinates not checked.
 * Path selection as qtx_greedy_decode_dfault (and its captured graphs: the golden ranges end
 * where the fault or upset takes effect); the faulty step itself is one eager step built from
 * the FaultArgs-aware GEMM at M = B, the row quantizers, the step's own attention kernel and,
 * for an attention target, a one-query recomputation of the affected (sentence, head).
 * Refused before anything is launched: both or neither of fault / upset, fault kind NONE or
 * module != 1, step < 0, any coordinate outside the step's shapes, j >= i, a scale bit 23..30,
 * CK / CV at step != 0: QTX_E_INVALID; a step fault with 4-bit weights: QTX_E_UNSUPPORTED; a
 * short workspace: QTX_E_WORKSPACE; B * tgt_vocab and B * max_len * d_model below 2^30.
 * Writes exactly ids, top_ids, top_logp, rec_ids, rec_logp.  ws:
 * qtx_greedy_kvfault_workspace_size bytes; a dfault resume header on it is dropped. */
typedef struct {
  int32_t cache;     /* 0 self K, 1 self V, 2 cross K, 3 cross V */
  int32_t layer;
  int32_t field;     /* 0 code, 1 scale */
  int32_t bit;
  int64_t row;
  int32_t col;
  int32_t reserved;
} qtx_cache_upset;
size_t qtx_greedy_kvfault_workspace_size(const qtx_model* m, int32_t B, int32_t S,
                                         int32_t max_len);
int32_t qtx_greedy_decode_kvfault(const qtx_model* m, const int64_t* src, const uint8_t* src_mask,
                                  int32_t B, int32_t S, int32_t max_len, int64_t start,
                                  int64_t* ids, int64_t* top_ids, float* top_logp,
                                  int64_t* rec_ids, float* rec_logp, void* ws, size_t ws_bytes,
                                  const qtx_fault* fault, const qtx_cache_upset* upset,
                                  int32_t step, void* stream);

/* ---- KV-cached fault decode: one independent trial per sentence ----
 * A campaign runs thousands of the trials above (what a trial is:
 * parallelized_inject_onnx_transformer.py:536-740), and sentences of a batch never interact:
 * every op is per token or per (sentence, head), and the integer GEMM accumulators are exact.
 * So one decode carries B trials, one per row, each at its own step; rows without a trial ride
 * along as golden controls.  The contract is tests/kvtrials_ref.py: row b of this call equals,
 * bit for bit, the stand-alone qtx_greedy_decode_kvfault call on sentence b alone — B = 1, scored
 * form, the same S, source row and mask row, trial b's fault or upset at trial b's step — in
 * ids, top_ids, top_logp and the record.
 *
 * trials: HOST array [B].  what 0: no trial (a golden row); 1: the step fault `fault`; 2: the
 * cache upset `upset`; `step` as in the stand-alone call.  Coordinates are those of the B = 1
 * call on the row's sentence:
 *   Linear INPUT* / OUTPUT: row = 0.  Linear WEIGHT*: row = out channel.
 *   Attention targets: the conventions above with b = 0, Sq = 1, Sk = step + 1 (self) or S
 *   (cross); a WEIGHT16 window that does not contain row 0 has no effect.
 *   Upset: row = j, the position within the sentence's cache (self: j < step; cross: j < S).
 *   A WEIGHT fault is seen by its own row only: every row is its own machine.
 * Two faults in one sentence (faults that interact) are not expressed here.
 *
 * Scored form only: the scored step and its tail always run, so ids follows the scored decode's
 * rule; top_ids / top_logp may both be NULL (not copied out).  rec_ids / rec_logp [B, 2, 2],
 * both or neither: row b holds the golden and the faulty top 2 of its own step, the golden pair
 * from one golden cached run of that step made before anything is applied at it.  A row with
 * what == 0 or step >= max_len - 1 decodes golden (its coordinates are not checked), and its
 * record row is written as zeros.
 * Schedule: the distinct trial steps in ascending order; between them the golden ranges run as
 * in qtx_greedy_decode_dfault (same graphs, same path selection); at a step the upsets of that
 * step flip, and if any row has a step fault there the step runs once, eager, on the whole
 * batch through a GEMM that gives each row the fault of its own trial (and one recomputation
 * of the affected (sentence, head) per attention-target trial); rows whose trial was earlier
 * continue from their own diverged caches.
 * Refused before anything is launched: trials NULL, a `what` outside 0..2, and per row what the
 * stand-alone call refuses for B = 1 (the error text names the row): QTX_E_INVALID, or
 * QTX_E_UNSUPPORTED for a step fault with 4-bit weights (upsets are allowed).  QTX_LIN_CK /
 * QTX_LIN_CV step faults: QTX_E_UNSUPPORTED — the one-time [B * S] memory K/V projection is
 * not made table-aware here (qtx_greedy_decode_kvfault takes them).  A short workspace:
 * QTX_E_WORKSPACE.  B * tgt_vocab and B * max_len * d_model below 2^30.
 * Writes exactly ids, top_ids, top_logp, rec_ids, rec_logp.  ws:
 * qtx_greedy_kvtrials_workspace_size bytes; a dfault resume header on it is dropped.  The call
 * waits for the stream once, before its first launch (the trial table's upload). */
typedef struct {
  int32_t what;            /* 0 none (golden row), 1 step fault, 2 cache upset */
  int32_t step;
  qtx_fault fault;         /* what == 1: module 1, B = 1 coordinates */
  qtx_cache_upset upset;   /* what == 2: row = position within the sentence */
} qtx_kv_trial;
size_t qtx_greedy_kvtrials_workspace_size(const qtx_model* m, int32_t B, int32_t S,
                                          int32_t max_len);
int32_t qtx_greedy_decode_kvtrials(const qtx_model* m, const int64_t* src, const uint8_t* src_mask,
                                   int32_t B, int32_t S, int32_t max_len, int64_t start,
                                   int64_t* ids, int64_t* top_ids, float* top_logp,
                                   int64_t* rec_ids, float* rec_logp, void* ws, size_t ws_bytes,
                                   const qtx_kv_trial* trials, void* stream);

/* ---- beam search with EOS stop ----
 * The reference has no beam search (its only decode is the fixed-length greedy loop above):
 * this entry cites generator.py:15 for the log-probabilities and nothing else.  The contract is
 * tests/beam_ref.py, a beam search over the oracle's KV-cached DecodeState; results are equal
 * bit for bit.
 * Rows are r = b * K + k with K = beam.  Per row: score (float32), a finished flag, length,
 * history [max_len] ([0] = start, every other entry starts as pad).
 * Start: score 0 for k = 0 and -inf for k > 0; no row finished; input token = start.
 * Step t = 0 .. max_len-2:
 *   1. one KV-cached decoder step at position t on all B * K rows; cross K/V and the source
 *      mask of row r are those of sentence r / K.
 *   2. logp = the canonical log-softmax of the row's logits (the scored decode's, above: qlog,
 *      not the platform logf).
 *   3. candidates of sentence b: a live row k gives V candidates (fl32(score[k] + logp[k][v]),
 *      flat = k * V + v), a value that is not finite (NaN, +-inf) taken as -inf; a finished row
 *      gives exactly one candidate (score[k], flat = k * V + pad): its score does not change.
 *   4. the K best under the total order "larger value, then smaller flat"; new slot j takes the
 *      j-th best: parent = flat / V, token = flat % V, score = value.  The order is total, so
 *      the result does not depend on the order of the reduction.
 *   5. history, length, finished flag and every layer's self K/V cache rows (codes and scales,
 *      positions 0 .. t) of slot j become those of its parent; history[t+1] = token; finished =
 *      parent finished or token == eos; length = t + 1 unless the parent was finished.
 *   6. stop when every row is finished, or after step max_len - 2.  (A step after the stop
 *      changes nothing: a finished row only re-selects itself with pad.)
 * Outputs: hyp_ids int64 [B, K, max_len]; hyp_score float [B, K], the raw cumulative
 * log-probability, in search order (best first); hyp_len int32 [B, K], tokens after the start
 * symbol including the EOS; steps_run (HOST pointer, may be NULL): decoder steps launched.
 * No length normalisation here (qtx/decode.py ranks).
 * The encoder and the cross K/V GEMM run once on the B sentences.  The step is the greedy
 * decode's on B * K rows — the fused step where the greedy decode would take it, else the
 * unfused one, so every config qtx_model_create accepts beam-decodes — with the tail replaced
 * by k_beam_select and k_beam_reorder (csrc/qtx_decode.hip; the caches are permuted in place).
 * Steps run in chunks of QTX_GRAPH_STEPS (default 8): the fused step as captured graphs of
 * that many steps and of one step (graphs of their own; QTX_NO_GRAPH and the unfused step run
 * eager); one group (QTX_DECODE_GROUPS is ignored).  early_exit != 0: after each chunk but the
 * last the count of live rows is copied to the host (one 4-byte synchronising copy) and the
 * decode stops at zero, so steps_run is the stop step rounded up to the chunk; early_exit == 0:
 * asynchronous, every step runs.  The outputs are the same either way.
 * Refused before anything is launched: beam outside 1 .. 8 or above tgt_vocab, start / eos /
 * pad outside the vocabulary, eos == pad, max_len above the positional table: QTX_E_INVALID;
 * B * beam * tgt_vocab or B * beam * max_len * d_model >= 2^30, tgt_vocab or B * beam >= 2^21
 * (the select's 32-bit embedding offsets): QTX_E_UNSUPPORTED; a short
 * workspace: QTX_E_WORKSPACE.  ws: qtx_beam_workspace_size bytes. */
size_t qtx_beam_workspace_size(const qtx_model* m, int32_t B, int32_t S, int32_t max_len,
                               int32_t beam);
int32_t qtx_beam_decode(const qtx_model* m, const int64_t* src, const uint8_t* src_mask,
                        int32_t B, int32_t S, int32_t max_len, int32_t beam, int64_t start,
                        int64_t eos, int64_t pad, int32_t early_exit, int64_t* hyp_ids,
                        float* hyp_score, int32_t* hyp_len, int32_t* steps_run, void* ws,
                        size_t ws_bytes, void* stream);

/* ---- teacher-forced target scoring: per-token log-prob, rank and top 2 ----
 * The reference's forward pass on a given target: EncoderDecoder.forward(src, tgt, src_mask,
 * tgt_mask) (encoder_decoder.py:19-23) with Batch.tgt = tgt[:, :-1], Batch.tgt_y = tgt[:, 1:]
 * and make_std_mask (batch.py:17-30, train.py:28-30), then generator.py:15's log_softmax.
 * src int64 [B, S], src_mask uint8 [B, S]; tgt int64 [R, L], R = B * K with K = tgt_per_src
 * >= 1, row r a target of sentence r / K (the beam search's numbering); L >= 2, T = L - 1.
 * The decoder's input is tgt[:, :T] (ids outside the vocabulary clamped, as qtx_embed), the
 * labels are y = tgt[:, 1:].  Target mask: pad >= 0: keep[r, i, j] = j <= i and
 * tgt[r, j] != pad (batch.py:25-30, a [R, T, T] mask); pad < 0: the causal mask alone.
 * One full-prefix decoder pass over all R * T positions per trial; the results equal the
 * KV-cached steps' (causal invariance).  Per position (r, t), x = the logits row of the final
 * LayerNorm's output in the canonical generator order and logp its canonical log-softmax
 * (scored decode above: qlog, not the platform logf):
 *   tok_logp  logp[y]
 *   rank      the number of v with logp[v] > logp[y], or logp[v] == logp[y] and v < y: the
 *             scored decode's total order, so rank 0 <=> y == top 1 and rank 1 <=> y == top 2
 *   top_ids / top_logp  the row's top 2 under the scored decode's rules
 *   a non-finite row (scored decode's definition): tok_logp NaN, rank -1, top ids (0, 1), both
 *   values NaN.  A label outside [0, tgt_vocab): tok_logp NaN, rank -1, nothing outside the
 *   row is read; the top 2 are still the row's.
 * Positions whose label is pad are computed and written like any other (the caller masks).
 * Trials: trial 0 is fault-free, trial n = 1 .. n_faults applies faults[n - 1] (HOST array)
 * alone; every output has a leading trial axis of n_faults + 1, and a trial's result equals a
 * stand-alone call with that one fault.  An encoder fault (module 0) reruns the encoder and
 * the cross K/V with the fault into buffers of their own; a decoder fault runs one faulty pass
 * on the golden memory, its row indexing the [R * T] tokens (QTX_LIN_CK / CV: [B * S], on a
 * cross copy of its own).  The golden memory and cross K/V serve every trial.
 * The encoder and the cross K/V GEMM run once on the B sentences (replicated to the R rows
 * when K > 1); the generator runs on chunks of rows, each followed by the scoring kernel
 * (csrc/qtx_kernels.hip k_lsm_score): no [R * T, tgt_vocab] log-probabilities are written.
 * Eager launches, no graphs.
 * Writes exactly tok_logp float and rank int32 [n_faults + 1, R, T], top_ids int64 and
 * top_logp float [n_faults + 1, R, T, 2] (both NULL: not wanted).
 * Refused before anything is launched: L < 2, K < 1, S or T above 512 or the positional
 * table, n_faults < 0, n_faults > 0 with faults NULL, a fault of kind NONE, a coordinate
 * outside the trial's shapes: QTX_E_INVALID; R * T * d_model >= 2^30, any fault with 4-bit
 * weights or K > 1 (the two row numberings would disagree): QTX_E_UNSUPPORTED; a short
 * workspace: QTX_E_WORKSPACE.  ws: qtx_score_workspace_size bytes. */
size_t qtx_score_workspace_size(const qtx_model* m, int32_t B, int32_t S, int32_t L,
                                int32_t tgt_per_src, int32_t n_faults);
int32_t qtx_score_targets(const qtx_model* m, const int64_t* src, const uint8_t* src_mask,
                          int32_t B, int32_t S, const int64_t* tgt, int32_t L,
                          int32_t tgt_per_src, int64_t pad, const qtx_fault* faults,
                          int32_t n_faults, float* tok_logp, int32_t* rank, int64_t* top_ids,
                          float* top_logp, void* ws, size_t ws_bytes, void* stream);
/* The scoring tail alone (generator.py:15 on given labels): logits float [M, V], y int64 [M]
 * -> tok_logp, rank [M], top_ids / top_logp [M, 2] (both NULL: not wanted), semantics above.
 * V >= 2, else QTX_E_INVALID.  Writes exactly those outputs. */
int32_t qtx_score_logits(const float* logits, const int64_t* y, int32_t M, int32_t V,
                         float* tok_logp, int32_t* rank, int64_t* top_ids, float* top_logp,
                         void* stream);
/* The generator in chunks of rows plus that tail (generator.py:14-15): x float [M, d_model]
 * (the final LayerNorm applied), y int64 [M].  ws holds one chunk's logits: the chunk is
 * min(M, floor(ws_bytes / (4 * tgt_vocab)) & ~15) rows; fewer than 16 rows' worth:
 * QTX_E_WORKSPACE.  The results do not depend on the chunk.  Writes exactly the outputs named
 * above (and ws).  qtx_score_targets runs the same function per trial. */
int32_t qtx_score_rows(const qtx_model* m, const float* x, int32_t M, const int64_t* y,
                       float* tok_logp, int32_t* rank, int64_t* top_ids, float* top_logp,
                       void* ws, size_t ws_bytes, void* stream);

/* Embeddings + positional encoding: which = 0 (src) / 1 (tgt); ids int64 [B,T] ->
 * out [B,T,d], positions pos0 .. pos0+T-1. */
int32_t qtx_embed(const qtx_model* m, int32_t which, const int64_t* ids, int32_t B, int32_t T,
                  int32_t pos0, float* out, void* stream);

/* Generator: x [M,d] -> logp [M,tgt_vocab] (may be NULL), ids int64 [M] (first argmax).
 * ws: M * tgt_vocab floats. */
int32_t qtx_generator(const qtx_model* m, const float* x, int32_t M, float* logp,
                      int64_t* ids, void* ws, size_t ws_bytes, void* stream);

/* Generator + torch.topk(prob, 2, dim=1) (generator.py:15,
 * parallelized_inject_onnx_transformer.py:718-740; semantics: scored decode above):
 * x [M,d] -> top_ids int64 [M,2], top_logp float [M,2], with no [M,tgt_vocab] log-prob
 * write.  ws: M * tgt_vocab floats (the raw logits, as qtx_generator).  No vocabulary cap. */
int32_t qtx_generator_top2(const qtx_model* m, const float* x, int32_t M, int64_t* top_ids,
                           float* top_logp, void* ws, size_t ws_bytes, void* stream);

/* ---- per-op entry points (parity tests, fault-injection hooks later) ---- */

/* q[r,:] = rint(x[r,:] / s[r]), s[r] = max(max|x[r,:]|, 1e-5) / qmax.  D a multiple of 256 up to 2048
 * (this and qtx_layernorm_quant: QTX_E_UNSUPPORTED otherwise). */
int32_t qtx_row_quant(const float* x, int32_t rows, int32_t D, float qmax, int8_t* q,
                      float* s, void* stream);

/* y = LN(x) (unbiased std, eps on std); optional fp32 y (may be NULL), optional q/s. */
int32_t qtx_layernorm_quant(const float* x, const float* a, const float* b, int32_t rows,
                            int32_t D, float* y, int8_t* q, float* s, void* stream);

/* out[m,n] = ((float(sum_k A[m,k] W[n,k]) * sa[m]) * sw[n]) + bias[n], then
 * flags: 1 = ReLU, 2 = residual (out = res + y).  weight_bits 8: W int8 [N,K];
 * 4: W packed [N,K/2] (low nibble = even k).  K % 64 == 0. */
int32_t qtx_linear_i8(const int8_t* A, const float* sa, const void* W, const float* sw,
                      const float* bias, int32_t M, int32_t N, int32_t K, int32_t weight_bits,
                      int32_t flags, const float* res, float* out, void* stream);

/* qtx_linear_i8 with 8-bit weights where every row m carries a fault of its own (the GEMM of
 * qtx_greedy_decode_kvtrials' eager step, k_gemm_rowfault): rows is a HOST array [M] of
 * qtx_fault in B = 1 coordinates — kind NONE: none; INPUT* / OUTPUT: row = 0 (the row itself),
 * the INPUT16 window over output columns; WEIGHT*: row = out channel, seen by row m alone, a
 * WEIGHT16 window that does not contain row 0 without effect; module / layer / linear are not
 * read.  Same expressions in the same order as qtx_linear_i8 with one fault.  A and W 16-byte
 * aligned.  Synchronises the stream (the table lives for the length of the call). */
int32_t qtx_linear_i8_rowfaults(const int8_t* A, const float* sa, const int8_t* W, const float* sw,
                                const float* bias, int32_t M, int32_t N, int32_t K, int32_t flags,
                                const float* res, float* out, const qtx_fault* rows, void* stream);

/* Pack int8 values in [-8,7] [N,K] into int4 [N,K/2]. */
int32_t qtx_pack_int4(const int8_t* q, int32_t N, int32_t K, uint8_t* packed, void* stream);

/* Attention core on quantized Q/K/V laid out [B,S,H*64] with per-token scales [B,S]:
 * ctx [B,Sq,H*64] fp32.  mask uint8 [B,Sq,Sk] with strides (m_bs, m_is) in elements
 * (m_is = 0 broadcasts one row, e.g. the encoder's [B,1,S] mask); NULL = keep all.
 * dec != 0: a decoder layer's attention (decoder.py:28-33), whose PV MatMul runs in the
 * decoder's canonical order (four partial chains); 0: the encoder's. */
int32_t qtx_attention_i8(const int8_t* q, const float* sq, const int8_t* k, const float* sk,
                         const int8_t* v, const float* sv, const uint8_t* mask, int64_t m_bs,
                         int64_t m_is, int32_t B, int32_t H, int32_t Sq, int32_t Sk,
                         float* ctx, int32_t dec, void* stream);

/* qtx_attention_i8 plus the attention MatMuls' intermediates, for the traced executor
 * (run_module(expose_intermediates=...), onnx_optimized_inference.py:57 stores every node
 * output by name): qk_acc [B,H,Sq,Sk] = float(sum_d q k), the exact integer accumulators of
 * QK^T ("FirstMatMul" MatMul_{8L+3}, before the / 8 and the mask); p_codes [B,H,Sq,Sk] =
 * rint(P * 127) (the Round of attention.py:33-35); ctx as qtx_attention_i8, bit for bit.
 * qk_acc / p_codes may be NULL.  Off the hot path (one wave per query row and head). */
int32_t qtx_attention_trace(const int8_t* q, const float* sq, const int8_t* k, const float* sk,
                            const int8_t* v, const float* sv, const uint8_t* mask, int64_t m_bs,
                            int64_t m_is, int32_t B, int32_t H, int32_t Sq, int32_t Sk,
                            float* ctx, float* qk_acc, float* p_codes, int32_t dec, void* stream);

/* Encoder self-attention with the context quantized per token for the O-projection
 * (attention.py:23-67 + quant_linear.py:30-43, replacing the MatMul_{8L+3,8L+4} pair of the
 * encoder graph and the following QuantizeLinear): q/k/v int8 [B,S,512] (8 heads) +
 * per-token scales [B,S], key mask uint8 [B,S] (NULL = keep all) -> ctx8 int8 [B,S,512] +
 * sctx [B,S].  S <= 128.  One workgroup per sentence. */
int32_t qtx_attention_i8_quant(const int8_t* q, const float* sq, const int8_t* k,
                               const float* sk, const int8_t* v, const float* sv,
                               const uint8_t* key_mask, int32_t B, int32_t S, int8_t* ctx8,
                               float* sctx, void* stream);

/* ---- fused decode-step kernels (the KV-cached greedy step is built from these) ---- */

/* Row-complete int8 GEMM (8-bit weights, N % 512 == 0, K % 64 == 0) whose epilogue sees
 * whole 512-wide row segments; y = ((float(sum_k A W) * sa[m]) * sw[n]) + bias[n]:
 *   epi 0  per-token quant of y over each 512-column tile t -> out8 + t*o8_ts [M,512]
 *          (row stride ldo8) and scale os + t*os_ts [M]  (Q/K/V outputs, attention.py:53-56)
 *   epi 1  (N == 512) x = res + y -> xout; LayerNorm(x; ln_a, ln_b) quantized per token
 *          -> lnq [M,512] + lns [M], or fp32 -> lnout when lnq is NULL (sublayer_connection.py
 *          + layer_norm.py of the next sublayer)
 *   epi 2  relu(y): per-row absmax of each tile -> pmax_out [N/512][M]
 *   epi 3  relu(y) quantized per token with m = max_p pmax_in[p][M] (p < pmax_n) ->
 *          out8 [M,N] (ld ldo8) + os [M]         (FFN hidden, position_feed_forward.py:12)
 * Strides (in elements): ldo8 >= 512 (epi 0) / >= N (epi 3), o8_ts >= 0 and os_ts >= 0 are
 * free — Q, K and V may share one pitched buffer (ldo8 = 1600, o8_ts = 512), the bytes
 * between the rows and the floats between the scale tiles are never written — but out8 is
 * stored in 16-byte vectors: out8 16-byte aligned, ldo8 % 16 == 0 (a KP out8: % 64) and
 * o8_ts % 16 == 0, else QTX_E_INVALID.  A and W must be 16-byte aligned too. */
typedef struct qtx_row_gemm {
  const int8_t* A; const float* sa; const int8_t* W; const float* sw; const float* bias;
  int32_t M, N, K, epi;
  int8_t* out8; int64_t ldo8, o8_ts; float* os; int64_t os_ts;
  const float* res; float* xout; const float* ln_a; const float* ln_b;
  int8_t* lnq; float* lns; float* lnout;
  float* pmax_out; const float* pmax_in; int32_t pmax_n;
  /* kp = 1: A [M (+1 if odd), K] and W in the KP layout (row pair p, K chunk c of 64 bytes
   * = one 128-byte line at ((p * K/64 + c) * 128), rows 2p | 2p+1 at +0 | +64; W packed by
   * qtx_pack_w_kp); lnq (epi 1) and out8 (epi 3) are then written KP, epi 0's out8 row-major.
   * K % 256 == 0.
   * kp = 2: the weight-stationary kernel (K == 512 only): A in the KP layout, W packed by
   * qtx_pack_w_ws; each workgroup keeps a 512-column slice of W on chip and streams 64-row
   * blocks of A.  Outputs exactly as kp = 1, except for the pad row of an odd M in the KP
   * outputs (epi 1's lnq, epi 3's out8; both hold M + (M & 1) rows in either layout): kp = 1
   * leaves it untouched, kp = 2 / 3 write it as scratch (their stores are clipped by a buffer
   * descriptor, which cannot end between the two interleaved rows of a pair).
   * kp = 3: epi 3 in ONE pass (N == 2048, K == 512, W as for kp = 2): the per-token row
   * maximum is exchanged between the column slices' workgroups inside the launch, so
   * pmax_in / pmax_n are not read; pmax_out is the exchange scratch (>= 32 * M + 2048 bytes,
   * overwritten).  The encoder's FFN1 (qtx_encoder_forward at M >= 2048).
   * kp = 4 / 5 (diagnostic library only: QTX_UNSUPPORTED here): kp = 2 epi 0 / kp = 3 on the
   * 32x32x32-MFMA kernels, W in their WS32 layout. */
  int32_t kp;
  /* kp = 3 only: device word OR-ed with 1 when a wait for the partner slices' row maxima
   * timed out (the affected codes came from a partial maximum: the call's outputs are
   * invalid).  NULL: the flag is the u32 at byte offset 1024 * ceil(M / 32) + 4 of pmax_out,
   * zeroed by each launch; read it after the stream completes. */
  uint32_t* status;
  /* epi 1 with kp = 1 only: split K over `ksplit` workgroups per 128-row tile (ksplit in
   * {2, 4, 8}, (K / 64) % (4 * ksplit) == 0), int32 partials in `part` (>= ksplit * M * 2 KB
   * of device scratch), then a row-wise residual + LayerNorm + quant epilogue; the same
   * results.  What the encoder does for FFN2 below 64 row tiles.  0: no split. */
  int32_t* part;
  int32_t ksplit;
} qtx_row_gemm;
int32_t qtx_linear_rows(const qtx_row_gemm* args, void* stream);
/* The encoder's FFN sublayer as ONE launch (position_feed_forward.py:11-12 with its
 * sublayer_connection.py:15-17 residual and the next layer_norm.py:12-15 + quant_linear.py:30-43),
 * replacing the FFN1 (qtx_linear_rows kp = 3) and FFN2 (kp = 1, epi 1) calls:
 *   h = relu(((float(A . W1^T) * sa) * sw1) + b1) quantized per token over all F columns,
 *   x = x + (((float(hq . W2^T) * s_h) * sw2) + b2)   (in place),
 *   LayerNorm(x; ln_a, ln_b) quantized per token -> lnq (KP) + lns [M], or fp32 -> lnout when
 *   lnq is NULL.  A: int8 [M (+1 if odd), 512] in the KP layout (qtx_linear_rows kp = 1);
 *   wf: W1 / W2 packed by qtx_pack_ffn.  lnq / lns may alias A / sa (each 128-row block reads
 *   its rows before it writes them).  F % 64 == 0, 256 <= F <= 2048.  Results equal the two
 *   calls it replaces bit for bit. */
typedef struct qtx_ffn_args {
  const int8_t* A; const float* sa; const int8_t* wf;
  const float* sw1; const float* b1; const float* sw2; const float* b2;
  float* x; const float* ln_a; const float* ln_b;
  int8_t* lnq; float* lns; float* lnout;
  int32_t M, F;
} qtx_ffn_args;
int32_t qtx_ffn_rows(const qtx_ffn_args* args, void* stream);
/* W1 int8 [F, 512] and W2 int8 [512, F] row-major -> the weight stream qtx_ffn_rows reads
 * (F * 1024 bytes): per 64-column chunk c four 16 KB slots of 16 fragments x 64 lanes x 16
 * bytes — slots 4c + h (h = 0, 1; W1 K steps 4h .. 4h+3), fragment 4s' + j', lane l:
 * W1[64c + 16j' + (l & 15)][64(4h + s') + 16(l >> 4) .. +16]; slots 4c + 2 + ch (W2, column
 * half ch), fragment j, lane l: byte 4j' + e = W2[col][64c + 16j' + 4(l >> 4) + e] with
 * col = 16(l & 15) + 8ch + j for j < 8, else 256 + 16(l & 15) + 8ch + j - 8. */
int32_t qtx_pack_ffn(const int8_t* W1, const int8_t* W2, int32_t F, int8_t* out, void* stream);
/* W int8 [N, K] row-major -> out [N, K] in the KP layout with the per-512-column-tile row
 * order qtx_linear_rows(kp = 1) reads.  N % 512 == 0, K % 64 == 0. */
int32_t qtx_pack_w_kp(const int8_t* W, int32_t N, int32_t K, int8_t* out, void* stream);
/* W int8 [N, 512] row-major -> out (N*512 bytes) in the order qtx_linear_rows(kp = 2) reads:
 * for 512-column slice t, wave w (0..7), K step s (0..7), column fragment j (0..3) one 1 KB
 * block at ((t*8 + w)*8 + s)*4 + j whose 16-byte lane l (0..63) holds
 * W[512t + 64w + 16((l & 15) >> 2) + 4j + (l & 3)][64s + 16(l >> 4) .. +16].
 * N % 512 == 0, K == 512. */
int32_t qtx_pack_w_ws(const int8_t* W, int32_t N, int32_t K, int8_t* out, void* stream);

/* Skinny int8 GEMM for decode (M small): out = epilogue(A . W^T) with the A operand made
 * in the prologue: amode 0 = int8 A [M,K] + sa; 1 = LayerNorm(X [M,512]; ln_a, ln_b) then
 * per-token quant; 2 = fp32 X [M,K] quantized per token with s = max(m, 1e-5)/127 where m =
 * max over p < pmax_n of pmax_in[p*M + row] (partial row absmaxima, e.g. per head or per
 * column tile; pmax_n <= 128); 3 = fp32 X [M,K] quantized per token from its own row
 * absmax (the scale amode 2 forms from complete partials).  flags: 1 ReLU, 2 residual
 * (res), 4 partial row absmax of the output per 16-column tile into pmax_out [N/16][M].
 * N % 16 == 0, K in {512, 2048} (amode 1: K = 512); M * max(ldx, K), M * N and N * K below
 * 2^30 (the kernels address their operands with 32-bit byte offsets), else QTX_E_UNSUPPORTED.
 * Supported flags: 0, 1, 2 and 1|4 (every other combination: QTX_E_UNSUPPORTED, nothing
 * written).  X rows are ldx floats apart and read in 16-byte vectors: X (amode 0: A) and W
 * 16-byte aligned, ldx % 4 == 0, ldx >= K, else QTX_E_INVALID; only the K floats of a row and
 * the pmax_n * M partial maxima are used.
 * quant_linear.py:111-119, layer_norm.py:12-15. */
int32_t qtx_skinny_linear(int32_t amode, const int8_t* A, const float* sa, const float* X,
                          int64_t ldx, const float* ln_a, const float* ln_b,
                          const float* pmax_in, int32_t pmax_n, const void* W, const float* sw,
                          const float* bias, int32_t M, int32_t N, int32_t K,
                          int32_t weight_bits, int32_t flags, const float* res, float* out,
                          float* pmax_out, void* stream);

/* One-query-per-sentence attention of the decode step (attention.py:23-67).
 * kv_new = 1 (self): y [B, 3*512] holds this step's q|k|v projections; they are quantized
 *   per token, k/v written to the caches at row b*kv_bs + *step_dev, keys 0..*step_dev
 *   (kv_bs <= 128).
 * kv_new = 0 (cross): y [B,512] holds q; keys = S cached rows per sentence, mask [B,S].
 * Caches: kc int8 [B][kv_bs][512]; vc int8 in groups of 4 keys, [B][ceil(kv_bs/4)][512][4]
 *   (byte ((b*G4 + j/4)*512 + d)*4 + j%4 holds v[b][j][d]: one dword = 4 keys of one dim);
 *   skc/svc [B][kv_bs].  Out: fp32 context ctx [B,512]
 * and the per-head absmax pmax [8][B] (the next GEMM's per-token quantization, amode 2 of
 * qtx_skinny_linear with pmax_n = 8).  Keys <= 128: this is the fused step's kernel; a decode
 * with S or max_len above 128 runs the unfused step, whose attention takes up to 512 keys
 * (qtx_attention_i8's kernel with the key count read from the step counter).  The PV MatMul
 * runs in the decoder's
 * canonical order (four partial chains; qtx_attention_i8 with dec = 1).
 * y rows are ldy floats apart (ldy >= the row width, ldy % 4 == 0; y, kc and vc 16-byte
 * aligned, else QTX_E_INVALID).  Self: only cache row *step_dev (k, v and both scales) is
 * written.  Cross: the caches are read only, S <= kv_bs, and rows S .. kv_bs - 1 (and the
 * pad keys of the last value group) are never used. */
int32_t qtx_decode_attention(int32_t kv_new, const float* y, int64_t ldy, int8_t* kc,
                             int8_t* vc, float* skc, float* svc, int32_t kv_bs,
                             const int32_t* step_dev, int32_t S, const uint8_t* mask,
                             int32_t B, float* ctx, float* pmax, void* stream);

/* The decode step's tail (onnx_reference_inference.py:632,640-643): per row m of logits
 * [M, tgt_vocab], the first argmax of log_softmax (generator.py:15, torch.max's tie rule)
 * into ids[m * ids_bs + s + 1], and the next decoder input tgt_embed(id) at position s + 1
 * into x_next [M, d_model], with s = step_dev[0]; step_dev[1] must be 0 (arrival counter);
 * the last workgroup advances step_dev[0] by one. */
int32_t qtx_decode_argmax_embed(const qtx_model* m, const float* logits, int32_t M,
                                int64_t* ids, int64_t ids_bs, int32_t* step_dev,
                                float* x_next, void* stream);

/* The scored decode step's tail (generator.py:15 + torch.topk(prob, 2, dim=1),
 * parallelized_inject_onnx_transformer.py:718-740; semantics: scored decode above):
 * qtx_decode_argmax_embed plus the row's two best (id, logp) into entry [m, s, :] of top_ids
 * int64 [M, ids_bs-1, 2] and top_logp float [M, ids_bs-1, 2].  Writes exactly ids[m, s+1],
 * those M entries of top_ids / top_logp, x_next [M, d_model] and the two step words.
 * 2 <= tgt_vocab <= 8192 and M * tgt_vocab < 2^30, else QTX_E_INVALID / QTX_E_UNSUPPORTED. */
int32_t qtx_decode_top2_embed(const qtx_model* m, const float* logits, int32_t M, int64_t* ids,
                              int64_t ids_bs, int64_t* top_ids, float* top_logp,
                              int32_t* step_dev, float* x_next, void* stream);

/* The beam step's tail, part 1 (beam search above, rules 2-5 without the caches): logits
 * [B * beam, tgt_vocab] of the step at position s = step_dev[0].  Rewrites score float / fin /
 * len int32 [B * beam] in place; writes parent [B * beam] (each slot's parent slot, 0 ..
 * beam-1), the back-pointers bp_par / bp_tok int32 [max_len-1][B * beam] at row s (parent slot
 * and token), the next decoder inputs x_next [B * beam, d_model] = tgt_embed(token) at
 * position s + 1, and the four step words: step_dev[0] advanced by one, [1] and [2] (arrival
 * counter and live accumulator: must be 0, left 0), [3] = the rows still live. */
int32_t qtx_beam_select(const qtx_model* m, const float* logits, int32_t B, int32_t beam,
                        int64_t eos, int64_t pad, int32_t max_len, int32_t* step_dev,
                        float* score, int32_t* fin, int32_t* len, int32_t* parent,
                        int32_t* bp_par, int32_t* bp_tok, float* x_next, void* stream);

/* The beam step's tail, part 2: every layer's self K/V caches of slot j become those of slot
 * parent[b * beam + j], in place (each byte offset of a sentence's beam regions is owned by one
 * thread, which loads its beam chunks and then stores them by parent).  Per layer l and row r:
 * kc + l * k_ls int8 [r][max_len][512]; vc + l * v_ls int8, v_grouped != 0: the fused step's
 * 4-key groups [r][ceil(max_len/4)][512][4], else [r][max_len][512]; skc / svc + l * s_ls float
 * [r][max_len] (k_ls, v_ls in bytes, multiples of 16; s_ls in floats).  Only the valid prefix
 * moves: positions 0 .. n-1 with n = step_dev[0] clamped to max_len (grouped V: ceil(n / 4)
 * groups); nothing else is written. */
int32_t qtx_beam_reorder(int8_t* kc, int8_t* vc, float* skc, float* svc, int32_t B, int32_t beam,
                         int32_t max_len, int32_t n_layers, int64_t k_ls, int64_t v_ls,
                         int64_t s_ls, int32_t v_grouped, const int32_t* step_dev,
                         const int32_t* parent, void* stream);

/* The decode step's generator launch: logits [M, tgt_vocab] = generator(final LayerNorm(x)),
 * x fp32 [M, d_model] (decoder.py:16, generator.py:14).  rec (may be NULL): float
 * [M, ceil(tgt_vocab / 16), 4], one record per row and 16-column strip of the vocabulary, which
 * the plain decode's next step reduces to the token instead of a tail kernel of its own:
 * {m1, m2, i1, flags} with m1 = the strip's maximum (fmaxf from -3.0e38f), m2 = the next value
 * in descending order (m2 == m1 for a duplicate of the maximum; -3.0e38f when there is none),
 * i1 (int32 bits) = the smallest vocabulary index holding m1 (INT32_MAX: none), flags (int32
 * bits) bit 0 = a NaN or +inf in the strip, bit 1 = a value above -inf.  The logits do not
 * depend on rec. */
int32_t qtx_decode_generator(const qtx_model* m, const float* x, int32_t M, float* logits,
                             float* rec, void* stream);

/* An empty one-wave kernel on `stream`: the dependent-launch floor that bench.py subtracts
 * from a chain of launches to get per-kernel durations (measurement only, no reference
 * counterpart). */
int32_t qtx_debug_nop(void* stream);

/* The model's cache of captured decode-step graphs: *entries = the entries it holds now (at
 * most 16; a capture that would pass that clears the cache first), *captures = the graphs
 * instantiated since the model was created, one per executable graph (a capture of G separate
 * sub-batch graphs counts G).  Takes the model's lock (test / measurement only, no
 * reference counterpart). */
int32_t qtx_debug_graph_stats(const qtx_model* m, int32_t* entries, int64_t* captures);

/* Re-read the library's environment switches (csrc/qtx_knobs.h), which are otherwise read
 * once: the path switches the tests use to force the library's alternative code paths
 * (QTX_NO_GRAPH, QTX_UNFUSED, QTX_DECODE_GROUPS, QTX_NO_WSX, ...) and the hooks of the FFN1
 * exchange's error path (QTX_WSX_SPIN_LIMIT, QTX_WSX_DROP_SLICE).  Not for concurrent use
 * with running calls (test / measurement only, no reference counterpart). */
int32_t qtx_debug_reload_knobs(void);

#ifdef __cplusplus
}
#endif
#endif /* QTX_H_ */

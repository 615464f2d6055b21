/* qtx_wide_vocab.h — the decode step's tails for target vocabularies of 8193 to 65536 words.
 *
 * The tails of qtx.h, qtx_decode_argmax_embed and qtx_decode_top2_embed, keep one row of logits
 * in a workgroup's registers and stop at 8192 words.  Above them qtx_greedy_decode,
 * qtx_greedy_decode_scored and qtx_beam_decode still run the fused step and its graphs, up to
 * 65536 words: the plain and the scored step end with the two kernels declared here as
 * stand-alone entries, which stream the row (the beam step's tail, qtx_beam_select, reads the
 * logits from memory at any width).  Both take every tgt_vocab up to 65536, the narrow range
 * included, with the narrow entries' results bit for bit.  Above 65536 words, and in the fault,
 * trials and score drivers above 8192, a decode takes the unfused step as before.
 *
 * This header declares what qtx.h does not; it includes qtx.h and follows its conventions
 * (status codes, qtx_last_error, device pointers unless stated, streams as void*). */
#ifndef QTX_WIDE_VOCAB_H
#define QTX_WIDE_VOCAB_H

#include "qtx.h"

#ifdef __cplusplus
extern "C" {
#endif

/* qtx_decode_argmax_embed for 1 <= tgt_vocab <= 65536, from the generator's records: rec float
 * [M, ceil(tgt_vocab / 16), 4] as qtx_decode_generator writes it beside these logits (16-byte
 * aligned).  The token is decided from the records alone unless a second logit lies within 4e-6
 * of the row's maximum; only then are the logits read, for the canonical log-softmax (the
 * denominator summed in the order of every other tail: lane l of 64 adds elements l, l + 64,
 * ... from 0, then one 64-lane tree).  Outputs and the step words: as qtx_decode_argmax_embed.
 * M * tgt_vocab < 2^30, else QTX_E_UNSUPPORTED. */
int32_t qtx_decode_tok_wide(const qtx_model* m, const float* logits, const float* rec, int32_t M,
                            int64_t* ids, int64_t ids_bs, int32_t* step_dev, float* x_next,
                            void* stream);

/* qtx_decode_top2_embed for 2 <= tgt_vocab <= 65536: the same entries of ids, top_ids, top_logp,
 * x_next and the step words, from three streamed passes over the logits (maximum, denominator,
 * the two best log-probabilities under "larger logp, then smaller index").  A non-finite row
 * gives ids (0, 1) and NaN values.  M * tgt_vocab < 2^30, else QTX_E_UNSUPPORTED. */
int32_t qtx_decode_top2_wide(const qtx_model* m, const float* logits, int32_t M, int64_t* ids,
                             int64_t ids_bs, int64_t* top_ids, float* top_logp,
                             int32_t* step_dev, float* x_next, void* stream);

#ifdef __cplusplus
}
#endif
#endif  /* QTX_WIDE_VOCAB_H */

/* qtx_beam_heads.h — the beam search past 128 target positions for models with 4 or 16 heads
 * at d_model 512, that is head widths of 128 and 32 columns.
 *
 * qtx.h's qtx_beam_decode runs such a model with max_len > 128 and beam > 1 on the fused step
 * through the ancestry table, as it runs the 8-head model: no new argument or switch.  The
 * per-op entry of qtx_beam_long.h, qtx_decode_attention_beam, is 64 columns wide; the entry
 * here takes the head count and runs k_dec_attn_beam_hd of csrc/qtx_decode_beam_heads.hip for
 * 4 and 16.  The arithmetic is qtx_decode_attention_heads' (qtx_heads.h): the score is
 * ((float(acc) * s_q) * s_k[j]) / c, c = fp32(sqrt(512 / n_heads)), a correctly rounded
 * division.
 *
 * This header declares what the others do not; it includes qtx.h and follows its conventions
 * (status codes, qtx_last_error, device pointers unless stated, streams as void*). */
#ifndef QTX_BEAM_HEADS_H
#define QTX_BEAM_HEADS_H

#include "qtx.h"

#ifdef __cplusplus
extern "C" {
#endif

/* qtx_decode_attention_beam for a model of n_heads heads: n_heads is 4, 8 or 16 (8 runs what
 * qtx_decode_attention_beam runs), else QTX_E_INVALID with nothing written.  pmax [8][B] is, for
 * every head count, the absmax of each 64-column block of the context row. */
int32_t qtx_decode_attention_beam_heads(const float* y, int64_t ldy, int8_t* kc, int8_t* vc,
                                        float* skc, float* svc, int32_t kv_bs,
                                        const int32_t* step_dev, const uint8_t* anc, int32_t beam,
                                        int32_t B, float* ctx, float* pmax, int32_t n_heads,
                                        void* stream);

#ifdef __cplusplus
}
#endif
#endif  /* QTX_BEAM_HEADS_H */

/* qtx_heads.h — the attention operations for models with 4 or 16 heads at d_model 512, that
 * is head widths of 128 and 32 columns.
 *
 * qtx_model_create takes n_heads 4, 8 or 16; the model-level entries of qtx.h then run such a
 * model through the existing names (the fault entries refuse it: qtx.h, qtx_config).  The two
 * per-op entries of qtx.h, qtx_attention_i8 and qtx_decode_attention, are 64 columns wide; the
 * entries here take the head width or count as an argument and run the kernels of
 * csrc/qtx_attn_heads.hip for 32 and 128.  The arithmetic is qtx_attention_i8's with one
 * change: the score is ((float(acc) * s_q) * s_k[j]) / c, c = fp32(sqrt(dk)), a correctly
 * rounded division (c is a power of two only for dk = 64).
 *
 * This header declares what qtx.h does not; it includes qtx.h and follows its conventions
 * (status codes, qtx_last_error, device pointers unless stated, streams as void*). */
#ifndef QTX_HEADS_H
#define QTX_HEADS_H

#include "qtx.h"

#ifdef __cplusplus
extern "C" {
#endif

/* qtx_attention_i8 for H heads of dk columns: q [B, Sq, H * dk], k / v [B, Sk, H * dk], ctx
 * [B, Sq, H * dk]; every other argument as qtx_attention_i8.  dk is 32, 64 or 128 (64 runs
 * what qtx_attention_i8 runs); for 32 and 128, q / k / v must be 16-byte aligned and
 * 1 <= H <= 65535.  Anything else: QTX_E_INVALID, nothing written. */
int32_t qtx_attention_heads_i8(const int8_t* q, const float* sq, const int8_t* k, const float* sk,
                               const int8_t* v, const float* sv, const uint8_t* mask,
                               int64_t m_bs, int64_t m_is, int32_t B, int32_t H, int32_t Sq,
                               int32_t Sk, float* ctx, int32_t dec, int32_t dk, void* stream);

/* qtx_decode_attention for a model of n_heads heads over the same 512-column rows and cache
 * layouts: n_heads is 4, 8 or 16 (8 runs what qtx_decode_attention runs), else QTX_E_INVALID
 * with nothing written.  pmax [8][B] is, for every head count, the absmax of each 64-column
 * block of the context row. */
int32_t qtx_decode_attention_heads(int32_t kv_new, const float* y, int64_t ldy, int8_t* kc,
                                   int8_t* vc, float* skc, float* svc, int32_t kv_bs,
                                   const int32_t* step_dev, int32_t S, const uint8_t* mask,
                                   int32_t B, float* ctx, float* pmax, int32_t n_heads,
                                   void* stream);

#ifdef __cplusplus
}
#endif
#endif  /* QTX_HEADS_H */

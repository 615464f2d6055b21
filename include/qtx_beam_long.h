/* qtx_beam_long.h — the per-op entries of the beam search past 128 target positions.
 *
 * Up to 128 positions the beam step permutes every layer's self K/V caches by parent
 * (qtx.h qtx_beam_reorder).  Past them qtx_beam_decode moves no cache: a byte table records, for
 * every hypothesis and position, which slot's cache row holds it; the step's self-attention
 * reads through the table and the step's tail permutes the table.  The two kernels are
 * declared here as stand-alone entries, on the pattern of qtx_decode_attention and
 * qtx_beam_reorder.
 *
 * This header declares what qtx.h does not; it includes qtx.h and follows its conventions
 * (status codes, qtx_last_error, device pointers unless stated, streams as void*). */
#ifndef QTX_BEAM_LONG_H
#define QTX_BEAM_LONG_H

#include "qtx.h"

#ifdef __cplusplus
extern "C" {
#endif

/* qtx_decode_attention's self form for the rows of a beam search that moves no cache: B =
 * sentences * beam rows, row r = b * beam + k.  anc uint8 [B][kv_bs]: position j of row r is
 * read from cache row b * beam + anc[r][j] (keys, both scales, and byte j % 4 of value group
 * j / 4); entries above beam - 1 are read as beam - 1, so no table leads outside the sentence's
 * beam cache rows.  The new k / v / scales are appended at row r's own position *step_dev, the
 * only cache bytes written, and the cached row at that position never reaches the result.
 * Everything else (layouts, alignment, canonical order, results on the gathered caches) is
 * qtx_decode_attention's with kv_new = 1, on the four-wave kernel for every kv_bs <= 512.
 * 1 <= beam <= 8 and B % beam == 0, else QTX_E_INVALID. */
int32_t qtx_decode_attention_beam(const float* y, int64_t ldy, int8_t* kc, int8_t* vc, float* skc,
                                  float* svc, int32_t kv_bs, const int32_t* step_dev,
                                  const uint8_t* anc, int32_t beam, int32_t B, float* ctx,
                                  float* pmax, void* stream);

/* The tail of such a beam step in place of qtx_beam_reorder: anc uint8 [B * beam][max_len],
 * row b * beam + j becomes row b * beam + parent[b * beam + j] over the valid prefix, positions
 * 0 .. n-1 with n = step_dev[0] clamped to max_len, in place (each offset of a sentence's beam
 * rows is owned by one thread, which loads its beam bytes and then stores them by parent).
 * Nothing else is written; an identity parent vector writes nothing.  max_len <= 512. */
int32_t qtx_beam_ancestry(uint8_t* anc, int32_t B, int32_t beam, int32_t max_len,
                          const int32_t* step_dev, const int32_t* parent, void* stream);

#ifdef __cplusplus
}
#endif
#endif  /* QTX_BEAM_LONG_H */

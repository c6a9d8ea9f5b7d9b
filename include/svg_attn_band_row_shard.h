/* Band (SVG1) attention of a ROW SHARD of the rows over a ROW SHARD of the keys: part of the C ABI of libsvgattn (include/svg_attn.h
 * includes this file; the types, error codes and conventions are the ones documented there, SVG_ABI_VERSION is unchanged).  The shard form
 * of include/svg_attn_band_shard.h for shards that cut through frames: a rank of a sequence sharded by rows may hold ANY contiguous range of
 * the video's rows, so the ranks can be balanced where whole frames cannot (33 frames over 8 ranks: 1.21 x the mean on the largest).  A
 * header of its own for the reason include/svg_attn_sparse_lse.h gives; the validation table of these entries is
 * tests/test_band_row_shard_cpu.py, and svg/_band_row_shard.py binds them from BAND_ROW_SHARD_ENTRIES. */
#ifndef SVG_ATTN_BAND_ROW_SHARD_H_
#define SVG_ATTN_BAND_ROW_SHARD_H_
#include "svg_attn.h"

#ifdef __cplusplus
extern "C" {
#endif

/* A shard of a sequence of S rows whose video is F = perm->num_frame frames of P = perm->frame_size rows from row perm->vid0 on, stored
 * frame-major: the video rows [row0, row0 + n_rows) counted from vid0 — sequence row vid0 + row0 + i at shard row i; inside [0, F * P),
 * n_rows may be 0 — and behind them a tail as in svg_band_shard_t: the sequence rows [tail_begin, tail_begin + n_tail) behind the video;
 * n_tail = 0: no tail, tail_begin is not read.  n_rows + n_tail rows in all. */
typedef struct svg_band_row_shard {
    int32_t row0, n_rows;
    int32_t tail_begin, n_tail;
} svg_band_row_shard_t;

/* svg_band_shard_attention_lse / svg_band_shard_attention_lse_f32 with row shards in the place of frame shards; every argument and every
 * statement of include/svg_attn_band_shard.h holds with these coordinate maps:
 *   head in logical order   shard row l is mask row g(l) = vid0 + row0 + l;
 *   token-major head        the shard's video rows (f, p) — frame f, position p, shard row f * P + p - row0 — are taken in increasing order
 *                           of (p, f): for p = 0 .. P - 1 the frames the shard holds of that position, ascending; such a row is mask row
 *                           vid0 + p * F + f.  With a = row0 % P, fa = row0 / P, e = row0 + n_rows, fb = (e - 1) / P, b = e - fb * P,
 *                           position p owns the frames fa + (p < a) .. fb - (p >= b) (possibly none): the count of rows in front of a
 *                           position is piecewise linear in p with breakpoints at min(a, b) and max(a, b), so g and its inverse are
 *                           closed forms of at most three pieces; the host computes the pieces once per launch;
 *   tail                    mask row tail_begin + its index in the tail, for both.
 * A row shard of whole frames (row0 and n_rows multiples of P) has the maps of the svg_band_shard_t {row0 / P, n_rows / P, ..} and the two
 * entries return the bits of svg_band_shard_attention_lse[_f32]; one shard over everything, those of svg_band_attention_lse[_f32].
 * A row that sees no key of the k shard has lse = -inf and o = 0.  Key tiles lie on the k shard's own grid.  No row outside the two shards
 * is read, nothing outside o / lse / o32 of the q shard is written.
 * Supported: head_dim 128, bf16 / fp16, plain q, the static mapping.
 * Return codes, all decided on the host before any launch, in the order of svg_band_shard_attention_lse, with these shard checks, for the q
 * shard, then the k shard: row0 < 0, n_rows < 0, row0 + n_rows > F * P, n_tail < 0, a tail outside [vid0 + F * P, S), an empty shard:
 * SVG_ERR_BAD_ARG. */
int svg_band_row_shard_attention_lse(const void* q, const void* k, const void* v, void* o, float* lse, int32_t BH, int32_t S, int32_t D,
                                     int32_t dtype, float sm_scale, const svg_band_mask_t* mask, const svg_perm_desc_t* perm,
                                     const svg_band_row_shard_t* q_shard, const svg_band_row_shard_t* k_shard,
                                     const svg_attn_layout_t* layout /* NULL: contiguous */, void* stream);
int svg_band_row_shard_attention_lse_f32(const void* q, const void* k, const void* v, float* o32, float* lse, int32_t BH, int32_t S,
                                         int32_t D, int32_t dtype, float sm_scale, const svg_band_mask_t* mask, const svg_perm_desc_t* perm,
                                         const svg_band_row_shard_t* q_shard, const svg_band_row_shard_t* k_shard,
                                         const svg_attn_layout_t* layout /* NULL: contiguous */, void* stream);

/* The coordinate maps the kernels use, evaluated on the host (no GPU), as svg_debug_band_shard_map: g_out[i] = g(x[i]) — x a shard index —
 * ginv_out[i] = the smallest shard index l with g(l) >= x[i] — x a mask coordinate; the shard's row count where there is none — and
 * phys_out[i] = the shard row index x[i] is read from and written to.  Any output may be NULL.  Returns n, or -1 for arguments the entries
 * above refuse. */
int32_t svg_debug_band_row_shard_map(const svg_perm_desc_t* perm, int32_t S, const svg_band_row_shard_t* shard, int32_t token_major,
                                     const int32_t* x, int32_t n, int32_t* g_out, int32_t* ginv_out, int32_t* phys_out);

#ifdef __cplusplus
}
#endif
#endif /* SVG_ATTN_BAND_ROW_SHARD_H_ */

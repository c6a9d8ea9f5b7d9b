/* Centroid tail of SVG2, merged where it is computed: the tail launch of include/svg_attn_centroid_tail.h with the two-part merge of
 * svg_merge_attention_states as its epilogue.  The tail's state of a row is complete in the registers of the one wave that owns the row;
 * that wave fetches the sparse launch's state of the same row while its last key tile is still in work, merges the two and stores the
 * result ONCE — instead of a second [H, Sq, 128] output, an lse and a launch that reads both parts to write a third.  Part of the C ABI of
 * libsvgattn (include/svg_attn.h includes this file; the types, error codes and conventions are the ones documented there,
 * SVG_ABI_VERSION is unchanged).  A header of its own for the reason include/svg_attn_sparse_lse.h gives; the validation table of these
 * entries is tests/test_centroid_tail_merged_cpu.py, their GPU test tests/test_gpu_centroid_tail_merged.py, and svg/_native.py binds them
 * from CENTROID_TAIL_MERGED_ENTRIES (wrapper: svg/_centroid_tail.py centroid_tail_attention(merge_with=...); the caller:
 * svg/models/_core.py CENTROID_TAIL_MERGED).  Kernel: csrc/centroid_tail.hip, TailMergePolicy.
 *
 * Statement.  With (o_t, lse_t) the tail's state of a row (include/svg_attn_centroid_tail.h) and (o_s, lse_s) the sparse part's:
 *     m = max(lse_s, lse_t),  w_x = exp(lse_x - m),  o = (w_s o_s + w_t o_t) / (w_s + w_t),  lse = m + ln(w_s + w_t)
 * in fp32, in the operation order of svg_merge_attention_states for two parts, part 0 the sparse one.  A part with lse = -inf or with a
 * weight that underflows to zero contributes nothing and its o is not looked at; both -inf: o = 0 and lse = -inf.
 *   svg_centroid_tail_merged_attention_lse      o_t is rounded to the tensor dtype in registers first: o and lse are BIT FOR BIT those of
 *                                               svg_centroid_tail_attention_lse followed by svg_merge_attention_states({o_sparse, o_t}).
 *   svg_centroid_tail_merged_attention_lse_f32  the sparse part is fp32 rows (svg_varblock_attention_lse_f32 / ..._lse_auto_f32), o_t stays
 *                                               unrounded, the arithmetic is that of svg_merge_attention_states_f32: ONE rounding between
 *                                               the accumulators of both launches and o.
 * In place: o may be o_sparse (16-bit form) and lse may be lse_sparse (both forms) — a row is read and written by the one wave that owns
 * it, the reads of a row are complete before its stores, and no other wave touches it; any other overlap of an output with an input is
 * undefined.  A row no block-row covers is neither read nor written.  The workspace is that of the parent entry
 * (svg_centroid_tail_workspace_bytes).
 *
 * Return codes: everything is decided on the host before any launch, in this order:
 *   1. - 5. the checks of svg_centroid_tail_attention_lse, in its order and with its codes, on the arguments the two entries share (o and
 *      lse are the merged outputs); in 3., the o member of `layout` is checked as the q member is (o is addressed through it), and with a
 *      layout the alignment of o is looked at there
 *   6. o_sparse / o32_sparse or lse_sparse NULL:                                                                          SVG_ERR_BAD_ARG
 *   7. an o_sparse / o32_sparse that is not 16-byte aligned:                                                              SVG_ERR_UNSUPPORTED */
#ifndef SVG_ATTN_CENTROID_TAIL_MERGED_H_
#define SVG_ATTN_CENTROID_TAIL_MERGED_H_
#include "svg_attn.h"

#ifdef __cplusplus
extern "C" {
#endif

/* q, kbar, vbar, block_map, map_cols, q_sizes, k_sizes, q_row_idx, workspace: as svg_centroid_tail_attention_lse takes them.
 *   o_sparse    [H, Sq, 128] of q's dtype, ADDRESSED AS o IS: contiguous for layout == NULL, otherwise through the o member of layout
 *               (the token-major output of svg_varblock_attention_lse under the same layout)
 *   lse_sparse  fp32 [H, Sq] contiguous, natural logarithm, -inf for a row without keys: both in the caller's row order
 *   o           [H, Sq, 128] of q's dtype: contiguous for layout == NULL, otherwise the o member of layout; lse fp32 [H, Sq] contiguous */
int svg_centroid_tail_merged_attention_lse(const void* q, const void* kbar, const void* vbar, const void* o_sparse, const float* lse_sparse,
                                           void* o, float* lse, int32_t H, int32_t Sq, int32_t KC, int32_t D, int32_t dtype, float sm_scale,
                                           const uint8_t* block_map, int32_t map_cols, const int32_t* q_sizes, const int32_t* k_sizes,
                                           int32_t QB, const int32_t* q_row_idx, void* workspace, size_t workspace_bytes,
                                           const svg_attn_layout_t* layout /* NULL: contiguous */, void* stream);

/* The same with the sparse part before its rounding: o32_sparse fp32 [H, Sq, 128] CONTIGUOUS whatever the layout says (as
 * svg_varblock_attention_lse_f32 writes it), 16-byte aligned; o is rounded once. */
int svg_centroid_tail_merged_attention_lse_f32(const void* q, const void* kbar, const void* vbar, const float* o32_sparse,
                                               const float* lse_sparse, void* o, float* lse, int32_t H, int32_t Sq, int32_t KC, int32_t D,
                                               int32_t dtype, float sm_scale, const uint8_t* block_map, int32_t map_cols,
                                               const int32_t* q_sizes, const int32_t* k_sizes, int32_t QB, const int32_t* q_row_idx,
                                               void* workspace, size_t workspace_bytes, const svg_attn_layout_t* layout /* NULL: contiguous */,
                                               void* stream);

#ifdef __cplusplus
}
#endif
#endif /* SVG_ATTN_CENTROID_TAIL_MERGED_H_ */

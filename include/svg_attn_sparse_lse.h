/* Row log-sum-exp forms of band (SVG1) and variable-block (SVG2) attention: part of the C ABI of libsvgattn (include/svg_attn.h includes
 * this file at its end; the types, error codes and conventions are the ones documented there, SVG_ABI_VERSION is unchanged).
 * They live in a header of their own because tests/test_entry_validation_cpu.py pins its validation table to the svg_band_attention* /
 * svg_varblock_attention* prototypes of svg_attn.h; the table of these two entries is tests/test_sparse_attention_lse_cpu.py, and
 * svg/_native.py binds them from SPARSE_LSE_SIGNATURES. */
#ifndef SVG_ATTN_SPARSE_LSE_H_
#define SVG_ATTN_SPARSE_LSE_H_
#include "svg_attn.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Band (SVG1) and variable-block (SVG2) attention that also return the softmax state of every query row, so that a sparse result over a
 * part of the keys can be merged with others (svg_merge_attention_states): the video x video block-sparse call + the video x text dense
 * call + merge_state of the reference, SVG2 over a subset of the key clusters, a band over the video keys with the text keys in a tensor of
 * their own.  head_dim 128, bf16 / fp16: the default two-phase 16x16x32 body of either family.
 * ref: BlockSparseAttentionWrapper.run(..., return_lse=True) + merge_state, svg/kernels/ops/attention_ops.py:178-188.
 *   lse   CONTIGUOUS fp32 [BH, S] (band) / [Hq, Sq] (variable-block; per q head under GQA) whatever `layout` says about o, indexed by the
 *         caller's row — the row o is written to: also on a token-major head (perm), under q_row_idx, and for both block-rows of a packed
 *         q-tile.  Natural logarithm: lse[row] = log sum_j exp(sm_scale * q[row] . k[j]) over the keys the mask / the block map gives the row.
 *   A row that sees no key (a block-row without active key blocks, or whose active key clusters are all empty) gets lse = -inf and o = 0.
 *   A row the plain entry does not write (variable-block: a row no block-row covers) is not written in lse either.
 *   o     bit-identical to svg_band_attention[_strided] (variant 0) / svg_varblock_attention (variant 3) / svg_varblock_attention_strided
 *         on the same inputs: the same kernel body (band, bf16: with the overflow test on every eighth tile and the replay), whose
 *         epilogue stores one more fp32 per row.  A band q-tile that is replayed stores o and lse once, in the replay.
 *   layout  NULL: contiguous tensors; otherwise as in svg_band_attention_strided / svg_varblock_attention_strided.
 * svg_varblock_attention_lse takes the arguments and the workspace of svg_varblock_attention_strided and ALWAYS runs the two-phase
 * 16x16x32 body in its default launch order (variant 3), also where variant -1 would pick 128-row tiles (Sq < 160 * QB).
 * Return codes, all decided on the host before any launch: lse NULL: SVG_ERR_BAD_ARG; then every argument fault of the plain entry with
 * the code and in the order of the plain entry (pointers and sizes, mask / head permutation, workspace, layout); then D != 128 or a dtype
 * other than bf16 / fp16: SVG_ERR_UNSUPPORTED.  The pre-scaled, fp8 and notify entries, the explicit schedule variants and head_dim 64
 * have no lse form; the device-switch and groups forms of the band entry are include/svg_attn_band_lse_forms.h.  svg_band_attention_lse
 * runs the work queue where svg_band_attention does (bit-identical to the static mapping). */
int svg_band_attention_lse(const void* q, const void* k, const void* v, void* o, float* lse, int32_t BH, int32_t S, int32_t D, int32_t dtype,
                           float sm_scale, const svg_band_mask_t* mask, const svg_perm_desc_t* perm,
                           const svg_attn_layout_t* layout /* NULL: contiguous */, void* stream);
int svg_varblock_attention_lse(const void* q, const void* k, const void* v, void* o, float* lse, int32_t Hq, int32_t Hkv, int32_t Sq,
                               int32_t Skv, int32_t D, int32_t dtype, float sm_scale, const uint8_t* block_map, const int32_t* q_sizes,
                               const int32_t* k_sizes, int32_t QB, int32_t KB, const int32_t* q_row_idx, const int32_t* kv_row_idx,
                               void* workspace, size_t workspace_bytes, const svg_attn_layout_t* layout /* NULL: contiguous */,
                               void* stream);

#ifdef __cplusplus
}
#endif
#endif /* SVG_ATTN_SPARSE_LSE_H_ */

/* fp32-row forms of band (SVG1) and variable-block (SVG2) attention: part of the C ABI of libsvgattn (include/svg_attn.h includes this
 * file at its end; the types, error codes and conventions are the ones documented there, SVG_ABI_VERSION is unchanged).
 * They live in a header of their own for the reason include/svg_attn_sparse_lse.h does: tests/test_entry_validation_cpu.py pins its
 * validation table to the svg_band_attention* / svg_varblock_attention* prototypes of svg_attn.h; the table of these two entries is
 * tests/test_attention_f32_parts_cpu.py, and svg/_native.py binds them from SPARSE_F32_SIGNATURES. */
#ifndef SVG_ATTN_F32_PARTS_H_
#define SVG_ATTN_F32_PARTS_H_
#include "svg_attn.h"

#ifdef __cplusplus
extern "C" {
#endif

/* svg_band_attention_lse / svg_varblock_attention_lse that hand out every row BEFORE its rounding, as svg_cross_attention_lse_f32 does:
 * parts for svg_merge_attention_states_f32, whose rounding is then the only one (a band over the video keys + dense attention over the
 * text keys, SVG2 over ranges of the key clusters, at the accuracy of one call).  The arguments are those of the _lse entries with
 *   o32   fp32 CONTIGUOUS [BH, S, D] (band) / [Hq, Sq, D] (variable-block) whatever `layout` says, indexed by the caller's row — the row
 *         lse uses: also on a token-major head (perm), under q_row_idx, and for both block-rows of a packed q-tile —
 * in the place of o.  No 16-bit o is written.  o32 rounded to nearest even is the o of the _lse entry bit for bit, lse is bit-identical:
 * the same kernel body (band, bf16: with the overflow test and the replay; a replayed q-tile stores o32 and lse once, in the replay) and
 * the same route through the dispatch; the band kernel runs on the static mapping, the variable-block entry always the body of variant 3.
 * A row that sees no key gets o32 = 0 and lse = -inf; a row the plain entry does not write (variable-block: a row no block-row covers) is
 * written in neither.  layout: NULL for contiguous q, k, v; otherwise it describes q, k and v, its o member is not read.
 * Return codes, all decided on the host before any launch: o32 or lse NULL: SVG_ERR_BAD_ARG; then every argument fault of the _lse entry
 * with its code and in its order; D != 128, a dtype other than bf16 / fp16 or an o32 that is not 16-byte aligned: SVG_ERR_UNSUPPORTED.
 * The pair, pre-scaled, fp8 and notify entries and head_dim 64 have no fp32 form; the device-switch and groups forms of the band entry
 * are include/svg_attn_band_lse_forms.h. */
int svg_band_attention_lse_f32(const void* q, const void* k, const void* v, float* o32, float* lse, int32_t BH, int32_t S, int32_t D,
                               int32_t dtype, float sm_scale, const svg_band_mask_t* mask, const svg_perm_desc_t* perm,
                               const svg_attn_layout_t* layout /* NULL: contiguous */, void* stream);
int svg_varblock_attention_lse_f32(const void* q, const void* k, const void* v, float* o32, float* lse, int32_t Hq, int32_t Hkv, int32_t Sq,
                                   int32_t Skv, int32_t D, int32_t dtype, float sm_scale, const uint8_t* block_map, const int32_t* q_sizes,
                                   const int32_t* k_sizes, int32_t QB, int32_t KB, const int32_t* q_row_idx, const int32_t* kv_row_idx,
                                   void* workspace, size_t workspace_bytes, const svg_attn_layout_t* layout /* NULL: contiguous */,
                                   void* stream);

#ifdef __cplusplus
}
#endif
#endif /* SVG_ATTN_F32_PARTS_H_ */

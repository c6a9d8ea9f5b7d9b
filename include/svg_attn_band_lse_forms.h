/* Row log-sum-exp and fp32-row forms of the device-switch and groups launches of band (SVG1) attention: part of the C ABI of libsvgattn
 * (include/svg_attn.h includes this file at its end; the types, error codes and conventions are the ones documented there,
 * SVG_ABI_VERSION is unchanged).  They live in a header of their own for the reason include/svg_attn_sparse_lse.h does:
 * tests/test_entry_validation_cpu.py pins its validation table to the svg_band_attention* prototypes of svg_attn.h; the table of these
 * four entries is tests/test_band_lse_forms_cpu.py, and svg/_native.py binds them from BAND_LSE_FORM_SIGNATURES. */
#ifndef SVG_ATTN_BAND_LSE_FORMS_H_
#define SVG_ATTN_BAND_LSE_FORMS_H_
#include "svg_attn.h"

#ifdef __cplusplus
extern "C" {
#endif

/* svg_band_attention_lse / svg_band_attention_lse_f32 for the launch forms the SVG1 processors take by default: the device switch
 * (svg_band_attention_switch[_strided]) and groups of heads under masks of their own (svg_band_groups_attention), so that a layer-call on
 * those forms can be one part of a partitioned attention (svg_merge_attention_states[_f32]).  head_dim 128, bf16 / fp16, plain q.
 *   o      the bits of svg_band_attention_switch[_strided] / svg_band_groups_attention(q_prescaled = 0) on the same arguments: the same
 *          kernel body on the same mapping (bf16: with the overflow test on every eighth tile and the replay; a q-tile that is replayed
 *          stores o and lse once, in the replay).
 *   lse    CONTIGUOUS fp32 [BH, S] whatever `layout` says, in the caller's row order — the row o is written to: the physical row of a
 *          token-major head under `mask` (flag 0), the logical row under `alt_mask` (flag != 0), which runs without the head permutation.
 *          Natural logarithm: lse[row] = log sum_j exp(sm_scale * q[row] . k[j]) over the keys the selected mask gives the row, the
 *          definition of svg_band_attention_lse.  A row with no allowed key has o = 0 (o32 = 0) and lse = -inf.
 *   layout NULL: contiguous tensors; otherwise as in svg_band_attention_switch_strided / svg_band_groups_attention.
 * The _f32 forms follow svg_band_attention_lse_f32: o32, CONTIGUOUS fp32 [BH, S, D] in the row order of lse, takes the place of o and
 * no 16-bit o is written; o32 rounded to nearest even is the o of the _lse form bit for bit and lse is bit-identical; of a layout the o
 * member is not read; o32 must be 16-byte aligned.
 * Groups: one launch per group with the bases of o / o32 and lse advanced to the group's first head (64-bit offsets): bit for bit one
 * svg_band_attention_lse[_f32] call per group (alt_masks == NULL, with use_alt_flag == NULL: the work queue where svg_band_attention
 * takes it) or one svg_band_attention_switch_lse[_f32] call per group (alt_masks and use_alt_flag given).
 * Return codes, all decided on the host before any launch: lse (or o32) NULL: SVG_ERR_BAD_ARG; then every argument fault of the plain
 * entry with the code and in the order of the plain entry; then D != 128 or a dtype other than bf16 / fp16: SVG_ERR_UNSUPPORTED; an o32
 * that is not 16-byte aligned: SVG_ERR_UNSUPPORTED.  The pre-scaled, fp8 and notify entries, the explicit schedule variants and head_dim 64
 * have no such form. */
int svg_band_attention_switch_lse(const void* q, const void* k, const void* v, void* o, float* lse, int32_t BH, int32_t S, int32_t D,
                                  int32_t dtype, float sm_scale, const svg_band_mask_t* mask, const svg_perm_desc_t* perm,
                                  const svg_band_mask_t* alt_mask, const int32_t* use_alt_flag,
                                  const svg_attn_layout_t* layout /* NULL: contiguous */, void* stream);
int svg_band_attention_switch_lse_f32(const void* q, const void* k, const void* v, float* o32, float* lse, int32_t BH, int32_t S, int32_t D,
                                      int32_t dtype, float sm_scale, const svg_band_mask_t* mask, const svg_perm_desc_t* perm,
                                      const svg_band_mask_t* alt_mask, const int32_t* use_alt_flag,
                                      const svg_attn_layout_t* layout /* NULL: contiguous */, void* stream);
int svg_band_groups_attention_lse(const void* q, const void* k, const void* v, void* o, float* lse, int32_t BH, int32_t S, int32_t D,
                                  int32_t dtype, float sm_scale, const svg_band_mask_t* masks, const svg_band_mask_t* alt_masks /* or NULL */,
                                  const int32_t* group_heads, int32_t n_groups, const svg_perm_desc_t* perm, const int32_t* use_alt_flag,
                                  const svg_attn_layout_t* layout /* NULL: contiguous */, void* stream);
int svg_band_groups_attention_lse_f32(const void* q, const void* k, const void* v, float* o32, float* lse, int32_t BH, int32_t S, int32_t D,
                                      int32_t dtype, float sm_scale, const svg_band_mask_t* masks,
                                      const svg_band_mask_t* alt_masks /* or NULL */, const int32_t* group_heads, int32_t n_groups,
                                      const svg_perm_desc_t* perm, const int32_t* use_alt_flag,
                                      const svg_attn_layout_t* layout /* NULL: contiguous */, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* SVG_ATTN_BAND_LSE_FORMS_H_ */

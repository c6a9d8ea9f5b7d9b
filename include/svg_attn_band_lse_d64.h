/* Band (SVG1) attention at head_dim 64 with the row log-sum-exp, and with fp32 rows: part of the C ABI of libsvgattn (include/svg_attn.h
 * includes this file near its end — tests pin the last four includes —; the types, error codes and conventions are the ones documented there, SVG_ABI_VERSION is unchanged).
 * A header and entries of their own: the head_dim-128 entries svg_band_attention_lse[_f32] and svg_band_attention_switch_lse[_f32] refuse
 * head_dim 64, and their validation tables pin that; these four take it and refuse everything else.  Their table is
 * tests/test_band_lse_d64_cpu.py, and svg/_native.py binds them from BAND_LSE_D64_ENTRIES. */
#ifndef SVG_ATTN_BAND_LSE_D64_H_
#define SVG_ATTN_BAND_LSE_D64_H_
#include "svg_attn.h"

#ifdef __cplusplus
extern "C" {
#endif

/* The arguments of svg_band_attention_lse[_f32] (include/svg_attn_sparse_lse.h, svg_attn_f32_parts.h) and of
 * svg_band_attention_switch_lse[_f32] (include/svg_attn_band_lse_forms.h), for D == 64, bf16 / fp16, plain q: what a CogVideoX layer-call
 * needs to be one part of a partitioned attention (svg_merge_attention_states[_f32]) and to report its kept mass.  The kernel is the body of
 * the plain head_dim-64 call (the 32x32x16 two-phase body, four waves per SIMD) on the static mapping over (head, q-tile).
 *   o      the bits of svg_band_attention / svg_band_attention_strided (switch: svg_band_attention_switch[_strided]) at D = 64 on the same
 *          arguments.
 *   lse    CONTIGUOUS fp32 [BH, S] whatever `layout` says, in the row order o is written in: the physical row of a token-major head under
 *          `mask`, the logical row under `alt_mask` (use_alt_flag[0] != 0), which runs without the head permutation.  Natural logarithm:
 *          lse[row] = log sum_j exp(sm_scale * q[row] . k[j]) over the keys the selected mask gives the row.  A row with no allowed key has
 *          o = 0 (o32 = 0) and lse = -inf; every row of [0, S) is written.
 *   layout NULL: contiguous [BH, S, 64] tensors; otherwise as in svg_band_attention_strided.
 * The _f32 forms: o32, CONTIGUOUS fp32 [BH, S, 64] in the row order of lse, takes the place of o and no 16-bit o is written; o32 rounded
 * to nearest even is the o of the 16-bit form bit for bit; of a layout the o member is not read; o32 must be
 * 16-byte aligned.
 * Return codes, all decided on the host before any launch, in the order of the head_dim-128 namesake: lse (or o32, alt_mask,
 * use_alt_flag) NULL: SVG_ERR_BAD_ARG; then every argument fault of the plain entry with its code; then D != 64: SVG_ERR_UNSUPPORTED; an o32
 * that is not 16-byte aligned, or a dtype other than bf16 / fp16: SVG_ERR_UNSUPPORTED.  No work queue, groups, window, shard, pre-scaled or
 * notify form. */
int svg_band_attention_lse_d64(const void* q, const void* k, const void* v, void* o, float* lse, int32_t BH, int32_t S, int32_t D,
                               int32_t dtype, float sm_scale, const svg_band_mask_t* mask, const svg_perm_desc_t* perm,
                               const svg_attn_layout_t* layout /* NULL: contiguous */, void* stream);
int svg_band_attention_lse_d64_f32(const void* q, const void* k, const void* v, float* o32, float* lse, int32_t BH, int32_t S, int32_t D,
                                   int32_t dtype, float sm_scale, const svg_band_mask_t* mask, const svg_perm_desc_t* perm,
                                   const svg_attn_layout_t* layout /* NULL: contiguous */, void* stream);
int svg_band_attention_switch_lse_d64(const void* q, const void* k, const void* v, void* o, float* lse, int32_t BH, int32_t S, int32_t D,
                                      int32_t dtype, float sm_scale, const svg_band_mask_t* mask, const svg_perm_desc_t* perm,
                                      const svg_band_mask_t* alt_mask, const int32_t* use_alt_flag,
                                      const svg_attn_layout_t* layout /* NULL: contiguous */, void* stream);
int svg_band_attention_switch_lse_d64_f32(const void* q, const void* k, const void* v, float* o32, float* lse, int32_t BH, int32_t S,
                                          int32_t D, int32_t dtype, float sm_scale, const svg_band_mask_t* mask,
                                          const svg_perm_desc_t* perm, const svg_band_mask_t* alt_mask, const int32_t* use_alt_flag,
                                          const svg_attn_layout_t* layout /* NULL: contiguous */, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* SVG_ATTN_BAND_LSE_D64_H_ */

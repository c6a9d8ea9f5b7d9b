/* Variable-block (SVG2) attention with the row log-sum-exp, and with fp32 rows, from the body svg_varblock_attention(variant = -1) picks:
 * part of the C ABI of libsvgattn (include/svg_attn.h includes this file near its end — tests pin its last includes —; the types, error
 * codes and conventions are the ones documented there, SVG_ABI_VERSION is unchanged).
 * A header and entries of their own: svg_varblock_attention_lse[_f32] (include/svg_attn_sparse_lse.h, svg_attn_f32_parts.h) ALWAYS run the
 * two-phase 16x16x32 body on 256-row q-tiles and refuse head_dim 64, and their validation tables pin that; these two follow the plain
 * call.  Their table is tests/test_varblock_lse_auto_cpu.py, and svg/_native.py binds them from VARBLOCK_LSE_AUTO_ENTRIES. */
#ifndef SVG_ATTN_VARBLOCK_LSE_AUTO_H_
#define SVG_ATTN_VARBLOCK_LSE_AUTO_H_
#include "svg_attn.h"

#ifdef __cplusplus
extern "C" {
#endif

/* The arguments, the workspace, lse and o32 of svg_varblock_attention_lse[_f32], for D == 128 and D == 64, bf16 / fp16.  The body is chosen
 * by the rule of svg_varblock_attention(variant = -1):
 *   Sq >= 160 * QB   256-row q-tiles in the default launch order: the two-phase 16x16x32 body at D = 128 (the kernels of
 *                    svg_varblock_attention_lse[_f32]), the two-phase 32x32x16 body at D = 64;
 *   Sq <  160 * QB   128-row q-tiles on the four-wave lock-step body, at either head size.
 *   o      the bits of svg_varblock_attention(variant = -1) (with a layout: svg_varblock_attention_strided) on the same arguments.
 *   lse    CONTIGUOUS fp32 [Hq, Sq], per q head under GQA, indexed by the physical q row — the row q_row_idx names, the sorted position
 *          without it — for both block-rows of a remainder-packed q-tile too.  Natural logarithm of the sum of exp(sm_scale * q . k) over
 *          the keys the block map gives the row; a row whose block-row selects no key (or only empty key clusters) gets lse = -inf and
 *          o = 0 (o32 = 0).  A row no block-row covers is written in neither.
 *   layout NULL: contiguous tensors.  Otherwise as in svg_varblock_attention_strided, which only the two-phase bodies take: with a layout
 *          and Sq < 160 * QB the call is refused, as the plain strided entry refuses it.
 * The _f32 form: o32, CONTIGUOUS fp32 [Hq, Sq, D] in the row order of lse, takes the place of o and no 16-bit o is written; o32 rounded
 * to nearest even is the o of the 16-bit form bit for bit; of a layout the o member is not read; o32 must be 16-byte aligned.
 * Return codes, all decided on the host before any launch, in this order: lse (or o32) NULL: SVG_ERR_BAD_ARG; then every argument fault of
 * svg_varblock_attention with its code and in its order (NULL pointers and non-positive sizes, Hq % Hkv: SVG_ERR_BAD_ARG; KB above the
 * run-list limit, Sq or Skv beyond the row limit of the head size: SVG_ERR_UNSUPPORTED; a workspace smaller than
 * svg_varblock_workspace_bytes: SVG_ERR_WORKSPACE); then the faults of `layout` with the codes of svg_varblock_attention_strided; then a
 * head size without a form (D = 64 and D = 128 have one): SVG_ERR_UNSUPPORTED; an o32 that is not 16-byte aligned: SVG_ERR_UNSUPPORTED; a
 * layout on 128-row tiles: SVG_ERR_UNSUPPORTED; a dtype other than bf16 / fp16, or a head size other than 64 / 128:
 * SVG_ERR_UNSUPPORTED.  No variant argument: the traced, block-row-ordered, 256-row lock-step and mixed schedules, the similarity order
 * and the fp8 entry have no lse form. */
int svg_varblock_attention_lse_auto(const void* q, const void* k, const void* v, void* o, float* lse, int32_t Hq, int32_t Hkv, int32_t Sq,
                                    int32_t Skv, int32_t D, int32_t dtype, float sm_scale, const uint8_t* block_map,
                                    const int32_t* q_sizes, const int32_t* k_sizes, int32_t QB, int32_t KB, const int32_t* q_row_idx,
                                    const int32_t* kv_row_idx, void* workspace, size_t workspace_bytes,
                                    const svg_attn_layout_t* layout /* NULL: contiguous */, void* stream);
int svg_varblock_attention_lse_auto_f32(const void* q, const void* k, const void* v, float* o32, float* lse, int32_t Hq, int32_t Hkv,
                                        int32_t Sq, int32_t Skv, int32_t D, int32_t dtype, float sm_scale, const uint8_t* block_map,
                                        const int32_t* q_sizes, const int32_t* k_sizes, int32_t QB, int32_t KB,
                                        const int32_t* q_row_idx, const int32_t* kv_row_idx, void* workspace, size_t workspace_bytes,
                                        const svg_attn_layout_t* layout /* NULL: contiguous */, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* SVG_ATTN_VARBLOCK_LSE_AUTO_H_ */

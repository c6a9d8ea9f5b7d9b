/* The device switch of band (SVG1) attention on FRAME SHARDS: part of the C ABI of libsvgattn (include/svg_attn.h includes this file at its
 * end, behind svg_attn_band_shard.h; the types, error codes and conventions are the ones documented there, SVG_ABI_VERSION is unchanged).  A
 * header of its own for the reason include/svg_attn_sparse_lse.h gives; the validation table of these entries is
 * tests/test_band_shard_switch_cpu.py, and svg/_native.py binds them from BAND_SHARD_SWITCH_SIGNATURES. */
#ifndef SVG_ATTN_BAND_SHARD_SWITCH_H_
#define SVG_ATTN_BAND_SHARD_SWITCH_H_
#include "svg_attn_band_shard.h"

#ifdef __cplusplus
extern "C" {
#endif

/* svg_band_shard_attention_lse / svg_band_shard_attention_lse_f32 with the mask chosen on the device, as svg_band_attention_switch_lse[_f32]
 * chooses it on the whole sequence: a rank of a sequence sharded by frames runs the sparse steps and the dense warm-up steps of an SVG1
 * processor from one launch sequence, and the host never reads the flag.  Every argument of the shard entries as documented there, plus
 *   alt_mask      a mask over the S rows of the WHOLE sequence, never NULL;
 *   use_alt_flag  device int32[1], never NULL, read by the kernel:
 *                   use_alt_flag[0] == 0: exactly svg_band_shard_attention_lse[_f32](mask, perm);
 *                   use_alt_flag[0] != 0: exactly svg_band_shard_attention_lse[_f32](alt_mask, perm'), perm' = perm with
 *                   head_perm_flag = NULL — every head in logical order, head_perm_flag is not read; perm's vid0 / num_frame /
 *                   frame_size still define the two shard maps.
 * o, o32 and lse are written at the shard row q was read from in both cases; a row that sees no key of the k shard under the mask the
 * flag selects has lse = -inf and o = 0 (o32 = 0).  One launch of max(q-tiles under mask, q-tiles under alt_mask) * BH workgroups.
 * With vid0 = 0 and both shards {0, F, F * P, S - F * P} the two entries return the bits of svg_band_attention_switch_lse[_f32] for
 * either flag value.
 * Supported: head_dim 128, bf16 / fp16, plain q, the static mapping.
 * Return codes, all decided on the host before any launch, in this order — the order of the shard entries, with alt_mask and use_alt_flag
 * where mask is: a NULL q, k, v, o (o32), lse, mask, perm, q_shard, k_shard, alt_mask or use_alt_flag: SVG_ERR_BAD_ARG; BH or S <= 0,
 * num_frame or frame_size <= 0, vid0 < 0 or a video that ends behind S: SVG_ERR_BAD_ARG; for the q shard, then the k shard: frames
 * outside [0, F), n_tail < 0, a tail outside [vid0 + F * P, S), an empty shard: SVG_ERR_BAD_ARG; then what every band entry checks, where it
 * checks it: mask against S (SVG_ERR_BAD_ARG), the size limits of svg_band_attention on (BH, S, D) (SVG_ERR_UNSUPPORTED), then alt_mask
 * against S (SVG_ERR_BAD_ARG) — as in svg_band_attention_switch —, the layout as in svg_band_attention_strided, against Sq and Sk; then
 * SVG_ERR_UNSUPPORTED for D != 128, an o32 that is not 16-byte aligned, a dtype other than bf16 / fp16. */
int svg_band_shard_attention_switch_lse(const void* q, const void* k, const void* v, void* o, float* lse, int32_t BH, int32_t S, int32_t D,
                                        int32_t dtype, float sm_scale, const svg_band_mask_t* mask, const svg_perm_desc_t* perm,
                                        const svg_band_mask_t* alt_mask, const int32_t* use_alt_flag, const svg_band_shard_t* q_shard,
                                        const svg_band_shard_t* k_shard, const svg_attn_layout_t* layout /* NULL: contiguous */,
                                        void* stream);
int svg_band_shard_attention_switch_lse_f32(const void* q, const void* k, const void* v, float* o32, float* lse, int32_t BH, int32_t S,
                                            int32_t D, int32_t dtype, float sm_scale, const svg_band_mask_t* mask,
                                            const svg_perm_desc_t* perm, const svg_band_mask_t* alt_mask, const int32_t* use_alt_flag,
                                            const svg_band_shard_t* q_shard, const svg_band_shard_t* k_shard,
                                            const svg_attn_layout_t* layout /* NULL: contiguous */, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* SVG_ATTN_BAND_SHARD_SWITCH_H_ */

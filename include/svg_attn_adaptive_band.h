/* SVG1's band width per head, on the device, steered by measured kept mass: band attention that reads its head's band from a device vector,
 * its device-switch form, and the controller step.  Part of the C ABI of libsvgattn (include/svg_attn.h includes this file in front of
 * svg_attn_adaptive_top_p.h, whose place and the place of svg_attn_profile_shard.h behind it are pinned by their own tests; the types, error
 * codes and conventions are the ones documented in svg_attn.h, SVG_ABI_VERSION is unchanged).  A header of its own for the reason
 * include/svg_attn_sparse_lse.h gives; the validation tables of these entries are tests/test_adaptive_band_cpu.py, and svg/_native.py binds
 * them from ADAPTIVE_BAND_ENTRIES (allocating wrappers: svg/_adaptive_band.py; the loop: svg/models/_core.py AdaptiveBand, BandStore,
 * svg1_attention_device_switch(adaptive=...)).
 *
 * A layer keeps one band per head in device memory.  A sparse layer-call runs the band kernel on it, probes R sampled rows densely (K
 * only, svg_sample_dense_lse), and steps every head's band towards the kept mass the user asked for; nothing is read back. */
#ifndef SVG_ATTN_ADAPTIVE_BAND_H_
#define SVG_ATTN_ADAPTIVE_BAND_H_
#include "svg_attn.h"
#include "svg_attn_sparse_lse.h"
#include "svg_attn_band_lse_forms.h"

#ifdef __cplusplus
extern "C" {
#endif

/* svg_band_attention_lse with one band per head: band is a DEVICE int32 [BH].  Head h gets the o and lse bits svg_band_attention_lse writes
 * for that head when mask->band is replaced by b_h = min(max(band[h], 1), S + 1); the clamp is done in the kernel (a device value cannot
 * be validated on the host).  Everything else — the other five fields of the mask, perm, layout, the row lse is indexed by, -inf / zeros
 * for a row without keys, the overflow test on every eighth tile and the replay for bf16 — is as there.  The launch maps q-tiles statically, as
 * the device switch does: a head partitions its rows into q-tiles as svg_band_attention_lse does for its b_h (a band above S does not cut
 * the full rows out, as there).  head_dim 128, bf16 / fp16 only.
 * Return codes, all decided on the host before any launch, in the order of svg_band_attention_lse: a NULL lse or band: SVG_ERR_BAD_ARG; a
 * NULL q, k, v, o or mask, BH or S <= 0, a mask that fails its checks (mask->band included, although no head runs it):
 * SVG_ERR_BAD_ARG; sizes beyond the limits of svg_band_attention: SVG_ERR_UNSUPPORTED; the layout: as in svg_band_attention_strided;
 * head_dim other than 128 or a dtype other than bf16 / fp16: SVG_ERR_UNSUPPORTED. */
int svg_band_attention_per_head_lse(const void* q, const void* k, const void* v, void* o, float* lse, int32_t BH, int32_t S, int32_t D,
                                    int32_t dtype, float sm_scale, const svg_band_mask_t* mask, const int32_t* band /* device [BH] */,
                                    const svg_perm_desc_t* perm, const svg_attn_layout_t* layout /* NULL: contiguous */, void* stream);

/* The device switch of the per-head form: use_alt[0] != 0 runs alt_mask as it is, without the head permutation, and ignores band — the
 * bits of svg_band_attention_switch_lse under that flag; otherwise the per-head form above.  What the processors launch.  band is never
 * written.
 * Return codes as above, with a NULL alt_mask or use_alt joining the NULL lse and band, and alt_mask checked where mask is. */
int svg_band_attention_switch_per_head_lse(const void* q, const void* k, const void* v, void* o, float* lse, int32_t BH, int32_t S,
                                           int32_t D, int32_t dtype, float sm_scale, const svg_band_mask_t* mask,
                                           const svg_band_mask_t* alt_mask, const int32_t* use_alt /* device [1] */,
                                           const int32_t* band /* device [BH] */, const svg_perm_desc_t* perm,
                                           const svg_attn_layout_t* layout, void* stream);

/* The controller: one launch, one wave per head — gather the sparse call's lse at the sampled rows, reduce to the kept mass, step the band.
 *   lse_sparse, rows, lse_dense, kept: as in svg_top_p_update (include/svg_attn_adaptive_top_p.h), kept with the same bits:
 *     kept[h]  = (1 / R) sum_i exp(lse_sparse[h, rows[i]] - lse_dense[h, i])        a -inf in lse_sparse counts 0; differences,
 *                exponentials and the sum in fp64, one rounding to fp32; a row outside [0, S) is not read and makes kept[h] NaN.
 *   Every word of kept is written.  band int32 [BH] is stepped in place:
 *     skip_flag && skip_flag[0] != 0     band[h] unchanged   (a dense warm-up step: its kept mass is 1 and says nothing)
 *     kept[h] not finite                 band[h] unchanged
 *     e = target - kept[h]
 *     x = e > 0 ? gain_up * e : (e < -dead ? gain_down * (e + dead) : 0)            gains: quanta per unit of kept mass
 *     x = min(max(x, -65536), 65536);  n = (int) rintf(x)
 *     band[h] = min(max(band[h] + n * quantum, band_min), band_max)                 (the sum in 64 bits: no wrap)
 *   e, x and the clamp are plain fp32, every product and sum rounded (no contraction).
 * SVG_ERR_BAD_ARG, on the host before any launch, for: a NULL pointer (skip_flag excepted); R outside [1, 64]; BH or S <= 0; a negative or
 * NaN gain_up, gain_down or dead; quantum outside [1, 4096]; anything but 1 <= band_min <= band_max <= S + 1.  target is not checked. */
int svg_band_width_update(const float* lse_sparse, const int64_t* rows, const float* lse_dense, int32_t R, int32_t BH, int32_t S,
                          float target, float gain_up, float gain_down, float dead, int32_t quantum, int32_t band_min, int32_t band_max,
                          const int32_t* skip_flag /* device [1] or NULL */, float* kept /* [BH] */, int32_t* band /* [BH], in place */,
                          void* stream);

#ifdef __cplusplus
}
#endif
#endif /* SVG_ATTN_ADAPTIVE_BAND_H_ */

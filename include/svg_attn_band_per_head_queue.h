/* The per-head band launch (include/svg_attn_adaptive_band.h) and its device switch as resident workgroups on the work queue, and the host
 * statement of the order the queue hands out.  Part of the C ABI of libsvgattn (include/svg_attn.h includes this file directly in front of
 * svg_attn_adaptive_band.h; the types, error codes and conventions are the ones documented in svg_attn.h, SVG_ABI_VERSION is unchanged).  A
 * header of its own for the reason include/svg_attn_sparse_lse.h gives; the validation tables of these entries are
 * tests/test_band_per_head_queue_cpu.py, and svg/_native.py binds them from ADAPTIVE_BAND_QUEUE_ENTRIES (allocating wrappers:
 * svg/_adaptive_band.py, work_queue=True; the processors: svg/models/_core.py PER_HEAD_BAND_QUEUE).
 *
 * The queue's order is a balance heuristic and never a correctness condition: every row sees the same keys in the same order whatever the
 * order of the q-tiles.  The host sorts by the band it knows, the hint min(mask->band, S) the heads' bands start from, and the dynamic
 * taking absorbs what the hint gets wrong.  Under unequal bands the tail's "longest first" therefore holds with respect to the hint
 * only: a head whose band has grown past the hint's has longer q-tiles in the tail than the order assumes. */
#ifndef SVG_ATTN_BAND_PER_HEAD_QUEUE_H_
#define SVG_ATTN_BAND_PER_HEAD_QUEUE_H_
#include "svg_attn.h"
#include "svg_attn_sparse_lse.h"
#include "svg_attn_band_lse_forms.h"

#ifdef __cplusplus
extern "C" {
#endif

/* svg_band_attention_per_head_lse on the work queue: o and lse are bit for bit what that entry writes on the same arguments; the argument
 * checks are that entry's, with the same codes in the same order, all on the host before any launch; band (DEVICE int32 [BH]) is clamped to
 * min(max(band[h], 1), S + 1) in the kernel and never written.  head_dim 128, bf16 / fp16.
 * The launch: min(work items, CUs) resident workgroups that take (head, q-tile) pairs from the queue of a launch under the hint
 * min(mask->band, S), on this stream's counter block.  A head whose clamped band exceeds S does not cut the full rows out: it takes the
 * index of a pair as its q-tile, and a pair whose index lies behind that head's last q-tile is dropped by the lane that took it, which
 * takes again.  Where no counter block is to be had (stream capture, more streams than blocks), or one round of workgroups covers the
 * launch and svg_debug_band_queue_cap is 0, the statically mapped kernels of svg_band_attention_per_head_lse run instead. */
int svg_band_attention_per_head_queue_lse(const void* q, const void* k, const void* v, void* o, float* lse, int32_t BH, int32_t S, int32_t D,
                                          int32_t dtype, float sm_scale, const svg_band_mask_t* mask, const int32_t* band /* device [BH] */,
                                          const svg_perm_desc_t* perm, const svg_attn_layout_t* layout /* NULL: contiguous */,
                                          void* stream);

/* svg_band_attention_switch_per_head_lse on the work queue, bit for bit and check for check as above.  use_alt[0] != 0 selects the queue of
 * alt_mask and the alternate block for the whole launch (no band vector, no head flags, nothing dropped); otherwise the form above.  The
 * launch is sized for the larger of the two queues. */
int svg_band_attention_switch_per_head_queue_lse(const void* q, const void* k, const void* v, void* o, float* lse, int32_t BH, int32_t S,
                                                 int32_t D, int32_t dtype, float sm_scale, const svg_band_mask_t* mask,
                                                 const svg_band_mask_t* alt_mask, const int32_t* use_alt /* device [1] */,
                                                 const int32_t* band /* device [BH] */, const svg_perm_desc_t* perm,
                                                 const svg_attn_layout_t* layout, void* stream);

/* What the two launches above hand out, on the host, as svg_band_queue_order states it for the plain queue: the eight XCD lists one after
 * the other, then the tail, each in the order its counter hands it out.  One quadruple of int32 per work item:
 *     out[4 i]      the list, 0 .. 7, or 8 for the tail
 *     out[4 i + 1]  the head
 *     out[4 i + 2]  the index the head runs as its q-tile, or -1 where the item is dropped (a head on the wide block, behind its last q-tile)
 *     out[4 i + 3]  the parameter block: 0 = the hint's, full rows cut out; 1 = wide (band above S); 2 = alternate
 * band is a HOST int32 [BH] here, clamped as the kernel clamps it; use_alt != 0 states the launch under the flag (alt_mask then must not
 * be NULL; band is not read).  alt_mask may be NULL with use_alt == 0.
 * out == NULL: the number of work items.  Otherwise the number written, or -1 if out_words cannot hold them (nothing is written past
 * out + out_words).  -1 also for a NULL mask or band, BH or S <= 0, a mask or alt_mask that fails the checks of svg_band_attention. */
int32_t svg_band_per_head_queue_order(int32_t BH, int32_t S, const svg_band_mask_t* mask, const svg_band_mask_t* alt_mask /* or NULL */,
                                      int32_t use_alt, const int32_t* band /* HOST int32 [BH] */, int32_t* out, int32_t out_words);

#ifdef __cplusplus
}
#endif
#endif /* SVG_ATTN_BAND_PER_HEAD_QUEUE_H_ */

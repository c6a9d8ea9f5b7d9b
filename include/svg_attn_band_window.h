/* Band (SVG1) attention over a ROW window and a KEY window of the mask: part of the C ABI of libsvgattn (include/svg_attn.h includes this
 * file at its end; the types, error codes and conventions are the ones documented there, SVG_ABI_VERSION is unchanged).  A header of its
 * own for the reason include/svg_attn_sparse_lse.h gives: tests/test_entry_validation_cpu.py pins its validation table to the
 * svg_band_attention* prototypes of svg_attn.h; the table of these two entries is tests/test_band_window_cpu.py, and svg/_native.py binds
 * them from BAND_WINDOW_SIGNATURES. */
#ifndef SVG_ATTN_BAND_WINDOW_H_
#define SVG_ATTN_BAND_WINDOW_H_
#include "svg_attn.h"

#ifdef __cplusplus
extern "C" {
#endif

/* svg_band_attention_lse / svg_band_attention_lse_f32 for a caller that holds only a part of the rows and a part of the keys of a sequence
 * of S rows — a rank of a token-sharded sequence that has received a peer's key shard, or a key partition of one band call:
 *   q, o   the rows [q_begin, q_begin + Sq) of the sequence: [BH, Sq, D] (or the layout's strides);
 *   k, v   the rows [k_begin, k_begin + Sk): [BH, Sk, D] (or the layout's strides);
 *   mask   row i of the q buffer sees row j of the k buffer exactly where the mask allows (q_begin + i, k_begin + j) — band, full columns,
 *          full rows and the two segments either side of real_len, all at the coordinates of the whole sequence.  A window is a clip of
 *          the mask, not a mask of its own;
 *   lse    CONTIGUOUS fp32 [BH, Sq]: natural log of sum_j exp(sm_scale * q[i] . k[j]) over the keys of the window the row may see; a row
 *          that sees none has lse = -inf and o = 0 (o32 = 0).  What svg_merge_attention_states[_f32] takes: the parts of one row window
 *          over disjoint key windows that cover [0, S) merge to the result of svg_band_attention_lse on the whole sequence;
 *   o32    (the _f32 form, in the place of o; no 16-bit o is written) CONTIGUOUS fp32 [BH, Sq, 128], 16-byte aligned: the rows before
 *          their rounding; rounded to nearest even they are the o of the _lse form bit for bit, lse is bit-identical.  Of a layout the o
 *          member is not read;
 *   layout NULL: contiguous tensors; otherwise as in svg_band_attention_strided, with Sq rows of q / o and Sk rows of k / v.
 * With q_begin = k_begin = 0 and Sq = Sk = S the two entries return the bits of svg_band_attention_lse[_f32] (perm = NULL).  No key row
 * outside [k_begin, k_begin + Sk) and no q row outside its window is read, nothing outside o / lse / o32 of the window is written.
 * Supported: head_dim 128, bf16 / fp16, plain q, the static mapping.  k_begin must be a multiple of 64 (key tiles stay aligned to the
 * mask's coordinates); q_begin, Sq and Sk are arbitrary.  There is NO head permutation: the tensors arrive in the logical order of the
 * mask — a window of a token-major head is not a window of physical rows.
 * Return codes, all decided on the host before any launch, in this order: a NULL q, k, v, o (o32), lse or mask: SVG_ERR_BAD_ARG; BH, S, Sq
 * or Sk <= 0, a negative begin or a window that ends behind S: SVG_ERR_BAD_ARG; the mask against S as in svg_band_attention, then the
 * layout as in svg_band_attention_strided (against Sq and Sk); then SVG_ERR_UNSUPPORTED for D != 128, k_begin % 64 != 0, the size limits of
 * svg_band_attention on (BH, S, D), an o32 that is not 16-byte aligned, a dtype other than bf16 / fp16. */
int svg_band_window_attention_lse(const void* q, const void* k, const void* v, void* o, float* lse, int32_t BH, int32_t S, int32_t q_begin,
                                  int32_t Sq, int32_t k_begin, int32_t Sk, int32_t D, int32_t dtype, float sm_scale,
                                  const svg_band_mask_t* mask, const svg_attn_layout_t* layout /* NULL: contiguous */, void* stream);
int svg_band_window_attention_lse_f32(const void* q, const void* k, const void* v, float* o32, float* lse, int32_t BH, int32_t S,
                                      int32_t q_begin, int32_t Sq, int32_t k_begin, int32_t Sk, int32_t D, int32_t dtype, float sm_scale,
                                      const svg_band_mask_t* mask, const svg_attn_layout_t* layout /* NULL: contiguous */, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* SVG_ATTN_BAND_WINDOW_H_ */

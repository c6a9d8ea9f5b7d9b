/* Band (SVG1) attention of a FRAME SHARD of the rows over a FRAME SHARD of the keys: part of the C ABI of libsvgattn (include/svg_attn.h
 * includes this file at its end; the types, error codes and conventions are the ones documented there, SVG_ABI_VERSION is unchanged).  A
 * header of its own for the reason include/svg_attn_sparse_lse.h gives; the validation table of these entries is
 * tests/test_band_shard_cpu.py, and svg/_native.py binds them from BAND_SHARD_SIGNATURES. */
#ifndef SVG_ATTN_BAND_SHARD_H_
#define SVG_ATTN_BAND_SHARD_H_
#include "svg_attn.h"

#ifdef __cplusplus
extern "C" {
#endif

/* A shard of a sequence of S rows whose video is F = perm->num_frame frames of P = perm->frame_size rows from row perm->vid0 on, stored
 * frame-major: the rows of the whole frames [f0, f0 + n_frames) — sequence row vid0 + f * P + p at shard row (f - f0) * P + p — and behind
 * them a tail, the sequence rows [tail_begin, tail_begin + n_tail) behind the video (text, padding); n_tail = 0: no tail, tail_begin is
 * not read.  P * n_frames + n_tail rows in all. */
typedef struct svg_band_shard {
    int32_t f0, n_frames;
    int32_t tail_begin, n_tail;
} svg_band_shard_t;

/* svg_band_attention_lse / svg_band_attention_lse_f32 for a caller that holds whole frames of the rows and whole frames of the keys — a
 * rank of a sequence sharded by frames that has received a peer's key shard — with both kinds of head in one launch:
 *   q, o   the rows of q_shard: [BH, Sq, D] (or the layout's strides), Sq = P * q_shard->n_frames + q_shard->n_tail;
 *   k, v   the rows of k_shard: [BH, Sk, D] (or the layout's strides);
 *   perm   never NULL: vid0, num_frame, frame_size describe the video of the WHOLE sequence; head_perm_flag (device, int64 per head, read
 *          by the kernel as svg_band_attention reads it) marks the token-major heads, NULL: every head in logical order;
 *   mask   over the S rows of the whole sequence, in the logical order of each head: for a head in logical order shard row l is mask row
 *          g(l) = vid0 + f0 * P + l; for a token-major head the shard's video rows are taken in the order l = p * n_frames + fl (read from
 *          shard row fl * P + p: the fused placement of svg_band_attention on a video of n_frames frames) and are mask row
 *          g(l) = vid0 + p * F + f0 + fl; a tail row is mask row tail_begin + its index in the tail for both.  Row lq of the q shard sees
 *          row lk of the k shard exactly where the mask allows (g_q(lq), g_k(lk)); o, lse and o32 are written at the shard row q was read from;
 *   lse    CONTIGUOUS fp32 [BH, Sq]: natural log of sum_j exp(sm_scale * q . k_j) over the keys of the k shard the row may see; a row that
 *          sees none has lse = -inf and o = 0 (o32 = 0).  The parts of one q shard over k shards that cover the sequence merge
 *          (svg_merge_attention_states[_f32]) to the q shard's rows of svg_band_attention_lse on the whole sequence;
 *   o32    (the _f32 form, in the place of o; no 16-bit o is written) CONTIGUOUS fp32 [BH, Sq, 128], 16-byte aligned; rounded to nearest
 *          even the o of the _lse form bit for bit.  Of a layout the o member is not read;
 *   layout NULL: contiguous tensors; otherwise as in svg_band_attention_strided, with Sq rows of q / o and Sk rows of k / v.
 * With vid0 = 0, both shards {0, F, F * P, S - F * P} the two entries return the bits of svg_band_attention_lse[_f32] with the same perm.
 * Key tiles lie on the k shard's own grid: no begin needs an alignment.  No row outside the two shards is read, nothing outside o / lse /
 * o32 of the q shard is written.  Rows in FRONT of the video (vid0 > 0) belong to no shard.
 * Supported: head_dim 128, bf16 / fp16, plain q, the static mapping.
 * Return codes, all decided on the host before any launch, in this order: a NULL q, k, v, o (o32), lse, mask, perm, q_shard or k_shard:
 * SVG_ERR_BAD_ARG; BH or S <= 0, num_frame or frame_size <= 0, vid0 < 0 or a video that ends behind S: SVG_ERR_BAD_ARG; for the q shard,
 * then the k shard: frames outside [0, F) (f0 < 0, n_frames < 0, f0 + n_frames > F), n_tail < 0, a tail outside [vid0 + F * P, S), an empty
 * shard: SVG_ERR_BAD_ARG; then what every band entry checks, where it checks it: the mask against S (SVG_ERR_BAD_ARG) and the size limits of
 * svg_band_attention on (BH, S, D) (SVG_ERR_UNSUPPORTED), the layout as in svg_band_attention_strided, against Sq and Sk; then
 * SVG_ERR_UNSUPPORTED for D != 128, an o32 that is not 16-byte aligned, a dtype other than bf16 / fp16. */
int svg_band_shard_attention_lse(const void* q, const void* k, const void* v, void* o, float* lse, int32_t BH, int32_t S, int32_t D,
                                 int32_t dtype, float sm_scale, const svg_band_mask_t* mask, const svg_perm_desc_t* perm,
                                 const svg_band_shard_t* q_shard, const svg_band_shard_t* k_shard,
                                 const svg_attn_layout_t* layout /* NULL: contiguous */, void* stream);
int svg_band_shard_attention_lse_f32(const void* q, const void* k, const void* v, float* o32, float* lse, int32_t BH, int32_t S, int32_t D,
                                     int32_t dtype, float sm_scale, const svg_band_mask_t* mask, const svg_perm_desc_t* perm,
                                     const svg_band_shard_t* q_shard, const svg_band_shard_t* k_shard,
                                     const svg_attn_layout_t* layout /* NULL: contiguous */, void* stream);

/* The coordinate maps the kernels use, evaluated on the host (no GPU): for a shard of the geometry of `perm` (head_perm_flag is not read)
 * and a head kind (token_major != 0), g_out[i] = g(x[i]) — x a shard index — and ginv_out[i] = the smallest shard index l with g(l) >= x[i]
 * — x a mask coordinate; the shard's row count where there is none.  Either output may be NULL.  Returns n, or -1 for arguments the
 * entries above refuse. */
int32_t svg_debug_band_shard_map(const svg_perm_desc_t* perm, int32_t S, const svg_band_shard_t* shard, int32_t token_major, const int32_t* x,
                                 int32_t n, int32_t* g_out, int32_t* ginv_out);

#ifdef __cplusplus
}
#endif
#endif /* SVG_ATTN_BAND_SHARD_H_ */

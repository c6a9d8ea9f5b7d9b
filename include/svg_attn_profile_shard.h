/* The online profiler (svg_sample_mse) of a sequence that lives sharded by whole frames: a partial per key shard and a combine over the
 * partials.  Part of the C ABI of libsvgattn (include/svg_attn.h includes this file at its end; the types, error codes and conventions are
 * the ones documented there, SVG_ABI_VERSION is unchanged).  A header of its own for the reason include/svg_attn_sparse_lse.h gives; the
 * validation table of these entries is tests/test_profile_shard_cpu.py, and svg/_native.py binds them from PROFILE_SHARD_SIGNATURES.
 *
 * svg_sample_mse is split-KV inside one GPU: un-normalised (O, m, l) per (output, head, KV chunk, sampled row), merged by a combine.  A key
 * shard (svg_band_shard_t, include/svg_attn_band_shard.h) is a set of chunks that lives on another GPU: every rank streams its own K / V
 * once (svg_sample_mse_shard_partial), one partial per rank travels, and every rank merges the same list in the same order
 * (svg_sample_mse_from_parts) to the same bits. */
#ifndef SVG_ATTN_PROFILE_SHARD_H_
#define SVG_ATTN_PROFILE_SHARD_H_
#include "svg_attn.h"
#include "svg_attn_band_shard.h"

#ifdef __cplusplus
extern "C" {
#endif

/* The partial of R sampled rows over the keys of ONE shard.
 *   q_rows    CONTIGUOUS [BH, R, D]: row i of a head is sequence row rows[i] of q (the caller has gathered them);
 *   rows      device int64 [R]: the GLOBAL row indices, used for the mask coordinates and for the rank order of the rows exactly as
 *             svg_sample_mse uses them;
 *   k, v      the Sk = P * k_shard->n_frames + k_shard->n_tail rows of k_shard: [BH, Sk, D], or the layout's k / v strides with Sk rows (the q
 *             and o members of the layout are not read).  prof->vid0 must be 0: rows in front of the video belong to no shard;
 *   S         rows of the WHOLE sequence; prof as for svg_sample_mse on the whole sequence;
 *   part      CONTIGUOUS fp32 [3, BH, R, D + 4], all of it written.  Output 0 is golden, 1 and 2 are under variant[0] and variant[1].  The
 *             row index is the position in the kernel's rank order — by coordinate under variant[1], ties broken by index: a function of
 *             `rows` alone, the same on every rank.  Columns [0, D): the un-normalised O; column D: m, the reference in the log2 domain as the
 *             kernel keeps it (the golden rows' maximum over this shard, for all three outputs); column D + 1: l; columns D + 2, D + 3: 0.  A
 *             row that sees no key of this shard under an output has l = 0 and O = 0 there (and a finite m).  The shard's KV chunks are
 *             reduced to ONE triple per (output, head, row): the size does not depend on the chunking;
 *   workspace svg_sample_mse_shard_workspace_bytes(BH, R, D, Sk);
 *   skip_flag NULL, or a device flag: skip_flag[0] != 0 -> every kernel returns at once and `part` is untouched.
 * Key tiles lie on the shard's own grid; no row outside the shard is read.  A shard whose frames do not end at F may still carry a tail (the
 * stored index then jumps inside one tile).
 * Supported: bf16, head_dim 128 (the second form of the kernel; the first one keeps a running maximum per output and has no shard form).
 * Return codes, all decided on the host before any launch, in this order:
 *   1. a NULL q_rows, k, v, rows, prof, k_shard, part or workspace: SVG_ERR_BAD_ARG;
 *   2. R, BH, S or D <= 0; prof->num_frame or frame_size <= 0, vid0 < 0 or a video that ends behind S: SVG_ERR_BAD_ARG;
 *   3. the shard, as the band shard entries check it (frames outside [0, F), n_tail < 0, a tail outside [vid0 + F * P, S), an empty shard):
 *      SVG_ERR_BAD_ARG;
 *   4. vid0 != 0: SVG_ERR_BAD_ARG;
 *   5. R > 64: SVG_ERR_UNSUPPORTED;
 *   6. frame_size < 64 with a token-major variant: SVG_ERR_UNSUPPORTED;
 *   7. S >= 2^24: SVG_ERR_UNSUPPORTED;
 *   8. workspace_bytes too small: SVG_ERR_WORKSPACE;
 *   9. the layout, as in svg_sample_mse_strided, against Sk rows (k and v members only);
 *  10. a dtype other than bf16 or D != 128: SVG_ERR_UNSUPPORTED. */
size_t svg_sample_mse_shard_workspace_bytes(int32_t BH, int32_t R, int32_t D, int32_t Sk);
int svg_sample_mse_shard_partial(const void* q_rows, const void* k, const void* v, const int64_t* rows, int32_t R, int32_t BH, int32_t S,
                                 int32_t D, int32_t dtype, float sm_scale, const svg_profile_desc_t* prof, const svg_band_shard_t* k_shard,
                                 float* part, void* workspace, size_t workspace_bytes, const int32_t* skip_flag /* or NULL */,
                                 const svg_attn_layout_t* layout /* k, v only; NULL: contiguous */, void* stream);

/* out_mse [2, BH] (device fp32) from the partials of shards that cover the keys: `parts` is a HOST array of n_parts device pointers, each a
 * `part` of svg_sample_mse_shard_partial for the same rows, 1 <= n_parts <= 64.  The parts are merged in list order with the arithmetic of
 * svg_sample_mse's own combine — weights 2^(m_c - M), NaN where the merged l is 0, the roundings of emulate_bf16 — so that ONE part made
 * from the shard {0, F, F * P, S - F * P} with q_rows = q[:, rows] gives the bits of svg_sample_mse on the same tensors.  A part with
 * O = 0, m = -inf, l = 0 (a rank without rows) changes nothing.  workspace: svg_sample_mse_from_parts_workspace_bytes(BH).  skip_flag as
 * above (out_mse untouched).
 * Return codes, on the host before any launch, in this order: a NULL parts, out_mse or workspace: SVG_ERR_BAD_ARG; n_parts outside
 * [1, 64], R, BH or D <= 0, a NULL parts[i]: SVG_ERR_BAD_ARG; R > 64: SVG_ERR_UNSUPPORTED; workspace_bytes too small: SVG_ERR_WORKSPACE; a
 * dtype other than bf16 or D != 128: SVG_ERR_UNSUPPORTED. */
size_t svg_sample_mse_from_parts_workspace_bytes(int32_t BH);
int svg_sample_mse_from_parts(const float* const* parts, int32_t n_parts, int32_t R, int32_t BH, int32_t D, int32_t dtype,
                              int32_t emulate_bf16, float* out_mse, void* workspace, size_t workspace_bytes,
                              const int32_t* skip_flag /* or NULL */, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* SVG_ATTN_PROFILE_SHARD_H_ */

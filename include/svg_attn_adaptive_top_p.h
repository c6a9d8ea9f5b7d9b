/* SVG2's top-p per head, on the device, steered by measured kept mass: the block map from a device vector of thresholds, the K-only half of
 * the quality probe, and the controller step.  Part of the C ABI of libsvgattn (include/svg_attn.h includes this file at its end; the types,
 * error codes and conventions are the ones documented there, SVG_ABI_VERSION is unchanged).  A header of its own for the reason
 * include/svg_attn_sparse_lse.h gives; the validation tables of these entries are tests/test_adaptive_top_p_cpu.py, and svg/_native.py binds
 * them from ADAPTIVE_TOP_P_SIGNATURES (allocating wrappers: svg/kmeans_utils.py identify_dynamic_map, svg/_probe.py sample_dense_lse;
 * the loop: svg/models/_core.py AdaptiveTopP, TopPStore, svg2_sparse_attention(adaptive=...)).
 *
 * A layer keeps one top_p per head in device memory.  A sparse layer-call builds its block map from it, runs its LSE form, probes R
 * sampled rows densely (K only), and steps every head's top_p towards the kept mass the user asked for; nothing is read back. */
#ifndef SVG_ATTN_ADAPTIVE_TOP_P_H_
#define SVG_ATTN_ADAPTIVE_TOP_P_H_
#include "svg_attn.h"
#include "svg_attn_sample_rows.h"

#ifdef __cplusplus
extern "C" {
#endif

/* svg_identify_dynamic_map with one top_p per head: top_p is a DEVICE fp32 [BH].  Head h gets exactly the map svg_identify_dynamic_map
 * gives it with the scalar top_p[h] — the same kernels (both forms: 256 < KC <= 1024 and the rest) read top_p[h] where they read the
 * scalar, and round it to the input dtype before the compares as they round the scalar.
 * A NaN entry keeps EVERY block of that head: a position is dropped when the cumulative sum in front of it compares greater than top_p,
 * and every compare with a NaN is false.
 * Return codes, on the host before any launch, in the order of svg_identify_dynamic_map: a NULL qc, kc, k_sizes, out_map or top_p, or
 * BH, QC or KC <= 0: SVG_ERR_BAD_ARG; KC > 4096: SVG_ERR_UNSUPPORTED; a head_dim other than 64 / 128 or a dtype other than bf16 / fp16:
 * SVG_ERR_UNSUPPORTED. */
int svg_identify_dynamic_map_per_head(const void* qc, const void* kc, const int32_t* k_sizes, uint8_t* out_map, int32_t BH, int32_t QC,
                                      int32_t KC, int32_t D, int32_t dtype, const float* top_p /* device [BH] */,
                                      int32_t preserve_length, void* stream);

/* The K-only half of svg_sample_dense_rows: lse [BH, R] alone, with the bits svg_sample_dense_rows writes to its lse on the same call.  V is
 * not an argument and nothing of it is read: the pass streams K once.  q, k, rows, valid_len, layout (its q and k members; v and o are
 * ignored) and the rules of the workspace are those of svg_sample_dense_rows; the tile and chunk partition, the running maximum, the row
 * sum and the merge of the chunks in chunk order are its own, so a permutation of `rows` permutes lse bit for bit.  A row outside [0, S) is
 * the CALLER's fault, as there.
 *   workspace svg_sample_dense_lse_workspace_bytes(BH, R, S) bytes, 16-byte aligned.
 * Every word of lse is written; nothing else is written outside the workspace.
 * Return codes, all decided on the host before any launch, in this order: a NULL q, k, rows, lse or workspace, R outside [1, 64], BH or
 * S <= 0: SVG_ERR_BAD_ARG; S >= 2^24 or S * D * 2 >= 2^32: SVG_ERR_UNSUPPORTED; a short workspace: SVG_ERR_WORKSPACE (a misaligned one:
 * SVG_ERR_UNSUPPORTED); the layout: as in svg_sample_mse_strided; a head_dim other than 64 / 128 or a dtype other than bf16 / fp16:
 * SVG_ERR_UNSUPPORTED. */
size_t svg_sample_dense_lse_workspace_bytes(int32_t BH, int32_t R, int32_t S);
int svg_sample_dense_lse(const void* q, const void* k, const int64_t* rows, int32_t R, int32_t BH, int32_t S, int32_t D, int32_t dtype,
                         float sm_scale, int32_t valid_len, float* lse /* [BH, R] */, void* workspace, size_t workspace_bytes,
                         const svg_attn_layout_t* layout /* NULL: contiguous; q, k only */, void* stream);

/* The controller: one launch, one wave per head — gather the sparse call's lse at the sampled rows, reduce to the kept mass, step top_p.
 *   lse_sparse fp32 [BH, S]: the row log-sum-exp of the sparse call, in the caller's row order;
 *   rows       device int64 [R], 1 <= R <= 64: the sampled rows (duplicates allowed).  A row outside [0, S) is not read: it makes the
 *              head's kept mass NaN, and the head's top_p stays;
 *   lse_dense  fp32 [BH, R]: svg_sample_dense_lse / svg_sample_dense_rows on the same rows;
 *   kept       fp32 [BH], every word written;  top_p fp32 [BH], updated in place.
 *     kept[h]  = (1 / R) sum_i exp(lse_sparse[h, rows[i]] - lse_dense[h, i])        a -inf in lse_sparse counts 0
 *     e        = target - kept[h]
 *     step     = e > 0 ? gain_up * e : (e < -band ? gain_down * (e + band) : 0)
 *     top_p[h] = min(max(top_p[h] + step, p_min), p_max)                            kept[h] not finite: top_p[h] unchanged
 * The differences, the exponentials and the sum are fp64 and kept is rounded once to fp32, so it does not depend on a summation order;
 * e, the step and the clamp are plain fp32, every product and sum rounded (no contraction).
 * SVG_ERR_BAD_ARG, on the host before any launch, for: a NULL pointer; R outside [1, 64]; BH or S <= 0; a negative or NaN gain_up,
 * gain_down or band; anything but 0 <= p_min <= p_max <= 1 (NaN included).  target is not checked: a target no head reaches drives
 * every top_p to p_max, a NaN target moves nothing. */
int svg_top_p_update(const float* lse_sparse, const int64_t* rows, const float* lse_dense, int32_t R, int32_t BH, int32_t S, float target,
                     float gain_up, float gain_down, float band, float p_min, float p_max, float* kept /* [BH] */,
                     float* top_p /* [BH], in place */, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* SVG_ATTN_ADAPTIVE_TOP_P_H_ */

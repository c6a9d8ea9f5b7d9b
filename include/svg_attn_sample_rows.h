/* Quality probe: dense attention of a few sampled query rows, fp32 rows and row log-sum-exp: part of the C ABI of libsvgattn
 * (include/svg_attn.h includes this file at its end; the types, error codes and conventions are the ones documented there, SVG_ABI_VERSION
 * is unchanged).  It lives in a header of its own for the reason include/svg_attn_sparse_lse.h gives: the tests of svg_attn.h pin their
 * tables to its prototypes; the table of this entry is tests/test_sample_rows_cpu.py, and svg/_native.py binds it from
 * SAMPLE_ROWS_SIGNATURES (the allocating wrapper is svg/_probe.py sample_dense_rows). */
#ifndef SVG_ATTN_SAMPLE_ROWS_H_
#define SVG_ATTN_SAMPLE_ROWS_H_
#include "svg_attn.h"

#ifdef __cplusplus
extern "C" {
#endif

/* What a sparse layer-call cost in accuracy: every default head_dim-128 sparse form returns a row log-sum-exp (svg_band_attention_lse,
 * svg_varblock_attention_lse, ...); this entry gives the dense truth on R sampled rows of every head, streamed in one pass over K and V
 * (each read once per call).  Then for any sparse form
 *     kept mass of a row = exp(lse_sparse[row] - lse[row])        the share of the dense softmax row the sparse form kept
 *     output error       = o_sparse[row] - o32[row]
 * (svg/models/_core.py sparse_quality).
 *   q, k, v   [BH, S, D] bf16 / fp16, head_dim 64 or 128.  layout NULL: contiguous; otherwise the token-major views of
 *             svg_sample_mse_strided (svg_attn_layout_t; v read where to_v wrote it; layout->o is ignored: there is no 16-bit output).
 *   rows      device int64 [R], 1 <= R <= 64: the sampled query rows.  Duplicates are allowed, the order is kept: output row i belongs to
 *             rows[i].  A row outside [0, S) cannot be checked on the host and is the CALLER's fault (q is read at that row); the Python
 *             wrapper checks the rows on the CPU tensor before the upload.
 *   valid_len the two-segment rule of dense attention on a padded sequence: valid_len <= 0 or >= S: every row sees all S keys; otherwise a
 *             row < valid_len sees the keys [0, valid_len) and a row >= valid_len sees [valid_len, S).
 *   lse       fp32 [BH, R]: lse[h][i] = log sum_j exp(sm_scale * q[rows[i]] . k[j]) over the keys the row sees; natural logarithm, the
 *             convention of svg_band_attention_lse.
 *   o32       fp32 [BH, R, D]: the normalised output row, NOT rounded to 16 bits.
 *   Every word of o32 and lse is written; nothing else is written outside the workspace.
 *   workspace svg_sample_dense_rows_workspace_bytes(BH, R, D, S) bytes, 16-byte aligned: the split-KV partials.  The chunks of a row are
 *             merged in chunk order: the results do not depend on timing, and a permutation of `rows` permutes them bit for bit.
 * Return codes, all decided on the host before any launch, in this order: a NULL pointer, R outside [1, 64], BH or S <= 0:
 * SVG_ERR_BAD_ARG; S >= 2^24 or S * D * 2 >= 2^32 (the limits of svg_sample_mse): SVG_ERR_UNSUPPORTED; a short workspace:
 * SVG_ERR_WORKSPACE (a misaligned one: SVG_ERR_UNSUPPORTED); the layout: as in svg_sample_mse_strided; a head_dim other than 64 / 128 or a
 * dtype other than bf16 / fp16: SVG_ERR_UNSUPPORTED. */
size_t svg_sample_dense_rows_workspace_bytes(int32_t BH, int32_t R, int32_t D, int32_t S);
int svg_sample_dense_rows(const void* q, const void* k, const void* v, const int64_t* rows, int32_t R, int32_t BH, int32_t S, int32_t D,
                          int32_t dtype, float sm_scale, int32_t valid_len, float* o32 /* [BH, R, D] */, float* lse /* [BH, R] */,
                          void* workspace, size_t workspace_bytes, const svg_attn_layout_t* layout /* NULL: contiguous; o not read */,
                          void* stream);

#ifdef __cplusplus
}
#endif
#endif /* SVG_ATTN_SAMPLE_ROWS_H_ */

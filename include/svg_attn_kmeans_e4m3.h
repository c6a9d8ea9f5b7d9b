/* flash-kmeans with an e4m3 assignment: the scores of svg_kmeans_assign on v_mfma_scale_f32_32x32x64_f8f6f4 (twice the 16-bit matrix rate
 * on gfx950), and a Lloyd loop whose first iterations assign with it while its last ones are the 16-bit assignment of
 * svg_kmeans_loop_grouped_strided.  Part of the C ABI of libsvgattn (include/svg_attn.h includes this file; the types, error codes and
 * conventions are the ones documented there, SVG_ABI_VERSION is unchanged).  A header of its own for the reason
 * include/svg_attn_sparse_lse.h gives; the validation table of these entries is tests/test_kmeans_e4m3_cpu.py, their float64 statement
 * tests/kmeans_e4m3_cases.py, and svg/_native.py binds them from KMEANS_E4M3_SIGNATURES (wrappers: kmeans_centre, kmeans_assign_e4m3,
 * kmeans_loop_e4m3; the caller: svg/kmeans_utils.py batch_kmeans_Euclid(fp8_iters=...)).  Kernels: csrc/kmeans.hip.
 *
 * Arithmetic, per batch (a batch is one head).  mu float [128] is a centre: |x - c|^2 does not depend on it, so any mu is admissible; it
 * keeps offsets common to all rows out of e4m3's 3-bit mantissa.  A row r is x_n - mu or c_k - mu, the differences taken in fp32.
 *     e    = floor(log2(448 / max_d |r_d|)), 0 for a zero row, at most 127 (a row maximum below 2^-118)
 *     q(r) = e4m3_rne(r_d 2^e)       OCP e4m3fn; by the choice of e it never saturates; the row stands for q(r) 2^-e
 *     s_k  = fp32 sum_d q(x - mu)_d q(c_k - mu)_d 2^-(e_x + e_k) - csq'_k / 2,   csq'_k = the fp32 sum of squares of the UNquantised c_k - mu
 * (the exponents travel as the instruction's E8M0 block scales; the accumulators start at -csq'_k / 2).  label = the lowest index of the
 * maximum of s_k.  A score error moves a point only between centroids that are almost equally near; the centroid update stays the exact
 * fp32 mean of 16-bit rows (svg_kmeans_update).
 *
 * Only head_dim 128, K <= 8192 and bf16 / fp16 are covered: anything else is SVG_ERR_UNSUPPORTED (there is no head_dim 64 form).
 *
 * Return codes: everything is decided on the host before any launch, in this order:
 *   1. a NULL pointer (mu of svg_kmeans_assign_e4m3 may be NULL: zeros); then a non-positive B, N, K, max_iters, a group <= 0 or not
 *      dividing B, fp8_iters outside [0, max_iters] (those the entry has):                                               SVG_ERR_BAD_ARG
 *   2. K > 8192, a D other than 128, a dtype other than bf16 / fp16:                                                     SVG_ERR_UNSUPPORTED
 *   3. a short workspace:                                                                                                 SVG_ERR_WORKSPACE
 *   4. loop: two of c_init, c_work_a, c_work_b the same buffer, or centroids_out one of the work buffers:                SVG_ERR_BAD_ARG
 *   5. loop: the stride checks of svg_kmeans_loop_strided with its codes — x_batch_stride < N * D: SVG_ERR_BAD_ARG; x_batch_stride not a
 *      multiple of 8 or x not 16-byte aligned: SVG_ERR_UNSUPPORTED.  assign: x or mu not 16-byte aligned: SVG_ERR_UNSUPPORTED. */
#ifndef SVG_ATTN_KMEANS_E4M3_H_
#define SVG_ATTN_KMEANS_E4M3_H_
#include "svg_attn.h"

#ifdef __cplusplus
extern "C" {
#endif

/* mu[b][d] = the fp32 mean over k of centroids[b][k][d].  centroids [B, K, 128] bf16 / fp16, mu float [B, 128]: every word is written. */
int svg_kmeans_centre(const void* centroids, float* mu, int32_t B, int32_t K, int32_t D, int32_t dtype, void* stream);

/* 0 for what the entry refuses. */
size_t svg_kmeans_assign_e4m3_workspace_bytes(int32_t B, int32_t N, int32_t K, int32_t D);

/* labels[b][n] = arg-max_k s_k of the statement above (lowest index on ties).  x [B, N, 128] and centroids [B, K, 128] contiguous, of one
 * dtype; mu float [B, 128] or NULL; labels int32 [B, N]: every word is written. */
int svg_kmeans_assign_e4m3(const void* x, const void* centroids, const float* mu, int32_t* labels, int32_t B, int32_t N, int32_t K, int32_t D,
                           int32_t dtype, void* workspace, size_t workspace_bytes, void* stream);

/* 0 for what the entry refuses. */
size_t svg_kmeans_loop_e4m3_workspace_bytes(int32_t B, int32_t N, int32_t K, int32_t D, int32_t group);

/* svg_kmeans_loop_grouped_strided (its arguments, their meaning and its results) whose iterations it < fp8_iters assign with the e4m3
 * scores; mu is computed once per call, the channel mean of c_init's K centroids (svg_kmeans_centre).  Every iteration runs the update,
 * sort and commit of that loop.  An e4m3 iteration never stops a group: its shift is not compared with tol.  From iteration fp8_iters
 * on, the rule of svg_kmeans_loop_grouped_strided holds unchanged (a converged group returns the centroids before its last update; a
 * NaN shift never converges).  With fp8_iters < max_iters the returned labels are therefore the 16-bit arg-max against the centroids
 * that entered the last iteration; with fp8_iters = 0 the call IS svg_kmeans_loop_grouped_strided, bit for bit. */
int svg_kmeans_loop_e4m3(const void* x, int64_t x_batch_stride, const void* c_init, void* c_work_a, void* c_work_b, int32_t* labels,
                         int32_t* counts, int32_t* sorted_idx, void* centroids_out, int32_t* n_iters, int32_t B, int32_t N, int32_t K,
                         int32_t D, int32_t dtype, int32_t group, int32_t max_iters, float tol, int32_t fp8_iters, void* workspace,
                         size_t workspace_bytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* SVG_ATTN_KMEANS_E4M3_H_ */

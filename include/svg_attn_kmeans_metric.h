/* flash-kmeans by direction: the cosine and the dot-product metric of the reference's batch_kmeans_Cosine / batch_kmeans_Dot
 * (svg/kmeans_utils.py:740-822) on the kernels and the device loop of the Euclidean family.  Part of the C ABI of libsvgattn
 * (include/svg_attn.h includes this file; the types, error codes and conventions are the ones documented there, SVG_ABI_VERSION is
 * unchanged).  A header of its own for the reason include/svg_attn_sparse_lse.h gives; the validation table of these entries is
 * tests/test_kmeans_metric_cpu.py, their float64 statement tests/test_gpu_kmeans_metric.py, and svg/_native.py binds them from
 * KMEANS_METRIC_ENTRIES (wrappers: svg/_kmeans_metric.py; the callers: svg/kmeans_metric.py batch_kmeans_Cosine, batch_kmeans_Dot,
 * triton_centroid_update_cosine, triton_centroid_update_sorted_cosine).  Kernels: csrc/kmeans.hip (assignment, loop) and
 * csrc/kmeans_metric.hip (update, initial normalisation).
 *
 * metric: SVG_KMEANS_COSINE or SVG_KMEANS_DOT.  0 (Euclid) is refused here: that metric keeps its own entries (svg_kmeans_*).
 *
 * Arithmetic, per batch (a batch is one head).
 *   assign:  labels[n] = arg-max_k <x_n, c_k>, fp32 accumulation on the matrix units, the lowest index on ties; centroids at or behind K
 *            never win.  Both metrics read the RAW x: scaling a row by 1 / |x_n| does not change its arg-max, so the cosine metric never
 *            materialises the reference's F.normalize(x).  A row whose scores are all equal (|x_n| = 0) gets label 0.
 *   update:  s_k = the sum over the rows of cluster k, in the order of the stable sort of the labels, of w_n x_n,
 *                cosine: w_n = 1 / max(|x_n|, 1e-12), |x_n| the fp32 norm of the row;   dot: w_n = 1
 *            m_k = s_k / count_k, or centroids_in[k] where count_k = 0, rounded to the tensor dtype;
 *            centroids_out[k] = m_k / max(|m_k|, 1e-12), rounded once.
 *            Every sum, norm and division is IEEE fp32 in a fixed order: the results are bit-reproducible (the reference's atomics are
 *            not).  The cosine metric adds fl(w_n x_n) in fp32 and never rounds a normalised row to 16 bits as the reference's x_norm is
 *            rounded: a deliberate departure from the reference's bits.
 *            shift[b] = max_k |centroids_out[k] - centroids_in[k]| with the differences rounded to the dtype, as svg_kmeans_update forms
 *            it; a NaN shift is kept (the canonical NaN).
 *   loop:    the Lloyd loop of svg_kmeans_loop_grouped_strided under the reference's stopping rule, with the two halves above.  The
 *            cosine metric first normalises c_init (c / max(|c|, 1e-12), rounded once) into the workspace — c_init is never written — and
 *            a group that converges in its first iteration returns those normalised rows; the dot metric uses c_init as given.
 *
 * D 64 / 128, bf16 / fp16, K <= 8192, as the Euclidean entries.
 *
 * Return codes: everything is decided on the host before any launch, in this order:
 *   1. a NULL pointer; then a non-positive B, N, K, max_iters, a group <= 0 or not dividing B, a metric outside
 *      {SVG_KMEANS_COSINE, SVG_KMEANS_DOT} (those the entry has):                                                        SVG_ERR_BAD_ARG
 *   2. K > 8192, a D other than 64 / 128, a dtype other than bf16 / fp16:                                                SVG_ERR_UNSUPPORTED
 *   3. a short workspace:                                                                                                 SVG_ERR_WORKSPACE
 *   4. loop: two of c_init, c_work_a, c_work_b the same buffer, or centroids_out one of the work buffers:                SVG_ERR_BAD_ARG
 *   5. loop: the stride checks of svg_kmeans_loop_strided with its codes — x_batch_stride < N * D: SVG_ERR_BAD_ARG; x_batch_stride not a
 *      multiple of 8 or x not 16-byte aligned: SVG_ERR_UNSUPPORTED. */
#ifndef SVG_ATTN_KMEANS_METRIC_H_
#define SVG_ATTN_KMEANS_METRIC_H_
#include "svg_attn.h"

#define SVG_KMEANS_EUCLID 0   /* refused by the entries of this header */
#define SVG_KMEANS_COSINE 1
#define SVG_KMEANS_DOT 2

#ifdef __cplusplus
extern "C" {
#endif

/* labels[b][n] = arg-max_k <x[b][n], centroids[b][k]> (the same for both metrics).  x [B, N, D], centroids [B, K, D] contiguous, of one
 * dtype; labels int32 [B, N]: every word is written.  workspace: svg_kmeans_workspace_bytes(B, N, K, D) (it is not written). */
int svg_kmeans_assign_metric(const void* x, const void* centroids, int32_t* labels, int32_t B, int32_t N, int32_t K, int32_t D, int32_t dtype,
                             int32_t metric, void* workspace, size_t workspace_bytes, void* stream);

/* The update on GIVEN labels (int32 [B, N], every one in [0, K)): counts int32 [B, K], sorted_idx int32 [B, N] (the stable argsort of the
 * labels), centroids_out [B, K, D] and shift float [B] of the statement above; every word of the four is written.  With
 * SVG_KMEANS_DOT the rows are summed as they are: a caller that hands in rows it has normalised itself gets the reference's
 * triton_centroid_update_cosine.  workspace: svg_kmeans_workspace_bytes(B, N, K, D). */
int svg_kmeans_update_metric(const void* x, const int32_t* labels, const void* centroids_in, void* centroids_out, int32_t* counts,
                             int32_t* sorted_idx, float* shift, int32_t B, int32_t N, int32_t K, int32_t D, int32_t dtype, int32_t metric,
                             void* workspace, size_t workspace_bytes, void* stream);

/* 0 for what svg_kmeans_loop_metric refuses by its sizes. */
size_t svg_kmeans_loop_metric_workspace_bytes(int32_t B, int32_t N, int32_t K, int32_t D, int32_t group);

/* svg_kmeans_loop_grouped_strided (its arguments, their meaning and its results: labels, counts, sorted_idx, centroids_out, n_iters int32
 * [B / group]) under `metric`.  x_batch_stride == N * D is the contiguous call, group == B one stopping rule over all batches.  A converged
 * group returns the centroids that entered its last iteration, unit rows from the first update on (cosine: from the start). */
int svg_kmeans_loop_metric(const void* x, int64_t x_batch_stride, const void* c_init, void* c_work_a, void* c_work_b, int32_t* labels,
                           int32_t* counts, int32_t* sorted_idx, void* centroids_out, int32_t* n_iters, int32_t B, int32_t N, int32_t K,
                           int32_t D, int32_t dtype, int32_t metric, int32_t group, int32_t max_iters, float tol, void* workspace,
                           size_t workspace_bytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* SVG_ATTN_KMEANS_METRIC_H_ */

/* The Lloyd loop of svg_kmeans_loop_grouped[_strided] in steps, with the stopping rule's group maxima handed out and taken back: the seam a
 * head-sharded caller needs for the collective that makes the rule a maximum over ALL heads.  Part of the C ABI of libsvgattn
 * (include/svg_attn.h includes this file; the types, error codes and conventions are the ones documented there, SVG_ABI_VERSION is
 * unchanged).  A header of its own for the reason include/svg_attn_sparse_lse.h gives; the validation table of these entries is
 * tests/test_kmeans_stepped_cpu.py, and svg/_native.py binds them from KMEANS_STEPPED_SIGNATURES (allocating wrapper:
 * svg/_kmeans_stepped.py KmeansSteppedSide; the driver: svg/kmeans_utils.py lloyd_stepped; the layer-call: svg/models/_core.py kmeans_clustering).
 *
 * svg_kmeans_loop* computes the group maxima inside its commit kernel, so nothing can sit between "maxima known" and "rule applied".  Here
 * the caller runs, ordered on the device (one stream, or events),
 *     iterate(0), commit(0), iterate(1), commit(1), ..., iterate(max_iters - 1), commit(max_iters - 1), finish
 * and may do anything to `maxima` between an iterate and its commit — an all-reduce(MAX) over ranks, a maximum with another loop's vector.
 * With `maxima` untouched, labels, counts, sorted indices, centroids and n_iters are bit for bit those of
 * svg_kmeans_loop_grouped[_strided] with the same max_iters and tol: the kernels are the same ones (csrc/kmeans.hip), launches only, no
 * host synchronisation, nothing on the device waits on anything.
 *
 * B batches of N rows, K clusters, head_dim D, G = B / group stopping groups of `group` consecutive batches (group = B: the rule of
 * svg_kmeans_loop).  x: batches x_batch_stride elements apart under the rules of svg_kmeans_loop_strided (rows of a batch contiguous;
 * x_batch_stride >= N * D, a multiple of 8, x 16-byte aligned).  c_init, c_work_a, c_work_b, centroids_out: [B, K, D] of x's dtype, pairwise
 * distinct; c_init is only read.  labels, sorted_idx int32 [B, N], counts int32 [B, K], n_iters int32 [G], maxima float [G]: device memory.
 * workspace: svg_kmeans_stepped_workspace_bytes(B, N, K, D, group) bytes, the same for all calls of one loop and kept between them; it
 * holds the iteration's scratch results and the state words (the state words lie in front, so that finish finds them without N).
 *
 * Return codes: everything is decided on the host before any launch, in this order:
 *   1. a NULL pointer; then a non-positive B, N, K (those the entry has), a group <= 0 or not dividing B, it < 0:       SVG_ERR_BAD_ARG
 *   2. K > 8192, a D other than 64 / 128, a dtype other than bf16 / fp16 (those the entry has):                         SVG_ERR_UNSUPPORTED
 *   3. a short workspace (finish, which has no N: shorter than the workspace of N = 1):                                  SVG_ERR_WORKSPACE
 *   4. two of c_init, c_work_a, c_work_b the same buffer, or centroids_out one of the work buffers:                      SVG_ERR_BAD_ARG
 *   5. iterate: the stride checks of svg_kmeans_loop_strided with its codes — x_batch_stride < N * D: SVG_ERR_BAD_ARG; x_batch_stride not a
 *      multiple of 8 or x not 16-byte aligned: SVG_ERR_UNSUPPORTED. */
#ifndef SVG_ATTN_KMEANS_STEPPED_H_
#define SVG_ATTN_KMEANS_STEPPED_H_
#include "svg_attn.h"

#ifdef __cplusplus
extern "C" {
#endif

/* 0 for what the entries refuse: a non-positive size, a group not dividing B, K > 8192, a D other than 64 / 128. */
size_t svg_kmeans_stepped_workspace_bytes(int32_t B, int32_t N, int32_t K, int32_t D, int32_t group);

/* One svg_kmeans_iter on x into the workspace's scratch.  The centroids rotate as in svg_kmeans_loop: it == 0 reads c_init and writes
 * c_work_a; an odd `it` reads c_work_a and writes c_work_b; an even it > 0 reads c_work_b and writes c_work_a.  it == 0 also clears the
 * state words.  maxima[g] = the maximum over the shifts of group g's batches, a NaN among them propagated as torch.max propagates it;
 * every word of maxima is written. */
int svg_kmeans_stepped_iterate(const void* x, int64_t x_batch_stride, const void* c_init, void* c_work_a, void* c_work_b, int32_t it,
                               float* maxima /* device [G], written */, int32_t B, int32_t N, int32_t K, int32_t D, int32_t dtype,
                               int32_t group, void* workspace, size_t workspace_bytes, void* stream);

/* The stopping rule of iteration `it` from maxima[g]: conv = !(m != m) && m < tol (a NaN never converges).  A group still running takes
 * the scratch labels, counts and sorted indices as its result; its n_iters, centroid selector and stopped flag are updated.  After
 * commit(0) every word of labels, counts and sorted_idx is written. */
int svg_kmeans_stepped_commit(const float* maxima /* device [G], read */, int32_t* labels, int32_t* counts, int32_t* sorted_idx, int32_t it,
                              float tol, int32_t B, int32_t N, int32_t K, int32_t group, void* workspace, size_t workspace_bytes,
                              void* stream);

/* Every group's centroids from the buffer its loop ended on (a converged group: the centroids BEFORE its last update, as the reference
 * returns them) and n_iters.  Every word of centroids_out and n_iters is written. */
int svg_kmeans_stepped_finish(const void* c_init, const void* c_work_a, const void* c_work_b, void* centroids_out,
                              int32_t* n_iters /* device [G] */, int32_t B, int32_t K, int32_t D, int32_t dtype, int32_t group,
                              void* workspace, size_t workspace_bytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* SVG_ATTN_KMEANS_STEPPED_H_ */

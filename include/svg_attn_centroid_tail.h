/* Centroid tail of SVG2: the key clusters a block map does NOT select, each standing in as ONE pseudo key — its mean key, its mean value,
 * its size as a weight — so that the mass the top-p map drops is estimated row by row instead of discarded.  Part of the C ABI of
 * libsvgattn (include/svg_attn.h includes this file; the types, error codes and conventions are the ones documented there,
 * SVG_ABI_VERSION is unchanged).  A header of its own for the reason include/svg_attn_sparse_lse.h gives; the validation table of these
 * entries is tests/test_centroid_tail_cpu.py, their float64 statement tests/centroid_tail_cases.py, and svg/_native.py binds them from
 * CENTROID_TAIL_ENTRIES (wrappers: svg/_centroid_tail.py cluster_means, centroid_tail_attention; the caller: svg/models/_core.py
 * svg2_sparse_attention(centroid_tail=True)).  Kernels: csrc/centroid_tail.hip.
 *
 * Statement.  For a query row i of block-row (query cluster) a, over the key clusters c < KC with block_map[a][c] == 0 and k_sizes[c] > 0:
 *     s_c = sm_scale * q_i . kbar_c + ln k_sizes[c]          lse_i = ln sum_c exp(s_c)          o_i = sum_c exp(s_c - lse_i) vbar_c
 * an attention state over at most KC keys with the additive bias ln n_c: k_sizes[c] copies of (kbar_c, vbar_c).  It is a PART for
 * svg_merge_attention_states beside the state svg_varblock_attention_lse returns under the same map.  With kbar_c the exact mean of the
 * cluster's keys, Jensen's inequality gives n_c exp(q . kbar_c) <= sum_{j in c} exp(q . k_j): the merged log-sum-exp lies between the
 * sparse and the dense one.  svg_cluster_means computes those means from the sorted indices and the counts of a k-means call.
 *
 * Return codes of svg_centroid_tail_attention_lse: everything is decided on the host before any launch, in this order:
 *   1. a NULL pointer (q_row_idx and layout may be NULL), a non-positive H, Sq, QB, KC:                                 SVG_ERR_BAD_ARG
 *   2. map_cols < KC:                                                                                                   SVG_ERR_BAD_ARG
 *   3. layout != NULL: the checks of svg_varblock_attention_strided on heads_per_batch and the q member, with its codes (a stride
 *      below D or negative, heads_per_batch <= 0 or not dividing H: SVG_ERR_BAD_ARG; a stride that is not a multiple of 8, a q that is
 *      not 16-byte aligned, a row stride of 2^23 or more: SVG_ERR_UNSUPPORTED); the k, v, o members are not read
 *   4. a short workspace:                                                                                                SVG_ERR_WORKSPACE
 *   5. a D other than 128, a dtype other than bf16 / fp16, KC > 4032 (the limit of the variable-block entries), Sq of 2^24 or more, H
 *      above 65535, a q, kbar, vbar, o or workspace that is not 16-byte aligned:                                         SVG_ERR_UNSUPPORTED
 * svg_cluster_means: a NULL pointer (strides may be NULL) or a non-positive B, N, K: SVG_ERR_BAD_ARG; strides != NULL with
 * heads_per_batch <= 0 or not dividing B, a row stride below D, a negative stride: SVG_ERR_BAD_ARG; a D other than 64 / 128 or a dtype
 * other than bf16 / fp16: SVG_ERR_UNSUPPORTED; a stride that is not a multiple of 8, x or means not 16-byte aligned: SVG_ERR_UNSUPPORTED. */
#ifndef SVG_ATTN_CENTROID_TAIL_H_
#define SVG_ATTN_CENTROID_TAIL_H_
#include "svg_attn.h"

#ifdef __cplusplus
extern "C" {
#endif

/* means[b][c][:] = the mean of the counts[b][c] rows of x that sorted_idx lists for cluster c of batch b (a batch is one head), summed in
 * sorted order in fp32 and rounded once to x's dtype; an empty cluster gives zeros.  Every element of means is written.
 *   x           [B, N, D] bf16 / fp16, D 64 / 128, read ONCE and in place: strides == NULL: contiguous; otherwise batch b is head
 *               b % heads_per_batch of video b / heads_per_batch — element (b, n, :) at x + (b / hpb) * batch + (b % hpb) * head + n * row
 *               (a token-major view of a projection output: { N * H * D, D, H * D })
 *   sorted_idx  int32 [B, N]: the rows of every batch grouped by cluster, clusters ascending (svg_argsort_labels, svg_kmeans_loop*)
 *   counts      int32 [B, K]: the cluster sizes; cluster c owns sorted_idx[b][sum(counts[b][:c]) ...]
 *   means       [B, K, D] contiguous, of x's dtype */
int svg_cluster_means(const void* x, const svg_tensor_strides_t* strides /* NULL: contiguous */, int32_t heads_per_batch,
                      const int32_t* sorted_idx, const int32_t* counts, void* means, int32_t B, int32_t N, int32_t K, int32_t D,
                      int32_t dtype, void* stream);

/* 0 for what the entry refuses. */
size_t svg_centroid_tail_workspace_bytes(int32_t H, int32_t QB, int32_t KC);

/* The statement above for every row a block-row covers.
 *   q          [H, Sq, 128] bf16 / fp16; layout == NULL: contiguous, otherwise its heads_per_batch and q member (svg_attn_layout_t)
 *   kbar, vbar [H, KC, 128] contiguous, of q's dtype; every row of vbar finite, also the rows of clusters the tail leaves out (their
 *              weight is zero, and svg_cluster_means writes zeros for an empty cluster)
 *   block_map  uint8 [H, QB, map_cols], map_cols >= KC: only columns [0, KC) are read (a map with further columns — HunyuanVideo's two
 *              text pseudo-clusters — is passed as it is); non-zero: the sparse call has the cluster, the tail leaves it out
 *   q_sizes    int32 [H, QB]: block-row a covers the next q_sizes[h][a] rows of head h in sorted order, as in svg_varblock_attention
 *   k_sizes    int32 [H, KC]: the weights n_c; a cluster of size 0 is never a pseudo key
 *   q_row_idx  int32 [H, Sq] or NULL: sorted position -> the caller's row
 *   o          [H, Sq, 128] contiguous, of q's dtype; lse fp32 [H, Sq], natural logarithm: both indexed by the caller's row, exactly as
 *              svg_varblock_attention_lse indexes them
 * A row whose key set is empty (every non-empty cluster selected) gets o = 0 and lse = -inf.  A row no block-row covers (behind
 * sum(q_sizes[h])) is not written, neither in o nor in lse. */
int svg_centroid_tail_attention_lse(const void* q, const void* kbar, const void* vbar, void* o, float* lse, int32_t H, int32_t Sq, int32_t KC,
                                    int32_t D, int32_t dtype, float sm_scale, const uint8_t* block_map, int32_t map_cols,
                                    const int32_t* q_sizes, const int32_t* k_sizes, int32_t QB, const int32_t* q_row_idx, void* workspace,
                                    size_t workspace_bytes, const svg_attn_layout_t* layout /* NULL: contiguous */, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* SVG_ATTN_CENTROID_TAIL_H_ */

// The launchers of csrc/kmeans_metric.hip (the cosine / dot-product centroid update and the initial normalisation), called by the metric
// forms of the iteration and of the Lloyd loop in csrc/kmeans.hip.  Everything is validated by the caller.
#pragma once
#include "svg_common.h"

namespace svg {

// The update of include/svg_attn_kmeans_metric.h on given labels: stable sort of the labels (sort_ws: svg_argsort_workspace_bytes),
// shift cleared, kmeans_update_sphere_kernel.  metric: SVG_KMEANS_COSINE (rows weighted by 1 / |x|) or SVG_KMEANS_DOT.
int run_kmeans_update_metric(const void* x, long long x_bs, const void* c_in, void* c_out, const int32_t* labels, int32_t* counts,
                             int32_t* sorted_idx, float* shift, int B, int N, int K, int D, int dtype, int metric, void* sort_ws,
                             hipStream_t st);

// out[r] = c[r] / max(|c[r]|, 1e-12), rounded once: `rows` rows of D elements (c and out may not overlap)
int run_kmeans_unit_rows(const void* c, void* out, long long rows, int D, int dtype, hipStream_t st);

}  // namespace svg

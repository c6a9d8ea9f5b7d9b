// The host records of the k-means entries (csrc/kmeans.hip): the call record every extern "C" entry fills from its arguments, the
// workspace blocks and what one iteration reads and writes — and the launchers of csrc/kmeans_metric.hip (the cosine / dot-product
// centroid update and the initial normalisation), which take them.  Everything is validated by the caller.
#pragma once
#include "svg_common.h"

namespace svg {

// One k-means call as its entry received it; an entry leaves what it does not take at the default.  x_bs: elements between the batches of
// x (N * D for the entries without a stride).  c_init / centroids_out are centroids_in / centroids_out of the single-iteration entries.
struct KmeansCall {
    const void* x = nullptr;
    long long x_bs = 0;
    const float* xsq = nullptr;   // may be NULL: the argmax form of the assignment does not use |x|^2 (kmeans_assign_kernel)
    const void* c_init = nullptr;
    void *c_work_a = nullptr, *c_work_b = nullptr;
    int32_t *labels = nullptr, *counts = nullptr, *sorted_idx = nullptr;
    void* centroids_out = nullptr;
    int32_t* n_iters = nullptr;
    const float* maxima = nullptr;   // svg_kmeans_stepped_commit: the group maxima the caller hands in
    int B = 0, N = 0, K = 0, D = 0, dtype = 0, metric = SVG_KMEANS_EUCLID, group = 0, max_iters = 0;
    float tol = 0.f;
    int fp8_iters = 0;               // the iterations in front of this one assign with the e4m3 scores
    void* workspace = nullptr;
    size_t workspace_bytes = 0;
    hipStream_t st = nullptr;
};

inline size_t up256(size_t n) { return (n + 255) / 256 * 256; }

// per-iteration scratch (svg_kmeans_workspace_bytes): |c|^2 of the Euclidean assignment, behind it the sort scratch of the update
struct KmeansIterWs {
    float* csq;
    void* sort;
    size_t sort_bytes, bytes;
};
// scratch of one e4m3 assignment (svg_kmeans_assign_e4m3_workspace_bytes): the centroid image, its scale bytes (one int32 each) and csq'
struct KmeansE4m3Ws {
    uint8_t* c8;
    int32_t* cscale;
    float* csq;
    size_t bytes;
};
// what one iteration reads and writes: an entry's own buffers, or the centroid buffers by iteration parity and the scratch of a loop
struct KmeansStep {
    const void* c_in;
    void* c_out;
    int32_t *labels, *counts, *sorted_idx;
    float* shift;
    KmeansIterWs ws;
    const float* mu;      // the e4m3 assignment: its centre (NULL: zeros) and its scratch
    KmeansE4m3Ws e4m3;
};

// The update of include/svg_attn_kmeans_metric.h on the labels of s: stable sort of the labels, shift cleared,
// kmeans_update_sphere_kernel.  a.metric: SVG_KMEANS_COSINE (rows weighted by 1 / |x|) or SVG_KMEANS_DOT.
int run_kmeans_update_metric(const KmeansCall& a, const KmeansStep& s);

// out[r] = c[r] / max(|c[r]|, 1e-12), rounded once: the B * K rows of a.c_init (c and out may not overlap)
int run_kmeans_unit_rows(const KmeansCall& a, void* out);

}  // namespace svg

// The controller of SVG2's per-head top-p (include/svg_attn_adaptive_top_p.h, svg_top_p_update): after a sparse layer-call, one wave per
// head gathers the call's row log-sum-exp at the R <= 64 sampled rows, sets it against the dense log-sum-exp of those rows — the kept mass,
// mean_i exp(lse_sparse - lse_dense) — and steps the head's top_p towards the mass the user asked for.  Everything stays on the device: the
// next call of the layer reads top_p[h] in the block-map kernels (dynmap.hip).
//   * lane i owns sampled row i: difference and exponential in fp64, a butterfly sum in fp64, ONE rounding to fp32 — R <= 64 terms in
//     [0, ~1] lose nothing that survives that rounding, whatever the order;
//   * the step is fp32 with every product and sum rounded (the file is built without contraction, like dynmap.hip), so that a float64
//     statement of the law reproduces it within the roundings it names.
#include "svg_common.h"

namespace svg {

constexpr int kTopPMaxRows = 64;

__global__ __launch_bounds__(64) void top_p_update_kernel(const float* __restrict__ lse_sparse, const int64_t* __restrict__ rows,
                                                          const float* __restrict__ lse_dense, int R, int S, float target, float gain_up,
                                                          float gain_down, float band, float p_min, float p_max, float* __restrict__ kept,
                                                          float* __restrict__ top_p) {
    const int h = blockIdx.x, lane = threadIdx.x;
    double term = 0.0;
    if (lane < R) {
        const int64_t row = rows[lane];
        if (row < 0 || row >= S) {
            term = __builtin_nan("");                      // (not read: the head's kept mass says so and its top_p stays)
        } else {
            const float ls = lse_sparse[(size_t)h * S + row];
            const float ld = lse_dense[(size_t)h * R + lane];
            term = (ls == -INFINITY) ? 0.0 : exp((double)ls - (double)ld);   // a row the sparse form gave no key kept nothing
        }
    }
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) term += __shfl_xor(term, o);
    if (lane != 0) return;
    const float kp = (float)(term / (double)R);
    kept[h] = kp;
    if (!(fabsf(kp) <= 3.402823466e38f)) return;           // NaN or inf: nothing to steer by
    const float e = target - kp;
    float step = 0.f;
    if (e > 0.f) step = gain_up * e;
    else if (e < -band) step = gain_down * (e + band);
    top_p[h] = fminf(fmaxf(top_p[h] + step, p_min), p_max);
}

}  // namespace svg

using namespace svg;

extern "C" int svg_top_p_update(const float* lse_sparse, const int64_t* rows, const float* lse_dense, int32_t R, int32_t BH, int32_t S,
                                float target, float gain_up, float gain_down, float band, float p_min, float p_max, float* kept,
                                float* top_p, void* stream) {
    if (!lse_sparse || !rows || !lse_dense || !kept || !top_p) return SVG_ERR_BAD_ARG;
    if (R < 1 || R > kTopPMaxRows || BH <= 0 || S <= 0) return SVG_ERR_BAD_ARG;
    if (!(gain_up >= 0.f) || !(gain_down >= 0.f) || !(band >= 0.f)) return SVG_ERR_BAD_ARG;       // (negative or NaN)
    if (!(p_min >= 0.f && p_min <= p_max && p_max <= 1.f)) return SVG_ERR_BAD_ARG;
    hipLaunchKernelGGL(top_p_update_kernel, dim3(BH), dim3(64), 0, (hipStream_t)stream, lse_sparse, rows, lse_dense, R, S, target, gain_up,
                       gain_down, band, p_min, p_max, kept, top_p);
    return launch_status();
}

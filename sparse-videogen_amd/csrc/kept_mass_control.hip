// The controllers steered by kept mass: SVG2's per-head top-p (include/svg_attn_adaptive_top_p.h, svg_top_p_update) and SVG1's per-head
// band width (include/svg_attn_adaptive_band.h, svg_band_width_update).  After a sparse layer-call, one wave per head gathers the call's
// row log-sum-exp at the R <= 64 sampled rows, sets it against the dense log-sum-exp of those rows — the kept mass, mean_i exp(lse_sparse -
// lse_dense) — and steps the head's value towards the mass the user asked for.  Everything stays on the device: the next call of the layer
// reads top_p[h] in the block-map kernels (dynmap.hip), band[h] in the per-head band kernels (attention.hip).
//   * lane i owns sampled row i: difference and exponential in fp64, a butterfly sum in fp64, ONE rounding to fp32 — R <= 64 terms in
//     [0, ~1] lose nothing that survives that rounding, whatever the order (head_kept_mass: one statement, the same bits for both knobs);
//   * the step is fp32 with every product and sum rounded (the file is built without contraction, like dynmap.hip), so that a float64
//     statement of the law reproduces it within the roundings it names (dead_zone_step); top-p adds it and clamps, the band rounds it to
//     the nearest whole number of quanta (ties to even) and adds in 64 bits, so no band wraps whatever the vector held.
#include "svg_common.h"

namespace svg {

constexpr int kKeptMassMaxRows = 64;

// fp32 kept mass of head h over the R sampled rows, on every lane of the wave; NaN where a row lies outside [0, S)
__device__ __forceinline__ float head_kept_mass(const float* __restrict__ lse_sparse, const int64_t* __restrict__ rows,
                                                const float* __restrict__ lse_dense, int R, int S, int h, int lane) {
    double term = 0.0;
    if (lane < R) {
        const int64_t row = rows[lane];
        if (row < 0 || row >= S) {
            term = __builtin_nan("");                      // (not read: the head's kept mass says so and its value stays)
        } else {
            const float ls = lse_sparse[(size_t)h * S + row];
            const float ld = lse_dense[(size_t)h * R + lane];
            term = (ls == -INFINITY) ? 0.0 : exp((double)ls - (double)ld);   // a row the sparse form gave no key kept nothing
        }
    }
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) term += __shfl_xor(term, o);
    return (float)(term / (double)R);
}

// the step before clamping or quantising: up by gain_up below target, down by gain_down beyond the dead zone above it, else none
// (a NaN target: e is NaN, both compares fail, the step is 0)
__device__ __forceinline__ float dead_zone_step(float kp, float target, float gain_up, float gain_down, float dead) {
    const float e = target - kp;
    float step = 0.f;
    if (e > 0.f) step = gain_up * e;
    else if (e < -dead) step = gain_down * (e + dead);
    return step;
}

__global__ __launch_bounds__(64) void top_p_update_kernel(const float* __restrict__ lse_sparse, const int64_t* __restrict__ rows,
                                                          const float* __restrict__ lse_dense, int R, int S, float target, float gain_up,
                                                          float gain_down, float band, float p_min, float p_max, float* __restrict__ kept,
                                                          float* __restrict__ top_p) {
    const int h = blockIdx.x, lane = threadIdx.x;
    const float kp = head_kept_mass(lse_sparse, rows, lse_dense, R, S, h, lane);
    if (lane != 0) return;
    kept[h] = kp;
    if (!(fabsf(kp) <= 3.402823466e38f)) return;           // NaN or inf: nothing to steer by
    const float step = dead_zone_step(kp, target, gain_up, gain_down, band);
    top_p[h] = fminf(fmaxf(top_p[h] + step, p_min), p_max);
}

__global__ __launch_bounds__(64) void band_width_update_kernel(const float* __restrict__ lse_sparse, const int64_t* __restrict__ rows,
                                                               const float* __restrict__ lse_dense, int R, int S, float target,
                                                               float gain_up, float gain_down, float dead, int quantum, int band_min,
                                                               int band_max, const int32_t* __restrict__ skip_flag,
                                                               float* __restrict__ kept, int32_t* __restrict__ band) {
    const int h = blockIdx.x, lane = threadIdx.x;
    const float kp = head_kept_mass(lse_sparse, rows, lse_dense, R, S, h, lane);
    if (lane != 0) return;
    kept[h] = kp;
    if (skip_flag && skip_flag[0] != 0) return;            // a dense warm-up step: its kept mass is 1 and says nothing
    if (!(fabsf(kp) <= 3.402823466e38f)) return;           // NaN or inf: nothing to steer by
    const float x = fminf(fmaxf(dead_zone_step(kp, target, gain_up, gain_down, dead), -65536.f), 65536.f);
    const long long n = (long long)rintf(x);
    const long long b = (long long)band[h] + n * (long long)quantum;
    band[h] = (int32_t)(b < band_min ? band_min : (b > band_max ? band_max : b));
}

// what both entries check of the operands they share
static int kept_mass_args(const void* lse_sparse, const void* rows, const void* lse_dense, const void* kept, const void* state, int R, int BH,
                          int S, float gain_up, float gain_down, float dead) {
    if (!lse_sparse || !rows || !lse_dense || !kept || !state) return SVG_ERR_BAD_ARG;
    if (R < 1 || R > kKeptMassMaxRows || BH <= 0 || S <= 0) return SVG_ERR_BAD_ARG;
    if (!(gain_up >= 0.f) || !(gain_down >= 0.f) || !(dead >= 0.f)) return SVG_ERR_BAD_ARG;       // (negative or NaN)
    return SVG_OK;
}

}  // namespace svg

using namespace svg;

extern "C" int svg_top_p_update(const float* lse_sparse, const int64_t* rows, const float* lse_dense, int32_t R, int32_t BH, int32_t S,
                                float target, float gain_up, float gain_down, float band, float p_min, float p_max, float* kept,
                                float* top_p, void* stream) {
    if (int rc = kept_mass_args(lse_sparse, rows, lse_dense, kept, top_p, R, BH, S, gain_up, gain_down, band)) return rc;
    if (!(p_min >= 0.f && p_min <= p_max && p_max <= 1.f)) return SVG_ERR_BAD_ARG;
    hipLaunchKernelGGL(top_p_update_kernel, dim3(BH), dim3(64), 0, (hipStream_t)stream, lse_sparse, rows, lse_dense, R, S, target, gain_up,
                       gain_down, band, p_min, p_max, kept, top_p);
    return launch_status();
}

extern "C" int svg_band_width_update(const float* lse_sparse, const int64_t* rows, const float* lse_dense, int32_t R, int32_t BH, int32_t S,
                                     float target, float gain_up, float gain_down, float dead, int32_t quantum, int32_t band_min,
                                     int32_t band_max, const int32_t* skip_flag, float* kept, int32_t* band, void* stream) {
    if (int rc = kept_mass_args(lse_sparse, rows, lse_dense, kept, band, R, BH, S, gain_up, gain_down, dead)) return rc;
    if (quantum < 1 || quantum > 4096) return SVG_ERR_BAD_ARG;
    if (band_min < 1 || band_min > band_max || (int64_t)band_max > (int64_t)S + 1) return SVG_ERR_BAD_ARG;
    hipLaunchKernelGGL(band_width_update_kernel, dim3(BH), dim3(64), 0, (hipStream_t)stream, lse_sparse, rows, lse_dense, R, S, target,
                       gain_up, gain_down, dead, quantum, band_min, band_max, skip_flag, kept, band);
    return launch_status();
}

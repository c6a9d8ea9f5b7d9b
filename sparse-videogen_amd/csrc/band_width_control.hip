// The controller of SVG1's per-head band width (include/svg_attn_adaptive_band.h, svg_band_width_update): after a sparse layer-call, one
// wave per head gathers the call's row log-sum-exp at the R <= 64 sampled rows, sets it against the dense log-sum-exp of those rows — the
// kept mass, mean_i exp(lse_sparse - lse_dense), with the arithmetic and the bits of top_p_control.hip — and steps the head's band by whole
// quanta towards the mass the user asked for.  Everything stays on the device: the next call of the layer reads band[h] in the per-head band
// kernels (attention.hip).
//   * lane i owns sampled row i: difference and exponential in fp64, a butterfly sum in fp64, ONE rounding to fp32;
//   * the step is fp32 with every product and sum rounded (the file is built without contraction, like top_p_control.hip), then rounded to
//     the nearest whole number of quanta (ties to even) and added in 64 bits, so no band wraps whatever the vector held.
#include "svg_common.h"

namespace svg {

constexpr int kBandMaxRows = 64;

__global__ __launch_bounds__(64) void band_width_update_kernel(const float* __restrict__ lse_sparse, const int64_t* __restrict__ rows,
                                                               const float* __restrict__ lse_dense, int R, int S, float target,
                                                               float gain_up, float gain_down, float dead, int quantum, int band_min,
                                                               int band_max, const int32_t* __restrict__ skip_flag,
                                                               float* __restrict__ kept, int32_t* __restrict__ band) {
    const int h = blockIdx.x, lane = threadIdx.x;
    double term = 0.0;
    if (lane < R) {
        const int64_t row = rows[lane];
        if (row < 0 || row >= S) {
            term = __builtin_nan("");                      // (not read: the head's kept mass says so and its band stays)
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
    if (skip_flag && skip_flag[0] != 0) return;            // a dense warm-up step: its kept mass is 1 and says nothing
    if (!(fabsf(kp) <= 3.402823466e38f)) return;           // NaN or inf: nothing to steer by
    const float e = target - kp;
    float x = 0.f;
    if (e > 0.f) x = gain_up * e;
    else if (e < -dead) x = gain_down * (e + dead);
    x = fminf(fmaxf(x, -65536.f), 65536.f);                // (a NaN target: e is NaN, both compares fail, x stays 0)
    const long long n = (long long)rintf(x);
    const long long b = (long long)band[h] + n * (long long)quantum;
    band[h] = (int32_t)(b < band_min ? band_min : (b > band_max ? band_max : b));
}

}  // namespace svg

using namespace svg;

extern "C" int svg_band_width_update(const float* lse_sparse, const int64_t* rows, const float* lse_dense, int32_t R, int32_t BH, int32_t S,
                                     float target, float gain_up, float gain_down, float dead, int32_t quantum, int32_t band_min,
                                     int32_t band_max, const int32_t* skip_flag, float* kept, int32_t* band, void* stream) {
    if (!lse_sparse || !rows || !lse_dense || !kept || !band) return SVG_ERR_BAD_ARG;
    if (R < 1 || R > kBandMaxRows || BH <= 0 || S <= 0) return SVG_ERR_BAD_ARG;
    if (!(gain_up >= 0.f) || !(gain_down >= 0.f) || !(dead >= 0.f)) return SVG_ERR_BAD_ARG;       // (negative or NaN)
    if (quantum < 1 || quantum > 4096) return SVG_ERR_BAD_ARG;
    if (band_min < 1 || band_min > band_max || (int64_t)band_max > (int64_t)S + 1) return SVG_ERR_BAD_ARG;
    hipLaunchKernelGGL(band_width_update_kernel, dim3(BH), dim3(64), 0, (hipStream_t)stream, lse_sparse, rows, lse_dense, R, S, target,
                       gain_up, gain_down, dead, quantum, band_min, band_max, skip_flag, kept, band);
    return launch_status();
}

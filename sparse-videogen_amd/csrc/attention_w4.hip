// SVG1 band attention / dense attention on the one-wave-per-SIMD body (attn_w4.h): kernels and launchers.
// A translation unit of its own: the body is large (two unrolled tile iterations x three instantiations) and compiles in
// parallel with attention.hip (the other band kernels) and attention_varblock.hip.
#include "attn_w4.h"
#include "band_policy.h"

namespace svg {

template <typename T, int D>
using BandW4 = BandPolicy<T, D, 4, 2>;   // 4 waves x 2 row blocks: 256-row q-tiles

template <typename T, int D>
__global__ __launch_bounds__(256, 1) void band_attn_w4_kernel(typename BandW4<T, D>::Params prm) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    attn_body_w4<T, D, BandW4<T, D>>(prm, smem, nullptr);
}

#ifdef SVG_ABLATIONS
// diagnostics build only: the same kernel with the per-phase cycle trace (svg_band_attention variant 32, svg_debug_pp_trace)
template <typename T, int D, int ABL>
__global__ __launch_bounds__(256, 1) void band_attn_w4_trace_kernel(typename BandW4<T, D>::Params prm) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    attn_body_w4<T, D, BandW4<T, D>, true, ABL>(prm, smem, nullptr);
}
#endif

template <typename T, int D>
static int run_w4(const BandCall& c) {
    using Pol = BandW4<T, D>;
    const int BH = c.BH;
    const hipStream_t st = c.stream;
    const typename Pol::Params p = make_band_params<Pol, T>(c);
    if (c.trace) {
#ifdef SVG_ABLATIONS
        if constexpr (D == 128 && std::is_same<T, __bf16>::value) {
            g_trace_reader = read_trace_here;
#define SVG_W4_TRACE(A) case A: return launch_attn(band_attn_w4_trace_kernel<T, D, A>, dim3(p.nqt * BH), 256, attn_w4_lds_bytes<D>(), st, p);
            switch (c.trace_abl) {
                SVG_W4_TRACE(0) SVG_W4_TRACE(1) SVG_W4_TRACE(2) SVG_W4_TRACE(3) SVG_W4_TRACE(4) SVG_W4_TRACE(5) SVG_W4_TRACE(6)
                default: return SVG_ERR_UNSUPPORTED;
            }
#undef SVG_W4_TRACE
        }
#endif
        return SVG_ERR_UNSUPPORTED;   // diagnostics builds only (-DSVG_ABLATIONS), bf16 / D = 128
    }
    return launch_attn(band_attn_w4_kernel<T, D>, dim3(p.nqt * BH), 256, attn_w4_lds_bytes<D>(), st, p);
}

int run_band_w4(const BandCall& c) {
    return dispatch_td(c.dtype, c.D, [&](auto t, auto d) { return run_w4<decltype(t), decltype(d)::value>(c); });
}

}  // namespace svg

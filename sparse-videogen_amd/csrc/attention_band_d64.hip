// SVG1 band attention at head_dim 64 with the row log-sum-exp, and with fp32 rows (include/svg_attn_band_lse_d64.h): the kernels that run
// attn_body_pp2 (attn_core.h) — the 32x32x16 two-phase body in its four-waves-per-SIMD (LEAN) form, the body of the plain head_dim-64
// kernels of attention.hip — on BandLsePolicy64 / BandF32Policy64 (band_policy.h), and their launcher.  The entries are in attention.hip
// (band_run validates; run_band_lse_d64 below launches).
// A translation unit of its own: it is compiled without packed fp32 instructions (build.py NO_PACKED_FP32), which the compiler would
// otherwise pick for the epilogue's products; what the 16-bit rows round and how is written out in pp2_row16_values, so o keeps the bits
// of the plain kernels whatever this unit's flags are.
#include "attn_core.h"
#include "band_policy.h"

namespace svg {

// Static mapping over (head, q-tile), BandPolicy::init.  128 registers and 64 KiB of LDS per workgroup: two workgroups per CU, as
// band_attn_pp2_kernel<T, 64>.  The fp32 form stages its rows in all four stages (8 waves x 32 rows x 256 bytes), the 16-bit form in the
// first 34 KiB as the plain kernel does.
template <typename T, typename Pol>
__global__ __launch_bounds__(512, 4) void band_attn_pp2_d64_kernel(typename Pol::Params prm) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    attn_body_pp2<T, 64, Pol, false, 0, false, true>(prm, smem, nullptr);
}
// Device switch (band_attn_pp2_switch64_kernel, attention.hip): `flag[0] != 0` selects prm_alt — the dense mask, built without the head
// permutation, so o, lse and o32 are then written in logical row order.
template <typename T, typename Pol>
__global__ __launch_bounds__(512, 4) void band_attn_pp2_d64_switch_kernel(typename Pol::Params prm, typename Pol::Params prm_alt,
                                                                          const int32_t* __restrict__ flag) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    if (flag[0] != 0) attn_body_pp2<T, 64, Pol, false, 0, false, true>(prm_alt, smem, nullptr);
    else attn_body_pp2<T, 64, Pol, false, 0, false, true>(prm, smem, nullptr);
}

template <typename T, typename Pol>
static int launch_band_d64(const BandCall& c) {
    constexpr int lds = attn_pp2_lds_bytes<64>();
    const typename Pol::Params p = make_band_params<Pol, T>(c);
    if (!c.use_alt) return launch_attn(band_attn_pp2_d64_kernel<T, Pol>, dim3(p.nqt * p.BH), 512, lds, c.stream, p);
    // the alternate block: alt_mask, no head permutation; the launch covers the q-tiles of the larger of the two
    BandCall alt = c;
    alt.mask = c.alt_mask, alt.perm = nullptr;
    const typename Pol::Params a = make_band_params<Pol, T>(alt);
    return launch_attn(band_attn_pp2_d64_switch_kernel<T, Pol>, dim3(std::max(p.nqt, a.nqt) * p.BH), 512, lds, c.stream, p, a, c.use_alt);
}

int run_band_lse_d64(const BandCall& c) {
    return dispatch_td(c.dtype, c.D, [&](auto t, auto d) -> int {
        using T = decltype(t);
        if constexpr (decltype(d)::value != 64) return SVG_ERR_UNSUPPORTED;
        else return c.o32 ? launch_band_d64<T, BandF32Policy64<T>>(c) : launch_band_d64<T, BandLsePolicy64<T>>(c);
    });
}

}  // namespace svg

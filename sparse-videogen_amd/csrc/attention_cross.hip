// Cross attention for gfx950: dense attention of Sq query rows over a short key set (Sq != Skv), the two-phase 16x16x32 body of
// attn_m16.h on the policy of cross_policy.h, and the svg_cross_attention / svg_cross_attention_keyrange entries.  (Band family: attention.hip; SVG2: attention_varblock.hip.)
#include <algorithm>

#include "attn_m16.h"
#include "cross_policy.h"

namespace svg {

// Resident workgroups: min(BH * nqt, CUs) of them, each walking the work items blockIdx.x, blockIdx.x + gridDim.x, ... — item w is
// (head, q-tile) = (w / nqt, w % nqt), head-major.  Every item costs the same (all Skv keys), so the static stride is balanced: no
// counters, no atomics.  One workgroup barrier between two q-tiles, as in band_attn_m16_queue_kernel (the epilogue of the first reads
// the stages the second fills).  Per row the keys are visited in ascending order: the result does not depend on the grid size.
// Windowed (svg_cross_attention_keyrange): an item costs the key tiles of its video's window, so the static stride is balanced only within
// a video; the same loop all the same (no queue): the tail is bounded by one item of the longest window, see DESIGN 3.1.4.
template <typename T, bool Windowed = false>
__global__ __launch_bounds__(512, 2) void cross_attn_m16_kernel(typename CrossPolicy<T, Windowed>::Params prm) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    using Pol = CrossPolicy<T, Windowed>;
    const int n_items = prm.BH * prm.nqt;
    for (int w = blockIdx.x; w < n_items; w += gridDim.x) {
        if (w != (int)blockIdx.x) __syncthreads();
        const int head = w / prm.nqt;
        typename Pol::Ctx ctx;
        Pol::init_tile(prm, ctx, head, w - head * prm.nqt);
        attn_m16_tile<T, Pol, false, 1>(prm, ctx, smem);
    }
}

// compute units of the current device (cached per thread and device; kNumCU when the runtime cannot say)
static int device_cus() {
    static thread_local int cached_dev = -1, cached_n = 0;
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess) {
        (void)hipGetLastError();
        return kNumCU;
    }
    if (dev != cached_dev) {
        int n = 0;
        if (hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || n <= 0) {
            (void)hipGetLastError();
            return kNumCU;
        }
        cached_dev = dev, cached_n = n;
    }
    return cached_n;
}

}  // namespace svg

using namespace svg;

// the checks and the launch of both entries; kv_end == nullptr: the plain kernel
static int cross_attention_launch(const void* q, const void* k, const void* v, void* o, int32_t BH, int32_t Sq, int32_t Skv, int32_t D, int32_t dtype,
                                  float sm_scale, const int32_t* kv_begin, const int32_t* kv_end, int32_t heads_per_window,
                                  const svg_attn_layout_t* layout, void* stream) {
    if (!q || !k || !v || !o || BH <= 0 || Sq <= 0 || Skv <= 0) return SVG_ERR_BAD_ARG;
    if (D != 128) return SVG_ERR_UNSUPPORTED;
    if (check_rows(Sq, D) != SVG_OK || check_rows(Skv, D) != SVG_OK) return SVG_ERR_UNSUPPORTED;
    if ((int64_t)BH * Sq * D >= (1ll << 40)) return SVG_ERR_UNSUPPORTED;
    AttnLayout lay = contiguous_layout(BH, BH, Sq, Skv, D);
    if (layout) {
        if (const int rc = layout_from_abi(layout, BH, BH, Sq, Skv, D, q, k, v, o, lay); rc != SVG_OK) return rc;
    }
    return dispatch_td(dtype, D, [&](auto t, auto d) -> int {
        using T = decltype(t);
        if constexpr (decltype(d)::value != 128) {
            return SVG_ERR_UNSUPPORTED;
        } else {
            auto launch = [&](auto windowed_c) -> int {
                constexpr bool kWindowed = decltype(windowed_c)::value;
                using Pol = CrossPolicy<T, kWindowed>;
                typename Pol::Params p;
                if constexpr (kWindowed) p.kv_begin = kv_begin, p.kv_end = kv_end, p.heads_per_window = heads_per_window;
                p.q = (const T*)q, p.k = (const T*)k, p.v = (const T*)v, p.o = (T*)o;
                p.Sq = Sq, p.Skv = Skv, p.BH = BH, p.nqt = (Sq + Pol::BM - 1) / Pol::BM;
                p.scale_log2 = sm_scale * 1.4426950408889634f;
                p.lay = lay;
                const int n_wg = (int)std::min<int64_t>((int64_t)BH * p.nqt, device_cus());
                return launch_attn(cross_attn_m16_kernel<T, kWindowed>, dim3(n_wg), 512, attn_m16_lds_bytes(), (hipStream_t)stream, p);
            };
            return kv_end ? launch(std::true_type{}) : launch(std::false_type{});
        }
    });
}

extern "C" int svg_cross_attention(const void* q, const void* k, const void* v, void* o, int32_t BH, int32_t Sq, int32_t Skv, int32_t D,
                                   int32_t dtype, float sm_scale, const svg_attn_layout_t* layout, void* stream) {
    return cross_attention_launch(q, k, v, o, BH, Sq, Skv, D, dtype, sm_scale, nullptr, nullptr, 1, layout, stream);
}

extern "C" int svg_cross_attention_keyrange(const void* q, const void* k, const void* v, void* o, int32_t BH, int32_t Sq, int32_t Skv, int32_t D,
                                            int32_t dtype, float sm_scale, const int32_t* kv_begin, const int32_t* kv_end,
                                            int32_t heads_per_window, const svg_attn_layout_t* layout, void* stream) {
    if (!kv_end || heads_per_window <= 0) return SVG_ERR_BAD_ARG;
    if (BH > 0 && BH % heads_per_window != 0) return SVG_ERR_BAD_ARG;
    return cross_attention_launch(q, k, v, o, BH, Sq, Skv, D, dtype, sm_scale, kv_begin, kv_end, heads_per_window, layout, stream);
}

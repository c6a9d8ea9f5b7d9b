// Cross attention for gfx950: dense attention of Sq query rows over a short key set (Sq != Skv), the two-phase 16x16x32 body of
// attn_m16.h on the policy of cross_policy.h, and the svg_cross_attention / svg_cross_attention_keyrange / svg_cross_attention_pair /
// svg_cross_attention_lse / svg_cross_attention_lse_f32 entries.  (Band family: attention.hip; SVG2: attention_varblock.hip.)
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
// One template: the policy is the only thing that differs between the instantiations — CrossPolicy, CrossLsePolicy (svg_cross_attention_lse: the
// epilogue of attn_m16_tile also stores one fp32 per query row) and CrossF32Policy (svg_cross_attention_lse_f32: it stores the rows as fp32, before
// their rounding, and no 16-bit o), each windowed or not — and each instantiation's listing is compared with the one it had as a kernel of
// its own (tools/asm_diff.py --pair, profiles/kernel_templates_asm_diff.txt).
template <typename T, typename Pol>
__global__ __launch_bounds__(512, 2) void cross_attn_m16_kernel(typename Pol::Params prm) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int n_items = prm.BH * prm.nqt;
    for (int w = blockIdx.x; w < n_items; w += gridDim.x) {
        if (w != (int)blockIdx.x) __syncthreads();
        const int head = w / prm.nqt;
        typename Pol::Ctx ctx;
        Pol::init_tile(prm, ctx, head, w - head * prm.nqt);
        attn_m16_tile<T, Pol, false, 1>(prm, ctx, smem);
    }
}

// Pair form (svg_cross_attention_pair): the same resident loop, every work item run twice — attn_m16_tile over key set A, whose epilogue
// stores T(o_A) to o; the workgroup barrier two q-tiles need between them (the epilogue reads the stages the next pass fills); attn_m16_tile
// over key set B, whose final row store loads the 8 bytes the lane stored in pass A, adds T(o_B) in fp32 and stores the rounded sum.  o_A
// is not kept in registers (48 VGPRs the body does not have at two waves per SIMD); q is read again in pass B, from L2.
// The read-back needs no fence and no barrier ONLY because the SAME lane wrote the same address in pass A: the epilogue's map from
// (wave, lane) to (row, column) of the q-tile depends on wave, lane and q0 — never on the key set, its length or its strides — and a lane
// reads its own stores in program order.  If that map ever differs between the two passes, a fence and a barrier have to go between them.
// One copy of the body: the pass is a run-time (scalar) value, the Params of a pass are selected from the kernel arguments.
template <typename T>
__global__ __launch_bounds__(512, 2) void cross_attn_pair_m16_kernel(CrossPairArgs<T> args) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    using Pol = CrossPairPolicy<T>;
    const int n_items = args.a.BH * args.a.nqt;
    for (int w = blockIdx.x; w < n_items; w += gridDim.x) {
        const int head = w / args.a.nqt;
        const int qt = w - head * args.a.nqt;
#pragma nounroll
        for (int set = 0; set < 2; ++set) {
            if (w != (int)blockIdx.x || set != 0) __syncthreads();
            typename Pol::Params prm;
            static_cast<typename Pol::Base::Params&>(prm) = args.a;
            prm.add_to_o = set;
            if (set != 0) {
                prm.k = args.k_b, prm.v = args.v_b, prm.Skv = args.Skv_b;
                prm.lay.hpb_kv = args.hpb_kv_b;
                prm.lay.k_bs = args.k_bs_b, prm.lay.k_hs = args.k_hs_b, prm.lay.k_rs = args.k_rs_b;
                prm.lay.v_bs = args.v_bs_b, prm.lay.v_hs = args.v_hs_b, prm.lay.v_rs = args.v_rs_b;
            }
            typename Pol::Ctx ctx;
            Pol::init_tile(prm, ctx, head, qt);
            attn_m16_tile<T, Pol, false, 1>(prm, ctx, smem);
        }
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

// the checks and the launch of the plain, keyrange, LSE and fp32 entries; kv_end == nullptr: not windowed; lse != nullptr: the LSE form;
// o32 != nullptr: the fp32 form — 16-byte aligned, `o` is then q, which stands in through the null and layout checks (the o member of
// `layout` is not read: it takes q's strides), and the kernel gets no 16-bit o
static int cross_attention_launch(const void* q, const void* k, const void* v, void* o, float* lse, float* o32, int32_t BH, int32_t Sq, int32_t Skv,
                                  int32_t D, int32_t dtype, float sm_scale, const int32_t* kv_begin, const int32_t* kv_end,
                                  int32_t heads_per_window, const svg_attn_layout_t* layout, void* stream) {
    if (!q || !k || !v || !o || BH <= 0 || Sq <= 0 || Skv <= 0) return SVG_ERR_BAD_ARG;
    if (D != 128) return SVG_ERR_UNSUPPORTED;
    if (check_rows(Sq, D) != SVG_OK || check_rows(Skv, D) != SVG_OK) return SVG_ERR_UNSUPPORTED;
    if ((int64_t)BH * Sq * D >= (1ll << 40)) return SVG_ERR_UNSUPPORTED;
    if (((size_t)o32 & 15) != 0) return SVG_ERR_UNSUPPORTED;
    AttnLayout lay = contiguous_layout(BH, BH, Sq, Skv, D);
    if (layout) {
        svg_attn_layout_t abi = *layout;
        if (o32) abi.o = abi.q;
        if (const int rc = layout_from_abi(&abi, BH, BH, Sq, Skv, D, q, k, v, o, lay); rc != SVG_OK) return rc;
    }
    return dispatch_td(dtype, D, [&](auto t, auto d) -> int {
        using T = decltype(t);
        if constexpr (decltype(d)::value != 128) {
            return SVG_ERR_UNSUPPORTED;
        } else {
            auto launch = [&](auto pol) -> int {
                using Pol = decltype(pol);
                typename Pol::Params p;
                p.q = (const T*)q, p.k = (const T*)k, p.v = (const T*)v, p.o = (T*)o;
                if constexpr (HasRowLse<Pol>::value) p.lse = lse;
                if constexpr (HasRowO32<Pol>::value) p.o32 = o32, p.o = nullptr;
                if constexpr (std::is_base_of_v<CrossPolicy<T, true>, Pol>) p.kv_begin = kv_begin, p.kv_end = kv_end, p.heads_per_window = heads_per_window;
                p.Sq = Sq, p.Skv = Skv, p.BH = BH, p.nqt = (Sq + Pol::BM - 1) / Pol::BM;
                p.scale_log2 = sm_scale * 1.4426950408889634f;
                p.lay = lay;
                const int n_wg = (int)std::min<int64_t>((int64_t)BH * p.nqt, device_cus());
                return launch_attn(cross_attn_m16_kernel<T, Pol>, dim3(n_wg), 512, attn_m16_lds_bytes(), (hipStream_t)stream, p);
            };
            if (o32) return kv_end ? launch(CrossF32Policy<T, true>()) : launch(CrossF32Policy<T, false>());
            if (lse) return kv_end ? launch(CrossLsePolicy<T, true>()) : launch(CrossLsePolicy<T, false>());
            return kv_end ? launch(CrossPolicy<T, true>()) : launch(CrossPolicy<T, false>());
        }
    });
}

extern "C" int svg_cross_attention(const void* q, const void* k, const void* v, void* o, int32_t BH, int32_t Sq, int32_t Skv, int32_t D,
                                   int32_t dtype, float sm_scale, const svg_attn_layout_t* layout, void* stream) {
    return cross_attention_launch(q, k, v, o, nullptr, nullptr, BH, Sq, Skv, D, dtype, sm_scale, nullptr, nullptr, 1, layout, stream);
}

extern "C" int svg_cross_attention_pair(const void* q, const void* k_a, const void* v_a, const void* k_b, const void* v_b, void* o, int32_t BH,
                                        int32_t Sq, int32_t Skv_a, int32_t Skv_b, int32_t D, int32_t dtype, float sm_scale,
                                        const svg_attn_layout_t* layout, const svg_attn_layout_t* layout_b, void* stream) {
    if (!q || !k_a || !v_a || !k_b || !v_b || !o || BH <= 0 || Sq <= 0 || Skv_a <= 0 || Skv_b <= 0) return SVG_ERR_BAD_ARG;
    if (D != 128) return SVG_ERR_UNSUPPORTED;
    if (check_rows(Sq, D) != SVG_OK || check_rows(Skv_a, D) != SVG_OK || check_rows(Skv_b, D) != SVG_OK) return SVG_ERR_UNSUPPORTED;
    if ((int64_t)BH * Sq * D >= (1ll << 40)) return SVG_ERR_UNSUPPORTED;
    AttnLayout lay = contiguous_layout(BH, BH, Sq, Skv_a, D);
    if (layout) {
        if (const int rc = layout_from_abi(layout, BH, BH, Sq, Skv_a, D, q, k_a, v_a, o, lay); rc != SVG_OK) return rc;
    }
    // set B: the heads per batch and the q / o strides are those of set A; its own k / v strides go through the same checks
    AttnLayout lay_b = contiguous_layout(lay.hpb_q, lay.hpb_kv, Sq, Skv_b, D);
    if (layout_b) {
        svg_attn_layout_t abi_b = *layout_b;
        abi_b.heads_per_batch = lay.hpb_q, abi_b.kv_heads_per_batch = lay.hpb_kv;
        abi_b.q = {lay.q_bs, lay.q_hs, lay.q_rs}, abi_b.o = {lay.o_bs, lay.o_hs, lay.o_rs};
        if (const int rc = layout_from_abi(&abi_b, BH, BH, Sq, Skv_b, D, q, k_b, v_b, o, lay_b); rc != SVG_OK) return rc;
    }
    return dispatch_td(dtype, D, [&](auto t, auto d) -> int {
        using T = decltype(t);
        if constexpr (decltype(d)::value != 128) {
            return SVG_ERR_UNSUPPORTED;
        } else {
            using Pol = CrossPairPolicy<T>;
            CrossPairArgs<T> p;
            p.a.q = (const T*)q, p.a.k = (const T*)k_a, p.a.v = (const T*)v_a, p.a.o = (T*)o;
            p.a.Sq = Sq, p.a.Skv = Skv_a, p.a.BH = BH, p.a.nqt = (Sq + Pol::BM - 1) / Pol::BM;
            p.a.scale_log2 = sm_scale * 1.4426950408889634f;
            p.a.lay = lay;
            p.k_b = (const T*)k_b, p.v_b = (const T*)v_b, p.Skv_b = Skv_b, p.hpb_kv_b = lay_b.hpb_kv;
            p.k_bs_b = lay_b.k_bs, p.k_hs_b = lay_b.k_hs, p.k_rs_b = lay_b.k_rs;
            p.v_bs_b = lay_b.v_bs, p.v_hs_b = lay_b.v_hs, p.v_rs_b = lay_b.v_rs;
            const int n_wg = (int)std::min<int64_t>((int64_t)BH * p.a.nqt, device_cus());
            return launch_attn(cross_attn_pair_m16_kernel<T>, dim3(n_wg), 512, attn_m16_lds_bytes(), (hipStream_t)stream, p);
        }
    });
}

extern "C" int svg_cross_attention_lse_f32(const void* q, const void* k, const void* v, float* o32, float* lse, int32_t BH, int32_t Sq,
                                           int32_t Skv, int32_t D, int32_t dtype, float sm_scale, const int32_t* kv_begin,
                                           const int32_t* kv_end, int32_t heads_per_window, const svg_attn_layout_t* layout, void* stream) {
    if (!o32 || !lse) return SVG_ERR_BAD_ARG;
    if (kv_end && (heads_per_window <= 0 || (BH > 0 && BH % heads_per_window != 0))) return SVG_ERR_BAD_ARG;
    return cross_attention_launch(q, k, v, const_cast<void*>(q), lse, o32, BH, Sq, Skv, D, dtype, sm_scale, kv_begin, kv_end, heads_per_window, layout,
                                  stream);
}

extern "C" int svg_cross_attention_keyrange(const void* q, const void* k, const void* v, void* o, int32_t BH, int32_t Sq, int32_t Skv, int32_t D,
                                            int32_t dtype, float sm_scale, const int32_t* kv_begin, const int32_t* kv_end,
                                            int32_t heads_per_window, const svg_attn_layout_t* layout, void* stream) {
    if (!kv_end || heads_per_window <= 0) return SVG_ERR_BAD_ARG;
    if (BH > 0 && BH % heads_per_window != 0) return SVG_ERR_BAD_ARG;
    return cross_attention_launch(q, k, v, o, nullptr, nullptr, BH, Sq, Skv, D, dtype, sm_scale, kv_begin, kv_end, heads_per_window, layout, stream);
}

extern "C" int svg_cross_attention_lse(const void* q, const void* k, const void* v, void* o, float* lse, int32_t BH, int32_t Sq, int32_t Skv,
                                       int32_t D, int32_t dtype, float sm_scale, const int32_t* kv_begin, const int32_t* kv_end,
                                       int32_t heads_per_window, const svg_attn_layout_t* layout, void* stream) {
    if (!lse) return SVG_ERR_BAD_ARG;
    if (kv_end && (heads_per_window <= 0 || (BH > 0 && BH % heads_per_window != 0))) return SVG_ERR_BAD_ARG;
    return cross_attention_launch(q, k, v, o, lse, nullptr, BH, Sq, Skv, D, dtype, sm_scale, kv_end ? kv_begin : nullptr, kv_end, heads_per_window, layout, stream);
}

// N-way merge of attention states (svg_merge_attention_states): n partial results of the SAME query rows, each computed over its own part
// of the keys — o_i (16-bit, contiguous [BH, Sq, D]) and its row log-sum-exp lse_i (fp32 [BH, Sq], svg_cross_attention_lse) — combined into
// the result over all keys.  Per row, in fp32, the parts visited in index order:
//     m = max_i lse_i,  w_i = exp(lse_i - m),  o = sum_i w_i o_i / sum_i w_i  (rounded ONCE to the 16-bit type),  lse = m + log sum_i w_i.
// A part with lse_i = -inf (its rows saw no key) or with a weight that underflows to zero contributes nothing — its o_i is not looked at,
// so a part 88 or more below the largest leaves the others' bits alone; all parts -inf: zeros and -inf; n == 1 copies the bits.
// ref: flashinfer.merge_state behind run(..., return_lse=True), svg/kernels/ops/attention_ops.py:178-188; the ring / Ulysses dense attention
//      of svg/models/wan_orig/distributed/xdit_context_parallel.py:120-169 merges its steps the same way.
// Why N-way and not a chain of pairwise merges: a pairwise merge hands a 16-bit o to the next one, so every step adds an output rounding.
// Exact partials rounded to bf16 and merged exactly with ONE final rounding sit at 2.35e-3 rel. L2 of the exact result (one rounding:
// 1.66e-3, so the two roundings add in quadrature); a pairwise chain that rounds every intermediate is at 2.98e-3 for 4 parts and 3.82e-3
// for 8 (N(0, 1) inputs, D 128).  Hence all parts in one pass, and at most kMergeMaxParts of them: the part pointers travel
// by value in the kernel arguments.
// Pure HBM-bandwidth work: every part is read once, o written once, 16 bytes per lane; a wave owns whole rows (D / 8 lanes each), so the
// weights are computed by the lanes that use them: no LDS, no shuffles, no atomics.
// svg_merge_attention_states_f32 (merge_states_f32_kernel below) takes the parts as fp32 rows, before any rounding.
#include "svg_common.h"

namespace svg {

constexpr int kMergeMaxParts = 8;
constexpr int kMergeThreads = 256;

struct MergeArgs {
    const void* o_part[kMergeMaxParts];
    const float* lse_part[kMergeMaxParts];
    void* o;
    float* lse;        // nullptr: not wanted
    long long rows;    // BH * Sq
    int n, Sq, hpb, o_rs;
    long long o_bs, o_hs;
};

// grid = ceil(rows / (kMergeThreads / (D / 8)))
template <typename T, int D>
__global__ __launch_bounds__(kMergeThreads) void merge_states_kernel(MergeArgs a) {
    using E = Elt<T>;
    using V8 = typename E::v8;
    constexpr int kLanesPerRow = D / 8;
    constexpr int kRowsPerWg = kMergeThreads / kLanesPerRow;
    const int sub = threadIdx.x / kLanesPerRow;
    const int col = (threadIdx.x - sub * kLanesPerRow) * 8;
    const long long row = (long long)blockIdx.x * kRowsPerWg + sub;
    if (row >= a.rows) return;

    // every load of the row first (the part index is compile-time, the pointers stay in scalar registers); the o_i of a part that turns
    // out to contribute nothing was read but never enters the arithmetic
    float l[kMergeMaxParts];
    V8 x[kMergeMaxParts];
#pragma unroll
    for (int i = 0; i < kMergeMaxParts; ++i)
        if (i < a.n) {
            l[i] = a.lse_part[i][row];
            x[i] = *(const V8*)((const T*)a.o_part[i] + row * D + col);
        }

    const int head = (int)(row / a.Sq);
    const int s = (int)(row - (long long)head * a.Sq);
    T* const dst = (T*)a.o + layout_head_off(a.o_bs, a.o_hs, a.hpb, head) + (size_t)s * a.o_rs + col;
    if (a.n == 1) {
        *(V8*)dst = x[0];
        if (a.lse && col == 0) a.lse[row] = l[0];
        return;
    }

    float m = -INFINITY;
#pragma unroll
    for (int i = 0; i < kMergeMaxParts; ++i)
        if (i < a.n) m = fmaxf(m, l[i]);
    float acc[8], sw = 0.f;
#pragma unroll
    for (int j = 0; j < 8; ++j) acc[j] = 0.f;
    bool first = true;
#pragma unroll
    for (int i = 0; i < kMergeMaxParts; ++i)
        if (i < a.n) {
            const float w = (l[i] == -INFINITY) ? 0.f : __builtin_amdgcn_exp2f((l[i] - m) * 1.4426950408889634f);
            if (w > 0.f) {   // (false for a NaN too)
                sw += w;
#pragma unroll
                for (int j = 0; j < 8; ++j) {
                    const float xf = E::to_float(x[i][j]);
                    acc[j] = first ? w * xf : fmaf(w, xf, acc[j]);   // the first part sets (a -0 stays one), the others add
                }
                first = false;
            }
        }
    V8 out;
    const float inv = sw > 0.f ? 1.f / sw : 0.f;
#pragma unroll
    for (int j = 0; j < 8; ++j) out[j] = E::from_float(acc[j] * inv);
    *(V8*)dst = out;
    if (a.lse && col == 0) a.lse[row] = sw > 0.f ? m + 0.6931471805599453f * __builtin_amdgcn_logf(sw) : -INFINITY;
}

// fp32 parts (svg_merge_attention_states_f32): o_i is the fp32 row the attention kernels hand out BEFORE their rounding
// (svg_cross_attention_lse_f32 and its band / variable-block siblings), so the rounding below is the only one between the accumulators and
// the merged o: exact parts merged this way sit at the 1.66e-3 (bf16) / 2.07e-4 (fp16) of one rounding instead of 2.35e-3 / 2.94e-4.
// The statement, the visiting order and the -inf / underflow rules are those of merge_states_kernel with xf read directly; the lane owns
// the same 8 columns and reads them as two 16-byte loads (twice the bytes per part).  n == 1 rounds the part once.
template <typename T, int D>
__global__ __launch_bounds__(kMergeThreads) void merge_states_f32_kernel(MergeArgs a) {
    using E = Elt<T>;
    using V8 = typename E::v8;
    constexpr int kLanesPerRow = D / 8;
    constexpr int kRowsPerWg = kMergeThreads / kLanesPerRow;
    const int sub = threadIdx.x / kLanesPerRow;
    const int col = (threadIdx.x - sub * kLanesPerRow) * 8;
    const long long row = (long long)blockIdx.x * kRowsPerWg + sub;
    if (row >= a.rows) return;

    float l[kMergeMaxParts];
    f32x4 x[kMergeMaxParts][2];
#pragma unroll
    for (int i = 0; i < kMergeMaxParts; ++i)
        if (i < a.n) {
            l[i] = a.lse_part[i][row];
            const f32x4* const src = (const f32x4*)((const float*)a.o_part[i] + row * D + col);
            x[i][0] = src[0], x[i][1] = src[1];
        }

    const int head = (int)(row / a.Sq);
    const int s = (int)(row - (long long)head * a.Sq);
    T* const dst = (T*)a.o + layout_head_off(a.o_bs, a.o_hs, a.hpb, head) + (size_t)s * a.o_rs + col;
    V8 out;
    if (a.n == 1) {   // one part: its rows rounded once, its lse as it is (no weight, no division)
#pragma unroll
        for (int j = 0; j < 8; ++j) out[j] = E::from_float(x[0][j >> 2][j & 3]);
        *(V8*)dst = out;
        if (a.lse && col == 0) a.lse[row] = l[0];
        return;
    }

    float m = -INFINITY;
#pragma unroll
    for (int i = 0; i < kMergeMaxParts; ++i)
        if (i < a.n) m = fmaxf(m, l[i]);
    float acc[8], sw = 0.f;
#pragma unroll
    for (int j = 0; j < 8; ++j) acc[j] = 0.f;
    bool first = true;
#pragma unroll
    for (int i = 0; i < kMergeMaxParts; ++i)
        if (i < a.n) {
            const float w = (l[i] == -INFINITY) ? 0.f : __builtin_amdgcn_exp2f((l[i] - m) * 1.4426950408889634f);
            if (w > 0.f) {   // (false for a NaN too)
                sw += w;
#pragma unroll
                for (int j = 0; j < 8; ++j) {
                    const float xf = x[i][j >> 2][j & 3];
                    acc[j] = first ? w * xf : fmaf(w, xf, acc[j]);   // the first part sets (a -0 stays one), the others add
                }
                first = false;
            }
        }
    const float inv = sw > 0.f ? 1.f / sw : 0.f;
#pragma unroll
    for (int j = 0; j < 8; ++j) out[j] = E::from_float(acc[j] * inv);
    *(V8*)dst = out;
    if (a.lse && col == 0) a.lse[row] = sw > 0.f ? m + 0.6931471805599453f * __builtin_amdgcn_logf(sw) : -INFINITY;
}

}  // namespace svg

using namespace svg;

// the checks and the launch of both entries; F32: the parts are fp32 rows (merge_states_f32_kernel), `dtype` is that of o either way
template <bool F32>
static int merge_states_launch(const void* const* o_parts, const float* const* lse_parts, int32_t n_parts, void* o, float* lse, int32_t BH,
                               int32_t Sq, int32_t D, int32_t dtype, const svg_attn_layout_t* layout, void* stream) {
    if (!o_parts || !lse_parts || !o || n_parts < 1 || n_parts > kMergeMaxParts || BH <= 0 || Sq <= 0 || D <= 0) return SVG_ERR_BAD_ARG;
    for (int i = 0; i < n_parts; ++i)
        if (!o_parts[i] || !lse_parts[i]) return SVG_ERR_BAD_ARG;
    if (D != 64 && D != 128) return SVG_ERR_UNSUPPORTED;
    if (check_rows(Sq, D) != SVG_OK || (int64_t)BH * Sq * D >= (1ll << 40)) return SVG_ERR_UNSUPPORTED;
    for (int i = 0; i < n_parts; ++i)
        if (((size_t)o_parts[i] & 15) != 0) return SVG_ERR_UNSUPPORTED;
    AttnLayout lay = contiguous_layout(BH, BH, Sq, Sq, D);
    if (layout) {   // of the caller's layout only heads_per_batch and the o strides are read; they pass the checks of every *_strided entry
        svg_attn_layout_t abi = *layout;
        const int hpb = abi.heads_per_batch > 0 ? abi.heads_per_batch : 1;
        abi.kv_heads_per_batch = 0;
        abi.q = abi.k = abi.v = {(int64_t)hpb * Sq * D, (int64_t)Sq * D, D};
        if (const int rc = layout_from_abi(&abi, BH, BH, Sq, Sq, D, o, o, o, o, lay); rc != SVG_OK) return rc;
    } else if (((size_t)o & 15) != 0) {
        return SVG_ERR_UNSUPPORTED;
    }
    return dispatch_td(dtype, D, [&](auto t, auto d) -> int {
        using T = decltype(t);
        constexpr int kD = decltype(d)::value;
        MergeArgs a{};
        for (int i = 0; i < n_parts; ++i) a.o_part[i] = o_parts[i], a.lse_part[i] = lse_parts[i];
        a.o = o, a.lse = lse, a.rows = (long long)BH * Sq, a.n = n_parts, a.Sq = Sq;
        a.hpb = lay.hpb_q, a.o_rs = lay.o_rs, a.o_bs = lay.o_bs, a.o_hs = lay.o_hs;
        constexpr int kRowsPerWg = kMergeThreads / (kD / 8);
        const long long n_wg = (a.rows + kRowsPerWg - 1) / kRowsPerWg;
        if constexpr (F32) hipLaunchKernelGGL((merge_states_f32_kernel<T, kD>), dim3((unsigned)n_wg), dim3(kMergeThreads), 0, (hipStream_t)stream, a);
        else hipLaunchKernelGGL((merge_states_kernel<T, kD>), dim3((unsigned)n_wg), dim3(kMergeThreads), 0, (hipStream_t)stream, a);
        return launch_status();
    });
}

extern "C" int svg_merge_attention_states(const void* const* o_parts, const float* const* lse_parts, int32_t n_parts, void* o, float* lse,
                                          int32_t BH, int32_t Sq, int32_t D, int32_t dtype, const svg_attn_layout_t* layout, void* stream) {
    return merge_states_launch<false>(o_parts, lse_parts, n_parts, o, lse, BH, Sq, D, dtype, layout, stream);
}

extern "C" int svg_merge_attention_states_f32(const float* const* o_parts, const float* const* lse_parts, int32_t n_parts, void* o, float* lse,
                                              int32_t BH, int32_t Sq, int32_t D, int32_t dtype, const svg_attn_layout_t* layout, void* stream) {
    return merge_states_launch<true>((const void* const*)o_parts, lse_parts, n_parts, o, lse, BH, Sq, D, dtype, layout, stream);
}

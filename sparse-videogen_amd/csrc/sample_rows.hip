// Quality probe (include/svg_attn_sample_rows.h): DENSE attention of R <= 64 sampled query rows per head — the fp32 output row and the
// row log-sum-exp — so that a sparse layer-call can be set against the truth on those rows: kept mass exp(lse_sparse - lse_dense) and the
// output error o_sparse - o_dense (svg/models/_core.py sparse_quality).
//
// The shape is "few rows x very long key set", the shape of the online profiler (profiler.hip), and the kernel stands on the pieces of its
// second form: grid = (BH, key chunks), one workgroup = 4 waves x 16 sampled rows on v_mfma_f32_16x16x32, K / V tiles of 64 keys staged by
// LDS-DMA in two stages (KvImage16, lds_dma16_kv), S^T = K Q^T so that a lane owns query rows and its score accumulators are its P
// fragment.  What differs: ONE output (16 + 16 MFMAs per tile and wave at head_dim 128, no masks' selections, no class table, no row
// ranking — the rows keep their order), the probabilities against the row's own running maximum (no bias: nothing shares the reference), the
// row sum in fp32 from the unrounded probabilities (the log-sum-exp is the product here, not a by-product), and the two key segments of
// dense_attention's valid_len.  K and V of a head are read once per call.
//   * the keys a row sees are [seg_lo, seg_hi) by INDEX: a key row behind S is never loaded (the request reads row 0 in its place) and its
//     score is replaced by -inf whatever it holds;
//   * a lane with r >= R reads row 0 and stores nothing;
//   * a chunk without a key of a row's segment leaves (O, m, l) = (0, -inf, 0): weight 0 in the merge, no exponential of inf - inf anywhere.
// sample_rows_combine_kernel merges the chunks of a row in chunk order (the bits do not depend on timing), normalises, writes o32 and lse.
#include "attn_core.h"
#include "attn_m16.h"

namespace svg {

constexpr int kSampleMaxRows = 64;

template <typename T>
struct SampleRowsParams {
    const T* q;
    const T* k;
    const T* v;
    const int64_t* rows;
    int S, BH, R, n_chunks, tiles_per_chunk;
    int valid_len;      // 0: every row sees [0, S); otherwise rows < valid_len see [0, valid_len), the others [valid_len, S)
    float scale_log2;   // sm_scale * log2(e)
    AttnLayout lay;     // strides of q, k, v
    float* part;        // [BH][n_chunks][R][D + 4]: O (un-normalised), m (log2 domain), l, two unused words
};
struct SampleRowsAccess : LayoutAccess<SampleRowsAccess> {};

// the chunk count of the online profiler (prof_chunks of profiler.hip): one round of two workgroups per CU, at most a tile per chunk, 64
static int sample_rows_chunks(int BH, int S) {
    const int ntiles = (S + kBN - 1) / kBN;
    int n = (2 * kNumCU) / BH;
    n = n < 1 ? 1 : n;
    n = n > ntiles ? ntiles : n;
    n = n > 64 ? 64 : n;
    return n;
}

// kWithV = false (svg_sample_dense_lse, include/svg_attn_adaptive_top_p.h): the K-only half — no V request, no PV MFMAs, no O accumulators,
// one LDS image per stage; the partial of a row is (m, l) alone, [BH][n_chunks][R][2].  Everything the log-sum-exp is made of — the tiles,
// the scores, the running maximum, the row sum — is the same statement, so that both forms give the same lse bits.
template <typename T, int D, bool kWithV = true>
__global__ __launch_bounds__(256, 2) void sample_rows_kernel(SampleRowsParams<T> prm) {
    using Acc = SampleRowsAccess;
    using E = Elt<T>;
    using M = Mfma16<T>;
    using V8 = typename E::v8;
    constexpr int KS = D / 32, NDB = D / 16;
    using Img = KvImage16<D>;
    constexpr int kImg = Img::kImg, kStage = kWithV ? Img::kStage : Img::kImg;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int head = blockIdx.x, chunk = blockIdx.y;
    const int tid = threadIdx.x, lane = tid & 63, wave = wave_id();
    const int g4 = lane >> 4, n16 = lane & 15;
    const int ntiles = (prm.S + kBN - 1) / kBN;
    const int t0 = chunk * prm.tiles_per_chunk;
    const int nT = max(0, min(prm.tiles_per_chunk, ntiles - t0));
    const T* __restrict__ qb = Acc::q_at(prm, head);
    const T* __restrict__ kb_ = Acc::k_at(prm, head);
    const T* __restrict__ vb = kWithV ? Acc::v_at(prm, head) : nullptr;

    // this lane's sampled row (rows >= R do not exist: they read row 0 and are never stored) and the keys it sees
    const int r = wave * 16 + n16;
    const bool have = r < prm.R;
    const int qrow = have ? (int)prm.rows[r] : 0;
    const int seg_lo = (prm.valid_len > 0 && qrow >= prm.valid_len) ? prm.valid_len : 0;
    const int seg_hi = (prm.valid_len > 0 && qrow < prm.valid_len) ? prm.valid_len : prm.S;
    V8 qf[KS];
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) qf[ks] = *(const V8*)(qb + (size_t)qrow * Acc::q_rs(prm) + ks * 32 + g4 * 8);

    // ---- LDS-DMA staging: wave w moves key group w (16 keys) of a tile, every 64-byte d-block, K and V ----
    const unsigned lds0 = (unsigned)(size_t)smem;
    const unsigned col_v = Img::col_v(lane);
    const int krow = 16 * wave + (lane >> 2);
    const unsigned k_rsb = (unsigned)Acc::k_rs(prm) * 2u, v_rsb = kWithV ? (unsigned)Acc::v_rs(prm) * 2u : 0u;
    auto dma_tile = [&](int t) {
        const int l = (t0 + t) * kBN + krow;
        const unsigned nphys = (unsigned)(l < prm.S ? l : 0);    // rows behind the keys: row 0 in their place, masked by index below
#pragma unroll
        for (int j = 0; j < D / 32; ++j) {
            const unsigned st = __builtin_amdgcn_readfirstlane(lds0 + (unsigned)((t & 1) * kStage) + (unsigned)(j * (kBN * 64) + wave * 1024));
            const unsigned ko = __umul24(nphys, k_rsb) + ((unsigned)(j * 64) | col_v);
            if constexpr (kWithV) {
                const unsigned vo = __umul24(nphys, v_rsb) + ((unsigned)(j * 64) | col_v);
                lds_dma16_kv<kImg>(st, ko, vo, kb_, vb);
            } else {
                lds_dma16(st, ko, kb_);
            }
        }
    };
    const int k_lane = Img::k_lane(g4, n16);
    const int v_lane0 = Img::v_lane0(g4, n16);
    const int v_lane1 = v_lane0 ^ 32;
    auto kfrag = [&](const char* st, int kblk, int ks) -> V8 { return __builtin_bit_cast(V8, Img::kfrag(st, k_lane, kblk, ks)); };
    auto vfrag = [&](const char* st, int kc, int db) -> V8 { return __builtin_bit_cast(V8, Img::vfrag(st, v_lane0, v_lane1, kc, db)); };

    // softmax state of the lane's row: running maximum (log2 domain, the same in the four lanes of a row), the lane's share of the row sum
    float m_run = -INFINITY, l_run = 0.f;
    f32x4 acc[NDB];
#pragma unroll
    for (int db = 0; db < NDB; ++db) acc[db] = f32x4{0.f, 0.f, 0.f, 0.f};
    const float c_log2 = prm.scale_log2;

    if (nT > 0) dma_tile(0);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    // (the q fragments are consumed here as far as the compiler's counter bookkeeping goes: left pending into the loop, their first use there
    //  gets an s_waitcnt vmcnt(0) — which waits for the tile prefetch just issued; profile16_kernel)
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) asm volatile("" : "+v"(qf[ks]));
    __syncthreads();
    for (int t = 0; t < nT; ++t) {
        if (t + 1 < nT) dma_tile(t + 1);      // into the stage every wave finished reading one barrier ago
        const char* st = smem + (t & 1) * kStage;
        const int k0 = (t0 + t) * kBN;
        const bool sees = (k0 < seg_hi) & (k0 + kBN > seg_lo);
        const bool inside = (k0 >= seg_lo) & (k0 + kBN <= seg_hi);
        if (__any(sees)) {     // (wave-uniform: a tile wholly in the other segment of all sixteen rows costs the wave nothing)
            // ---- S^T = K Q^T (lane: query row n16, keys 16 b + 4 g4 + [0, 4)) ----
            f32x4 sc[4];
#pragma unroll
            for (int b = 0; b < 4; ++b) sc[b] = f32x4{0.f, 0.f, 0.f, 0.f};
            {   // K fragments one 32-wide d-block ahead
                V8 kf[2][4];
#pragma unroll
                for (int b = 0; b < 4; ++b) kf[0][b] = kfrag(st, b, 0);
#pragma unroll
                for (int ks = 0; ks < KS; ++ks) {
                    if (ks + 1 < KS) {
#pragma unroll
                        for (int b = 0; b < 4; ++b) kf[(ks + 1) & 1][b] = kfrag(st, b, ks + 1);
                    }
                    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
                    for (int b = 0; b < 4; ++b) sc[b] = M::mfma(kf[ks & 1][b], qf[ks], sc[b]);
                    __builtin_amdgcn_sched_barrier(0);
                }
            }
            // scores in the log2 domain; the keys outside the row's segment (and behind S) by index
#pragma unroll
            for (int b = 0; b < 4; ++b) sc[b] *= c_log2;
            if (!__all(inside)) {
#pragma unroll
                for (int b = 0; b < 4; ++b)
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
                        const int key = k0 + 16 * b + 4 * g4 + j;
                        sc[b][j] = ((key >= seg_lo) & (key < seg_hi)) ? sc[b][j] : -INFINITY;
                    }
            }
            float mx = fmaxf(fmaxf(sc[0][0], sc[0][1]), fmaxf(sc[0][2], sc[0][3]));
#pragma unroll
            for (int b = 1; b < 4; ++b) mx = fmaxf(fmaxf(mx, sc[b][0]), fmaxf(fmaxf(sc[b][1], sc[b][2]), sc[b][3]));
            // the running maximum moves in a few tiles per row: only then the cross-lane reduction and the rescaling (a step of 0 is exact)
            if (__any(mx > m_run)) {
                const float m_new = fmaxf(m_run, quad_group_max(mx));
                const float alpha = (m_new == -INFINITY) ? 1.f : __builtin_amdgcn_exp2f(m_run - m_new);   // (-inf -> finite: 2^-inf = 0)
                m_run = m_new;
                l_run *= alpha;
                if constexpr (kWithV) {
#pragma unroll
                    for (int db = 0; db < NDB; ++db)
#pragma unroll
                        for (int j = 0; j < 4; ++j) acc[db][j] *= alpha;
                }
            }
            const float m_use = (m_run == -INFINITY) ? 0.f : m_run;   // a row that has seen no key yet: every p is 2^-inf = 0
            // ---- probabilities: the P fragment is the lane's score accumulators of key blocks 2 kc, 2 kc + 1 ----
            V8 pf[2];
#pragma unroll
            for (int b = 0; b < 4; ++b)
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const float p = __builtin_amdgcn_exp2f(sc[b][j] - m_use);
                    l_run += p;
                    if constexpr (kWithV) pf[b >> 1][4 * (b & 1) + j] = E::from_float(p);
                }
            // ---- O^T += V^T P^T: V^T fragments in groups of four 16-wide d-blocks, two groups in flight ----
            if constexpr (kWithV) {
                constexpr int G = 4, NG = 2 * NDB / G;
                V8 vf[2][G];
#pragma unroll
                for (int i = 0; i < G; ++i) vf[0][i] = vfrag(st, 0, i);
#pragma unroll
                for (int g = 0; g < NG; ++g) {
                    if (g + 1 < NG) {
#pragma unroll
                        for (int i = 0; i < G; ++i) vf[(g + 1) & 1][i] = vfrag(st, ((g + 1) * G + i) / NDB, ((g + 1) * G + i) % NDB);
                    }
                    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
                    for (int i = 0; i < G; ++i) acc[(g * G + i) % NDB] = M::mfma(vf[g & 1][i], pf[(g * G + i) / NDB], acc[(g * G + i) % NDB]);
                    __builtin_amdgcn_sched_barrier(0);
                }
            }
        }
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();
    }
    // ---- the chunk's partial of the row: the four lanes of a row hold 4 + 4 + 4 + 4 keys of every 16-key block ----
    const float l_tot = quad_group_sum(l_run);
    if constexpr (!kWithV) {
        if (have && g4 == 0) {
            float2* dst = (float2*)prm.part + ((size_t)head * prm.n_chunks + chunk) * prm.R + r;
            *dst = float2{m_run, l_tot};
        }
    } else if (have) {
        float* dst = prm.part + (((size_t)head * prm.n_chunks + chunk) * prm.R + r) * (D + 4);
#pragma unroll
        for (int db = 0; db < NDB; ++db) *(f32x4*)(dst + 16 * db + 4 * g4) = acc[db];
        if (g4 == 0) {
            dst[D] = m_run;
            dst[D + 1] = l_tot;
        }
    }
}

// grid = (R, BH), block = D: element d of sampled row r of head h.  M = max_c m_c, w_c = 2^(m_c - M) (0 for a chunk without keys),
// L = sum_c l_c w_c and O = sum_c O_c w_c in chunk order; o32 = O / L, lse = ln 2 (M + log2 L).  A row no chunk gave a key (not
// reachable through the entry: both segments of valid_len hold keys) gets zeros and -inf.
template <int D>
__global__ __launch_bounds__(D) void sample_rows_combine_kernel(const float* __restrict__ part, float* __restrict__ o32,
                                                                float* __restrict__ lse, int R, int n_chunks) {
    const int r = blockIdx.x, h = blockIdx.y, d = threadIdx.x;
    const size_t cs = (size_t)R * (D + 4);
    const float* base = part + ((size_t)h * n_chunks * R + r) * (D + 4);
    float Mx = -INFINITY;
    for (int c = 0; c < n_chunks; ++c) Mx = fmaxf(Mx, base[c * cs + D]);
    float L = 0.f, O = 0.f;
    for (int c = 0; c < n_chunks; ++c) {
        const float mc = base[c * cs + D];
        const float w = (mc == -INFINITY) ? 0.f : exp2f(mc - Mx);
        L += base[c * cs + D + 1] * w;
        O += base[c * cs + d] * w;
    }
    const bool seen = L > 0.f;
    o32[((size_t)h * R + r) * D + d] = seen ? O / L : 0.f;
    if (d == 0) lse[(size_t)h * R + r] = seen ? 0.6931471805599453f * (Mx + log2f(L)) : -INFINITY;
}

// The combine of the K-only form: grid = BH, block = 64, thread r = sampled row r.  M, the weights and L as above.
__global__ __launch_bounds__(kSampleMaxRows) void sample_lse_combine_kernel(const float2* __restrict__ part, float* __restrict__ lse, int R,
                                                                            int n_chunks) {
    const int r = threadIdx.x, h = blockIdx.x;
    if (r >= R) return;
    const float2* base = part + (size_t)h * n_chunks * R + r;
    float Mx = -INFINITY;
    for (int c = 0; c < n_chunks; ++c) Mx = fmaxf(Mx, base[(size_t)c * R].x);
    // L with the arithmetic sample_rows_combine_kernel is COMPILED to, stated here and fenced so that it stays: the file is built with fast
    // math, and hipcc vectorises that kernel's chunk loop by two — the even chunks and the odd chunks are summed apart by fused
    // multiply-adds, the two sums added, an odd last chunk fused in behind them.  Still a fixed order, a function of n_chunks alone; the
    // same source without the fence leaves the choice to the compiler, kernel by kernel, and the two lse would differ in the last bit.
    float L;
    {
#pragma clang fp reassociate(off) contract(off)
        auto weighted = [&](int c, float acc) {
            const float2 ml = base[(size_t)c * R];
            const float w = (ml.x == -INFINITY) ? 0.f : exp2f(ml.x - Mx);
            return __builtin_fmaf(ml.y, w, acc);
        };
        float L0 = 0.f, L1 = 0.f;
        for (int c = 0; c + 1 < n_chunks; c += 2) {
            L0 = weighted(c, L0);
            L1 = weighted(c + 1, L1);
        }
        L = L0 + L1;
        if (n_chunks & 1) L = weighted(n_chunks - 1, L);
    }
    lse[(size_t)h * R + r] = (L > 0.f) ? 0.6931471805599453f * (Mx + log2f(L)) : -INFINITY;
}

template <typename T, int D>
static int run_sample_lse(const void* q, const void* k, const int64_t* rows, int R, int BH, int S, float sm_scale, int valid_len, float* lse,
                          void* ws, const AttnLayout* lay, hipStream_t st) {
    SampleRowsParams<T> p;
    p.q = (const T*)q, p.k = (const T*)k, p.v = nullptr;
    p.rows = rows;
    p.S = S, p.BH = BH, p.R = R;
    p.n_chunks = sample_rows_chunks(BH, S);
    const int ntiles = (S + kBN - 1) / kBN;
    p.tiles_per_chunk = (ntiles + p.n_chunks - 1) / p.n_chunks;
    p.valid_len = (valid_len <= 0 || valid_len >= S) ? 0 : valid_len;
    p.scale_log2 = sm_scale * 1.4426950408889634f;
    p.lay = lay ? *lay : contiguous_layout(BH, BH, S, S, D);
    p.part = (float*)ws;
    constexpr int lds = 2 * KvImage16<D>::kImg;    // two stages of a K image
    auto kern = sample_rows_kernel<T, D, false>;
    if (const int rc = configure_lds((const void*)kern, lds); rc != SVG_OK) return rc;
    hipLaunchKernelGGL(kern, dim3(BH, p.n_chunks), dim3(256), lds, st, p);
    hipLaunchKernelGGL(sample_lse_combine_kernel, dim3(BH), dim3(kSampleMaxRows), 0, st, (const float2*)ws, lse, R, p.n_chunks);
    return launch_status();
}

template <typename T, int D>
static int run_sample_rows(const void* q, const void* k, const void* v, const int64_t* rows, int R, int BH, int S, float sm_scale, int valid_len,
                           float* o32, float* lse, void* ws, const AttnLayout* lay, hipStream_t st) {
    SampleRowsParams<T> p;
    p.q = (const T*)q, p.k = (const T*)k, p.v = (const T*)v;
    p.rows = rows;
    p.S = S, p.BH = BH, p.R = R;
    p.n_chunks = sample_rows_chunks(BH, S);
    const int ntiles = (S + kBN - 1) / kBN;
    p.tiles_per_chunk = (ntiles + p.n_chunks - 1) / p.n_chunks;
    p.valid_len = (valid_len <= 0 || valid_len >= S) ? 0 : valid_len;
    p.scale_log2 = sm_scale * 1.4426950408889634f;
    p.lay = lay ? *lay : contiguous_layout(BH, BH, S, S, D);
    p.part = (float*)ws;
    constexpr int lds = 2 * KvImage16<D>::kStage;    // two stages of a K and a V image
    auto kern = sample_rows_kernel<T, D>;
    if (const int rc = configure_lds((const void*)kern, lds); rc != SVG_OK) return rc;
    hipLaunchKernelGGL(kern, dim3(BH, p.n_chunks), dim3(256), lds, st, p);
    hipLaunchKernelGGL((sample_rows_combine_kernel<D>), dim3(R, BH), dim3(D), 0, st, (const float*)ws, o32, lse, R, p.n_chunks);
    return launch_status();
}

}  // namespace svg

using namespace svg;

// An upper bound of BH * chunks * R rows of D + 4 words that grows with every argument (BH * sample_rows_chunks(BH, S) itself does not:
// 512 / BH rounds down).
extern "C" size_t svg_sample_dense_rows_workspace_bytes(int32_t BH, int32_t R, int32_t D, int32_t S) {
    if (BH <= 0 || R <= 0 || D <= 0 || S <= 0) return 0;
    const size_t ntiles = ((size_t)S + kBN - 1) / kBN;
    const size_t per_head = ntiles < 64 ? ntiles : 64;
    const size_t round = (size_t)BH > 2 * kNumCU ? (size_t)BH : 2 * kNumCU;
    const size_t terms = (size_t)BH * per_head < round ? (size_t)BH * per_head : round;
    return terms * (size_t)R * ((size_t)D + 4) * sizeof(float);
}

extern "C" int svg_sample_dense_rows(const void* q, const void* k, const void* v, const int64_t* rows, int32_t R, int32_t BH, int32_t S,
                                     int32_t D, int32_t dtype, float sm_scale, int32_t valid_len, float* o32, float* lse, void* workspace,
                                     size_t workspace_bytes, const svg_attn_layout_t* abi_layout, void* stream) {
    if (!q || !k || !v || !rows || !o32 || !lse || !workspace) return SVG_ERR_BAD_ARG;
    if (R < 1 || R > kSampleMaxRows || BH <= 0 || S <= 0) return SVG_ERR_BAD_ARG;
    if (S >= (1 << 24) || (D > 0 && check_rows(S, D) != SVG_OK)) return SVG_ERR_UNSUPPORTED;
    if (workspace_bytes < svg_sample_dense_rows_workspace_bytes(BH, R, D, S)) return SVG_ERR_WORKSPACE;
    if (((size_t)workspace & 15) != 0) return SVG_ERR_UNSUPPORTED;    // (the partials are stored four words at a time)
    AttnLayout lay_storage;
    const AttnLayout* lay = nullptr;
    if (abi_layout) {   // (o is not a tensor of this call: q stands in for the alignment test)
        svg_attn_layout_t a = *abi_layout;
        a.o = a.q;
        if (const int rc = layout_from_abi(&a, BH, BH, S, S, D, q, k, v, q, lay_storage); rc != SVG_OK) return rc;
        lay = &lay_storage;
    }
    return dispatch_td(dtype, D, [&](auto t, auto d) {
        return run_sample_rows<decltype(t), decltype(d)::value>(q, k, v, rows, R, BH, S, sm_scale, valid_len, o32, lse, workspace, lay,
                                                                (hipStream_t)stream);
    });
}

// include/svg_attn_adaptive_top_p.h.  The bound of svg_sample_dense_rows_workspace_bytes with two words per row.
extern "C" size_t svg_sample_dense_lse_workspace_bytes(int32_t BH, int32_t R, int32_t S) {
    if (BH <= 0 || R <= 0 || S <= 0) return 0;
    const size_t ntiles = ((size_t)S + kBN - 1) / kBN;
    const size_t per_head = ntiles < 64 ? ntiles : 64;
    const size_t round = (size_t)BH > 2 * kNumCU ? (size_t)BH : 2 * kNumCU;
    const size_t terms = (size_t)BH * per_head < round ? (size_t)BH * per_head : round;
    return ((terms * (size_t)R * 2 * sizeof(float)) + 15) & ~(size_t)15;
}

extern "C" int svg_sample_dense_lse(const void* q, const void* k, const int64_t* rows, int32_t R, int32_t BH, int32_t S, int32_t D,
                                    int32_t dtype, float sm_scale, int32_t valid_len, float* lse, void* workspace, size_t workspace_bytes,
                                    const svg_attn_layout_t* abi_layout, void* stream) {
    if (!q || !k || !rows || !lse || !workspace) return SVG_ERR_BAD_ARG;
    if (R < 1 || R > kSampleMaxRows || BH <= 0 || S <= 0) return SVG_ERR_BAD_ARG;
    if (S >= (1 << 24) || (D > 0 && check_rows(S, D) != SVG_OK)) return SVG_ERR_UNSUPPORTED;
    if (workspace_bytes < svg_sample_dense_lse_workspace_bytes(BH, R, S)) return SVG_ERR_WORKSPACE;
    if (((size_t)workspace & 15) != 0) return SVG_ERR_UNSUPPORTED;
    AttnLayout lay_storage;
    const AttnLayout* lay = nullptr;
    if (abi_layout) {   // (v and o are not tensors of this call: k and q stand in for them)
        svg_attn_layout_t a = *abi_layout;
        a.v = a.k;
        a.o = a.q;
        if (const int rc = layout_from_abi(&a, BH, BH, S, S, D, q, k, k, q, lay_storage); rc != SVG_OK) return rc;
        lay = &lay_storage;
    }
    return dispatch_td(dtype, D, [&](auto t, auto d) {
        return run_sample_lse<decltype(t), decltype(d)::value>(q, k, rows, R, BH, S, sm_scale, valid_len, lse, workspace, lay,
                                                               (hipStream_t)stream);
    });
}

// Centroid tail of SVG2 (include/svg_attn_centroid_tail.h): what the top-p block map leaves out, estimated row by row.  Every key cluster c
// the map does not select for a block-row enters that block-row's rows as ONE pseudo key (kbar_c, vbar_c) with the weight n_c:
//     s_c = sm_scale q . kbar_c + ln n_c,   lse = ln sum_c exp(s_c),   o = sum_c exp(s_c - lse) vbar_c
// — a part for svg_merge_attention_states beside the sparse launch's (o, lse).  Two entries:
//   svg_cluster_means               kbar / vbar: the exact means of the clusters of a k-means call (Jensen's bound needs the mean, and the
//                                   stored centroids may be one update away from the labels).  HBM-bound: x is read once, run by run of the
//                                   sorted indices, as kmeans_update_kernel (kmeans.hip) reads it.
//   svg_centroid_tail_attention_lse dense attention of every block-row's rows over the KC centroids of its head with an additive bias per
//                                   key.  It stands on the pieces of sample_rows.hip: one workgroup = 4 waves x 16 query rows on
//                                   v_mfma_f32_16x16x32, centroid tiles of 64 keys staged by LDS-DMA in two stages (KvImage16,
//                                   lds_dma16_kv), S^T = K Q^T so that a lane owns query rows and its score accumulators are its P fragment,
//                                   online softmax against the row's running maximum, fp32 accumulators.
// The mask is uniform over a workgroup (no two block-rows share one), so mask and bias are ONE fp32 vector of KC entries in LDS, built once
// per workgroup: -inf where the map selects the cluster, where the cluster is empty and behind KC, log2 n_c elsewhere — one add per score.
// A tile whose 64 entries are all -inf costs a wave four LDS reads and a vote.  Every block-row of a head streams the same 2 x KC x 256 bytes
// of kbar / vbar, which live in L2; the launch is about 5 % of the layer's FLOPs at Wan 720p, so the schedule is the plain one: every wave
// runs QK -> softmax -> PV per tile, one barrier per tile.
#include <algorithm>

#include "attn_core.h"
#include "attn_m16.h"
#include "varblock_policy.h"

namespace svg {

// ---- cluster means: grid = (groups, B), block = 256 = 16 row slots x 16 lanes (D = 128) / 32 x 8 (D = 64).  A workgroup owns a run of
// consecutive clusters of its batch: the offset of the first one is one block-wide sum over counts, the others follow by addition.  Per
// cluster: slot s sums rows s, s + SLOTS, ... of the cluster's run of sorted_idx in fp32 (four rows in flight), the slots are added in
// slot order, the sum is divided by the count and rounded ONCE.
template <typename T, int D>
__global__ __launch_bounds__(256) void cluster_means_kernel(const T* __restrict__ x, const int32_t* __restrict__ sorted_idx,
                                                            const int32_t* __restrict__ counts, T* __restrict__ means, int N, int K,
                                                            int per_wg, int hpb, long long x_bs, long long x_hs, int x_rs) {
    constexpr int LPR = D / 8;
    constexpr int SLOTS = 256 / LPR;
    __shared__ float red[SLOTS][D + 4];
    __shared__ int wsum[4];
    using V8 = typename Elt<T>::v8;
    const int b = blockIdx.y, tid = threadIdx.x;
    const int slot = tid / LPR, li = tid - slot * LPR;
    const int k_lo = blockIdx.x * per_wg, k_hi = min(k_lo + per_wg, K);
    if (k_lo >= K) return;
    const T* xb = x + layout_head_off(x_bs, x_hs, hpb, b);
    const int32_t* cnt_b = counts + (size_t)b * K;
    const int32_t* sidx_b = sorted_idx + (size_t)b * N;
    // rows in front of cluster k_lo
    int s = 0;
    for (int i = tid; i < k_lo; i += 256) s += max(cnt_b[i], 0);
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) s += __shfl_xor(s, o);
    if ((tid & 63) == 0) wsum[tid >> 6] = s;
    __syncthreads();
    int start = wsum[0] + wsum[1] + wsum[2] + wsum[3];
    for (int k = k_lo; k < k_hi; ++k) {
        const int cnt_raw = cnt_b[k];
        // (a run never leaves [0, N): counts that do not add up to N would otherwise index behind sorted_idx)
        const int cnt = max(0, min(cnt_raw, N - start));
        const int32_t* sidx = sidx_b + start;
        float acc[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) acc[j] = 0.f;
        {
#pragma clang fp reassociate(off)
            int r = slot;
            for (; r + 3 * SLOTS < cnt; r += 4 * SLOTS) {
                int row[4];
                V8 v[4];
#pragma unroll
                for (int u = 0; u < 4; ++u) row[u] = sidx[r + u * SLOTS];
#pragma unroll
                for (int u = 0; u < 4; ++u) v[u] = *(const V8*)(xb + (size_t)min((unsigned)row[u], (unsigned)(N - 1)) * x_rs + li * 8);
#pragma unroll
                for (int u = 0; u < 4; ++u)
#pragma unroll
                    for (int j = 0; j < 8; ++j) acc[j] += Elt<T>::to_float(v[u][j]);
            }
            for (; r < cnt; r += SLOTS) {
                const V8 w = *(const V8*)(xb + (size_t)min((unsigned)sidx[r], (unsigned)(N - 1)) * x_rs + li * 8);
#pragma unroll
                for (int j = 0; j < 8; ++j) acc[j] += Elt<T>::to_float(w[j]);
            }
        }
#pragma unroll
        for (int j = 0; j < 8; ++j) red[slot][li * 8 + j] = acc[j];
        __syncthreads();
        if (tid < D) {
            float sum = 0.f;
            {
#pragma clang fp reassociate(off)
                for (int sl = 0; sl < SLOTS; ++sl) sum += red[sl][tid];   // fixed order -> deterministic
            }
            means[((size_t)b * K + k) * D + tid] = Elt<T>::from_float(cnt > 0 ? sum / (float)cnt : 0.f);
        }
        __syncthreads();   // red is written again by the next cluster
        start += max(cnt_raw, 0);
    }
}

// ---- row_start[h][a] = sum of q_sizes[h][0 .. a): the first sorted position of block-row a.  grid = H, block = 256: thread t owns a run of
// consecutive block-rows, thread 0 scans the 256 run sums.
__global__ __launch_bounds__(256) void tail_row_start_kernel(const int32_t* __restrict__ q_sizes, int32_t* __restrict__ row_start, int QB) {
    __shared__ int part[256];
    const int tid = threadIdx.x;
    const int32_t* qs = q_sizes + (size_t)blockIdx.x * QB;
    int32_t* out = row_start + (size_t)blockIdx.x * QB;
    const int per = (QB + 255) / 256;
    const int lo = min(tid * per, QB), hi = min(lo + per, QB);
    int s = 0;
    for (int i = lo; i < hi; ++i) s += max(qs[i], 0);
    part[tid] = s;
    __syncthreads();
    if (tid == 0) {
        int run = 0;
        for (int i = 0; i < 256; ++i) {
            const int t = part[i];
            part[i] = run;
            run += t;
        }
    }
    __syncthreads();
    int run = part[tid];
    for (int i = lo; i < hi; ++i) {
        out[i] = run;
        run += max(qs[i], 0);
    }
}

template <typename T>
struct CentroidTailParams {
    const T* q;
    const T* kbar;
    const T* vbar;
    T* o;
    float* lse;
    const uint8_t* block_map;
    const int32_t* q_sizes;
    const int32_t* k_sizes;
    const int32_t* q_row_idx;   // nullptr: sorted position = row
    const int32_t* row_start;   // [H][QB], tail_row_start_kernel
    int Sq, KC, QB, map_cols, nT;
    float scale_log2;           // sm_scale * log2(e)
    int hpb_q, q_rs;
    long long q_bs, q_hs;
};

constexpr int kTailRows = 64;   // query rows per workgroup pass: 4 waves x 16

// grid = (QB, Z, H): workgroup (a, z, h) runs the 64-row sub-tiles z, z + Z, ... of block-row a of head h
template <typename T>
__global__ __launch_bounds__(256, 2) void centroid_tail_kernel(CentroidTailParams<T> prm) {
    constexpr int D = 128;
    using E = Elt<T>;
    using M = Mfma16<T>;
    using V8 = typename E::v8;
    using V4 = typename E::v4;
    constexpr int KS = D / 32, NDB = D / 16;
    using Img = KvImage16<D>;
    constexpr int kImg = Img::kImg, kStage = Img::kStage;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    float* const bias = (float*)(smem + 2 * kStage);   // [nT * 64], log2 domain
    const int a = blockIdx.x, head = blockIdx.z;
    const int tid = threadIdx.x, lane = tid & 63, wave = wave_id();
    const int g4 = lane >> 4, n16 = lane & 15;
    const int nT = prm.nT;

    const int start = prm.row_start[(size_t)head * prm.QB + a];
    // (the block-row ends where the head ends: sizes that add up to more than Sq index no row behind it)
    const int qsz = min(prm.q_sizes[(size_t)head * prm.QB + a], prm.Sq - start);
    const int nsub = (qsz + kTailRows - 1) / kTailRows;
    if ((int)blockIdx.y >= nsub) return;   // (workgroup-uniform, in front of every barrier)

    // ---- mask and bias of the block-row, once ----
    {
        const uint8_t* mrow = prm.block_map + ((size_t)head * prm.QB + a) * prm.map_cols;
        const int32_t* ks = prm.k_sizes + (size_t)head * prm.KC;
        for (int c = tid; c < nT * kBN; c += 256) {
            float bv = -INFINITY;
            if (c < prm.KC) {
                const int n = ks[c];
                if (mrow[c] == 0 && n > 0) bv = __builtin_amdgcn_logf((float)n);   // v_log_f32: log2
            }
            bias[c] = bv;
        }
    }

    const T* __restrict__ qb = prm.q + layout_head_off(prm.q_bs, prm.q_hs, prm.hpb_q, head);
    const T* __restrict__ kb_ = prm.kbar + (size_t)head * prm.KC * D;
    const T* __restrict__ vb = prm.vbar + (size_t)head * prm.KC * D;

    // ---- LDS-DMA staging: wave w moves key group w (16 keys) of a tile, every 64-byte d-block, K and V ----
    const unsigned lds0 = (unsigned)(size_t)smem;
    const unsigned col_v = Img::col_v(lane);
    const int krow = 16 * wave + (lane >> 2);
    auto dma_tile = [&](int t) {
        const int l = t * kBN + krow;
        const unsigned nphys = (unsigned)(l < prm.KC ? l : 0);   // rows behind the centroids: row 0 in their place, their bias is -inf
#pragma unroll
        for (int j = 0; j < D / 32; ++j) {
            const unsigned st = __builtin_amdgcn_readfirstlane(lds0 + (unsigned)((t & 1) * kStage) + (unsigned)(j * (kBN * 64) + wave * 1024));
            const unsigned off = nphys * (unsigned)(2 * D) + ((unsigned)(j * 64) | col_v);
            lds_dma16_kv<kImg>(st, off, off, kb_, vb);
        }
    };
    const int k_lane = Img::k_lane(g4, n16);
    const int v_lane0 = Img::v_lane0(g4, n16);
    const int v_lane1 = v_lane0 ^ 32;
    auto kfrag = [&](const char* st, int kblk, int ks) -> V8 { return __builtin_bit_cast(V8, Img::kfrag(st, k_lane, kblk, ks)); };
    auto vfrag = [&](const char* st, int kc, int db) -> V8 { return __builtin_bit_cast(V8, Img::vfrag(st, v_lane0, v_lane1, kc, db)); };
    const float c_log2 = prm.scale_log2;

    for (int sub = blockIdx.y; sub < nsub; sub += gridDim.y) {
        // this lane's row: sorted position start + pos (a position behind the block-row reads its first row and stores nothing)
        const int pos = sub * kTailRows + wave * 16 + n16;
        const bool in_row = pos < qsz;
        const int srow = start + (in_row ? pos : 0);
        int qrow = prm.q_row_idx ? prm.q_row_idx[(size_t)head * prm.Sq + srow] : srow;
        const bool have = in_row && (unsigned)qrow < (unsigned)prm.Sq;   // (an index outside the head is neither read nor written)
        qrow = have ? qrow : 0;
        V8 qf[KS];
#pragma unroll
        for (int ks = 0; ks < KS; ++ks) qf[ks] = *(const V8*)(qb + (size_t)qrow * prm.q_rs + ks * 32 + g4 * 8);

        // softmax state of the lane's row: running maximum (log2 domain, the same in the four lanes of a row), the lane's share of the row sum
        float m_run = -INFINITY, l_run = 0.f;
        f32x4 acc[NDB];
#pragma unroll
        for (int db = 0; db < NDB; ++db) acc[db] = f32x4{0.f, 0.f, 0.f, 0.f};

        dma_tile(0);
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        // (the q fragments count as consumed here: left pending into the loop, their first use would wait for the tile prefetch as well)
#pragma unroll
        for (int ks = 0; ks < KS; ++ks) asm volatile("" : "+v"(qf[ks]));
        __syncthreads();   // (the first pass: the bias vector as well)
        for (int t = 0; t < nT; ++t) {
            if (t + 1 < nT) dma_tile(t + 1);      // into the stage every wave finished reading one barrier ago
            const char* st = smem + (t & 1) * kStage;
            // the lane's 16 bias entries: keys 16 b + 4 g4 + [0, 4) of the tile — the 64 lanes of a wave cover the tile's 64 keys
            f32x4 bs[4];
#pragma unroll
            for (int b = 0; b < 4; ++b) bs[b] = *(const f32x4*)(bias + t * kBN + 16 * b + 4 * g4);
            bool live = false;
#pragma unroll
            for (int b = 0; b < 4; ++b)
#pragma unroll
                for (int j = 0; j < 4; ++j) live |= bs[b][j] != -INFINITY;
            if (__any(live)) {     // (wave-uniform; the same in every wave)
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
                // scores in the log2 domain plus the bias; a masked key is -inf whatever its centroid holds
#pragma unroll
                for (int b = 0; b < 4; ++b)
#pragma unroll
                    for (int j = 0; j < 4; ++j) sc[b][j] = bs[b][j] == -INFINITY ? -INFINITY : fmaf(sc[b][j], c_log2, bs[b][j]);
                float mx = fmaxf(fmaxf(sc[0][0], sc[0][1]), fmaxf(sc[0][2], sc[0][3]));
#pragma unroll
                for (int b = 1; b < 4; ++b) mx = fmaxf(fmaxf(mx, sc[b][0]), fmaxf(fmaxf(sc[b][1], sc[b][2]), sc[b][3]));
                // the running maximum moves in a few tiles per row: only then the cross-lane reduction and the rescaling (a step of 0 is exact)
                if (__any(mx > m_run)) {
                    const float m_new = fmaxf(m_run, quad_group_max(mx));
                    const float alpha = (m_new == -INFINITY) ? 1.f : __builtin_amdgcn_exp2f(m_run - m_new);   // (-inf -> finite: 2^-inf = 0)
                    m_run = m_new;
                    l_run *= alpha;
#pragma unroll
                    for (int db = 0; db < NDB; ++db)
#pragma unroll
                        for (int j = 0; j < 4; ++j) acc[db][j] *= alpha;
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
                        pf[b >> 1][4 * (b & 1) + j] = E::from_float(p);
                    }
                // ---- O^T += V^T P^T: V^T fragments in groups of four 16-wide d-blocks, two groups in flight ----
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
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            __syncthreads();
        }
        // ---- the row: the four lanes of a row hold 4 + 4 + 4 + 4 keys of every 16-key block; lane (g4, n16) holds d 16 db + 4 g4 + [0, 4) ----
        const float l_tot = quad_group_sum(l_run);
        if (have) {
            const float inv = l_tot > 0.f ? 1.f / l_tot : 0.f;   // no key: zeros and -inf
            T* dst = prm.o + ((size_t)head * prm.Sq + qrow) * D + 4 * g4;
#pragma unroll
            for (int db = 0; db < NDB; ++db) {
                V4 w;
#pragma unroll
                for (int j = 0; j < 4; ++j) w[j] = E::from_float(acc[db][j] * inv);
                *(V4*)(dst + 16 * db) = w;
            }
            if (g4 == 0)
                prm.lse[(size_t)head * prm.Sq + qrow] = l_tot > 0.f ? 0.6931471805599453f * (m_run + __builtin_amdgcn_logf(l_tot)) : -INFINITY;
        }
    }
}

static size_t tail_ws_bytes(int H, int QB) { return (((size_t)H * QB * sizeof(int32_t)) + 15) & ~(size_t)15; }

}  // namespace svg

using namespace svg;

extern "C" int svg_cluster_means(const void* x, const svg_tensor_strides_t* strides, int32_t heads_per_batch, const int32_t* sorted_idx,
                                 const int32_t* counts, void* means, int32_t B, int32_t N, int32_t K, int32_t D, int32_t dtype,
                                 void* stream) {
    if (!x || !sorted_idx || !counts || !means || B <= 0 || N <= 0 || K <= 0) return SVG_ERR_BAD_ARG;
    int hpb = B;
    long long bs = (long long)B * N * D, hs = (long long)N * D, rs = D;
    if (strides) {
        if (heads_per_batch <= 0 || B % heads_per_batch != 0) return SVG_ERR_BAD_ARG;
        if (strides->row < D || strides->head < 0 || strides->batch < 0) return SVG_ERR_BAD_ARG;
        hpb = heads_per_batch, bs = strides->batch, hs = strides->head, rs = strides->row;
    }
    if ((D != 64 && D != 128) || (dtype != SVG_DTYPE_BF16 && dtype != SVG_DTYPE_F16)) return SVG_ERR_UNSUPPORTED;
    if (bs % 8 != 0 || hs % 8 != 0 || rs % 8 != 0 || rs >= (1ll << 23) || ((size_t)x & 15) != 0 || ((size_t)means & 15) != 0)
        return SVG_ERR_UNSUPPORTED;
    return dispatch_td(dtype, D, [&](auto t, auto d) -> int {
        using T = decltype(t);
        constexpr int kD = decltype(d)::value;
        // workgroups per batch: three per CU over the whole launch, as svg_kmeans_update (kmeans.hip run_kmeans_update)
        const int groups = std::max(1, std::min(K, (3 * kNumCU + B - 1) / B));
        const int per_wg = (K + groups - 1) / groups;
        hipLaunchKernelGGL((cluster_means_kernel<T, kD>), dim3((K + per_wg - 1) / per_wg, B), dim3(256), 0, (hipStream_t)stream, (const T*)x,
                           sorted_idx, counts, (T*)means, N, K, per_wg, hpb, bs, hs, (int)rs);
        return launch_status();
    });
}

extern "C" size_t svg_centroid_tail_workspace_bytes(int32_t H, int32_t QB, int32_t KC) {
    if (H <= 0 || QB <= 0 || KC <= 0 || KC > kVbMaxKB) return 0;
    return tail_ws_bytes(H, QB);
}

extern "C" int svg_centroid_tail_attention_lse(const void* q, const void* kbar, const void* vbar, void* o, float* lse, int32_t H, int32_t Sq,
                                               int32_t KC, int32_t D, int32_t dtype, float sm_scale, const uint8_t* block_map, int32_t map_cols,
                                               const int32_t* q_sizes, const int32_t* k_sizes, int32_t QB, const int32_t* q_row_idx,
                                               void* workspace, size_t workspace_bytes, const svg_attn_layout_t* layout, void* stream) {
    if (!q || !kbar || !vbar || !o || !lse || !block_map || !q_sizes || !k_sizes || !workspace) return SVG_ERR_BAD_ARG;
    if (H <= 0 || Sq <= 0 || KC <= 0 || QB <= 0) return SVG_ERR_BAD_ARG;
    if (map_cols < KC) return SVG_ERR_BAD_ARG;
    AttnLayout lay = contiguous_layout(H, H, Sq, KC, D);
    if (layout) {   // of the caller's layout only heads_per_batch and the q strides are read; they pass the checks of every *_strided entry
        svg_attn_layout_t abi = *layout;
        const int hpb = abi.heads_per_batch > 0 ? abi.heads_per_batch : 1;
        abi.kv_heads_per_batch = 0;
        abi.k = abi.v = abi.o = {(int64_t)hpb * D, (int64_t)D, D};
        if (const int rc = layout_from_abi(&abi, H, H, Sq, 1, D, q, q, q, q, lay); rc != SVG_OK) return rc;
    }
    if (workspace_bytes < svg_centroid_tail_workspace_bytes(H, QB, KC)) return SVG_ERR_WORKSPACE;
    if (D != 128 || (dtype != SVG_DTYPE_BF16 && dtype != SVG_DTYPE_F16) || KC > kVbMaxKB) return SVG_ERR_UNSUPPORTED;
    if (Sq >= (1 << 24) || H > 65535) return SVG_ERR_UNSUPPORTED;   // (H: the grid's z extent)
    if ((((size_t)q | (size_t)kbar | (size_t)vbar | (size_t)o | (size_t)workspace) & 15) != 0) return SVG_ERR_UNSUPPORTED;
    return dispatch_td(dtype, D, [&](auto t, auto d) -> int {
        using T = decltype(t);
        if constexpr (decltype(d)::value != 128) {
            return SVG_ERR_UNSUPPORTED;
        } else {
            hipStream_t st = (hipStream_t)stream;
            int32_t* row_start = (int32_t*)workspace;
            hipLaunchKernelGGL(tail_row_start_kernel, dim3(H), dim3(256), 0, st, q_sizes, row_start, QB);
            CentroidTailParams<T> p;
            p.q = (const T*)q, p.kbar = (const T*)kbar, p.vbar = (const T*)vbar, p.o = (T*)o, p.lse = lse;
            p.block_map = block_map, p.q_sizes = q_sizes, p.k_sizes = k_sizes, p.q_row_idx = q_row_idx, p.row_start = row_start;
            p.Sq = Sq, p.KC = KC, p.QB = QB, p.map_cols = map_cols, p.nT = (KC + kBN - 1) / kBN;
            p.scale_log2 = sm_scale * 1.4426950408889634f;
            p.hpb_q = lay.hpb_q, p.q_rs = lay.q_rs, p.q_bs = lay.q_bs, p.q_hs = lay.q_hs;
            // sub-tile slots per block-row: twice what an average block-row needs; a larger one walks its sub-tiles slot by slot, a smaller
            // one's spare workgroups leave at once
            const long long avg = ((long long)Sq + (long long)QB * kTailRows - 1) / ((long long)QB * kTailRows);
            const int Z = (int)std::max<long long>(1, std::min<long long>(2 * avg, 1024));
            const int lds = 2 * KvImage16<128>::kStage + p.nT * kBN * (int)sizeof(float);
            return launch_attn(centroid_tail_kernel<T>, dim3(QB, Z, H), 256, lds, st, p);
        }
    });
}

// SVG2 variable-block attention for gfx950: the kernels that run the bodies of attn_core.h / attn_m16.h / attn_f8.h on the policy of
// varblock_policy.h, the planning / launch-order kernels in front of them, the svg_varblock_* entries (svg_varblock_attention_lse: row
// log-sum-exp output; svg_varblock_attention_lse_f32: fp32 rows).  (Band family: attention.hip.)
#include <utility>

#include "attn_f8.h"
#include "attn_m16.h"
#include "varblock_policy.h"

namespace svg {

template <typename T, int D, int NW>
__global__ __launch_bounds__(NW * 64, 2) void varblock_attn_kernel(typename VarblockPolicy<T, D, NW>::Params prm) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    attn_body<T, D, NW, VarblockPolicy<T, D, NW>>(prm, smem, smem + attn_lds_bytes<D, NW>());
}

// two-phase ping-pong body for the variable-block policy (256-row q tiles)
template <typename T, int D>
__global__ __launch_bounds__(512, 2) void varblock_attn_pp2_kernel(typename VarblockPolicy<T, D, 8>::Params prm) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    attn_body_pp2<T, D, VarblockPolicy<T, D, 8>>(prm, smem, smem + attn_pp2_lds_bytes<D>());
}

// the two-phase body on 16x16x32 MFMAs (attn_m16.h) for the variable-block policies: head_dim 128; svg_varblock_attention variant 8.  One
// template: the policy is the only thing that differs between the instantiations — VarblockPolicy<T, 128, 8>, VarblockLsePolicy
// (svg_varblock_attention_lse: the epilogue of attn_m16_tile also stores one fp32 per query row) and VarblockF32Policy
// (svg_varblock_attention_lse_f32: it stores the rows as fp32, before their rounding, and no 16-bit o) — and each instantiation's listing is
// compared with the one it had as a kernel of its own (tools/asm_diff.py --pair, profiles/kernel_templates_asm_diff.txt).
template <typename T, typename Pol>
__global__ __launch_bounds__(512, 2) void varblock_attn_m16_kernel(typename Pol::Params prm) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    attn_body_m16<T, Pol>(prm, smem, smem + attn_m16_lds_bytes());
}

#ifdef SVG_ABLATIONS
// the same kernel with the launch timeline of svg_debug_wg_trace (variant 5, diagnostics build only)
template <typename T, int D>
__global__ __launch_bounds__(512, 2) void varblock_attn_pp2_trace_kernel(typename VarblockPolicy<T, D, 8>::Params prm) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    attn_body_pp2<T, D, VarblockPolicy<T, D, 8>, true>(prm, smem, smem + attn_pp2_lds_bytes<D>());
}
#endif

// fp8 (e4m3) form: gathering fp8 body of attn_f8.h, NW x 32-row q tiles, two waves per SIMD (8 / NW workgroups per CU).  The waves
// of this lock-step body are independent between barriers, so a tile's time follows its ACTIVE waves and smaller tiles only cost
// more K / V staging per row: the ragged q-clusters of SVG2 (252 +- 160 rows) fill 69 % of 256-row tiles, 80 % of 128-row tiles,
// 89 % of 64-row tiles (tools/vb_stats.py).
constexpr int kVbF8Waves = 4;
template <typename T>
__global__ __launch_bounds__(kVbF8Waves * 64, 2) void varblock_attn_f8_kernel(typename VarblockPolicy<T, 128, kVbF8Waves>::Params prm,
                                                                              F8GArgs fa) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    attn_body_f8g<T, VarblockPolicy<T, 128, kVbF8Waves>, kVbF8Waves>(prm, fa, smem, smem + attn_f8_lds_bytes<128, kVbF8Waves>());
}

// plan: exclusive prefix sums of q_sizes, k_sizes and of the per-block-row tile counts.  grid = (Hkv), block = 256
__global__ __launch_bounds__(256) void varblock_plan_kernel(const int32_t* __restrict__ q_sizes,
                                                            const int32_t* __restrict__ k_sizes, int32_t* __restrict__ q_off,
                                                            int32_t* __restrict__ k_off, int32_t* __restrict__ tile_off,
                                                            int32_t* __restrict__ tile_off2, int QB, int KB, int BM) {
    __shared__ int32_t wtot[4];
    const int h = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    // div > 0: ceil(v / div); div == -1: number of full kVbFull-row tiles; div == -2: 128-row tiles of the remainder
    auto scan = [&](const int32_t* in, int32_t* out, int n, int div) {
        int carry = 0;
        for (int i0 = 0; i0 < n; i0 += 256) {
            const int i = i0 + tid;
            int v = i < n ? in[i] : 0;
            if (div > 0) v = (v + div - 1) / div;
            else if (div == -1) v = v / kVbFull;
            else if (div == -2) v = (v % kVbFull + 127) / 128;
            int incl = v;
#pragma unroll
            for (int o = 1; o < 64; o <<= 1) {
                const int t = __shfl_up(incl, o);
                if (lane >= o) incl += t;
            }
            __syncthreads();
            if (lane == 63) wtot[wv] = incl;
            __syncthreads();
            int wb = carry;
            for (int x = 0; x < wv; ++x) wb += wtot[x];
            if (i < n) out[i] = wb + incl - v;
            carry += wtot[0] + wtot[1] + wtot[2] + wtot[3];
        }
        if (tid == 0) out[n] = carry;
        __syncthreads();
    };
    scan(q_sizes + (size_t)h * QB, q_off + (size_t)h * (QB + 1), QB, 0);
    scan(k_sizes + (size_t)h * KB, k_off + (size_t)h * (KB + 1), KB, 0);
    if (BM > 0) {
        scan(q_sizes + (size_t)h * QB, tile_off + (size_t)h * (QB + 1), QB, BM);
    } else {  // mixed tiling
        scan(q_sizes + (size_t)h * QB, tile_off + (size_t)h * (QB + 1), QB, -1);
        scan(q_sizes + (size_t)h * QB, tile_off2 + (size_t)h * (QB + 1), QB, -2);
    }
}

// Longest-first launch order of the 256-row variable-block kernel.  The work of a workgroup is the number of active keys of its
// block-row (top-p keeps between a few and all key clusters); in block-row order the last round of the launch ends with whatever
// rows come last (modelled makespan 2.4 % over the ideal at Wan 720p, 0.5 % longest-first).  The order stays head-major — a global
// longest-first order interleaves all heads and their K/V (1.5 GB at Wan 720p) no longer stay in the Infinity Cache: 38.4 ms
// instead of 33.6 — and is longest-first inside every kv head.  A counting sort on (head, 64-key tile count / 16), in three small
// launches: histogram (one wave per block-row), scan, scatter.
constexpr int kVbBuckets = 64;   // per kv head

// Remainder packing (round 3).  k-means clusters are ragged (Wan 720p: 252 +- 160 rows), so the last q-tile of a block-row is mostly
// padding: only 69 % of the rows of the 256-row tiles are real, and a tile costs its key-tile iterations whatever its row count.
// Two block-rows i, j of a kv head whose ragged last tiles fit into ONE tile (r_i + r_j <= BM) share that tile: it walks the key
// blocks both attend once instead of twice (see VarblockPolicy::Ctx).  q-clusters of the same neighbourhood of the data select
// nearly the same key blocks (median Jaccard of best partners 0.94 on the bench data), so the shared part is most of the list.
// One workgroup per kv head: bitmap rows of the map in LDS (key blocks without rows count as inactive), every block-row keeps its
// own row in registers and looks for the unmatched partner with the most common key blocks among those its remainder fits with;
// mutual choices are matched ("handshake"), a few rounds.  partner[h][i] = j >= 0: i's last tile carries j's too (i is the primary);
// -2: carried by its partner; -1: alone.  Exactness: the mask inside a shared tile is exact (two key intervals per row), so the
// result does not depend on which rows are paired.
constexpr int kVbPairThreads = 512;
constexpr int kVbPairRounds = 3;
constexpr int kVbPairMinCommon = 8;   // common key blocks (~ 8 x 76 keys = 10 key tiles) that pay for the three-pass run-list build
constexpr int kVbPairRows = 64;       // block-rows scored by one workgroup (8 threads each, an eighth of the candidates per thread)
static inline int vb_pair_ws(int KB) { return (((KB + 31) / 32) + 3) & ~3; }   // bitmap row stride in words (16-byte rows)
static inline size_t vb_pair_lds(int QB, int KB) { return ((size_t)QB * vb_pair_ws(KB) + (size_t)QB + kVbPairRows) * sizeof(int32_t); }

// bitmap rows of the map: bit j of word w of row (h, i) = block (i, 32 w + j) active and key block 32 w + j not empty
__global__ __launch_bounds__(256) void varblock_bitmap_kernel(const uint8_t* __restrict__ block_map, const int32_t* __restrict__ k_sizes,
                                                              uint32_t* __restrict__ bits, int Hkv, int QB, int KB, int WS) {
    const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
    if (idx >= (long long)Hkv * QB * WS) return;
    const int w = (int)(idx % WS);
    const long long row = idx / WS;
    const int h = (int)(row / QB);
    uint32_t b = 0;
    if (w * 32 < KB) {
        const uint8_t* m = block_map + row * KB + w * 32;
        const int32_t* ks = k_sizes + (size_t)h * KB + w * 32;
        const int n = min(32, KB - w * 32);
        for (int j = 0; j < n; ++j) b |= (m[j] && ks[j] > 0) ? (1u << j) : 0u;
    }
    bits[idx] = b;
}
// one round, scoring half: grid = (ceil(QB / 64), Hkv).  Thread (il, part): block-row i = 64 blockIdx.x + il looks at an eighth of
// the candidates j for the unmatched one with the most common key blocks whose remainder fits beside its own; the eight partial
// results meet in an LDS arg-max (key = common << 12 | inverted index: ties go to the lowest index).  Branch-free scan, 16-byte
// broadcast loads of the candidates' rows; the thread's own row lives in registers.
__global__ __launch_bounds__(kVbPairThreads) void varblock_pair_score_kernel(const uint32_t* __restrict__ bits_g,
                                                                             const int32_t* __restrict__ q_sizes,
                                                                             const int32_t* __restrict__ rem_g, int32_t* __restrict__ best_g,
                                                                             int QB, int WS, int BM, int round) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    uint32_t* bits = (uint32_t*)smem;                     // [QB][WS]
    int32_t* rem = (int32_t*)(bits + (size_t)QB * WS);    // [QB]
    int32_t* sbest = rem + QB;                            // [kVbPairRows]
    const int h = blockIdx.y, tid = threadIdx.x, il = tid & (kVbPairRows - 1), part = tid / kVbPairRows;
    constexpr int kParts = kVbPairThreads / kVbPairRows;
    {
        const u32x4* src = (const u32x4*)(bits_g + (size_t)h * QB * WS);
        u32x4* dst = (u32x4*)bits;
        for (int x = tid; x < QB * WS / 4; x += kVbPairThreads) dst[x] = src[x];
    }
    for (int x = tid; x < QB; x += kVbPairThreads) rem[x] = round == 0 ? q_sizes[(size_t)h * QB + x] % BM : rem_g[(size_t)h * QB + x];
    if (tid < kVbPairRows) sbest[tid] = (kVbPairMinCommon << 12) - 1;
    __syncthreads();
    const int i = blockIdx.x * kVbPairRows + il;
    constexpr int kRegW = 32;
    u32x4 mine[kRegW / 4];
#pragma unroll
    for (int w4 = 0; w4 < kRegW / 4; ++w4)
        mine[w4] = (i < QB && 4 * w4 < WS) ? *(const u32x4*)(bits + (size_t)i * WS + 4 * w4) : u32x4{0u, 0u, 0u, 0u};
    const int ri = i < QB ? rem[i] : 0;
    const int chunk = (QB + kParts - 1) / kParts, j_lo = part * chunk, j_hi = min(QB, j_lo + chunk);
    int bkey = -1;
    for (int j = j_lo; j < j_hi; ++j) {
        const int rj = rem[j];
        const u32x4* row = (const u32x4*)(bits + (size_t)j * WS);
        int common = 0;
#pragma unroll
        for (int w4 = 0; w4 < kRegW / 4; ++w4) {
            if (4 * w4 < WS) {
                const u32x4 r = row[w4];
                common += __popc(mine[w4][0] & r[0]) + __popc(mine[w4][1] & r[1]) + __popc(mine[w4][2] & r[2]) + __popc(mine[w4][3] & r[3]);
            }
        }
        const bool ok = (j != i) & (rj > 0) & (ri > 0) & (ri + rj <= BM);
        const int key = ok ? ((common << 12) | (0xFFF - j)) : -1;
        bkey = key > bkey ? key : bkey;
    }
    if (bkey >= (kVbPairMinCommon << 12)) atomicMax(&sbest[il], bkey);
    __syncthreads();
    if (part == 0 && i < QB) {
        const int k2 = sbest[il];
        best_g[(size_t)h * QB + i] = k2 >= (kVbPairMinCommon << 12) ? 0xFFF - (k2 & 0xFFF) : -1;
    }
}
// one round, matching half ("handshake"): mutual choices become pairs.  partner[h][i] = j >= 0: i's last tile carries j's too (the
// lower index is the primary); -2: carried by its partner; -1: alone.
__global__ __launch_bounds__(256) void varblock_pair_match_kernel(const int32_t* __restrict__ q_sizes, const int32_t* __restrict__ best,
                                                                  int32_t* __restrict__ rem, int32_t* __restrict__ partner, int n_rows,
                                                                  int QB, int BM, int round) {
    const int row = blockIdx.x * 256 + threadIdx.x;
    if (row >= n_rows) return;
    const int h = row / QB, i = row - h * QB;
    const int bj = best[row];
    const bool matched = bj >= 0 && best[(size_t)h * QB + bj] == i;
    const int r = round == 0 ? q_sizes[row] % BM : rem[row];
    rem[row] = matched ? 0 : r;
    if (matched) partner[row] = i < bj ? bj : -2;
    else if (round == 0) partner[row] = -1;
}

// Launch order: counting sort on (head, descending work class).  A block-row contributes its full tiles (work = its active keys)
// and, unless its partner carries it, its ragged last tile (work = the keys of the union with the partner's list).
__global__ __launch_bounds__(256) void varblock_work_kernel(const uint8_t* __restrict__ block_map, const int32_t* __restrict__ q_sizes,
                                                            const int32_t* __restrict__ k_sizes, const int32_t* __restrict__ partner,
                                                            int32_t* __restrict__ work, int32_t* __restrict__ hist, int Hkv, int QB,
                                                            int KB, int group, int BM) {
    // (bucket = head-major key: h * kVbBuckets + descending work class)
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (row >= Hkv * QB) return;
    const int h = row / QB, i = row - h * QB;
    const int pj = partner ? partner[row] : -1;
    const uint8_t* m = block_map + (size_t)row * KB;
    const uint8_t* m2 = pj >= 0 ? block_map + ((size_t)h * QB + pj) * KB : m;
    const int32_t* ks = k_sizes + (size_t)h * KB;
    int keys = 0, ukeys = 0;
    for (int j = lane; j < KB; j += 64) {
        keys += m[j] ? ks[j] : 0;
        ukeys += (m[j] | m2[j]) ? ks[j] : 0;
    }
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) keys += __shfl_xor(keys, o), ukeys += __shfl_xor(ukeys, o);
    if (lane == 0) {
        auto bucket_of = [&](int k) {
            const int tiles = (k + kBN - 1) / kBN;
            return h * kVbBuckets + (kVbBuckets - 1 - min(tiles / 16, kVbBuckets - 1));   // descending work inside the head
        };
        const int n = q_sizes[row];
        const int nfull = n / BM, has_rem = (n % BM) > 0 && pj != -2;
        const int b_full = bucket_of(keys), b_rem = bucket_of(ukeys);
        work[2 * row] = b_full;
        work[2 * row + 1] = has_rem ? b_rem : -1;
        if (nfull > 0) atomicAdd(hist + b_full, nfull * group);
        if (has_rem) atomicAdd(hist + b_rem, group);
    }
}
__global__ __launch_bounds__(256) void varblock_scan_kernel(int32_t* __restrict__ hist, int32_t* __restrict__ order, int nb) {
    __shared__ int32_t part[256];
    const int tid = threadIdx.x;
    const int per = (nb + 255) / 256, lo = min(tid * per, nb), hi = min(lo + per, nb);
    int sum = 0;
    for (int x = lo; x < hi; ++x) sum += hist[x];
    part[tid] = sum;
    __syncthreads();
    if (tid == 0) {
        int run = 0;
        for (int x = 0; x < 256; ++x) {
            const int t = part[x];
            part[x] = run;
            run += t;
        }
        order[0] = run;   // number of workgroups
    }
    __syncthreads();
    int run = part[tid];
    for (int x = lo; x < hi; ++x) {   // the histogram becomes the scatter cursor of each bucket
        const int t = hist[x];
        hist[x] = run;
        run += t;
    }
}
__global__ __launch_bounds__(256) void varblock_scatter_kernel(const int32_t* __restrict__ q_sizes, const int32_t* __restrict__ partner,
                                                               const int32_t* __restrict__ work, int32_t* __restrict__ cursor,
                                                               int32_t* __restrict__ order, int Hkv, int QB, int group, int BM) {
    const int row = blockIdx.x * 256 + threadIdx.x;
    if (row >= Hkv * QB) return;
    const int h = row / QB, i = row - h * QB;
    const int n = q_sizes[row], nfull = n / BM;
    const int b_full = work[2 * row], b_rem = work[2 * row + 1];
    if (nfull > 0) {
        int pos = atomicAdd(cursor + b_full, nfull * group);
        for (int g = 0; g < group; ++g)
            for (int sub = 0; sub < nfull; ++sub, ++pos) {
                order[2 + 3 * pos] = h * group + g;
                order[3 + 3 * pos] = (i << 16) | sub;
                order[4 + 3 * pos] = -1;
            }
    }
    if (b_rem >= 0) {
        int pos = atomicAdd(cursor + b_rem, group);
        const int pj = partner ? partner[row] : -1;
        for (int g = 0; g < group; ++g, ++pos) {
            order[2 + 3 * pos] = h * group + g;
            order[3 + 3 * pos] = (i << 16) | nfull;
            order[4 + 3 * pos] = pj >= 0 ? pj : -1;
        }
    }
}

// Similarity order of the 256-row variable-block kernel (variant 7; measured in round 3, NOT the default: see svg_varblock_attention).  The longest-first order above hands an XCD 32
// unrelated block-rows of a head at a time: every workgroup streams its own quarter of the head's K / V through that XCD's 4 MiB
// L2 (PMC, Wan 720p: hit rate 31 %, 117 GB per launch between L2 and the fabric for 3.1 GB of tensors).  Block-rows whose key
// lists are (nearly) the same — q-clusters of the same neighbourhood of the data select the same k-clusters — read the same K / V
// rows in the same order, so this kernel puts them next to each other and hands CONSECUTIVE workgroups to the SAME XCD:
//   * one workgroup per kv head builds a nearest-neighbour chain over the block-rows (bitmap rows of the map in LDS, Jaccard
//     similarity of the active key-block sets, start at the block-row with the most active key blocks; QB steps of one block-wide
//     arg-max each);
//   * the sub-tiles of a block-row and the q heads of a GQA group (same key list by construction) stay adjacent;
//   * position p of the head-major chain order is mapped to dispatch id b so that, inside every window of 256 consecutive
//     positions, XCD x (= b % 8, the hardware's round-robin) receives positions [32 x, 32 x + 32) — the remap of the band kernel.
constexpr int kVbChainThreads = 512;
static inline size_t vb_chain_lds(int QB, int KB) {
    const int W = (KB + 31) / 32;
    return ((size_t)QB * (W + 1) + 3 * (size_t)QB + 64) * sizeof(int32_t);
}
__global__ __launch_bounds__(kVbChainThreads) void varblock_chain_kernel(const uint8_t* __restrict__ block_map,
                                                                         const int32_t* __restrict__ k_sizes,
                                                                         const int32_t* __restrict__ tile_off, int32_t* __restrict__ order,
                                                                         int Hkv, int QB, int KB, int group) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int W = (KB + 31) / 32, WS = W + 1;   // (row stride W + 1 words: thread c reads word w of row c — conflict-free)
    uint32_t* bits = (uint32_t*)smem;            // [QB][WS]
    int32_t* pc = (int32_t*)(bits + (size_t)QB * WS);   // [QB] active key blocks of a block-row; -1 once it is in the chain
    int32_t* chain = pc + QB;                    // [QB] block-row at chain position
    int32_t* cnt = chain + QB;                   // [QB] workgroups of the block-row at chain position (then their exclusive prefix)
    unsigned long long* red = (unsigned long long*)(cnt + QB);   // [8] per-wave arg-max
    const int h = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int32_t* toff = tile_off + (size_t)h * (QB + 1);
    const int32_t* ks = k_sizes + (size_t)h * KB;
    // ---- bitmap rows: bit j of row i = block (i, j) active and key block j not empty ----
    for (int idx = tid; idx < QB * W; idx += kVbChainThreads) {
        const int i = idx / W, w = idx - i * W;
        const uint8_t* m = block_map + ((size_t)h * QB + i) * KB + w * 32;
        uint32_t b = 0;
        const int n = min(32, KB - w * 32);
        for (int j = 0; j < n; ++j) b |= (m[j] && ks[w * 32 + j] > 0) ? (1u << j) : 0u;
        bits[(size_t)i * WS + w] = b;
    }
    __syncthreads();
    int n_live = 0;
    for (int i = tid; i < QB; i += kVbChainThreads) {
        int c = 0;
        for (int w = 0; w < W; ++w) c += __popc(bits[(size_t)i * WS + w]);
        const bool live = toff[i + 1] > toff[i];   // block-rows without query rows launch nothing
        pc[i] = live ? c : -1;
        n_live += live;
    }
    __syncthreads();
    // ---- nearest-neighbour chain ----
    // One step = one block-wide arg-max of the Jaccard similarity to the current block-row.  A thread keeps ITS candidate's bitmap
    // row in registers for the whole chain (QB <= 512: one candidate per thread; larger maps loop over LDS), the current row is
    // read from LDS with broadcast 16-byte loads, and the arg-max is one LDS atomic per thread on a 32-bit key (similarity in 20
    // bits, inverted index in 12: ties go to the lowest index) — one barrier per step.
    constexpr int kRegW = 32;   // bitmap words a thread can hold (KB <= 1024)
    const bool in_regs = (W <= kRegW) && (QB <= kVbChainThreads);
    uint32_t mine[kRegW];
#pragma unroll
    for (int w = 0; w < kRegW; ++w) mine[w] = (in_regs && tid < QB && w < W) ? bits[(size_t)tid * WS + w] : 0u;
    uint32_t* slot = (uint32_t*)red;   // [3] arg-max slots, used round-robin so that the reset needs no barrier of its own
    if (tid < 3) slot[tid] = 0u;
    // start: the live block-row with the most active key blocks (ties: lowest index)
    __syncthreads();
    for (int i = tid; i < QB; i += kVbChainThreads)
        if (pc[i] >= 0) atomicMax(&slot[0], ((uint32_t)min(pc[i] + 1, 0xFFFFF) << 12) | (uint32_t)(0xFFF - (i & 0xFFF)));
    __syncthreads();
    uint32_t best = slot[0];
    int npos = 0, step = 0;
    const bool wide_idx = QB > 4096;   // (never: KB and QB are limited by the LDS budget of this kernel; kept as a guard)
    while (best != 0u && !wide_idx) {
        const int cur = 0xFFF - (int)(best & 0xFFFu);
        const int pcur = pc[cur];
        ++step;
        __syncthreads();   // everybody has read slot[(step - 1) % 3] and pc[cur]
        if (tid == 0) {
            chain[npos] = cur;
            pc[cur] = -1;
            slot[(step + 1) % 3] = 0u;   // the slot of the NEXT step (last read two steps ago)
        }
        ++npos;
        const uint32_t* crow = bits + (size_t)cur * WS;
        uint32_t key = 0u;
        if (in_regs) {
            if (tid < QB && tid != cur && pc[tid] >= 0) {   // (pc[cur] is being cleared by thread 0: tid != cur covers the race)
                int inter = 0;
#pragma unroll
                for (int w = 0; w < kRegW; ++w)
                    if (w < W) inter += __popc(mine[w] & crow[w]);
                const int uni = pcur + pc[tid] - inter;
                const float jac = uni > 0 ? (float)inter / (float)uni : 1.f;
                key = ((uint32_t)(jac * 1048574.f + 1.f) << 12) | (uint32_t)(0xFFF - tid);
            }
            if (key) atomicMax(&slot[step % 3], key);
        } else {
            for (int i = tid; i < QB; i += kVbChainThreads) {
                if (i == cur || pc[i] < 0) continue;
                int inter = 0;
                for (int w = 0; w < W; ++w) inter += __popc(bits[(size_t)i * WS + w] & crow[w]);
                const int uni = pcur + pc[i] - inter;
                const float jac = uni > 0 ? (float)inter / (float)uni : 1.f;
                atomicMax(&slot[step % 3], ((uint32_t)(jac * 1048574.f + 1.f) << 12) | (uint32_t)(0xFFF - i));
            }
        }
        __syncthreads();
        best = slot[step % 3];
    }
    // ---- workgroups per chain position, exclusive prefix, scatter with the XCD remap ----
    for (int p = tid; p < npos; p += kVbChainThreads) {
        const int i = chain[p];
        cnt[p] = (toff[i + 1] - toff[i]) * group;
    }
    __syncthreads();
    __shared__ int32_t s_base, s_total, s_head_total;
    if (tid == 0) {
        int run = 0;
        for (int p = 0; p < npos; ++p) {   // (npos <= QB <= a few hundred: a serial scan is ~1 us)
            const int t = cnt[p];
            cnt[p] = run;
            run += t;
        }
        int base = 0, total = 0;
        for (int hh = 0; hh < Hkv; ++hh) {
            const int t = tile_off[(size_t)hh * (QB + 1) + QB] * group;
            if (hh < h) base += t;
            total += t;
        }
        s_base = base, s_total = total, s_head_total = run;
        if (h == 0) order[0] = total;
    }
    __syncthreads();
    const int base = s_base, full = (s_total / (kNumXCD * 32)) * (kNumXCD * 32);
    for (int p = tid; p < npos; p += kVbChainThreads) {
        const int i = chain[p];
        const int nsub = toff[i + 1] - toff[i];
        int pos = base + cnt[p];
        for (int g = 0; g < group; ++g)
            for (int sub = 0; sub < nsub; ++sub, ++pos) {
                int b = pos;
                if (pos < full) {
                    const int win = pos / (kNumXCD * 32), r = pos - win * (kNumXCD * 32);
                    b = win * (kNumXCD * 32) + (r % 32) * kNumXCD + r / 32;
                }
                order[2 + 3 * b] = h * group + g;
                order[3 + 3 * b] = (i << 16) | sub;
                order[4 + 3 * b] = -1;
            }
    }
}

// The bodies of svg_varblock_attention* (`variant` picks one, include/svg_attn.h).  k-means clusters are ragged (Wan 720p bench: mean
// 252 rows, sigma 161): uniform 256-row tiles keep 68 % of the processed rows real, uniform 128-row tiles 79 % but run the slower
// 4-wave schedule everywhere; mixed keeps 79 % with most rows on the 8-wave kernel.
enum class VbBody {
    kLockstep128,   // lock-step body, 4 waves, 128-row q tiles (2-D grid)
    kLockstep256,   // lock-step body, 8 waves, 256-row q tiles (2-D grid)
    kMixed,         // the full 256-row tiles of every block-row on the 8-wave lock-step kernel, its remaining rows on 128-row tiles of the 4-wave one
    kPP2,           // two-phase body on 32x32x16 MFMAs, 256-row q tiles (launch order, 1-D grid)
    kM16,           // two-phase body on 16x16x32 MFMAs (attn_m16.h; head_dim 128), 256-row q tiles (launch order)
    kF8,            // fp8 gathering body (attn_f8.h; head_dim 128), kVbF8Waves x 32-row q tiles (launch order)
};

// One variable-block call (the counterpart of BandCall): the arguments of the entries in their order, then how to run them
struct VbCall {
    const void *q, *k, *v;
    void* o;
    int32_t Hq, Hkv, Sq, Skv, D, dtype;
    float sm_scale;
    const uint8_t* block_map;
    const int32_t *q_sizes, *k_sizes;
    int32_t QB, KB;
    const int32_t *q_row_idx, *kv_row_idx;
    void* workspace;
    size_t workspace_bytes;
    hipStream_t st;
    VbBody body = VbBody::kLockstep128;
    bool block_row_order = false, trace = false;   // the ordered bodies on the 2-D grid; the traced two-phase body (diagnostics builds)
    int order_mode = 0;                             // 0: longest-first + remainder packing, 1: longest-first, 2: similarity order
    const AttnLayout* lay = nullptr;                // strided tensors (svg_varblock_attention_strided); nullptr: contiguous [H, S, D]
    F8GArgs f8{};                                   // kF8: the quantised tensors and scales of f8g_quantize
    float* lse = nullptr;                           // kM16: row log-sum-exp output, contiguous fp32 [Hq, Sq] (svg_varblock_attention_lse), or nullptr
    float* o32 = nullptr;                           // with lse: fp32 rows, contiguous [Hq, Sq, 128], instead of o (svg_varblock_attention_lse_f32)
};

// The workspace of a call, and the one definition of its layout (_native.varblock_launch_order / varblock_partners read it at fixed
// offsets): plan prefix sums, two buckets and the packing partner per block-row, the bucket histogram, the launch order (count,
// pad, entries[3 * max workgroups]; q tiles of >= 64 rows), then the bitmap rows of remainder packing.
struct VbWs {
    int32_t *q_off, *tile_off, *k_off, *tile_off2, *work, *partner, *hist, *order;
    uint32_t* bits;
    size_t bytes;   // up to the end of the last region: svg_varblock_workspace_bytes (taken from ws == nullptr)
};
static VbWs vb_ws(void* ws, int Hq, int Hkv, int Sq, int QB, int KB) {
    uintptr_t at = (uintptr_t)ws;
    auto take = [&](size_t words) { return (int32_t*)std::exchange(at, at + words * sizeof(int32_t)); };
    VbWs w;
    w.q_off = take((size_t)Hkv * (QB + 1));
    w.tile_off = take((size_t)Hkv * (QB + 1));
    w.k_off = take((size_t)Hkv * (KB + 1));
    w.tile_off2 = take((size_t)Hkv * (QB + 1));
    w.work = take(2 * (size_t)Hkv * QB);
    w.partner = take((size_t)Hkv * QB);
    w.hist = take((size_t)Hkv * kVbBuckets);
    w.order = take(2 + 3 * ((size_t)Sq / 64 + QB) * Hq);
    // The bitmap rows start at the next 16-byte boundary wherever the caller's buffer starts: four words of slack go with them.
    // Remainder packing needs KB <= 1024 (vb_launch_order): a larger map has no bitmap region, and nothing reads `bits`.
    w.bits = (uint32_t*)((at + 15) & ~(uintptr_t)15);
    if (KB <= 1024) take((size_t)Hkv * QB * vb_pair_ws(KB) + 4);
    w.bytes = at - (uintptr_t)ws;
    return w;
}

// Launch order of the ordered bodies (BM-row q tiles) into w.order: the similarity order (order_mode 2), or longest-first inside every
// kv head with the ragged last tiles packed in pairs (order_mode 0) or not (1).
static int vb_launch_order(const VbWs& w, const VbCall& c, int BM) {
    const int Hkv = c.Hkv, QB = c.QB, KB = c.KB;
    const hipStream_t st = c.st;
    const int group = c.Hq / Hkv, nb = Hkv * kVbBuckets;
    const size_t chain_lds = vb_chain_lds(QB, KB);
    if (c.order_mode == 2 && chain_lds <= 64 * 1024 && QB <= 4096) {   // similarity order, consecutive workgroups on one XCD (variant 7)
        hipLaunchKernelGGL(varblock_chain_kernel, dim3(Hkv), dim3(kVbChainThreads), chain_lds, st, c.block_map, c.k_sizes, w.tile_off,
                           w.order, Hkv, QB, KB, group);
        return SVG_OK;
    }
    const size_t pair_lds = vb_pair_lds(QB, KB);
    const bool pack = c.order_mode == 0 && pair_lds <= 64 * 1024 && QB <= 4095 && KB <= 1024;   // (bitmap row in registers; 12-bit index in the arg-max key)
    if (pack) {   // bitmap rows once, then kVbPairRounds x (score, match); scratch: the bitmap area behind the order, and the bucket
                  // array `work` (free until varblock_work_kernel runs) for the remainders and choices
        const int WSp = vb_pair_ws(KB);
        int32_t* rem = w.work;
        int32_t* best = w.work + (size_t)Hkv * QB;
        const long long nw = (long long)Hkv * QB * WSp;
        hipLaunchKernelGGL(varblock_bitmap_kernel, dim3((unsigned)((nw + 255) / 256)), dim3(256), 0, st, c.block_map, c.k_sizes, w.bits,
                           Hkv, QB, KB, WSp);
        for (int round = 0; round < kVbPairRounds; ++round) {
            hipLaunchKernelGGL(varblock_pair_score_kernel, dim3((QB + kVbPairRows - 1) / kVbPairRows, Hkv), dim3(kVbPairThreads), pair_lds,
                               st, w.bits, c.q_sizes, rem, best, QB, WSp, BM, round);
            hipLaunchKernelGGL(varblock_pair_match_kernel, dim3((Hkv * QB + 255) / 256), dim3(256), 0, st, c.q_sizes, best, rem, w.partner,
                               Hkv * QB, QB, BM, round);
        }
    }
    if (hipMemsetAsync(w.hist, 0, (size_t)nb * sizeof(int32_t), st) != hipSuccess) return SVG_ERR_LAUNCH;
    hipLaunchKernelGGL(varblock_work_kernel, dim3((Hkv * QB + 3) / 4), dim3(256), 0, st, c.block_map, c.q_sizes, c.k_sizes,
                       pack ? w.partner : nullptr, w.work, w.hist, Hkv, QB, KB, group, BM);
    hipLaunchKernelGGL(varblock_scan_kernel, dim3(1), dim3(256), 0, st, w.hist, w.order, nb);
    hipLaunchKernelGGL(varblock_scatter_kernel, dim3((Hkv * QB + 255) / 256), dim3(256), 0, st, c.q_sizes, pack ? w.partner : nullptr,
                       w.work, w.hist, w.order, Hkv, QB, group, BM);
    return SVG_OK;
}

// One variable-block call in three steps: the plan (prefix sums), the launch order of the ordered bodies, the body.
template <typename T, int D>
static int run_varblock(const VbCall& c) {
    const int Hq = c.Hq, Sq = c.Sq, QB = c.QB, KB = c.KB;
    const hipStream_t st = c.st;
    const VbWs w = vb_ws(c.workspace, Hq, c.Hkv, Sq, QB, KB);
    const VbBody body = c.body;
    const bool ordered_body = body == VbBody::kPP2 || body == VbBody::kM16 || body == VbBody::kF8;
    const int BM = body == VbBody::kMixed ? 0 : body == VbBody::kLockstep128 ? 128 : body == VbBody::kF8 ? kVbF8Waves * 32 : 256;
    hipLaunchKernelGGL(varblock_plan_kernel, dim3(c.Hkv), dim3(256), 0, st, c.q_sizes, c.k_sizes, w.q_off, w.k_off, w.tile_off, w.tile_off2,
                       QB, KB, BM);
    const int32_t* order = nullptr;
    if (ordered_body && !c.block_row_order && QB < 32768 && Sq / 256 + 1 < 65536) {   // packing of (block-row, sub-tile) in one word
        if (const int rc = vb_launch_order(w, c, BM); rc != SVG_OK) return rc;
        order = w.order;
    }
    const int kb_cap = (KB + 63) / 64 * 64, lds_vb = vb_policy_lds(kb_cap);
    auto params = [&](auto nw_c, int mode, const int32_t* toff, int max_tiles) {
        typename VarblockPolicy<T, D, decltype(nw_c)::value>::Params p;
        p.q = (const T*)c.q, p.k = (const T*)c.k, p.v = (const T*)c.v, p.o = (T*)c.o;
        p.Hq = Hq, p.Hkv = c.Hkv, p.group = Hq / c.Hkv, p.Sq = Sq, p.Skv = c.Skv, p.QB = QB, p.KB = KB;
        p.max_tiles = max_tiles, p.tile_mode = mode, p.kb_cap = kb_cap;
        p.scale_log2 = c.sm_scale * 1.4426950408889634f;
        p.block_map = c.block_map, p.q_off = w.q_off, p.k_off = w.k_off, p.tile_off = toff;
        p.q_row_idx = c.q_row_idx, p.kv_row_idx = c.kv_row_idx;
        p.lay = c.lay ? *c.lay : contiguous_layout(Hq, c.Hkv, Sq, c.Skv, D);
        p.order = order;
        return p;
    };
    auto lockstep = [&](auto nw_c, int mode, const int32_t* toff, int max_tiles) {
        constexpr int W = decltype(nw_c)::value;
        return launch_attn(varblock_attn_kernel<T, D, W>, dim3(max_tiles, Hq), W * 64, attn_lds_bytes<D, W>() + lds_vb, st,
                           params(nw_c, mode, toff, max_tiles));
    };
    using W4 = std::integral_constant<int, 4>;
    using W8 = std::integral_constant<int, 8>;
    switch (body) {
        case VbBody::kLockstep128: return lockstep(W4{}, 0, w.tile_off, Sq / 128 + QB);
        case VbBody::kLockstep256: return lockstep(W8{}, 0, w.tile_off, Sq / 256 + QB);
        case VbBody::kMixed:
            if (Sq >= kVbFull) {
                if (const int rc = lockstep(W8{}, 1, w.tile_off, Sq / kVbFull); rc != SVG_OK) return rc;
            }
            return lockstep(W4{}, 2, w.tile_off2, 2 * QB);
        case VbBody::kF8:
            if constexpr (D == 128) {
                if (!order) return SVG_ERR_UNSUPPORTED;   // (the fp8 kernel takes the ordered 1-D launch only)
                const int max_tiles = Sq / (kVbF8Waves * 32) + QB;
                return launch_attn(varblock_attn_f8_kernel<T>, dim3(max_tiles * Hq), kVbF8Waves * 64,
                                   attn_f8_lds_bytes<128, kVbF8Waves>() + lds_vb, st,
                                   params(std::integral_constant<int, kVbF8Waves>{}, 0, w.tile_off, max_tiles), c.f8);
            }
            return SVG_ERR_UNSUPPORTED;
        default: {   // the two-phase bodies
            const int max_tiles = Sq / 256 + QB;
            const auto p = params(W8{}, 0, w.tile_off, max_tiles);
            const dim3 grid = order ? dim3(max_tiles * Hq) : dim3(max_tiles, Hq);
            if (order && c.trace) {
#ifdef SVG_ABLATIONS
                if constexpr (D == 128 && std::is_same<T, __bf16>::value) {
                    g_trace_reader = read_trace_here;
                    return launch_attn(varblock_attn_pp2_trace_kernel<T, D>, grid, 512, attn_pp2_lds_bytes<D>() + lds_vb, st, p);
                }
#endif
                return SVG_ERR_UNSUPPORTED;   // diagnostics builds only (-DSVG_ABLATIONS)
            }
            if constexpr (D == 128) {
                if (body == VbBody::kM16) {   // the same plan, launch order and grid for the policies that also store lse, or fp32 rows and no 16-bit o
                    auto launch = [&](auto pol) {
                        using Pol = decltype(pol);
                        typename Pol::Params px;
                        static_cast<typename VarblockPolicy<T, 128, 8>::Params&>(px) = p;
                        if constexpr (HasRowLse<Pol>::value) px.lse = c.lse;
                        if constexpr (HasRowO32<Pol>::value) px.o32 = c.o32, px.o = nullptr;
                        return launch_attn(varblock_attn_m16_kernel<T, Pol>, grid, 512, attn_m16_lds_bytes() + lds_vb, st, px);
                    };
                    if (c.lse) return c.o32 ? launch(VarblockF32Policy<T>()) : launch(VarblockLsePolicy<T>());
                    return launch(VarblockPolicy<T, 128, 8>());
                }
            }
            if (c.lse) return SVG_ERR_UNSUPPORTED;
            return launch_attn(varblock_attn_pp2_kernel<T, D>, grid, 512, attn_pp2_lds_bytes<D>() + lds_vb, st, p);
        }
    }
}

}  // namespace svg

using namespace svg;

extern "C" size_t svg_varblock_workspace_bytes(int32_t Hq, int32_t Hkv, int32_t QB, int32_t KB, int32_t Sq) {
    if (Hq <= 0 || Hkv <= 0 || QB <= 0 || KB <= 0 || Sq <= 0) return 0;
    return vb_ws(nullptr, Hq, Hkv, Sq, QB, KB).bytes;
}

extern "C" size_t svg_varblock_attention_fp8_workspace_bytes(int32_t Hq, int32_t Hkv, int32_t QB, int32_t KB, int32_t Sq, int32_t Skv,
                                                             int32_t D) {
    if (D != 128) return 0;
    const size_t plan = svg_varblock_workspace_bytes(Hq, Hkv, QB, KB, Sq);
    if (plan == 0 || Skv <= 0) return 0;
    return ((plan + 255) & ~(size_t)255) + f8g_ws_bytes(Hq, Hkv, Sq, Skv);   // (the quantised tensors: 256-byte aligned)
}

// The checks every svg_varblock_attention* entry shares, in the order the ABI promises; `fp8` adds the limits of the e4m3 body
// (head_dim 128; block-row and sub-tile of the ordered launch packed in one word) where that entry has them.
static int varblock_check_args(const VbCall& c, bool fp8) {
    if (!c.q || !c.k || !c.v || !c.o || !c.block_map || !c.q_sizes || !c.k_sizes || !c.workspace) return SVG_ERR_BAD_ARG;
    if (c.Hq <= 0 || c.Hkv <= 0 || c.Hq % c.Hkv != 0 || c.Sq <= 0 || c.Skv <= 0 || c.QB <= 0 || c.KB <= 0) return SVG_ERR_BAD_ARG;
    if (fp8 && (c.D != 128 || c.QB >= 32768 || c.Sq / 256 + 1 >= 65536)) return SVG_ERR_UNSUPPORTED;
    if (c.KB > kVbMaxKB) return SVG_ERR_UNSUPPORTED;
    if (check_rows(c.Sq, c.D) != SVG_OK || check_rows(c.Skv, c.D) != SVG_OK) return SVG_ERR_UNSUPPORTED;
    const size_t need = fp8 ? svg_varblock_attention_fp8_workspace_bytes(c.Hq, c.Hkv, c.QB, c.KB, c.Sq, c.Skv, c.D)
                            : svg_varblock_workspace_bytes(c.Hq, c.Hkv, c.QB, c.KB, c.Sq);
    return c.workspace_bytes < need ? SVG_ERR_WORKSPACE : SVG_OK;
}

// `variant` of svg_varblock_attention (-1 ... 9, include/svg_attn.h) -> body, block-row order, trace and order mode; false otherwise.
// 0: 4 waves, 128-row q tiles; 1: 8 waves, 256-row q tiles; 2: mixed (full 256-row tiles on 8 waves, rest on 4)
// (6 = 3: the longest-first order is the default again — the similarity order, variant 7, raised the L2 hit rate from 31 % to 48 %
//  and cut the L2 <-> fabric traffic by a quarter but not the kernel time, and its chain kernel costs 0.7 - 1.0 ms per call)
// two-phase body (variant >= 3): on 16x16x32 MFMAs at head_dim 128 (attn_m16.h: 28.3 vs 29.1 ms at Wan 720p, profiles/r04d_ab_svg2_m16_first.txt);
// 8 = 3 with that body named explicitly, 9 = 3 on the 32x32x16 body (A/B)
// -1 (auto): 256-row q tiles with the two-phase ping-pong body once the average block-row is large enough to fill them
// (Wan 720p, 252-row clusters: 40.4 ms; lock-step 8 waves 45.5, 4 waves 47.7, mixed 46.9), 128-row tiles otherwise
static bool vb_decode_variant(int variant, VbCall& c) {
    const bool force_pp2 = (variant == 9);
    if (variant == 8 || variant == 9) variant = 3;
    if (variant < -1 || variant > 7) return false;
    c.block_row_order = (variant == 4), c.trace = (variant == 5);
    c.order_mode = variant == 7 ? 2 : (variant == 6 ? 1 : 0);
    if (variant == -1) variant = ((int64_t)c.Sq >= (int64_t)160 * c.QB) ? 3 : 0;
    c.body = variant == 0   ? VbBody::kLockstep128
             : variant == 1 ? VbBody::kLockstep256
             : variant == 2 ? VbBody::kMixed
             : (c.D == 128 && !force_pp2) ? VbBody::kM16
                                          : VbBody::kPP2;
    return true;
}

// svg_varblock_attention (layout == nullptr: contiguous [H, S, D] tensors) and svg_varblock_attention_strided
static int varblock_entry(VbCall& c, int variant, const svg_attn_layout_t* layout) {
    if (const int rc = varblock_check_args(c, false); rc != SVG_OK) return rc;
    AttnLayout lay;
    if (layout) {
        if (const int rc = layout_from_abi(layout, c.Hq, c.Hkv, c.Sq, c.Skv, c.D, c.q, c.k, c.v, c.o, lay); rc != SVG_OK) return rc;
        c.lay = &lay;
    }
    if (!vb_decode_variant(variant, c)) return SVG_ERR_BAD_ARG;
    if (c.lse && (c.D != 128 || c.body != VbBody::kM16 || c.trace || c.block_row_order)) return SVG_ERR_UNSUPPORTED;   // (fp32 etc.: dispatch_td)
    if (c.o32 && ((size_t)c.o32 & 15) != 0) return SVG_ERR_UNSUPPORTED;   // 16-byte stores
    const bool two_phase = c.body == VbBody::kM16 || c.body == VbBody::kPP2;
    if (c.lay && !(two_phase && !c.trace)) return SVG_ERR_UNSUPPORTED;   // strided tensors: the two-phase bodies only (see svg_attn_layout_t)
    return dispatch_td(c.dtype, c.D, [&](auto t, auto d) { return run_varblock<decltype(t), decltype(d)::value>(c); });
}

extern "C" int svg_varblock_attention(const void* q, const void* k, const void* v, void* o, int32_t Hq, int32_t Hkv,
                                      int32_t Sq, int32_t Skv, int32_t D, int32_t dtype, float sm_scale,
                                      const uint8_t* block_map, const int32_t* q_sizes, const int32_t* k_sizes, int32_t QB,
                                      int32_t KB, const int32_t* q_row_idx, const int32_t* kv_row_idx, void* workspace,
                                      size_t workspace_bytes, int32_t variant, void* stream) {
    VbCall c{q, k, v, o, Hq, Hkv, Sq, Skv, D, dtype, sm_scale, block_map, q_sizes, k_sizes, QB, KB, q_row_idx, kv_row_idx, workspace,
             workspace_bytes, (hipStream_t)stream};
    return varblock_entry(c, variant, nullptr);
}

extern "C" int svg_varblock_attention_strided(const void* q, const void* k, const void* v, void* o, int32_t Hq, int32_t Hkv,
                                              int32_t Sq, int32_t Skv, int32_t D, int32_t dtype, float sm_scale,
                                              const uint8_t* block_map, const int32_t* q_sizes, const int32_t* k_sizes, int32_t QB,
                                              int32_t KB, const int32_t* q_row_idx, const int32_t* kv_row_idx, void* workspace,
                                              size_t workspace_bytes, const svg_attn_layout_t* layout, void* stream) {
    if (!layout) return SVG_ERR_BAD_ARG;
    VbCall c{q, k, v, o, Hq, Hkv, Sq, Skv, D, dtype, sm_scale, block_map, q_sizes, k_sizes, QB, KB, q_row_idx, kv_row_idx, workspace,
             workspace_bytes, (hipStream_t)stream};
    return varblock_entry(c, -1, layout);
}

// always the two-phase 16x16x32 body in its default launch order: what variant 3 selects, also where -1 would pick 128-row tiles
extern "C" int svg_varblock_attention_lse(const void* q, const void* k, const void* v, void* o, float* lse, int32_t Hq, int32_t Hkv,
                                          int32_t Sq, int32_t Skv, int32_t D, int32_t dtype, float sm_scale, const uint8_t* block_map,
                                          const int32_t* q_sizes, const int32_t* k_sizes, int32_t QB, int32_t KB,
                                          const int32_t* q_row_idx, const int32_t* kv_row_idx, void* workspace, size_t workspace_bytes,
                                          const svg_attn_layout_t* layout, void* stream) {
    if (!lse) return SVG_ERR_BAD_ARG;
    VbCall c{q, k, v, o, Hq, Hkv, Sq, Skv, D, dtype, sm_scale, block_map, q_sizes, k_sizes, QB, KB, q_row_idx, kv_row_idx, workspace,
             workspace_bytes, (hipStream_t)stream};
    c.lse = lse;
    return varblock_entry(c, 3, layout);
}

// o32 travels in the place of o through varblock_entry (its null check); of `layout` the o member is not read: it takes q's strides
extern "C" int svg_varblock_attention_lse_f32(const void* q, const void* k, const void* v, float* o32, float* lse, int32_t Hq, int32_t Hkv,
                                              int32_t Sq, int32_t Skv, int32_t D, int32_t dtype, float sm_scale, const uint8_t* block_map,
                                              const int32_t* q_sizes, const int32_t* k_sizes, int32_t QB, int32_t KB,
                                              const int32_t* q_row_idx, const int32_t* kv_row_idx, void* workspace, size_t workspace_bytes,
                                              const svg_attn_layout_t* layout, void* stream) {
    if (!o32 || !lse) return SVG_ERR_BAD_ARG;
    VbCall c{q, k, v, layout ? const_cast<void*>(q) : (void*)o32, Hq, Hkv, Sq, Skv, D, dtype, sm_scale, block_map, q_sizes, k_sizes, QB, KB,
             q_row_idx, kv_row_idx, workspace, workspace_bytes, (hipStream_t)stream};
    c.lse = lse, c.o32 = o32;
    svg_attn_layout_t abi{};
    if (layout) abi = *layout, abi.o = abi.q;
    return varblock_entry(c, 3, layout ? &abi : nullptr);
}

extern "C" int svg_varblock_attention_fp8(const void* q, const void* k, const void* v, void* o, int32_t Hq, int32_t Hkv, int32_t Sq,
                                          int32_t Skv, int32_t D, int32_t dtype, float sm_scale, const uint8_t* block_map,
                                          const int32_t* q_sizes, const int32_t* k_sizes, int32_t QB, int32_t KB,
                                          const int32_t* q_row_idx, const int32_t* kv_row_idx, void* workspace, size_t workspace_bytes,
                                          void* stream) {
    VbCall c{q, k, v, o, Hq, Hkv, Sq, Skv, D, dtype, sm_scale, block_map, q_sizes, k_sizes, QB, KB, q_row_idx, kv_row_idx, workspace,
             workspace_bytes, (hipStream_t)stream};
    if (const int rc = varblock_check_args(c, true); rc != SVG_OK) return rc;
    c.body = VbBody::kF8;
    char* const f8_ws = (char*)workspace + ((svg_varblock_workspace_bytes(Hq, Hkv, QB, KB, Sq) + 255) & ~(size_t)255);
    if (const int rc = f8g_quantize(q, k, v, Hq, Hkv, Sq, Skv, dtype, sm_scale, f8_ws, &c.f8, c.st); rc != SVG_OK) return rc;
    return dispatch_td(dtype, D, [&](auto t, auto d) { return run_varblock<decltype(t), decltype(d)::value>(c); });
}

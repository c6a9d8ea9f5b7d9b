// SVG2 variable-block policy for the attention bodies of attn_core.h / attn_m16.h / attn_f8.h.  The kernels that instantiate it, the
// planning kernels and the host path are attention_varblock.hip; tests/test_schedule_model.py mirrors the policy line by line.
#pragma once
#include "attn_core.h"

namespace svg {

// =====================================================================================================
// Variable-block policy (SVG2): q rows of block-row i attend the kv rows of the active block-cols.
// The active, non-empty column blocks of the workgroup's block-row are compacted into a run list in LDS
// (start, inclusive prefix of lengths); KV tiles are cut from the *concatenation* of the runs, so tiles are
// always full except the last one — no per-cluster padding waste on the key side.
// =====================================================================================================
constexpr int kVbMaxKB = 4032;   // the run list of a block-row ((KB rounded up to 64) + 2 pairs of ints) has to fit beside the four 32 KB stages in 160 KB of LDS
constexpr int kVbFull = 256;   // mixed tiling: full 256-row tiles go to the 8-wave kernel, the rest of a block-row to 128-row tiles

template <typename T, int D, int NW>
struct VarblockPolicy : LayoutAccess<VarblockPolicy<T, D, NW>> {
    static constexpr bool kFixup = false;
    static constexpr bool kPartialOut = false;
    static constexpr bool kIntervalMask = true;
    static constexpr bool kFastPartial = false;
    static constexpr int kShadow128 = 2;   // the vector phase also resolves rows through the run list and the index arrays
    static constexpr bool kOneBarrier = true;   // two-phase body: one barrier per tile (attn_core.h kOneBar: -1.7 % at Wan 720p)
    static constexpr int kRowBlocks = 1;
    static constexpr int BM = NW * 32;

    struct Params {
        const T* q;
        const T* k;
        const T* v;
        T* o;
        int Hq, Hkv, group, Sq, Skv, QB, KB, max_tiles, kb_cap;
        int tile_mode;              // 0: ceil(n / BM) tiles per block-row; 1: only its full 256-row tiles; 2: its rows after them
        float scale_log2;
        const uint8_t* block_map;   // [Hkv, QB, KB]
        const int32_t* q_off;       // [Hkv, QB + 1] exclusive prefix of q_sizes
        const int32_t* k_off;       // [Hkv, KB + 1]
        const int32_t* tile_off;    // [Hkv, QB + 1] exclusive prefix of ceil(q_size / BM)
        const int32_t* order;       // launch order (or nullptr): [0] = #workgroups, then triples (hq, block-row << 16 | sub-tile, partner):
                                    // partner >= 0: the ragged last tile of that block-row also carries the ragged last tile of block-row
                                    // `partner` (same kv head) — "remainder packing", see varblock_pair_kernel
        const int32_t* q_row_idx;   // [Hq, Sq] or null
        const int32_t* kv_row_idx;  // [Hkv, Skv] or null
        AttnLayout lay;             // strides of q, k, v, o (contiguous [H, S, D] unless the call came through svg_varblock_attention_strided)
    };
    struct Ctx {
        int hq, hkv, q0, q_end, nT, total;  // q rows [q0, q_end) in permuted coordinates; total = active keys
        // Remainder packing: tile rows [0, ra) are the rows [q0, q_end) of the block-row ("member A"), tile rows [ra, ra + rb) the last rb
        // rows of the partner block-row ("member B", permuted positions jb0 ...).  The run list holds the key blocks both members
        // attend first (kC keys), then those only A attends (up to kCA), then those only B attends (up to total): a row of A may see
        // [0, kCA), a row of B [0, kC) u [kCA, total) — two intervals per row, which is what the bodies' masks take.  Without a
        // partner rb = 0 and kC = kCA = total.
        int ra, rb, jb0, kC, kCA;
        // per WAVE (like BandPolicy::fk_lo): key ranges on which every row of the wave may see every key (FULL tiles) and on which some
        // row may see some key (anything else is SKIP)
        int f1_lo, f1_hi, f2_lo, f2_hi, any1_hi, any2_lo;
        // LDS run list: .x = inclusive prefix of the run lengths (the end of run j in compact coordinates), .y = permuted start
        // position of run j minus the compact position it starts at — one 8-byte read resolves a key: perm = pos + .y
        const int2* run;
        const int32_t* qidx;
        const int32_t* kidx;
        int nruns;
    };
    struct KvCursor {
        int j;
        int2 r, rn;   // run[j] and run[j + 1], kept across tiles: a lane crosses into the next run every other tile (mean run: 119
    };            // keys) and then finds the entry in a register; the read that refills rn has until the next crossing to land

    static __device__ __forceinline__ bool init(const Params& p, Ctx& c, char* plds) {
        int i, sub, partner = -1;
        if (p.order) {   // 1-D grid in longest-first order (varblock_scatter_kernel)
            const int b = blockIdx.x;
            if (b >= p.order[0]) return false;
            c.hq = p.order[2 + 3 * b];
            const int e = p.order[3 + 3 * b];
            partner = p.order[4 + 3 * b];
            i = e >> 16, sub = e & 0xFFFF;
            c.hkv = c.hq / p.group;
        } else {
            c.hq = blockIdx.y;
            c.hkv = c.hq / p.group;
            const int32_t* toff = p.tile_off + (size_t)c.hkv * (p.QB + 1);
            const int w = blockIdx.x;
            if (w >= toff[p.QB]) return false;
            // block-row i with tile_off[i] <= w < tile_off[i+1]
            int a = 0, bnd = p.QB;
            while (bnd - a > 1) {
                const int mid = (a + bnd) >> 1;
                if (toff[mid] <= w) a = mid; else bnd = mid;
            }
            i = a;
            sub = w - toff[i];
        }
        const int32_t* qoff = p.q_off + (size_t)c.hkv * (p.QB + 1);
        const int base = qoff[i] + (p.tile_mode == 2 ? ((qoff[i + 1] - qoff[i]) / kVbFull) * kVbFull : 0);
        c.q0 = base + sub * BM;
        c.q_end = min(qoff[i + 1], c.q0 + BM);
        c.ra = max(c.q_end - c.q0, 0), c.rb = 0, c.jb0 = 0;
        if (partner >= 0) {   // the partner's ragged last tile: its last (size % BM) rows
            const int nj = qoff[partner + 1] - qoff[partner];
            c.rb = nj % BM;
            c.jb0 = qoff[partner + 1] - c.rb;
        }
        c.qidx = p.q_row_idx ? p.q_row_idx + (size_t)c.hq * p.Sq : nullptr;
        c.kidx = p.kv_row_idx ? p.kv_row_idx + (size_t)c.hkv * p.Skv : nullptr;

        // ---- compact the active non-empty column blocks into the LDS run list: one pass per class of key blocks
        //      (both members | only A | only B; without a partner everything is the first class) ----
        int2* run = (int2*)plds;
        int32_t* wave_cnt = (int32_t*)(run + p.kb_cap + 2);  // [NW] counts, [NW] lengths
        const uint8_t* mrow = p.block_map + ((size_t)c.hkv * p.QB + i) * p.KB;
        const uint8_t* mrow2 = partner >= 0 ? p.block_map + ((size_t)c.hkv * p.QB + partner) * p.KB : mrow;
        const int32_t* koff = p.k_off + (size_t)c.hkv * (p.KB + 1);
        const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
        constexpr int NT = NW * 64;
        int base_cnt = 0, base_len = 0;
        auto scan_class = [&](int want) {   // want: 3 = both, 1 = only A, 2 = only B
            for (int j0 = 0; j0 < p.KB; j0 += NT) {
                const int j = j0 + tid;
                int len = 0, st = 0;
                if (j < p.KB) {
                    const int cls = (mrow[j] ? 1 : 0) | (mrow2[j] ? 2 : 0);
                    if (cls == want) {
                        st = koff[j];
                        len = koff[j + 1] - st;
                    }
                }
                const int flag = len > 0;
                int icnt = flag, ilen = len;
#pragma unroll
                for (int o = 1; o < 64; o <<= 1) {
                    const int t1 = __shfl_up(icnt, o), t2 = __shfl_up(ilen, o);
                    if (lane >= o) icnt += t1, ilen += t2;
                }
                __syncthreads();  // previous round's readers of wave_cnt are done
                if (lane == 63) wave_cnt[wv] = icnt, wave_cnt[NW + wv] = ilen;
                __syncthreads();
                int wc = base_cnt, wl = base_len;
                for (int x = 0; x < wv; ++x) wc += wave_cnt[x], wl += wave_cnt[NW + x];
                if (flag) {
                    run[wc + icnt - 1] = make_int2(wl + ilen, st - (wl + ilen - len));
                }
                for (int x = 0; x < NW; ++x) base_cnt += wave_cnt[x], base_len += wave_cnt[NW + x];
            }
        };
        scan_class(3);
        c.kC = base_len;
        if (partner >= 0) {
            scan_class(1);
            c.kCA = base_len;
            scan_class(2);
        } else {
            c.kCA = base_len;
        }
        // two sentinels behind the last run: the cursor (kv_phys_at) reads one entry ahead and stops at them
        if (tid < 2) run[base_cnt + tid] = make_int2(0x7fffffff, 0);
        __syncthreads();
        c.nruns = base_cnt;
        c.total = base_len;
        c.run = run;
        c.nT = (c.total + kBN - 1) / kBN;
        // per-wave tile classes: rows of this wave = tile rows [w0, w1)
        {
            const int w0 = wave_id() * 32, w1 = min(w0 + 32, c.ra + c.rb);
            const bool only_a = w1 <= c.ra, only_b = w0 >= c.ra;
            c.f1_lo = 0, c.f1_hi = only_a ? c.kCA : c.kC;                 // every row of the wave sees all of [f1_lo, f1_hi)
            c.f2_lo = c.kCA, c.f2_hi = only_b ? c.total : c.kCA;          // ... and of [f2_lo, f2_hi)
            c.any1_hi = only_a ? c.kCA : (only_b ? c.kC : c.total);        // some row sees some key of [0, any1_hi) u [any2_lo, total)
            c.any2_lo = only_b ? c.kCA : c.total;
        }
        return true;
    }

    static __device__ __forceinline__ int q_head(const Ctx& c) { return c.hq; }    // LayoutAccess: q_base .. o_base, q_rs .. o_rs
    static __device__ __forceinline__ int kv_head(const Ctx& c) { return c.hkv; }

    // (the "logical" index of a query row is its row inside the tile here: all the mask needs is which member it belongs to)
    static __device__ __forceinline__ int q_logical(const Ctx&, int row) { return row; }
    static __device__ __forceinline__ bool wave_active(const Ctx& c, int wrow0) { return wrow0 < c.ra + c.rb; }
    static __device__ __forceinline__ int q_phys(const Params&, const Ctx& c, int row) {
        if (row >= c.ra + c.rb) return -1;
        const int l = row < c.ra ? c.q0 + row : c.jb0 + (row - c.ra);
        return c.qidx ? c.qidx[l] : l;
    }
    static __device__ __forceinline__ int tile_key0(const Ctx&, int t) { return t * kBN; }
    struct TileCur {
        int k0;
    };
    static __device__ __forceinline__ void tile_cur_init(const Ctx&, TileCur& tc) { tc.k0 = 0; }
    static __device__ __forceinline__ void tile_cur_next(const Ctx&, TileCur& tc) { tc.k0 += kBN; }
    static __device__ __forceinline__ void tile_cur_step(TileCur& tc) { tc.k0 += kBN; }
    static __device__ __forceinline__ bool tile_cur_ended(const TileCur&) { return false; }
    static __device__ __forceinline__ void tile_cur_fix(const Ctx&, TileCur&) {}
    static constexpr bool kRowStep = false;   // rows come from the run list (kv_phys_at), resolved between the phases
    static __device__ __forceinline__ bool fast_full(const Ctx& c, int k0) {
        return (k0 >= c.f1_lo && k0 + kBN <= c.f1_hi) || (k0 >= c.f2_lo && k0 + kBN <= c.f2_hi);
    }
    static __device__ __forceinline__ void kv_cursor_init(const Params&, const Ctx& c, KvCursor& cu, int) {
        cu.j = 0;
        cu.r = c.run[0], cu.rn = c.run[1];   // (entries behind the last run are never used: a key behind the last run is clamped)
    }
    static __device__ __forceinline__ int kv_phys(const Params& p, const Ctx& c, KvCursor& cu, int t, int row) {
        return kv_phys_at(p, c, cu, t * kBN, row);
    }
    static __device__ __forceinline__ int kv_phys_at(const Params&, const Ctx& c, KvCursor& cu, int k0, int row) {
        // compact coordinate; keys behind the last one (ragged last tile; masked by allowed()) read the last key: no branch
        const int pos = min(k0 + row, c.total - 1);
        int j = cu.j;
        int2 r = cu.r, rn = cu.rn;
        while (r.x <= pos) {   // tiles advance monotonically: amortised O(1)
            r = rn;
            ++j;
            rn = c.run[j + 1];
        }
        cu.j = j, cu.r = r, cu.rn = rn;
        const int perm = pos + r.y;
        return c.kidx ? c.kidx[perm] : perm;
    }
    static __device__ __forceinline__ int classify(const Params&, const Ctx& c, int k0, int wrow0) {
        if (wrow0 >= c.ra + c.rb) return TILE_SKIP;
        if (fast_full(c, k0)) return TILE_FULL;
        // no row of the wave sees any key of the tile (a tile of the other member's own key blocks): nothing to compute
        const bool any = (k0 < c.any1_hi) || (k0 + kBN > c.any2_lo && k0 < c.total);
        return any ? TILE_PARTIAL : TILE_SKIP;
    }
    static __device__ __forceinline__ bool allowed(const Params&, const Ctx& c, int row, int k) {
        return row < c.ra ? (k < c.kCA) : ((k < c.kC) | ((k >= c.kCA) & (k < c.total)));
    }
    static __device__ __forceinline__ void row_intervals(const Params&, const Ctx& c, int row, int& a0, unsigned& alen, int& b0,
                                                         unsigned& blen) {
        const bool a = row < c.ra;
        a0 = 0, alen = (unsigned)(a ? c.kCA : c.kC), b0 = c.kCA, blen = a ? 0u : (unsigned)(c.total - c.kCA);
    }
    static __device__ __forceinline__ void notify(const Params&, const Ctx&) {}
    static __device__ __forceinline__ float score_fixup(const Params&, float s) { return s; }
};

// LSE form (svg_varblock_attention_lse): the head_dim-128 policy of the 16x16x32 body plus the row log-sum-exp (attn_m16.h: HasRowLse,
// switched on by lse_base below), as CrossLsePolicy adds it to the cross policy.  lse is a contiguous fp32 [Hq, Sq] whatever the layout
// of q / o, one row per q head (GQA: not per kv head); the index inside a head is the row q_phys returns — the caller's row order under
// q_row_idx, for both members of a packed q-tile.  A row whose block-row has no key (or only empty key clusters) gets -inf.
template <typename T>
struct VarblockLsePolicy : VarblockPolicy<T, 128, 8> {
    using Base = VarblockPolicy<T, 128, 8>;
    struct Params : Base::Params {
        float* lse;   // [Hq, Sq]
    };
    static __device__ __forceinline__ float* lse_base(const Params& p, const typename Base::Ctx& c) { return p.lse + (size_t)c.hq * (size_t)p.Sq; }
};

// fp32 form (svg_varblock_attention_lse_f32): the LSE policy plus the rows before their rounding (attn_m16.h: HasRowO32, switched on by
// o32_base below), as CrossF32Policy adds them to the cross policy.  o32 is a contiguous fp32 [Hq, Sq, 128] whatever the layout of q, the
// row inside a head the one lse uses; Params::o is not used.
template <typename T>
struct VarblockF32Policy : VarblockLsePolicy<T> {
    using Base = VarblockLsePolicy<T>;
    struct Params : Base::Params {
        float* o32;   // [Hq, Sq, 128]
    };
    static __device__ __forceinline__ float* o32_base(const Params& p, const typename Base::Ctx& c) {
        return p.o32 + (size_t)c.hq * (size_t)p.Sq * 128;
    }
};

static inline int vb_policy_lds(int kb_cap) { return (2 * (kb_cap + 2) + 32) * (int)sizeof(int32_t); }

}  // namespace svg

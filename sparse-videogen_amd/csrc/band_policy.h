// SVG1 band policy (analytic mask family, see svg_band_mask_t in svg_attn.h) for the attention bodies of attn_core.h / attn_w4.h:
// which KV tiles a workgroup visits, where rows live in HBM, which elements are masked — plus the work queue of the resident
// kernels and the host-side parameter builder, for the translation units that instantiate band kernels (attention.hip,
// attention_w4.hip, attention_f8.hip).  The launch helpers are svg_common.h; the variable-block policy is varblock_policy.h.
#pragma once
#include <algorithm>
#include <type_traits>
#include <utility>

#include "attn_core.h"

namespace svg {

// One band call, from its entry to its launch (no process- or thread-global state): what every svg_band_attention* entry is given, in the
// entries' order, then what single entries add.  An entry fills one and hands it to band_run (attention.hip); the parameter builders below
// and the launchers read it.
enum BandForm : int { kBandWhole = 0, kBandWindow, kBandShard, kBandPerHead };
struct BandCall {
    const void *q = nullptr, *k = nullptr, *v = nullptr;
    void* o = nullptr;         // (the *_f32 entries leave it null: band_run puts a stand-in of o32 here)
    int32_t BH = 0, S = 0, D = 0, dtype = 0;
    float sm_scale = 1.f;
    const svg_band_mask_t* mask = nullptr;
    const svg_perm_desc_t* perm = nullptr;
    const svg_attn_layout_t* layout = nullptr;   // the tensors as the ABI describes them, or nullptr: contiguous [BH, S, D]
    hipStream_t stream = nullptr;
    int32_t variant = 0;       // schedule (svg_band_attention); 0: the default of the head size
    int32_t* done = nullptr;   // completion counters (svg_band_attention_notify*), or nullptr
    int32_t done_words = 0;    // ... as many words
    int done_nseg = 1;         // counters per head
    bool prescaled = false;    // q carries sm_scale * log2(e) (svg_band_attention_prescaled; two-phase body only)
    bool trace = false;        // diagnostics builds: the traced kernel (svg_debug_pp_trace)
    int trace_abl = 0;         // ... and its timing ablation
    bool strided = false;      // `lay` describes the tensors (set with `layout`; svg_band_attention_strided sets it whatever `layout` is)
    AttnLayout lay{};          // `layout`, checked (band_run)
    // device switch (svg_band_attention_switch*): `*use_alt != 0` on the device selects alt_mask without the layout permutation
    const svg_band_mask_t* alt_mask = nullptr;
    const int32_t* use_alt = nullptr;
    float* lse = nullptr;      // row log-sum-exp output, contiguous fp32 [BH, S] (svg_band_attention_lse: BandLsePolicy), or nullptr
    float* o32 = nullptr;      // with lse: fp32 rows, contiguous [BH, S, 128], instead of o (svg_band_attention_lse_f32: BandF32Policy)
    BandForm form = kBandWhole;
    // kBandWindow (with lse): q / o / lse / o32 hold the rows [q_begin, q_begin + win_Sq), k / v the keys [k_begin, k_begin + win_Sk)
    int32_t q_begin = 0, win_Sq = 0, k_begin = 0, win_Sk = 0;
    // kBandShard (with lse): q / o / lse / o32 hold the rows of q_shard, k / v those of k_shard (BandShardOf)
    const svg_band_shard_t* q_shard = nullptr;
    const svg_band_shard_t* k_shard = nullptr;
    // kBandPerHead (with lse): one band per head (BandPerHeadLsePolicy), on the work queue where `queue` is set and a queue is to be had
    const int32_t* band = nullptr;
    bool queue = false;

    // rows of q / o and of k / v: the window's, the (checked) shard's of the video `perm` describes, or S
    static int shard_rows(const svg_band_shard_t* s, const svg_perm_desc_t* perm) { return perm->frame_size * s->n_frames + s->n_tail; }
    int Sq() const { return form == kBandWindow ? win_Sq : form == kBandShard ? shard_rows(q_shard, perm) : S; }
    int Sk() const { return form == kBandWindow ? win_Sk : form == kBandShard ? shard_rows(k_shard, perm) : S; }
};

// the mask and the head permutation of a band call over S rows (mask != nullptr)
inline int check_band_mask(int S, const svg_band_mask_t* mask, const svg_perm_desc_t* perm) {
    if (mask->real_len < 0 || mask->real_len > S || mask->band < 0 || mask->band > S + 1) return SVG_ERR_BAD_ARG;
    if (mask->colfull_lo > mask->colfull_hi || mask->rowfull_lo > mask->rowfull_hi) return SVG_ERR_BAD_ARG;
    if (perm && perm->head_perm_flag) {
        if (perm->num_frame <= 0 || perm->frame_size <= 0 || perm->vid0 < 0 ||
            (int64_t)perm->vid0 + (int64_t)perm->num_frame * perm->frame_size > S)
            return SVG_ERR_BAD_ARG;
    }
    return SVG_OK;
}

// does a policy's Ctx carry a band of its own (BandPerHeadLsePolicy: one band per head)?  See BandPolicy::band_of.
template <typename C, typename = void>
struct CtxHasBand : std::false_type {};
template <typename C>
struct CtxHasBand<C, std::void_t<decltype(std::declval<const C&>().band)>> : std::true_type {};

// =====================================================================================================
// Band policy: analytic mask family (see svg_band_mask_t in svg_attn.h)
// =====================================================================================================
template <typename T, int D, int NW, int RB = 1>
struct BandPolicy : LayoutAccess<BandPolicy<T, D, NW, RB>> {
    static constexpr int kHeadDim = D;
    static constexpr bool kFixup = false;
    static constexpr bool kPartialOut = false;
    static constexpr bool kIntervalMask = true;   // row_intervals() describes the mask (two-phase body)
    static constexpr bool kFastPartial = false;
    static constexpr int kShadow128 = 1;   // two-phase body, D = 128: probability steps in the MFMA shadow (measured best)
    static constexpr bool kOneBarrier = false;   // two-phase body: two barriers per tile (one measured neutral for this policy)
    static constexpr int kRowBlocks = RB;    // 32-row blocks per wave
    static constexpr int kWR = 32 * RB;      // rows per wave
    static constexpr int BM = NW * kWR;

    struct Params {
        const T* q;
        const T* k;
        const T* v;
        T* o;
        int S, BH, nqt;
        float scale_log2;
        int real_len, band, cf_lo, cf_hi, rf_lo, rf_hi;
        const int64_t* head_flag;
        int vid0, F, P, V;
        int q64, r64;          // 64 / F, 64 % F: tile-to-tile step of the (patch, frame) decomposition
        int q128, r128;        // the same for a 128-row step (unused since the two-tiles-per-stage schedule went; kept: argument layout)
        int sp64, sp128;       // physical-row step of a token-major head: q + r * P (the patch index advances by q, the frame by r)
        int wrap_phys;         // 1 - F * P: correction when the frame index wraps
        int heavy_lo, n_heavy; // q-tiles [heavy_lo, heavy_lo + n_heavy) of every head see ALL keys (text rows): scheduled first
        // Row regions: q-tiles never straddle rowfull_lo / rowfull_hi / real_len, so every q-tile is homogeneous (band rows, full
        // rows or rows behind real_len).  Region r = rows [reg_lo[r], reg_hi[r]), its first q-tile is reg_t0[r].
        int reg_lo[4], reg_hi[4], reg_t0[4];
        // completion counters (or nullptr): every wave of a workgroup adds 1 to done[head] after its last store, so done[h] ==
        // 8 * (q-tiles of a head) means head h of O is complete and visible — a consumer on another stream (svg_wait_counters) can
        // start exchanging it while the launch is still working on the next heads (dispatch is head-major)
        int32_t* done;             // int32 [BH * done_nseg + BH]: segment counters, then one hidden counter per head (see notify)
        int done_nseg, done_tps;   // counters per head: segment of q-tile qt (row order) = min(qt / done_tps, done_nseg - 1)
        AttnLayout lay;            // strides of q, k, v, o (contiguous [BH, S, D] unless the call came through a *_strided entry point)
    };
    struct Ctx {
        int head, qt, q0, q_end, nT, perm;
        int seg_lo[3], seg_n[3];
        int fk_lo, fk_hi;  // per WAVE: tiles with first key in [fk_lo, fk_hi] are FULL for this wave's 32 rows (fast path)
    };
    struct KvCursor {
        int physv, f, prev_k0;  // token-major head: frame f and physical row vid0 + f * P + pp of this thread's row in the previous tile,
    };                          // with (row - vid0) = pp * F + f

    static __device__ __forceinline__ int phys_row(const Params& p, const Ctx& c, int logical) {
        if (c.perm) {
            const unsigned i = (unsigned)(logical - p.vid0);
            if (i < (unsigned)p.V) {
                const unsigned pp = i / (unsigned)p.F;
                const unsigned f = i - pp * (unsigned)p.F;
                return p.vid0 + (int)(f * (unsigned)p.P + pp);
            }
        }
        return logical;
    }

    // The band of the q-tile c describes: the launch's (p.band), unless the policy's Ctx carries one of its own.  Every reader of the band
    // below goes through this with the type of the Ctx as a template argument; with this policy's own Ctx it is p.band and nothing else.
    template <typename C>
    static __host__ __device__ __forceinline__ int band_of(const Params& p, const C& c) {
        if constexpr (CtxHasBand<C>::value) return c.band;
        else return p.band;
    }

    static __device__ __forceinline__ bool init(const Params& p, Ctx& c, char*) {
        // Work mapping.  The hardware hands dispatch id b to XCD b % 8 and each XCD schedules its share on its own 32 CUs, so the
        // load has to be balanced across XCDs by construction.
        //  * longest-processing-time-first: the few q-tiles that contain text rows visit every KV tile, all of them on the
        //    masked path (~11x the time of a band tile at Hunyuan 720p).  They take the first dispatch ids, un-swizzled:
        //    first so that they do not form the tail of the launch, round-robin so that every XCD gets its share (with the
        //    swizzle below applied to them they all landed on XCD 0, which then ran 16 % longer than the other seven).
        //  * the remaining q-tiles: every XCD gets 32 neighbouring q-tiles of the same 256-tile window, so their KV windows
        //    overlap in that XCD's L2 while the whole chip stays within one or two heads (KV working set fits the 256 MiB
        //    Infinity Cache).
        int qt;
        const int nh = p.BH * p.n_heavy;
        const int b = blockIdx.x;
        if (b >= p.nqt * p.BH) return false;   // (the device-switched launch is sized for the larger of its two masks)
        if (b < nh) {
            c.head = b / p.n_heavy;
            qt = p.heavy_lo + (b - c.head * p.n_heavy);
        } else {
            const int b2 = b - nh;
            const int full = ((p.nqt * p.BH - nh) / (kNumXCD * 32)) * (kNumXCD * 32);
            int w2 = b2;
            if (b2 < full) {   // (dispatch id = work id instead measured 5 % slower: profiles/r06e_*)
                const int xcd = b2 % kNumXCD, s = b2 / kNumXCD;
                w2 = (s / 32) * (kNumXCD * 32) + xcd * 32 + (s % 32);
            }
            const int nl = p.nqt - p.n_heavy;
            c.head = w2 / nl;
            const int r = w2 - c.head * nl;
            qt = r < p.heavy_lo ? r : r + p.n_heavy;
        }
        init_tile(p, c, c.head, qt);
        return true;
    }

    // the rows, the KV schedule and the fast-path interval of q-tile `qt` (row order) of head `head`: everything of Ctx.  Split from
    // init() for the kernels that take their (head, q-tile) pairs from a work queue (BandQueue below) instead of blockIdx.
    static __device__ __forceinline__ void init_tile(const Params& p, Ctx& c, int head, int qt) {
        c.head = head;
        c.perm = (p.head_flag != nullptr) && (p.head_flag[c.head] != 0);
        kv_schedule(p, c, qt);
        // fast-path classification: inside the band, away from its edges, every (row, key) pair of a wave x tile
        // rectangle is allowed; those tiles (98-99 % of all) are recognised with two scalar compares.
        wave_fast_interval(p, c, wave_id(), c.fk_lo, c.fk_hi);
    }
    // the fast-path interval [lo, hi] of first keys for the rows of wave `wave` of the q-tile c describes (empty: lo > hi).  Also evaluated on
    // the host (svg_debug_band_tile_run).
    template <typename C>
    static __host__ __device__ __forceinline__ void wave_fast_interval(const Params& p, const C& c, int wave, int& lo, int& hi) {
#ifndef __HIP_DEVICE_COMPILE__   // (device: HIP's min / max, as init_tile always used them — std's select the other way round, and the
        using std::max;            //  listings of every kernel on this policy would move)
        using std::min;
#endif
        const int real = p.real_len;
        const int w0 = c.q0 + wave * kWR, w1 = min(w0 + kWR, c.q_end);
        lo = 1, hi = 0;
        if (w0 < c.q_end && w1 <= real) {
            const bool full_rows = w0 >= p.rf_lo && w1 <= p.rf_hi;   // a wave of full (text) rows: every key tile below real_len
            lo = full_rows ? 0 : max(w1 - band_of(p, c), 0);
            hi = min(full_rows ? real : w0 + band_of(p, c) - kBN, min(real, p.S) - kBN);
        }
    }

    // rows [q0, q_end) and key-tile segments of q-tile `qt` (row order); the same for every head.  Also evaluated on the host:
    // make_band_queue sorts the q-tiles of a launch by c.nT.
    template <typename C>
    static __host__ __device__ __forceinline__ void kv_schedule(const Params& p, C& c, int qt) {
        using std::max;
        using std::min;
        // (explicit selects: a run-time index into the kernel-argument arrays would go through scratch)
        const bool r1 = qt >= p.reg_t0[1], r2 = qt >= p.reg_t0[2], r3 = qt >= p.reg_t0[3];
        const int rlo = r3 ? p.reg_lo[3] : r2 ? p.reg_lo[2] : r1 ? p.reg_lo[1] : p.reg_lo[0];
        const int rhi = r3 ? p.reg_hi[3] : r2 ? p.reg_hi[2] : r1 ? p.reg_hi[1] : p.reg_hi[0];
        const int rt0 = r3 ? p.reg_t0[3] : r2 ? p.reg_t0[2] : r1 ? p.reg_t0[1] : 0;
        c.qt = qt;
        c.q0 = rlo + (qt - rt0) * BM;
        c.q_end = min(rhi, c.q0 + BM);

        // ---- KV schedule: up to three key intervals -> sorted, merged, tile-aligned ranges ----
        // (explicit scalars, no runtime-indexed arrays: keeps everything in SGPRs, no scratch)
        constexpr int BIG = 1 << 28;
        int alo = BIG, ahi = BIG, blo = BIG, bhi = BIG, clo = BIG, chi = BIG;
        const int real = p.real_len;
        if (c.q0 < real) {
            const int qr1 = min(c.q_end, real);
            if (c.q0 < p.rf_hi && qr1 > p.rf_lo) {
                alo = 0, ahi = (real + kBN - 1) / kBN;
            } else {
                alo = max(0, c.q0 - band_of(p, c) + 1) / kBN;
                ahi = (min(real, qr1 - 1 + band_of(p, c)) + kBN - 1) / kBN;
                const int ch = min(p.cf_hi, real);
                if (ch > p.cf_lo) blo = p.cf_lo / kBN, bhi = (ch + kBN - 1) / kBN;
            }
        }
        if (c.q_end > real) clo = real / kBN, chi = (p.S + kBN - 1) / kBN;
#define SVG_CSWAP(x, xh, y, yh) if (y < x) { int t_ = x; x = y; y = t_; t_ = xh; xh = yh; yh = t_; }
        SVG_CSWAP(alo, ahi, blo, bhi)
        SVG_CSWAP(blo, bhi, clo, chi)
        SVG_CSWAP(alo, ahi, blo, bhi)
#undef SVG_CSWAP
        if (blo < BIG && blo <= ahi) {
            ahi = max(ahi, bhi);
            blo = clo, bhi = chi, clo = BIG, chi = BIG;
            if (blo < BIG && blo <= ahi) ahi = max(ahi, bhi), blo = BIG, bhi = BIG;
        } else if (clo < BIG && clo <= bhi) {
            bhi = max(bhi, chi), clo = BIG, chi = BIG;
        }
        // (Round 4 tried a cyclic sweep start here — the 32 q-tiles an XCD works on together start at a common key tile and wrap, so that
        //  the group reads at most two different key tiles at any time — to cut the L2 <-> fabric traffic.  Measured: 87.9 GB per launch
        //  with all 32 on the same tile, 68.4 GB staggered by one tile, against 32.7 GB for the plain sweep, and 1 - 4.5 % more time: the
        //  L2 does not merge requests for a line that is still in flight.  Removed; profiles/r04z_rotate_traffic.txt, r04c_ab_rotate_stagger.txt.)
        c.seg_lo[0] = alo, c.seg_n[0] = ahi - alo;
        c.seg_lo[1] = blo, c.seg_n[1] = bhi - blo;
        c.seg_lo[2] = clo, c.seg_n[2] = chi - clo;
        c.nT = c.seg_n[0] + c.seg_n[1] + c.seg_n[2];
    }

    static __device__ __forceinline__ int q_logical(const Ctx& c, int row) { return c.q0 + row; }
    static __device__ __forceinline__ bool wave_active(const Ctx& c, int wrow0) { return c.q0 + wrow0 < c.q_end; }
    static __device__ __forceinline__ int q_phys(const Params& p, const Ctx& c, int row) {
        const int l = c.q0 + row;
        return l < c.q_end ? phys_row(p, c, l) : -1;
    }
    static __host__ __device__ __forceinline__ int tile_key0(const Ctx& c, int t) {
        // selects, not branches: this runs once per tile on the scalar unit of every wave
        const int n01 = c.seg_n[0] + c.seg_n[1];
        const int a = c.seg_lo[0] + t, b = c.seg_lo[1] + (t - c.seg_n[0]), d = c.seg_lo[2] + (t - n01);
        const int bd = t < n01 ? b : d;
        return (t < c.seg_n[0] ? a : bd) * kBN;
    }
    // Stateful form of tile_key0 for bodies that walk the tiles in order (attn_body_w4): ~3 scalar instructions per tile instead of
    // the ~10 of the three-way select above.  Behind the last tile the cursor holds harmless values.
    struct TileCur {
        int k0, left;       // first key of the tile, tiles left in its segment (this one included)
        int k1, left1;      // the segments behind it (scalars that shift down: a run-time index into the segment arrays of
        int k2, left2;      //  Ctx would send them through scratch)
    };
    static __device__ __forceinline__ void tile_cur_shift(TileCur& tc) {
        tc.k0 = tc.k1, tc.left = tc.left1;
        tc.k1 = tc.k2, tc.left1 = tc.left2;
        tc.left2 = 0;
    }
    static __device__ __forceinline__ void tile_cur_init(const Ctx& c, TileCur& tc) {
        tc.k0 = c.seg_lo[0] * kBN, tc.left = c.seg_n[0];
        tc.k1 = c.seg_lo[1] * kBN, tc.left1 = c.seg_n[1];
        tc.k2 = c.seg_lo[2] * kBN, tc.left2 = c.seg_n[2];
        if (tc.left <= 0) tile_cur_shift(tc);
        if (tc.left <= 0) tile_cur_shift(tc);
    }
    static __device__ __forceinline__ void tile_cur_next(const Ctx& c, TileCur& tc) {
        tile_cur_step(tc);
        if (tile_cur_ended(tc)) tile_cur_fix(c, tc);   // (rare: at most twice per q-tile)
    }
    // the same in two halves, for a caller that folds the rare case into a branch of its own
    static __device__ __forceinline__ void tile_cur_step(TileCur& tc) {
        tc.k0 += kBN;
        --tc.left;
    }
    static __device__ __forceinline__ bool tile_cur_ended(const TileCur& tc) { return tc.left <= 0; }
    static __device__ __forceinline__ void tile_cur_fix(const Ctx&, TileCur& tc) {
        tile_cur_shift(tc);
        if (tc.left <= 0) tile_cur_shift(tc);
    }
    // Branch-free row stepping for bodies that keep their phases straight-line (attn_body_w4): rows_seek places a lane on row
    // `row` of the tile that starts at key k0 (exact, with the division of a token-major head), rows_step advances it by one tile
    // inside a segment, rows_phys gives the physical row (0 for rows behind the sequence: those keys are masked).
    static constexpr bool kRowStep = true;
    struct RowState {
        int l, f, physv;   // logical row; token-major head: frame f and physical row vid0 + f * P + pp of (l - vid0) = pp * F + f
    };
    static __device__ __forceinline__ void rows_seek(const Params& p, const Ctx& c, RowState& st, int k0, int row) {
        st.l = k0 + row;
        const int i = st.l - p.vid0;
        const int a = i >= 0 ? i : -i - 1;              // floor division also for rows in front of the video
        const int qd = (int)((unsigned)a / (unsigned)p.F);
        const int pp = i >= 0 ? qd : -qd - 1;
        st.f = i - pp * p.F;
        st.physv = p.vid0 + st.f * p.P + pp;
    }
    static __device__ __forceinline__ void rows_step(const Params& p, const Ctx&, RowState& st) {
        st.l += kBN;
        int f = st.f + p.r64, physv = st.physv + p.sp64;
        const bool wrap = f >= p.F;
        st.f = wrap ? f - p.F : f;
        st.physv = wrap ? physv + p.wrap_phys : physv;
    }
    static __device__ __forceinline__ int rows_phys(const Params& p, const Ctx& c, const RowState& st) {
        const bool in_video = (unsigned)(st.l - p.vid0) < (unsigned)p.V;
        const int phys = (c.perm && in_video) ? st.physv : st.l;
        return st.l < p.S ? phys : 0;
    }
    // wave-uniform: every (row, key) pair of this wave's rows x the tile at key k0 is allowed (the per-wave interval of init())
    static __host__ __device__ __forceinline__ bool fast_full(const Ctx& c, int k0) { return k0 >= c.fk_lo && k0 <= c.fk_hi; }
    static __device__ __forceinline__ void kv_cursor_init(const Params&, const Ctx&, KvCursor& cu, int) {
        cu.physv = 0, cu.f = 0, cu.prev_k0 = -(1 << 30);
    }
    static __device__ __forceinline__ int kv_phys(const Params& p, const Ctx& c, KvCursor& cu, int t, int row) {
        return kv_phys_at(p, c, cu, tile_key0(c, t), row);
    }
    // the same for a tile given by its first key (a TileCur)
    static __device__ __forceinline__ int kv_phys_at(const Params& p, const Ctx& c, KvCursor& cu, int k0, int row) {
        const int l = k0 + row;
        if (!c.perm) return l < p.S ? l : 0;
        // token-major head: physical row = vid0 + f * P + pp with (l - vid0) = pp * F + f.  Consecutive tiles advance by 64 rows,
        // so the frame and the physical row are stepped (5 VALU, no multiply) instead of divided (~30 VALU); segment jumps re-divide.
        // A tile that lies inside the video range (scalar test) needs neither the range selects nor the bounds test.
        int f, physv;
        // a cursor advances by one tile (64 keys) per call
        const int delta = __builtin_amdgcn_readfirstlane(k0 - cu.prev_k0);
        if (delta == kBN) {
            f = cu.f + p.r64;
            physv = cu.physv + p.sp64;
            const bool wrap = f >= p.F;
            f = wrap ? f - p.F : f;
            physv = wrap ? physv + p.wrap_phys : physv;
        } else {
            const int i = l - p.vid0;
            const int a = i >= 0 ? i : -i - 1;              // floor division also for rows in front of the video
            const int qd = (int)((unsigned)a / (unsigned)p.F);
            const int pp = i >= 0 ? qd : -qd - 1;
            f = i - pp * p.F;
            physv = p.vid0 + f * p.P + pp;
        }
        cu.physv = physv, cu.f = f, cu.prev_k0 = k0;
        if (k0 >= p.vid0 && k0 + kBN <= p.vid0 + p.V) return physv;
        const bool in_video = (unsigned)(l - p.vid0) < (unsigned)p.V;
        const int phys = in_video ? physv : l;
        return l < p.S ? phys : 0;
    }

    // Row cursor of the 16x16x32 body (attn_m16.h picks it by HasRowCursor): ONE per-lane variable, the physical row of the lane's key
    // row in the latest resolved tile, stepped in place.  Everything that decides how a tile is resolved is wave-uniform and stays
    // on the scalar unit (RowWalk: loop constants of the q-tile and the first key of the latest resolved tile).
    //   cheap step   the tile follows the latest one (first key + kBN) and lies wholly inside [lo, hi + kBN): no bounds select.
    //                contiguous head: [lo, hi + kBN) = [.., S) and phys += kBN: one VALU instruction.
    //                token-major head: the tile AND the one before it lie inside the video (so every lane holds a video row), and with
    //                phys - vid0 = f * P + pp, x = phys + sp64 has left the video, x - vid0 >= F * P, exactly when the frame index
    //                wrapped (pp < P for a row inside the video): x += 1 - V then.  The frame index is no state.  Four instructions.
    //   exact        every other tile — the first of a q-tile, a segment jump, a tile that straddles an end of the video or S:
    //                row_exact, the division of kv_phys_at.
    static constexpr bool kRowCursor = true;
    struct RowWalk {
        int perm, lo, hi;        // token-major head?; first keys in [lo, hi] admit the cheap step
        int step, end, unwrap;   // physical-row step of a tile (sp64 or kBN); token-major head: vid0 + V, 1 - V (step and unwrap per lane on the device, see row_walk_init)
        int vlen;                // rows that are permuted: V or 0 (exact path)
        int prev_k0;             // first key of the latest resolved tile
    };
    static __host__ __device__ __forceinline__ void row_walk_init(const Params& p, const Ctx& c, RowWalk& w) {
        const bool perm = c.perm != 0;
        w.perm = perm;
        w.lo = perm ? p.vid0 + kBN : -(1 << 30);
        w.hi = (perm ? p.vid0 + p.V : p.S) - kBN;
        w.step = perm ? p.sp64 : kBN, w.end = p.vid0 + p.V, w.unwrap = 1 - p.V;
        w.vlen = perm ? p.V : 0;
        w.prev_k0 = -(1 << 30);
#ifdef __HIP_DEVICE_COMPILE__
        // the two addends of the token-major step live in VGPRs (opaque: not rematerialised from the arguments): the kernels are short
        // of SGPRs, not of VGPRs, and a constant that the allocator keeps in a spill lane costs a v_readlane per tile
        asm volatile("" : "+v"(w.step), "+v"(w.unwrap));
        // (and the head kind as an integer of its own: tested as the lane mask it was derived from, the compiler carries it into the
        //  exact path through a VGPR, two VALU instructions on every tile)
        w.perm = __builtin_amdgcn_readfirstlane(w.perm);
        asm volatile("" : "+s"(w.perm));
#endif
    }
    // wave-uniform: the tile at k0 takes the cheap step; records k0 as the latest resolved tile
    static __host__ __device__ __forceinline__ bool row_walk_cheap(RowWalk& w, int k0) {
        const bool cheap = (k0 == w.prev_k0 + kBN) & (k0 >= w.lo) & (k0 <= w.hi);
        w.prev_k0 = k0;
        return cheap;
    }
    // (device: every write of the cursor is one instruction with a tied operand, so the row stays in the register it lives in; as
    //  plain C++ the allocator keeps the old and the new row apart and copies one into the other on every tile)
    static __host__ __device__ __forceinline__ void row_add(int& phys, int d) {
#ifdef __HIP_DEVICE_COMPILE__
        asm("v_add_u32 %0, %0, %1" : "+v"(phys) : "v"(d));
#else
        phys += d;
#endif
    }
    static __host__ __device__ __forceinline__ void row_set(int& phys, int x) {
#ifdef __HIP_DEVICE_COMPILE__
        asm("v_mov_b32 %0, %1" : "+v"(phys) : "v"(x));
#else
        phys = x;
#endif
    }
    // (`vlen`: V on a token-major head, 0 on a contiguous one — no row is a video row there.  The head kind reaches this path as a
    //  number, not as a condition: a condition that is also live here is rebuilt through a VGPR at the head of every tile.)
    static __host__ __device__ __forceinline__ int row_exact(const Params& p, int vlen, int l) {
        const int i = l - p.vid0;
        const int a = i >= 0 ? i : -i - 1;              // floor division also for rows in front of the video
        const int qd = (int)((unsigned)a / (unsigned)p.F);
        const int pp = i >= 0 ? qd : -qd - 1;
        const int f = i - pp * p.F;
        const int physv = p.vid0 + f * p.P + pp;
        const bool in_video = (unsigned)i < (unsigned)vlen;
        const int phys = in_video ? physv : l;
        return l < p.S ? phys : 0;
    }
    // `phys`, the row of the lane (row `row` of a tile) in the latest resolved tile, becomes its row in the tile at k0.  (One-armed
    // branches on scalars, each around in-place writes: with the exact path as the else-arm of the step, the merge of "stepped" and
    // "divided" costs two copies of the cursor per tile.  A tile of the exact path steps first and overwrites the result.)
    static __host__ __device__ __forceinline__ void row_walk_next(const Params& p, RowWalk& w, int& phys, int k0, int row) {
        const bool cheap = row_walk_cheap(w, k0);
        row_walk_step(w, phys);
        if (__builtin_expect(!cheap, 0)) row_set(phys, row_exact(p, w.vlen, k0 + row));
    }
    // row_walk_next in its two halves, for a caller that knows of some tiles that they take the cheap step (tile_run below): the per-lane
    // step, which every tile takes, then row_walk_cheap and, where it says no, row_walk_exact; inside a run row_walk_in_run stands for those two.
    static __host__ __device__ __forceinline__ void row_walk_step(const RowWalk& w, int& phys) {
        row_add(phys, w.step);
        if (w.perm) row_add(phys, phys >= w.end ? w.unwrap : 0);
    }
    static __host__ __device__ __forceinline__ void row_walk_exact(const Params& p, const RowWalk& w, int& phys, int k0, int row) {
        row_set(phys, row_exact(p, w.vlen, k0 + row));
    }
    static __host__ __device__ __forceinline__ void row_walk_in_run(RowWalk& w) { w.prev_k0 += kBN; }

    // Tile run of the 16x16x32 body (attn_m16.h picks it by HasTileRun; a policy that overrides classify or row_walk_next sets kTileRun =
    // false).  For one wave of a q-tile the tiles t for which the vector phase N(t) has nothing to decide form one interval
    // [run_lo, run_lo + run_n):
    //   (a) tile t is FULL by the fast-path interval, fk_lo <= tile_key0(t) <= fk_hi;
    //   (b) tile t follows tile t - 1 in its segment, tile_key0(t) == tile_key0(t - 1) + kBN;
    //   (c) the tile N(t) resolves, t + dist + 1, lies in the same segment (so it exists and follows t + dist, the latest resolved one)
    //       and takes the cheap step: its first key lies in [w.lo, w.hi].
    // All three are intervals of the tile's index inside a segment.  The fast-path interval lies inside ONE segment of a band q-tile (the
    // band's, with which a neighbouring column range has been merged; text rows have one segment), so there is one run; written per segment,
    // the longest wins.  A tile of a run has t + dist + 1 < nT: runs lie inside the unguarded steady-state loop.
    static constexpr bool kTileRun = true;
    static __host__ __device__ __forceinline__ void tile_run(const Ctx& c, const RowWalk& w, int dist, int& run_lo, int& run_n) {
        using std::max;
        using std::min;
        static_assert(kBN == 64, "tile_run divides by the tile size with a shift");
        run_lo = 0, run_n = 0;
        const int ahead = (dist + 1) * kBN;
        const int k_lo = max(c.fk_lo, w.lo - ahead), k_hi = min(c.fk_hi, w.hi - ahead);   // first keys that satisfy (a) and the range of (c)
        int t0 = 0;
        // (written out per segment: a loop index into the arrays of Ctx could send them through scratch.  x >> 6: the floor for a negative x)
#define SVG_RUN_SEG(i)                                                                         \
    {                                                                                          \
        const int n = c.seg_n[i];                                                              \
        if (n > dist + 2) {                                                                    \
            const int kf = c.seg_lo[i] * kBN;                                                  \
            const int j_lo = max(1, (k_lo - kf + kBN - 1) >> 6);                               \
            const int j_hi = min(n - dist - 2, (k_hi - kf) >> 6);                              \
            if (j_hi - j_lo + 1 > run_n) run_lo = t0 + j_lo, run_n = j_hi - j_lo + 1;          \
        }                                                                                      \
        t0 += n;                                                                               \
    }
        SVG_RUN_SEG(0) SVG_RUN_SEG(1) SVG_RUN_SEG(2)
#undef SVG_RUN_SEG
    }

    template <typename C>
    static __device__ __forceinline__ int classify(const Params& p, const C& c, int k0, int wrow0) {
        if (k0 >= c.fk_lo && k0 <= c.fk_hi) return TILE_FULL;
        const int w0 = c.q0 + wrow0;
        if (w0 >= c.q_end) return TILE_SKIP;
        const int w1 = min(w0 + kWR, c.q_end);      // rows [w0, w1)
        const int k1 = min(k0 + kBN, p.S);          // keys [k0, k1)
        const int real = p.real_len;
        // ---- every pair allowed? ----
        bool all = false;
        if (k0 + kBN <= p.S) {
            if (w1 <= real && k1 <= real) {
                const bool band_all = (k1 - 1 - w0 < band_of(p, c)) && (w1 - 1 - k0 < band_of(p, c));
                const bool col_all = (k0 >= p.cf_lo && k1 <= p.cf_hi);
                const bool row_all = (w0 >= p.rf_lo && w1 <= p.rf_hi);
                all = band_all || col_all || row_all;
            } else if (w0 >= real && k0 >= real) {
                all = true;
            }
        }
        if (all) return TILE_FULL;
        // ---- any pair allowed? ----
        bool any = false;
        if (w0 < real && k0 < real) {
            const int w1r = min(w1, real), k1r = min(k1, real);
            const bool band_any = (k0 - (w1r - 1) < band_of(p, c)) && (w0 - (k1r - 1) < band_of(p, c));
            const bool col_any = (k0 < p.cf_hi && k1r > p.cf_lo);
            const bool row_any = (w0 < p.rf_hi && w1r > p.rf_lo);
            any = band_any || col_any || row_any;
        }
        if (w1 > real && k1 > real) any = true;
        return any ? TILE_PARTIAL : TILE_SKIP;
    }
    template <typename C>
    static __device__ __forceinline__ bool allowed(const Params& p, const C& c, int q, int k) {
        const bool rq = q < p.real_len, rk = k < p.real_len;
        const bool in_band = (band_of(p, c) > 0) & ((unsigned)(q - k + band_of(p, c) - 1) < (unsigned)(2 * band_of(p, c) - 1));   // band 0: |q - k| < 0 admits nothing
        const bool colf = (unsigned)(k - p.cf_lo) < (unsigned)(p.cf_hi - p.cf_lo);
        const bool rowf = (unsigned)(q - p.rf_lo) < (unsigned)(p.rf_hi - p.rf_lo);
        // bitwise on purpose: branch-free, one v_cndmask per element in the caller
        return ((rq & rk) & (in_band | colf | rowf)) | ((!rq & !rk) & (k < p.S));
    }
    // The same predicate as two key intervals of one query row, [a0, a0 + alen) u [b0, b0 + blen) (unsigned lengths, 0 = empty):
    // the two-phase body keeps them per lane across the tile loop, so a masked element costs 2 x (add, compare) + or + select.
    //   real row, not a full row:  band n [0, real)  u  full columns n [0, real)
    //   full row (text):           [0, real)
    //   row behind real_len:       [real_len, S)
    template <typename C>
    static __device__ __forceinline__ void row_intervals(const Params& p, const C& c, int q, int& a0, unsigned& alen, int& b0,
                                                         unsigned& blen) {
        const int real = p.real_len;
        const bool rq = q < real;
        const bool rowf = (unsigned)(q - p.rf_lo) < (unsigned)(p.rf_hi - p.rf_lo);
        const int band_lo = max(q - band_of(p, c) + 1, 0), band_hi = min(q + band_of(p, c), real);
        const int lo = rq ? (rowf ? 0 : band_lo) : real;
        const int hi = rq ? (rowf ? real : band_hi) : p.S;
        a0 = lo, alen = (unsigned)max(hi - lo, 0);
        const int ch = min(p.cf_hi, real);
        b0 = p.cf_lo, blen = (rq && !rowf) ? (unsigned)max(ch - p.cf_lo, 0) : 0u;
    }
    static __device__ __forceinline__ float score_fixup(const Params&, float s) { return s; }
    // Completion counters (svg_band_attention_notify*).  Contract: counter (head, s) reaching its target means the PHYSICAL rows
    // [row_bounds[s], row_bounds[s + 1]) of the head are complete and visible.  Segments are cut in logical (q-tile) order; a head
    // run with the fused layout permutation scatters the rows of a logical segment over every frame, so such a head is released
    // at head granularity: its waves count in a hidden per-head counter (done[BH * nseg + head]) and the last arriver raises
    // all segment counters of the head to their targets at once.
    static __device__ __forceinline__ void notify(const Params& p, const Ctx& c) {
        if (p.done) {
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            __threadfence();
            if ((threadIdx.x & 63) == 0) {
                int32_t* cnt = p.done + c.head * p.done_nseg;
                if (!c.perm) {
                    atomicAdd(cnt + min(c.qt / p.done_tps, p.done_nseg - 1), 1);
                } else if (atomicAdd(p.done + p.BH * p.done_nseg + c.head, 1) == p.nqt * NW - 1) {
                    __threadfence();
                    for (int sgm = 0; sgm < p.done_nseg; ++sgm) {
                        const int t_lo = sgm * p.done_tps;
                        const int t_hi = (sgm == p.done_nseg - 1) ? p.nqt : min(p.nqt, (sgm + 1) * p.done_tps);
                        atomicAdd(cnt + sgm, (t_hi - t_lo) * NW);
                    }
                }
            }
        }
    }
};

// LSE form (svg_band_attention_lse): the head_dim-128 band policy of the 16x16x32 body plus the row log-sum-exp (attn_m16.h: HasRowLse,
// switched on by lse_base below), as CrossLsePolicy adds it to the cross policy.  lse is a contiguous fp32 [BH, S] whatever the layout of
// q / o; the index inside a head is the physical q row q_phys returns — the row o is written to, also on a token-major head.
template <typename T>
struct BandLsePolicy : BandPolicy<T, 128, 8> {
    using Base = BandPolicy<T, 128, 8>;
    struct Params : Base::Params {
        float* lse;   // [BH, S]
    };
    static __device__ __forceinline__ float* lse_base(const Params& p, const typename Base::Ctx& c) { return p.lse + (size_t)c.head * (size_t)p.S; }
};

// Per-head form (svg_band_attention_per_head_lse, include/svg_attn_adaptive_band.h): the LSE policy with ONE BAND PER HEAD, read from a
// device vector.  The band travels in the Ctx (band_of above picks it up in kv_schedule, wave_fast_interval, classify and row_intervals; the
// tile runs and the row cursor follow from those), clamped to [1, S + 1] here: a device value cannot be validated on the host.  The launch is
// the static mapping of BandPolicy::init over (head, q-tile), the heavy q-tiles of every head first and the rest in windows of 32 per XCD.
// Nothing else differs, so head h keeps the bits of svg_band_attention_lse with mask->band = band[h].  band_vec == nullptr (the alternate
// block of the device switch): p.band for every head.
// The row regions are the one thing the host derives from the band — a band above S does not cut the full rows out (band_row_regions) — so
// the kernels get a parameter block for either case and pick per head (map_block, per_head_band_of, before the body).  Both blocks map
// dispatch ids through the SAME numbers (map_*: those of the block that cuts the full rows out, which has no fewer q-tiles), so every
// (head, index) pair is visited once whichever block a head runs; a head on the other block takes the index as its q-tile and leaves
// what lies behind its last one.  (A grid row per head with a mapping per head: 33.196 against 31.587 ms for the device switch at
// HunyuanVideo 720p, profiles/adaptive_band_ab_grid_row_per_head.jsonl — only the first 256 of a head's 466 q-tiles got their XCD windows.)
template <typename T>
struct BandPerHeadLsePolicy : BandLsePolicy<T> {
    using Base = BandLsePolicy<T>;
    using Band = BandPolicy<T, 128, 8>;
    struct Params : Base::Params {
        const int32_t* band_vec;   // device int32 [BH], or nullptr
        int map_nqt, map_n_heavy, map_heavy_lo;   // the mapping's nqt, n_heavy, heavy_lo (this block's own, or its sibling's)
    };
    struct Ctx : Band::Ctx {
        int band;
    };
    static __device__ __forceinline__ int per_head_band_of(const Params& p, int head) {
        if (!p.band_vec) return p.band;
        return min(max(__builtin_amdgcn_readfirstlane(p.band_vec[head]), 1), p.S + 1);   // (a uniform load: the band stays on the scalar unit)
    }
    static __device__ __forceinline__ void init_tile(const Params& p, Ctx& c, int head, int qt) {
        c.head = head;
        c.perm = (p.head_flag != nullptr) && (p.head_flag[c.head] != 0);
        c.band = per_head_band_of(p, head);
        Band::kv_schedule(p, c, qt);
        Band::wave_fast_interval(p, c, wave_id(), c.fk_lo, c.fk_hi);
    }
    // dispatch id -> (head, index of a q-tile): BandPolicy::init's mapping on map_*
    static __device__ __forceinline__ bool map_block(const Params& p, int& head, int& qt) {
        const int nh = p.BH * p.map_n_heavy;
        const int b = blockIdx.x;
        if (b >= p.map_nqt * p.BH) return false;   // (the device-switched launch is sized for the larger of its masks)
        if (b < nh) {
            head = b / p.map_n_heavy;
            qt = p.map_heavy_lo + (b - head * p.map_n_heavy);
        } else {
            const int b2 = b - nh;
            const int full = ((p.map_nqt * p.BH - nh) / (kNumXCD * 32)) * (kNumXCD * 32);
            int w2 = b2;
            if (b2 < full) {
                const int xcd = b2 % kNumXCD, s = b2 / kNumXCD;
                w2 = (s / 32) * (kNumXCD * 32) + xcd * 32 + (s % 32);
            }
            const int nl = p.map_nqt - p.map_n_heavy;
            head = w2 / nl;
            const int r = w2 - head * nl;
            qt = r < p.map_heavy_lo ? r : r + p.map_n_heavy;
        }
        return true;
    }
    static __device__ __forceinline__ bool init(const Params& p, Ctx& c, char*) {
        int head, qt;
        if (!map_block(p, head, qt) || qt >= p.nqt) return false;
        init_tile(p, c, head, qt);
        return true;
    }
};

// fp32 form (svg_band_attention_lse_f32): the LSE policy plus the rows before their rounding (attn_m16.h: HasRowO32, switched on by
// o32_base below), as CrossF32Policy adds them to the cross policy.  o32 is a contiguous fp32 [BH, S, 128] whatever the layout of q, the
// row inside a head the one lse uses; Params::o is not used.
template <typename T>
struct BandF32Policy : BandLsePolicy<T> {
    using Base = BandLsePolicy<T>;
    struct Params : Base::Params {
        float* o32;   // [BH, S, 128]
    };
    static __device__ __forceinline__ float* o32_base(const Params& p, const typename Base::Ctx& c) {
        return p.o32 + (size_t)c.head * (size_t)p.S * 128;
    }
};

// Window forms (svg_band_window_attention_lse[_f32], include/svg_attn_band_window.h): the LSE / fp32 policy over a ROW window and a KEY
// window of the mask — q / o / lse / o32 hold the rows [q_begin, q_begin + Sq), k / v the keys [k_begin, k_end) of a sequence of S rows, and
// the mask is evaluated at the global coordinates.  A window is a clip, not a new mask:
//   rows     the host intersects the row regions with the row window (make_band_window_params), so q0 / q_end, the mask intervals and the
//            per-wave fast-path interval stay global; q_phys — the row q is read from and o / lse / o32 are written to — subtracts q_begin.
//   keys     the key-tile segments of kv_schedule are clipped to the tiles of the key window (k_begin is a multiple of kBN: tiles stay
//            aligned to the mask's coordinates, so no tile starts in front of the window); wherever S bounds the keys — the partial last
//            tile (classify, row_intervals), the redirect of rows behind the sequence (row_exact), the cheap step of the row cursor and
//            fk_hi — k_end does.  A key behind the window is masked, and its row is never read: the redirect goes to the window's first row.
//            The row the cursor holds is relative to k_begin.
// The element predicate allowed() is NOT clipped: the 16x16x32 body, the only one these policies are built for, masks through
// row_intervals (kIntervalMask).
// No head permutation (the kernels are launched without one).  With the whole sequence as both windows every value above is the one the
// base policy computes, so the kernels keep the bits of their siblings.
template <typename BasePol>
struct BandWindowOf : BasePol {
    using Ctx = typename BasePol::Ctx;
    using RowWalk = typename BasePol::RowWalk;
    static constexpr bool kTileRun = false;   // classify and row_walk_next are this policy's own: the per-tile decisions stay
    struct Params : BasePol::Params {
        int q_begin, Sq;       // row window [q_begin, q_begin + Sq): what q / o / lse / o32 hold
        int k_begin, k_end;    // key window [k_begin, k_end): what k / v hold; k_begin % kBN == 0
    };
    static __host__ __device__ __forceinline__ void clip_keys(const Params& p, Ctx& c) {
        using std::max;
        using std::min;
        const int t_lo = p.k_begin / kBN, t_hi = (p.k_end + kBN - 1) / kBN;
        // (written out per segment: a loop index into the arrays of Ctx could send them through scratch)
#define SVG_CLIP_SEG(i)                                                                  \
    {                                                                                    \
        const int lo = max(c.seg_lo[i], t_lo), hi = min(c.seg_lo[i] + c.seg_n[i], t_hi); \
        c.seg_lo[i] = lo, c.seg_n[i] = max(hi - lo, 0);                                  \
    }
        SVG_CLIP_SEG(0) SVG_CLIP_SEG(1) SVG_CLIP_SEG(2)
#undef SVG_CLIP_SEG
        c.nT = c.seg_n[0] + c.seg_n[1] + c.seg_n[2];
    }
    static __host__ __device__ __forceinline__ void kv_schedule(const Params& p, Ctx& c, int qt) {
        BasePol::kv_schedule(p, c, qt);
        clip_keys(p, c);
    }
    static __device__ __forceinline__ void init_tile(const Params& p, Ctx& c, int head, int qt) {
        BasePol::init_tile(p, c, head, qt);
        clip_keys(p, c);
        c.fk_hi = min(c.fk_hi, p.k_end - kBN);
    }
    static __device__ __forceinline__ bool init(const Params& p, Ctx& c, char* lds) {
        if (!BasePol::init(p, c, lds)) return false;
        clip_keys(p, c);
        c.fk_hi = min(c.fk_hi, p.k_end - kBN);
        return true;
    }
    static __device__ __forceinline__ int q_phys(const Params& p, const Ctx& c, int row) {
        const int l = c.q0 + row;
        return l < c.q_end ? l - p.q_begin : -1;
    }
    static __host__ __device__ __forceinline__ void row_walk_init(const Params& p, const Ctx& c, RowWalk& w) {
        BasePol::row_walk_init(p, c, w);
        w.hi = p.k_end - kBN;
    }
    static __host__ __device__ __forceinline__ int row_exact(const Params& p, int l) { return l < p.k_end ? l - p.k_begin : 0; }
    static __host__ __device__ __forceinline__ void row_walk_next(const Params& p, RowWalk& w, int& phys, int k0, int row) {
        const bool cheap = BasePol::row_walk_cheap(w, k0);
        BasePol::row_add(phys, w.step);
        if (__builtin_expect(!cheap, 0)) BasePol::row_set(phys, row_exact(p, k0 + row));
    }
    static __device__ __forceinline__ int classify(const Params& p, const Ctx& c, int k0, int wrow0) {
        const int cls = BasePol::classify(p, c, k0, wrow0);
        return (cls == TILE_FULL && k0 + kBN > p.k_end) ? TILE_PARTIAL : cls;   // (never through the fast-path interval: fk_hi is clipped)
    }
    static __device__ __forceinline__ void row_intervals(const Params& p, const Ctx& c, int q, int& a0, unsigned& alen, int& b0,
                                                         unsigned& blen) {
        BasePol::row_intervals(p, c, q, a0, alen, b0, blen);
        alen = (unsigned)max(min(a0 + (int)alen, p.k_end) - a0, 0);
        blen = (unsigned)max(min(b0 + (int)blen, p.k_end) - b0, 0);
    }
    static __device__ __forceinline__ float* lse_base(const Params& p, const Ctx& c) { return p.lse + (size_t)c.head * (size_t)p.Sq; }
};
template <typename T>
using BandWindowLsePolicy = BandWindowOf<BandLsePolicy<T>>;
template <typename T>
struct BandWindowF32Policy : BandWindowOf<BandF32Policy<T>> {
    using Base = BandWindowOf<BandF32Policy<T>>;
    static __device__ __forceinline__ float* o32_base(const typename Base::Params& p, const typename Base::Ctx& c) {
        return p.o32 + (size_t)c.head * (size_t)p.Sq * 128;
    }
};

// Shard forms (svg_band_shard_attention_lse[_f32], include/svg_attn_band_shard.h): the LSE / fp32 policy over a q SHARD and a k SHARD of the
// sequence.  A shard is the physical rows of the whole frames [f0, f0 + Fl) of the video, stored as row fl * P + p, and behind them a tail:
// the global rows [tail_begin, tail_begin + n_tail) behind the video (text, padding).  Every index the body sees is LOCAL to a shard — q0 /
// q_end, the key tiles, the mask intervals, the fast-path interval, the row cursor — and one map per shard and head kind ties a local
// index l to the coordinate of the mask:
//   head in logical order    g(l) = vid0 + f0 * P + l                       read from local row l
//   token-major head         g(l) = vid0 + (l / Fl) * F + f0 + l % Fl       read from local row (l % Fl) * P + l / Fl: the fused placement
//   tail (l >= P * Fl)       g(l) = tail_begin + (l - P * Fl)               read from local row l                      of a video of Fl frames
// g is strictly increasing, so an interval [a, b) of global keys is the interval [ginv(a), ginv(b)) of local keys (ginv(x): the smallest l
// with g(l) >= x — one division by F), and row lq sees key lk exactly where the mask allows (g_q(lq), g_k(lk)):
//   rows       the host cuts the row regions at ginv_q of rowfull_lo / rowfull_hi / real_len, once per head kind (shard_regions);
//   schedule   the base's key intervals for the hull [g_q(q0), g_q(q_end - 1)] of the q-tile, their ends through ginv_k onto the local
//              tile grid (more than the rows need where the hull holds rows of other shards: those tiles are masked);
//   mask       the base's row intervals at g_q(row), their ends through ginv_k;
//   fast path  a tile is FULL for a wave where the band holds for the hulls of the wave's rows and of the tile's keys: an interval of
//              local first keys again; classify proves FULL on the hulls or answers TILE_PARTIAL.
// Tiles lie on the local grids, so no begin needs an alignment.  With vid0 = 0, f0 = 0, Fl = F and the tail [F * P, S) on both sides g is the
// identity and every value above is the one the base policy computes with the head permutation: the kernels keep the bits of their siblings.
// Divisions: by Fl per row (q, once per q-tile) and per key row on the exact path of the row cursor, by F per interval end.
struct BandShardMap {
    int f0, Fl, nv, n, tail_begin;   // frames [f0, f0 + Fl): nv = P * Fl video rows; n rows in all, the tail = global rows [tail_begin, ..)
    int fdiv;                        // max(Fl, 1): the divisor (a shard may be a tail alone)
    int sp64;                        // token-major head: physical-row step of a 64-row tile, 64 / Fl + (64 % Fl) * P
    // local index -> coordinate of the mask (kind != 0: token-major head)
    __host__ __device__ __forceinline__ int g(int vid0, int F, int P, int kind, int l) const {
        const int pp = (int)((unsigned)l / (unsigned)fdiv), fl = l - pp * fdiv;
        const int gv = kind ? vid0 + pp * F + f0 + fl : vid0 + f0 * P + l;
        return l < nv ? gv : tail_begin + (l - nv);
    }
    // the smallest local index whose coordinate is >= x (n: none)
    __host__ __device__ __forceinline__ int ginv(int vid0, int F, int P, int kind, int x) const {
        using std::max;
        using std::min;
        const int y = x - vid0, yc = max(y, 0);
        const int pp = (int)((unsigned)yc / (unsigned)F), r = yc - pp * F;
        const int l1 = pp * Fl + min(max(r - f0, 0), Fl);
        const int lv = min(kind ? l1 : max(y - f0 * P, 0), nv);
        const int lt = nv + min(max(x - tail_begin, 0), n - nv);
        return lv < nv ? lv : lt;
    }
    // local index -> local physical row
    __host__ __device__ __forceinline__ int phys(int P, int kind, int l) const {
        const int pp = (int)((unsigned)l / (unsigned)fdiv), fl = l - pp * fdiv;
        return (kind && l < nv) ? fl * P + pp : l;
    }
};

template <typename BasePol>
struct BandShardOf : BasePol {
    using RowWalk = typename BasePol::RowWalk;
    static constexpr bool kTileRun = false;   // classify and row_walk_next are this policy's own: the per-tile decisions stay
    struct Ctx : BasePol::Ctx {
        int gw0, gw1;   // per WAVE: the coordinates of its rows lie in [gw0, gw1) (gw0 >= gw1: an idle wave)
    };
    struct Params : BasePol::Params {
        BandShardMap qs, ks;                       // what q / o / lse / o32 hold, what k / v hold
        int reg1_lo[4], reg1_hi[4], reg1_t0[4];    // row regions of the token-major heads (reg_* of the base: heads in logical order)
    };
    static __device__ __forceinline__ int gq(const Params& p, const Ctx& c, int l) { return p.qs.g(p.vid0, p.F, p.P, c.perm, l); }
    static __device__ __forceinline__ int gk(const Params& p, const Ctx& c, int l) { return p.ks.g(p.vid0, p.F, p.P, c.perm, l); }
    static __device__ __forceinline__ int ginv_k(const Params& p, const Ctx& c, int x) { return p.ks.ginv(p.vid0, p.F, p.P, c.perm, x); }

    // local rows [q0, q_end) of q-tile `qt` of a head of c.perm's kind and its key-tile segments on the k shard's grid
    static __device__ __forceinline__ void kv_schedule(const Params& p, Ctx& c, int qt) {
        // (explicit selects: a run-time index into the kernel-argument arrays would go through scratch)
        const bool k1 = c.perm != 0;
#define SVG_REG(a, i) (k1 ? p.reg1_##a[i] : p.reg_##a[i])
        const bool r1 = qt >= SVG_REG(t0, 1), r2 = qt >= SVG_REG(t0, 2), r3 = qt >= SVG_REG(t0, 3);
        const int rlo = r3 ? SVG_REG(lo, 3) : r2 ? SVG_REG(lo, 2) : r1 ? SVG_REG(lo, 1) : SVG_REG(lo, 0);
        const int rhi = r3 ? SVG_REG(hi, 3) : r2 ? SVG_REG(hi, 2) : r1 ? SVG_REG(hi, 1) : SVG_REG(hi, 0);
        const int rt0 = r3 ? SVG_REG(t0, 3) : r2 ? SVG_REG(t0, 2) : r1 ? SVG_REG(t0, 1) : 0;
#undef SVG_REG
        c.qt = qt;
        c.q0 = rlo + (qt - rt0) * BasePol::BM;
        c.q_end = min(rhi, c.q0 + BasePol::BM);
        constexpr int BIG = 1 << 28;
        int alo = BIG, ahi = BIG, blo = BIG, bhi = BIG, clo = BIG, chi = BIG;
        if (c.q0 < c.q_end) {
            // the base's key intervals for the rows [g0, g1) of the mask, as local keys [x, y): an interval without a key of this shard
            // is dropped (one that is empty in the mask's own coordinates — band 0 — keeps the tiles the base gives it)
            const int g0 = gq(p, c, c.q0), g1 = gq(p, c, c.q_end - 1) + 1;
            const int real = p.real_len;
            auto tiles = [&](int a, int b, int& lo, int& hi) {
                const int x = ginv_k(p, c, a), y = ginv_k(p, c, b);
                if (b > a && y <= x) return;
                lo = x / kBN, hi = max((y + kBN - 1) / kBN, lo);
            };
            if (g0 < real) {
                const int qr1 = min(g1, real);
                if (g0 < p.rf_hi && qr1 > p.rf_lo) {
                    tiles(0, real, alo, ahi);
                } else {
                    tiles(max(0, g0 - p.band + 1), min(real, qr1 - 1 + p.band), alo, ahi);
                    const int ch = min(p.cf_hi, real);
                    if (ch > p.cf_lo) tiles(p.cf_lo, ch, blo, bhi);
                }
            }
            if (g1 > real) tiles(real, p.S, clo, chi);
        }
#define SVG_CSWAP(x, xh, y, yh) if (y < x) { int t_ = x; x = y; y = t_; t_ = xh; xh = yh; yh = t_; }
        SVG_CSWAP(alo, ahi, blo, bhi)
        SVG_CSWAP(blo, bhi, clo, chi)
        SVG_CSWAP(alo, ahi, blo, bhi)
#undef SVG_CSWAP
        if (blo < BIG && blo <= ahi) {
            ahi = max(ahi, bhi);
            blo = clo, bhi = chi, clo = BIG, chi = BIG;
            if (blo < BIG && blo <= ahi) ahi = max(ahi, bhi), blo = BIG, bhi = BIG;
        } else if (clo < BIG && clo <= bhi) {
            bhi = max(bhi, chi), clo = BIG, chi = BIG;
        }
        c.seg_lo[0] = alo, c.seg_n[0] = ahi - alo;
        c.seg_lo[1] = blo, c.seg_n[1] = bhi - blo;
        c.seg_lo[2] = clo, c.seg_n[2] = chi - clo;
        c.nT = c.seg_n[0] + c.seg_n[1] + c.seg_n[2];
    }
    // everything of Ctx for q-tile `qt` of head `head`; false: the head's kind has no such q-tile (the launch is sized for the kind with more)
    static __device__ __forceinline__ bool init_tile(const Params& p, Ctx& c, int head, int qt) {
        c.head = head;
        c.perm = (p.head_flag != nullptr) && (p.head_flag[c.head] != 0);
        kv_schedule(p, c, qt);
        if (c.q0 >= c.q_end) return false;
        // the wave's rows and its fast-path interval: first keys k0 of the local grid with every (row, key) pair of the hulls allowed —
        // g_k(k0) >= gw1 - band and g_k(k0 + 63) <= gw0 + band - 1, below real_len; g_k increases, so both bounds are ginv_k of one number
        const int w0 = c.q0 + wave_id() * BasePol::kWR, w1 = min(w0 + BasePol::kWR, c.q_end);
        c.gw0 = 0, c.gw1 = 0;
        c.fk_lo = 1, c.fk_hi = 0;
        if (w0 < c.q_end) {
            c.gw0 = gq(p, c, w0), c.gw1 = gq(p, c, w1 - 1) + 1;
            const int real = p.real_len;
            if (c.gw1 <= real) {
                const bool full_rows = c.gw0 >= p.rf_lo && c.gw1 <= p.rf_hi;
                c.fk_lo = full_rows ? 0 : ginv_k(p, c, max(c.gw1 - p.band, 0));
                c.fk_hi = ginv_k(p, c, full_rows ? real : min(c.gw0 + p.band, real)) - kBN;
            }
        }
        return true;
    }
    // static mapping: head-major, the q-tiles of a head from the last one down (the tail's rows — text: every key — first)
    static __device__ __forceinline__ bool init(const Params& p, Ctx& c, char*) {
        const int b = blockIdx.x;
        if (b >= p.nqt * p.BH) return false;
        const int head = b / p.nqt;
        return init_tile(p, c, head, p.nqt - 1 - (b - head * p.nqt));
    }
    static __device__ __forceinline__ int q_phys(const Params& p, const Ctx& c, int row) {
        const int l = c.q0 + row;
        return l < c.q_end ? p.qs.phys(p.P, c.perm, l) : -1;
    }
    // the row cursor over the k shard: the base's walk on a video of Fl frames at local row 0 (cheap step of a token-major head: the tile and
    // the one before it inside the shard's video rows; of a head in logical order: inside the shard)
    static __device__ __forceinline__ void row_walk_init(const Params& p, const Ctx& c, RowWalk& w) {
        const bool perm = c.perm != 0;
        w.perm = perm;
        w.lo = perm ? kBN : -(1 << 30);
        w.hi = (perm ? p.ks.nv : p.ks.n) - kBN;
        w.step = perm ? p.ks.sp64 : kBN, w.end = p.ks.nv, w.unwrap = 1 - p.ks.nv;
        w.vlen = perm ? p.ks.nv : 0;
        w.prev_k0 = -(1 << 30);
        asm volatile("" : "+v"(w.step), "+v"(w.unwrap));   // (as the base keeps them: see BandPolicy::row_walk_init)
        w.perm = __builtin_amdgcn_readfirstlane(w.perm);
        asm volatile("" : "+s"(w.perm));
    }
    // local key index -> local physical row (`vlen`: the shard's video rows on a token-major head, 0 otherwise); a key behind the shard is
    // masked and never read: the redirect goes to the shard's first row
    static __device__ __forceinline__ int row_exact(const Params& p, int vlen, int l) {
        const int pp = (int)((unsigned)l / (unsigned)p.ks.fdiv), fl = l - pp * p.ks.fdiv;
        const int phys = (unsigned)l < (unsigned)vlen ? fl * p.P + pp : l;
        return l < p.ks.n ? phys : 0;
    }
    static __device__ __forceinline__ void row_walk_next(const Params& p, RowWalk& w, int& phys, int k0, int row) {
        const bool cheap = BasePol::row_walk_cheap(w, k0);
        BasePol::row_add(phys, w.step);
        if (w.perm) BasePol::row_add(phys, phys >= w.end ? w.unwrap : 0);
        if (__builtin_expect(!cheap, 0)) BasePol::row_set(phys, row_exact(p, w.vlen, k0 + row));
    }
    // FULL only where it is proven for the hulls of the wave's rows and of the tile's keys; everything else is masked element by element
    static __device__ __forceinline__ int classify(const Params& p, const Ctx& c, int k0, int) {
        if (k0 >= c.fk_lo && k0 <= c.fk_hi) return TILE_FULL;
        if (c.gw0 >= c.gw1) return TILE_SKIP;
        if (k0 + kBN > p.ks.n) return TILE_PARTIAL;
        const int k_lo = gk(p, c, k0), k_hi = gk(p, c, k0 + kBN - 1) + 1;   // the tile's keys lie in [k_lo, k_hi)
        const int real = p.real_len;
        bool all = false;
        if (c.gw1 <= real && k_hi <= real) {
            const bool band_all = (k_hi - 1 - c.gw0 < p.band) && (c.gw1 - 1 - k_lo < p.band);
            const bool col_all = (k_lo >= p.cf_lo && k_hi <= p.cf_hi);
            const bool row_all = (c.gw0 >= p.rf_lo && c.gw1 <= p.rf_hi);
            all = band_all || col_all || row_all;
        } else if (c.gw0 >= real && k_lo >= real) {
            all = true;
        }
        return all ? TILE_FULL : TILE_PARTIAL;
    }
    static __device__ __forceinline__ void row_intervals(const Params& p, const Ctx& c, int q, int& a0, unsigned& alen, int& b0,
                                                         unsigned& blen) {
        BasePol::row_intervals(p, c, gq(p, c, q), a0, alen, b0, blen);
        const int a1 = ginv_k(p, c, a0 + (int)alen), b1 = ginv_k(p, c, b0 + (int)blen);
        a0 = ginv_k(p, c, a0), b0 = ginv_k(p, c, b0);
        alen = (unsigned)max(a1 - a0, 0), blen = (unsigned)max(b1 - b0, 0);
    }
    static __device__ __forceinline__ float* lse_base(const Params& p, const Ctx& c) { return p.lse + (size_t)c.head * (size_t)p.qs.n; }
};
template <typename T>
using BandShardLsePolicy = BandShardOf<BandLsePolicy<T>>;
template <typename T>
struct BandShardF32Policy : BandShardOf<BandF32Policy<T>> {
    using Base = BandShardOf<BandF32Policy<T>>;
    static __device__ __forceinline__ float* o32_base(const typename Base::Params& p, const typename Base::Ctx& c) {
        return p.o32 + (size_t)c.head * (size_t)p.qs.n * 128;
    }
};

// =====================================================================================================
// Work queue of the resident band kernels (band_attn_m16_queue_kernel in attention.hip): min(work items, CUs) workgroups, each
// taking (head, q-tile) pairs until the queue is dry, instead of one workgroup per pair bound to an XCD by its dispatch id.
//
// Order of the work items (index w):
//   [0, nh)   the q-tiles of text rows, head-major (they visit every key tile: first, as in BandPolicy::init);
//   bulk      the full-length band q-tiles, head-major in row order; then the shortened q-tiles — the band-edge tiles at both ends of
//             a head and the rows behind real_len — by their RANK (0 = next to the full-length ones, growing towards the first / the
//             last row of the head: the higher the rank, the fewer key tiles) in tiers of 32 ranks: tier t holds, head by head, ranks
//             32 t .. 32 t + 31 at the front of the head and then the same ranks at its back;
//   tail      the highest ranks of all heads, about kQueueTail work items (one per CU), strictly rank-major: rank by rank, head by
//             head, front then back — the shortest q-tiles of the launch, longest first.
// Who takes what: the bulk is cut into chunks of 32 neighbours; chunk j belongs to the list of XCD j % 8 and text-row item w to list
// w % 8.  A workgroup reads its XCD from the hardware and takes from that XCD's list (one atomicAdd), so the 32 CUs of an XCD work on
// neighbouring q-tiles of one head as they did under the static mapping (their KV windows overlap in the XCD's L2).  A workgroup
// that finds its list dry takes from the next XCD's list, and so on round the chip; when all eight are dry, from the tail, which has
// one chip-wide counter: the last round of a launch is handed out one q-tile at a time in descending length to whichever CU is
// free (tools/band_queue_sim.py: makespan over ideal 1.005 / 1.015 / 1.044 for HunyuanVideo 720p, 480p and a 3-head launch, against
// 1.012 / 1.052 / 1.173 of the static mapping; without the tail the chunk granularity leaves 1.009 / 1.030 / 1.083).  No workgroup
// ever waits for another one.  An index behind a list's end means dry whatever the counter held, so a counter block with arbitrary
// contents costs work items, never a hang.  The last workgroup to leave zeroes the block for the next launch.
// =====================================================================================================
constexpr int kQueueChunk = 32;
constexpr int kQueueTail = 256;                               // work items of the tail, rounded up to whole ranks
constexpr int kQueueStride = 16;                              // int32 words from one counter to the next: a 64-byte line each
constexpr int kQueueCounters = kNumXCD + 2;                   // the eight list counters, the tail counter, the workgroups that left
constexpr int kQueueWords = kQueueCounters * kQueueStride;    // a counter block

struct BandQueue {
    int32_t* ctr;             // device, kQueueWords zeroed words owned by this launch (band_queue_block)
    int n_items;              // BH * nqt
    int BH, nh, n_heavy, heavy_lo;
    int nl;                   // light q-tiles per head (all but the text-row tiles); light index r -> q-tile r (+ n_heavy behind heavy_lo)
    int e_lo, e_hi;           // shortened light tiles at the front / at the back of a head; [e_lo, nl - e_hi) are the full-length ones
    int r0;                   // ranks [0, r0) are bulk, ranks from r0 on tail
    int n_tail;               // work items of the tail: the last n_tail indices

    // light index of the tile of rank `rank` at the front (back = false) or at the back of a head
    __host__ __device__ int edge_tile(int rank, bool back) const { return back ? nl - e_hi + rank : e_lo - 1 - rank; }
    // work item w -> (head, q-tile in row order)
    __host__ __device__ void decode(int w, int& head, int& qt) const {
        if (w < nh) {
            head = w / n_heavy;
            qt = heavy_lo + (w - head * n_heavy);
            return;
        }
        int w2 = w - nh, r = 0;
        const int nf = nl - e_lo - e_hi;
        head = 0;
        if (w >= n_items - n_tail) {
            w2 = w - (n_items - n_tail);
            const int m = e_lo < e_hi ? e_lo : e_hi;          // ranks below m exist on both sides of a head
            const int both = m > r0 ? (m - r0) * 2 * BH : 0;
            if (w2 < both) {
                const int rank = r0 + w2 / (2 * BH), j = w2 % (2 * BH);
                head = j >> 1;
                r = edge_tile(rank, j & 1);
            } else {
                w2 -= both;
                head = w2 % BH;
                r = edge_tile((m > r0 ? m : r0) + w2 / BH, e_hi > e_lo);
            }
        } else if (w2 < BH * nf) {
            head = w2 / nf;
            r = e_lo + (w2 - head * nf);
        } else {
            w2 -= BH * nf;
            const int b_lo = e_lo < r0 ? e_lo : r0, b_hi = e_hi < r0 ? e_hi : r0;   // bulk ranks at the front / at the back
            for (int t0 = 0; t0 < r0; t0 += kQueueChunk) {   // tier of ranks [t0, t0 + 32)
                const int cl = b_lo - t0 < 0 ? 0 : (b_lo - t0 > kQueueChunk ? kQueueChunk : b_lo - t0);
                const int ct = b_hi - t0 < 0 ? 0 : (b_hi - t0 > kQueueChunk ? kQueueChunk : b_hi - t0);
                const int c = cl + ct;
                if (w2 < BH * c) {
                    head = w2 / c;
                    const int j = w2 - head * c;
                    r = j < cl ? edge_tile(t0 + j, false) : edge_tile(t0 + j - cl, true);
                    break;
                }
                w2 -= BH * c;
            }
        }
        qt = r < heavy_lo ? r : r + n_heavy;
    }
    // entry i of XCD xcd's list, or -1 behind its end
    __host__ __device__ int item(int xcd, unsigned i) const {
        if (i >= (unsigned)n_items) return -1;
        const int nhx = nh > xcd ? (nh - xcd + kNumXCD - 1) / kNumXCD : 0;
        if ((int)i < nhx) return xcd + kNumXCD * (int)i;
        const int i2 = (int)i - nhx;
        const int w = nh + ((i2 / kQueueChunk) * kNumXCD + xcd) * kQueueChunk + i2 % kQueueChunk;
        return w < n_items - n_tail ? w : -1;
    }
    // entry i of the tail, or -1 behind its end
    __host__ __device__ int tail_item(unsigned i) const { return i < (unsigned)n_tail ? n_items - n_tail + (int)i : -1; }
    // One lane of a workgroup: the next work item for a workgroup on XCD `xcd`, -1 when the queue is dry.  `k` (0 at entry of the
    // kernel) counts the lists this workgroup has found dry: a dry list stays dry.
    __device__ int take(int xcd, int& k) const {
        for (; k < kNumXCD; ++k) {
            const int x = (xcd + k) & (kNumXCD - 1);
            const int w = item(x, (unsigned)atomicAdd(ctr + x * kQueueStride, 1));
            if (w >= 0) return w;
        }
        if (k == kNumXCD) {
            const int w = tail_item((unsigned)atomicAdd(ctr + kNumXCD * kQueueStride, 1));
            if (w >= 0) return w;
            ++k;
        }
        return -1;
    }
    // One lane of a workgroup that takes no more work: the last of `n_wg` to leave hands the block back zeroed.
    __device__ void leave(int n_wg) const {
        __threadfence();
        if (atomicAdd(ctr + (kQueueCounters - 1) * kQueueStride, 1) == n_wg - 1) {
            for (int x = 0; x < kQueueCounters; ++x) atomicExch(ctr + x * kQueueStride, 0);
        }
    }
};

// the queue of a launch with parameters p (ctr is left null: band_queue_block)
template <typename Pol>
inline BandQueue make_band_queue(const typename Pol::Params& p) {
    BandQueue qd{};
    qd.n_items = p.BH * p.nqt, qd.BH = p.BH;
    qd.n_heavy = p.n_heavy, qd.heavy_lo = p.heavy_lo, qd.nh = p.BH * p.n_heavy, qd.nl = p.nqt - p.n_heavy;
    // the shortened tiles: what lies in front of the first / behind the last light tile with the largest number of key tiles
    int longest = -1, first = 0, last = -1;
    for (int r = 0; r < qd.nl; ++r) {
        typename Pol::Ctx c;
        Pol::kv_schedule(p, c, r < p.heavy_lo ? r : r + p.n_heavy);
        if (c.nT > longest) longest = c.nT, first = r;
        if (c.nT == longest) last = r;
    }
    qd.e_lo = first, qd.e_hi = qd.nl - 1 - last;
    if (qd.nl == 0) qd.e_lo = qd.e_hi = 0;
    const int ranks = std::max(qd.e_lo, qd.e_hi);
    qd.r0 = std::max(0, ranks - (kQueueTail + 2 * p.BH - 1) / (2 * p.BH));
    qd.n_tail = p.BH * (std::max(0, qd.e_lo - qd.r0) + std::max(0, qd.e_hi - qd.r0));
    return qd;
}

// A zeroed counter block for a queue launch on `st` of the current device, or nullptr (the caller then launches the statically
// mapped kernel).  The library owns one pool per device and gives every stream a block of its own: launches on one stream run one
// after the other and each leaves the block zeroed, launches on different streams never share one.  nullptr: the stream is being
// captured into a graph (a replay can run beside a launch on the same stream), the pool cannot be allocated, or more streams
// than the pool has blocks have launched band attention on this device.
int32_t* band_queue_block(hipStream_t st, int& n_cu);   // n_cu: compute units of the device
// diagnostics (svg_debug_band_queue_cap): at most this many resident workgroups per queue launch; 0 = as many as the device has CUs
int band_queue_cap();

// Row regions of a launch (see BandPolicy::Params): the rows [row_lo, row_hi) of a sequence of S rows — the whole sequence, or the row
// window of a window launch — cut at rowfull_lo, rowfull_hi (inside [0, real_len)) and real_len; unused slots are empty regions behind
// the last tile.  A q-tile of full rows visits every key tile on the unmasked fast path (with the text rows sharing a tile with band rows
// or rows behind real_len, all 1861 tiles of it took the per-element masked path: 9.5 ms instead of 3.2).  Also nqt, the heavy q-tiles
// and the segments of the completion counters.
template <typename Pol>
inline void band_row_regions(typename Pol::Params& p, int S, int row_lo, int row_hi, int done_nseg) {
    const int real = std::min(std::max(p.real_len, 0), S);
    const bool has_rf = p.rf_hi > p.rf_lo && p.rf_lo < real && p.band <= S;
    const int a = has_rf ? std::max(p.rf_lo, 0) : 0, b = has_rf ? std::min(p.rf_hi, real) : 0;
    auto clip = [&](int x) { return std::min(std::max(x, row_lo), row_hi); };
    const int cuts[5] = {clip(0), clip(a), clip(b), clip(real), clip(S)};
    int nreg = 0, t0 = 0, heavy_reg = -1;
    for (int i = 0; i < 4; ++i) {
        if (cuts[i + 1] <= cuts[i]) continue;
        p.reg_lo[nreg] = cuts[i], p.reg_hi[nreg] = cuts[i + 1], p.reg_t0[nreg] = t0;
        if (has_rf && i == 1) heavy_reg = nreg;
        t0 += (cuts[i + 1] - cuts[i] + Pol::BM - 1) / Pol::BM;
        ++nreg;
    }
    p.nqt = t0;
    p.done_nseg = std::max(1, std::min(done_nseg, t0));
    p.done_tps = (t0 + p.done_nseg - 1) / p.done_nseg;
    for (int i = nreg; i < 4; ++i) p.reg_lo[i] = S, p.reg_hi[i] = S, p.reg_t0[i] = 1 << 30;
    p.heavy_lo = 0, p.n_heavy = 0;
    if (heavy_reg >= 0) {
        p.heavy_lo = p.reg_t0[heavy_reg];
        p.n_heavy = (heavy_reg + 1 < nreg ? p.reg_t0[heavy_reg + 1] : p.nqt) - p.heavy_lo;
        if (p.n_heavy >= p.nqt) p.heavy_lo = 0, p.n_heavy = 0;
    }
}

// parameters of a launch of call `c` under c.mask and c.perm (the tensors may be null: the host-side walks of the svg_debug_* entries)
template <typename Pol, typename T>
inline typename Pol::Params make_band_params(const BandCall& c) {
    const int BH = c.BH, S = c.S;
    const svg_band_mask_t* const mask = c.mask;
    const svg_perm_desc_t* const perm = c.perm;
    typename Pol::Params p;
    p.q = (const T*)c.q, p.k = (const T*)c.k, p.v = (const T*)c.v, p.o = (T*)c.o;
    p.lay = c.strided ? c.lay : contiguous_layout(BH, BH, S, S, Pol::kHeadDim);
    p.S = S, p.BH = BH, p.nqt = (S + Pol::BM - 1) / Pol::BM;
    p.scale_log2 = c.sm_scale * 1.4426950408889634f;
    p.real_len = mask->real_len, p.band = mask->band;
    p.cf_lo = mask->colfull_lo, p.cf_hi = mask->colfull_hi, p.rf_lo = mask->rowfull_lo, p.rf_hi = mask->rowfull_hi;
    p.done = c.done, p.done_nseg = 1, p.done_tps = 1 << 30;   // (done_tps is set once nqt is known, below)
    p.head_flag = nullptr, p.vid0 = 0, p.F = 1, p.P = 1, p.V = 0;
    if (perm && perm->head_perm_flag) {
        p.head_flag = perm->head_perm_flag;
        p.vid0 = perm->vid0, p.F = perm->num_frame, p.P = perm->frame_size, p.V = perm->num_frame * perm->frame_size;
    }
    p.q64 = kBN / p.F, p.r64 = kBN % p.F;
    p.q128 = 2 * kBN / p.F, p.r128 = 2 * kBN % p.F;
    p.sp64 = p.q64 + p.r64 * p.P, p.sp128 = p.q128 + p.r128 * p.P;
    p.wrap_phys = 1 - p.F * p.P;
    band_row_regions<Pol>(p, S, 0, S, c.done_nseg);
    // what the LSE / fp32 policies (BandLsePolicy, BandF32Policy and what is built on them) add: lse, and o32 in the place of the 16-bit o
    if constexpr (std::is_base_of_v<BandLsePolicy<T>, Pol>) p.lse = c.lse;
    if constexpr (std::is_base_of_v<BandF32Policy<T>, Pol>) p.o32 = c.o32, p.o = nullptr;
    return p;
}

// parameters of a window launch (BandWindowOf): those of the sequence of S rows, the row regions intersected with the row window — heavy_lo,
// n_heavy and nqt follow the clipped regions — and the tensors as [BH, Sq | Sk, D] (or `c.lay`)
template <typename Pol, typename T>
inline typename Pol::Params make_band_window_params(const BandCall& c) {
    typename Pol::Params p = make_band_params<Pol, T>(c);   // (the window entries take no head permutation: c.perm is null)
    if (!c.strided) p.lay = contiguous_layout(c.BH, c.BH, c.win_Sq, c.win_Sk, Pol::kHeadDim);
    p.q_begin = c.q_begin, p.Sq = c.win_Sq, p.k_begin = c.k_begin, p.k_end = c.k_begin + c.win_Sk;
    band_row_regions<Pol>(p, c.S, c.q_begin, c.q_begin + c.win_Sq, 1);
    return p;
}

// one side of a shard launch (BandShardOf) from its ABI descriptor; a shard without a tail gets the tail's place behind the video
inline BandShardMap make_band_shard_map(const svg_band_shard_t& s, int vid0, int F, int P) {
    BandShardMap m;
    m.f0 = s.f0, m.Fl = s.n_frames, m.nv = P * s.n_frames, m.n = m.nv + s.n_tail;
    m.tail_begin = s.n_tail > 0 ? s.tail_begin : vid0 + F * P;
    m.fdiv = std::max(s.n_frames, 1);
    m.sp64 = kBN / m.fdiv + (kBN % m.fdiv) * P;
    return m;
}

// Row regions of a shard launch for the heads of one kind: band_row_regions in the local order of the q shard — the cuts of the mask
// (rowfull_lo, rowfull_hi, real_len) through ginv_q.  Returns the number of q-tiles.
template <typename Pol>
inline int band_shard_regions(const typename Pol::Params& p, int kind, int* lo, int* hi, int* t0) {
    const int S = p.S, real = std::min(std::max(p.real_len, 0), S);
    const bool has_rf = p.rf_hi > p.rf_lo && p.rf_lo < real && p.band <= S;
    const int a = has_rf ? std::max(p.rf_lo, 0) : 0, b = has_rf ? std::min(p.rf_hi, real) : 0;
    auto loc = [&](int x) { return p.qs.ginv(p.vid0, p.F, p.P, kind, x); };
    const int cuts[5] = {0, loc(a), loc(b), loc(real), p.qs.n};
    int nreg = 0, nqt = 0;
    for (int i = 0; i < 4; ++i) {
        if (cuts[i + 1] <= cuts[i]) continue;
        lo[nreg] = cuts[i], hi[nreg] = cuts[i + 1], t0[nreg] = nqt;
        nqt += (cuts[i + 1] - cuts[i] + Pol::BM - 1) / Pol::BM;
        ++nreg;
    }
    for (int i = nreg; i < 4; ++i) lo[i] = p.qs.n, hi[i] = p.qs.n, t0[i] = 1 << 30;
    return nqt;
}

// parameters of a shard launch (BandShardOf): those of the sequence of S rows with the video geometry of `perm` (its flags may be null: every
// head in logical order), the two shard maps, the row regions of both head kinds — nqt is the larger count — and the tensors as
// [BH, Sq | Sk, D] (or `c.lay`)
template <typename Pol, typename T>
inline typename Pol::Params make_band_shard_params(const BandCall& c) {
    const svg_perm_desc_t* const perm = c.perm;
    BandCall whole = c;   // (the strides of the row cursor are those of a call without a head permutation)
    whole.perm = nullptr;
    typename Pol::Params p = make_band_params<Pol, T>(whole);
    p.head_flag = perm->head_perm_flag;
    p.vid0 = perm->vid0, p.F = perm->num_frame, p.P = perm->frame_size, p.V = perm->num_frame * perm->frame_size;
    p.qs = make_band_shard_map(*c.q_shard, p.vid0, p.F, p.P), p.ks = make_band_shard_map(*c.k_shard, p.vid0, p.F, p.P);
    if (!c.strided) p.lay = contiguous_layout(c.BH, c.BH, p.qs.n, p.ks.n, Pol::kHeadDim);
    p.nqt = band_shard_regions<Pol>(p, 0, p.reg_lo, p.reg_hi, p.reg_t0);
    const int nqt1 = band_shard_regions<Pol>(p, 1, p.reg1_lo, p.reg1_hi, p.reg1_t0);
    if (p.head_flag) p.nqt = std::max(p.nqt, nqt1);
    p.heavy_lo = 0, p.n_heavy = 0, p.done_nseg = 1, p.done_tps = 1 << 30;
    return p;
}

// 4 waves x 64 rows, one wave per SIMD (attn_body_w4, attention_w4.hip)
int run_band_w4(const BandCall& c);
// waves that report per 256-row q-tile of the kernel `variant` selects (completion-counter targets); -1: no counters
int band_waves_per_tile(int variant);

}  // namespace svg

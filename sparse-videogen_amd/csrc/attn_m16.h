// attn_body_m16 — the two-phase ping-pong schedule of attn_body_pp2 (attn_core.h) on v_mfma_f32_16x16x32_{bf16,f16}, head_dim 128.
//
// Why a second matrix shape (round 4, profiles/r04b_energy_table.txt, tools/energy_table.hip): the 16-bit attention kernels run at
// the chip's power limit, and with operand data that changes from one MFMA to the next — real K, V, P — the matrix pipe ALONE is
// power-limited: back-to-back v_mfma_f32_32x32x16_bf16 on all 1024 SIMDs is granted 1.75 GHz (0.72 of the 2.5 PFLOP/s the peak is
// quoted at; 2.39 GHz with constant operands), the same FLOPs issued as v_mfma_f32_16x16x32_bf16 2.15 GHz (0.88).  A 16x16x32 MFMA
// contracts 32 products into each fp32 accumulator per instruction, a 32x32x16 one 16: half the accumulator read-modify-writes per
// FLOP.  Everything else of the schedule is energy-neutral between the shapes: the same LDS operand bytes per tile (every fragment
// read feeds TWO MFMAs here: the two 16-row blocks of a wave's 32 query rows), the same registers, the same vector phase.
//
// Shapes (both GEMMs "swapped" as in attn_core.h, so that a lane owns query rows, not keys):
//   S^T[key][q] = K Q^T      A = K fragment: lane (g4, n): key 16 kb + n, d 32 ks + 8 g4 + [0, 8)       one ds_read_b128
//                            B = Q fragment: lane (g4, n): query row 16 rb + n of the wave, the same d     registers (32 VGPRs)
//                            D: lane (g4, n): query row 16 rb + n, keys 16 kb + 4 g4 + [0, 4)
//   O^T[d][q]   = V^T P^T    A = V^T fragment: lane (g4, n): d 16 dblk + n, k-index 8 g4 + [0, 8) of a 32-key chunk kc
//                            B = P fragment: lane (g4, n): query row 16 rb + n, k-index 8 g4 + [0, 8)
//                            D: lane (g4, n): query row 16 rb + n, d 16 dblk + 4 g4 + [0, 4)
//   with g4 = lane >> 4, n = lane & 15.  The contraction order of the PV GEMM is free, so k-index 8 g4 + j of chunk kc means key
//   32 kc + 4 g4 + j (j < 4) and key 32 kc + 16 + 4 g4 + (j - 4) (j >= 4): the P fragment of a lane is exactly its S^T accumulators of
//   key blocks 2 kc and 2 kc + 1 — no LDS round trip, no shuffles, as in the 32x32x16 bodies — and the V^T fragment is two
//   ds_read_b64_tr_b16 (4 keys x 16 columns each per 16-lane group).
// A lane holds TWO query rows (rb = 0, 1), each spread over the four lane groups g4: the softmax state (reference, partial row sum,
// mask intervals) is per (lane, rb); the row sum is completed across g4 once, in the epilogue; the row maximum crosses lanes on the
// exact path only (max-free softmax, see attn_body_pp2).
//
// LDS images (in code: KvImage16 below).
// Both tensors sub-tiled [D/32][64 keys][4 x 16 B] as in attn_body_pp2, both with ONE swizzle: 16-byte chunk c of key k sits
// in slot c ^ (((k >> 2) & 1) << 1), i.e. the two 32-byte halves of a row are swapped for keys 4 - 7, 12 - 15, ...  (MI355X_MICROARCH.md
// §LDS gives the lane groups that share an LDS cycle):
//   * K, ds_read_b128 (four groups of 16 lanes: {0-3, 12-15, 20-27}, {4-11, 16-19, 28-31}, ...): lane (g4, n) reads key n, chunk g4 —
//     a group is 8 keys of one g4 plus 4 + 4 keys of another; with this swizzle their 16 slots x 4 banks are disjoint.  (The swizzle of
//     the 32x32x16 bodies, slot = c ^ ((k >> 2) & 3), is two-way here: SQ_LDS_BANK_CONFLICT 2.6e9 cycles per launch in the first
//     version, profiles/r04e_pmc_lds_m16_first.txt.)
//   * V, ds_read_b64_tr_b16 (two groups of 32 lanes): a wave's transposing read covers 16 keys x 16 columns = 16 rows x 32 B at a 64 B
//     stride; the swap makes every 8 consecutive rows (one lane group pair) cover all 64 banks.
// The swizzle is applied to the per-lane SOURCE address of the LDS-DMA (the same address for K and V), so one lane still resolves one
// key row per tile for both tensors.
#pragma once
#include "attn_core.h"

namespace svg {

template <typename T>
struct Mfma16;
// (mfma_keep_c: D = A B + C with D and C in DIFFERENT registers, as inline asm — for a C that stays live hipcc selects the tied form of
//  the builtin and copies C first; see Elt::mfma_keep_c in svg_common.h.  The caller owns the hazards: tools/asm_hazards.py audits the
//  kept listing, tests/test_w4_asm_audit.py.)
template <>
struct Mfma16<__bf16> {
    static __device__ __forceinline__ f32x4 mfma(bf16x8 a, bf16x8 b, f32x4 c) { return __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b, c, 0, 0, 0); }
    static __device__ __forceinline__ f32x4 mfma_keep_c(bf16x8 a, bf16x8 b, const f32x4& c) {
        f32x4 d;
        asm volatile("v_mfma_f32_16x16x32_bf16 %0, %1, %2, %3" : "=&v"(d) : "v"(a), "v"(b), "v"(c));
        return d;
    }
};
template <>
struct Mfma16<_Float16> {
    static __device__ __forceinline__ f32x4 mfma(f16x8 a, f16x8 b, f32x4 c) { return __builtin_amdgcn_mfma_f32_16x16x32_f16(a, b, c, 0, 0, 0); }
    static __device__ __forceinline__ f32x4 mfma_keep_c(f16x8 a, f16x8 b, const f32x4& c) {
        f32x4 d;
        asm volatile("v_mfma_f32_16x16x32_f16 %0, %1, %2, %3" : "=&v"(d) : "v"(a), "v"(b), "v"(c));
        return d;
    }
};

constexpr int attn_m16_lds_bytes() { return attn_pp2_lds_bytes<128>(); }

// The K / V image of the 16x16x32 bodies (attn_m16_tile, profile16_kernel of profiler.hip), see "LDS images" in the file header: the single
// definition of its write side (the source column a lane hands the LDS-DMA) and its read side (the fragment addresses, raw bits).
template <int D>
struct KvImage16 {
    static constexpr int kImg = kBN * D * 2, kStage = 2 * kImg;   // bytes of a K or V image / of a stage: [K image | V image]
    static constexpr unsigned col_v(int lane) {    // the same source column for both tensors; XOR: ((key >> 2) & 1) << 1 of the lane's key row
        return ((lane & 3) ^ ((unsigned)((lane >> 4) & 1) << 1)) * 16u;
    }
    static constexpr unsigned col_k(int lane) { return col_v(lane); }
    // read side, lane (g4, n16) = (lane >> 4, lane & 15): the lane's part of the K fragment address / the V^T one (even d blocks;
    // odd ones: ^ 32)
    static constexpr int k_lane(int g4, int n16) { return (n16 << 6) | ((g4 ^ (((n16 >> 2) & 1) << 1)) << 4); }
    static constexpr int v_lane0(int g4, int n16) { return kImg + (4 * g4 + (n16 >> 2)) * 64 + (((g4 & 1) * 16) + 4 * (n16 & 3)) * 2; }
    // K fragment of 16-key block kblk, contraction step ks / half h of the V^T fragment of 32-key chunk kc, 16-wide d block db
    // ("Shapes" in the file header)
    static constexpr int k_off(int k_lane, int kblk, int ks) { return k_lane + ks * (kBN * 64) + kblk * 1024; }
    static constexpr int v_off(int v_lane0, int v_lane1, int kc, int db, int h) {
        return ((db & 1) ? v_lane1 : v_lane0) + (db >> 1) * (kBN * 64) + (32 * kc + 16 * h) * 64;
    }
    static __device__ __forceinline__ i16x8 kfrag(const char* st, int k_lane, int kblk, int ks) {
        return *(const i16x8*)(st + k_off(k_lane, kblk, ks));
    }
    static __device__ __forceinline__ i16x8 vfrag(const char* st, int v_lane0, int v_lane1, int kc, int db) {
        return lds_read_tr16x2(st + v_off(v_lane0, v_lane1, kc, db, 0), st + v_off(v_lane0, v_lane1, kc, db, 1));
    }
    static constexpr int k_read(int key, int c) { return k_off(k_lane(c & 3, key & 15), key >> 4, c >> 2); }
    static constexpr int v_read(int key, int d) {
        const int lane = 16 * ((key >> 2) & 3) + (d & 15), src = tr16_src_lane(lane, key & 3), vl0 = v_lane0(src >> 4, src & 15);
        return v_off(vl0, vl0 ^ 32, key >> 5, d >> 4, (key >> 4) & 1) + 2 * (lane & 3);
    }
};
static_assert(kv_image_consistent<KvImage16<64>, 64>() && kv_image_consistent<KvImage16<128>, 128>(),
              "KvImage16: DMA columns and fragment reads disagree");

// lanes l, l ^ 16, l ^ 32, l ^ 48 hold one query row: maximum / sum over them (rare paths and the epilogue only)
__device__ __forceinline__ float quad_group_max(float x) {
    x = vmax2(x, __shfl_xor(x, 16));
    return vmax2(x, __shfl_xor(x, 32));
}
__device__ __forceinline__ float quad_group_sum(float x) {
    x += __shfl_xor(x, 16);
    return x + __shfl_xor(x, 32);
}

// Add-on-store (detected: a policy with a static add_on_store(prm), cross_policy.h CrossPairPolicy; every other policy compiles the row
// store it had): where add_on_store(prm) holds, the final row store ADDS the q-tile's rounded result to the 16-bit values already in o —
// T(float(o) + float(T(result))), one fp32 add and one conversion per element, what torch's add of two 16-bit tensors does.
template <typename P, typename = void>
struct HasAddOnStore : std::false_type {};
template <typename P>
struct HasAddOnStore<P, std::void_t<decltype(&P::add_on_store)>> : std::true_type {};

// Row log-sum-exp (detected: a policy with a static lse_base(prm, ctx), cross_policy.h CrossLsePolicy; every other policy
// compiles the epilogue it had): the epilogue also stores, per query row, lse = log sum_j exp(sm_scale * q.k_j) over the keys the row saw,
// natural log, fp32, at lse_base(prm, ctx)[physical q row].  At the end of the tile loop the probabilities of a row are
// 2^(s * scale_log2 - m_use - kBias) and l_tot is their sum, so lse = ln2 * (m_use + kBias + log2(l_tot)); a row without keys (l_tot == 0)
// gives -inf.  Lanes 0..15 of a wave store (one lane per row, 2 x 16 stores per wave and q-tile), rows behind the q-tile's end are not
// written; no LDS, no barrier.
template <typename P, typename = void>
struct HasRowLse : std::false_type {};
template <typename P>
struct HasRowLse<P, std::void_t<decltype(&P::lse_base)>> : std::true_type {};

// fp32 rows (detected: a policy with a static o32_base(prm, ctx), the *F32Policy of cross_policy.h / band_policy.h / varblock_policy.h;
// every other policy compiles the epilogue it had): the epilogue stores acc_o * inv — the value the 16-bit store rounds — as fp32 at
// o32_base(prm, ctx)[physical q row * D + column], a contiguous [heads, rows, D] in the caller's row order (the row index of the lse
// store), and writes no 16-bit o.  What a merge over parts of the keys takes without a rounding per part (svg_merge_attention_states_f32).
// Straight from the accumulator registers: a lane holds four consecutive floats per (db, rb) at column 16 * db + 4 * g4, so one 16-byte
// store per (db, rb) — the four lanes of a row's quad group fill one 64-byte run; no LDS (the staging region holds 16-bit rows) and no
// barrier.  Rows behind the q-tile's end (q_phys < 0) store nothing, a row without keys stores zeros (inv == 0).
template <typename P, typename = void>
struct HasRowO32 : std::false_type {};
template <typename P>
struct HasRowO32<P, std::void_t<decltype(&P::o32_base)>> : std::true_type {};
// The four fp32 values of one (db, rb).  bf16: the 16-bit store rounds the fp32 product, so the product is the value.  fp16: the 16-bit
// store of the same accumulators is compiled (-ffast-math contraction) to a mix of v_fma_mixlo_f16 — the exact product rounded once — and
// v_pk_mul_f32 + v_cvt_pk_f16_f32 — rounded twice — so the fp32 product rounded again by the caller differs from it where the product lies
// exactly on the midpoint of two fp16 values and the store took the other neighbour (about 3e-5 of the elements).  So the fp16 form
// also evaluates the 16-bit store's own expression, and where the fp32 product does not round to that value it moves ONE fp32 step
// towards it: o32 rounded to nearest even is then the 16-bit o, and o32 stays within one fp32 step of acc * inv.  (The empty asm
// statements keep the two evaluations apart: without them the compiler folds both into one and the comparison is always true.)
template <typename T, typename E>
__device__ __forceinline__ f32x4 o32_values(const f32x4& acc, float inv) {
    f32x4 o4;
    if constexpr (std::is_same_v<T, _Float16>) {
        typename E::v4 h4;
#pragma unroll
        for (int j = 0; j < 4; ++j) h4[j] = E::from_float(acc[j] * inv);   // the expression of the 16-bit store
        u32x2 hb = __builtin_bit_cast(u32x2, h4);
        asm("" : "+v"(hb));
        h4 = __builtin_bit_cast(typename E::v4, hb);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            float a = acc[j];
            asm("" : "+v"(a));
            float p = a * inv;
            asm("" : "+v"(p));
            const float h = (float)h4[j];
            if ((float)(_Float16)p != h)   // p is a midpoint and the store took the other neighbour (false for 0 against -0; a NaN stays one)
                p = __uint_as_float(fabsf(h) > fabsf(p) ? __float_as_uint(p) + 1u : __float_as_uint(p) - 1u);
            o4[j] = p;
        }
    } else {
#pragma unroll
        for (int j = 0; j < 4; ++j) o4[j] = acc[j] * inv;
    }
    return o4;
}

// Row cursor (detected: a policy with kRowCursor, band_policy.h BandPolicy; every other policy keeps kv_cursor_init / kv_phys and compiles
// the request pipeline it had): the lane's key row is ONE variable stepped in place by P::row_walk_next, the decision between the
// cheap step and the exact path is scalar, and the two byte offsets of a request are formed when the request pipeline takes the row.
template <typename P, typename = void>
struct HasRowCursor : std::false_type {};
template <typename P>
struct HasRowCursor<P, std::void_t<decltype(P::kRowCursor)>> : std::true_type {};

// Tile run (detected: a policy whose kTileRun is true, band_policy.h BandPolicy::tile_run; every other policy — those without the member and
// those that set it to false — compiles the per-tile decisions it had): inside [run_lo, run_lo + run_n), computed once per q-tile and wave,
// the vector phase knows that its tile is FULL and that the tile it resolves takes the cheap step, so the scalar unit runs one compare and
// one add there instead of tile_key0 twice, row_walk_cheap and classify.
template <typename P, typename = void>
struct HasTileRun : std::false_type {};
template <typename P>
struct HasTileRun<P, std::enable_if_t<P::kTileRun>> : std::true_type {};
// the parts of the cursor's step the run form calls: P's for a policy with tile runs; for every other policy stand-ins that are never executed
// (the run form is compiled out by a constant there) and only have to compile inside the generic lambda of the vector phase
template <typename P, bool = HasTileRun<P>::value>
struct TileRunOps {
    template <typename... A> static __device__ __forceinline__ void step(A&...) {}
    template <typename... A> static __device__ __forceinline__ void in_run(A&...) {}
    template <typename... A> static __device__ __forceinline__ bool cheap(A&...) { return true; }
    template <typename... A> static __device__ __forceinline__ void exact(A&...) {}
};
template <typename P>
struct TileRunOps<P, true> {
    using W = typename P::RowWalk;
    static __device__ __forceinline__ void step(const W& w, int& phys) { P::row_walk_step(w, phys); }
    static __device__ __forceinline__ void in_run(W& w) { P::row_walk_in_run(w); }
    static __device__ __forceinline__ bool cheap(W& w, const int& k0) { return P::row_walk_cheap(w, k0); }
    static __device__ __forceinline__ void exact(const typename P::Params& p, const W& w, int& phys, const int& k0, const int& row) {
        P::row_walk_exact(p, w, phys, k0, row);
    }
};

// pp_barrier_if for a predicate that is already a scalar: the workgroup barrier where (flag != 0) == when_set.  One scalar serves
// both barriers of a tile (leading / lagging waves keep opposite ones), and nothing is fetched from a VGPR.
template <bool when_set>
__device__ __forceinline__ void pp_barrier_sel(int flag) {
    __builtin_amdgcn_sched_barrier(0);
    if constexpr (when_set) asm volatile("s_cmp_eq_u32 %0, 0\n\ts_cbranch_scc1 1f\n\ts_waitcnt lgkmcnt(0)\n\ts_barrier\n1:" ::"s"(flag) : "memory", "scc");
    else asm volatile("s_cmp_lg_u32 %0, 0\n\ts_cbranch_scc1 1f\n\ts_waitcnt lgkmcnt(0)\n\ts_barrier\n1:" ::"s"(flag) : "memory", "scc");
    __builtin_amdgcn_sched_barrier(0);
}

template <typename T>
__device__ __forceinline__ u32x2 add_rounded16(u32x2 a, u32x2 b) {
    using E = Elt<T>;
    const typename E::v4 x = __builtin_bit_cast(typename E::v4, a), y = __builtin_bit_cast(typename E::v4, b);
    typename E::v4 s;
#pragma unroll
    for (int j = 0; j < 4; ++j) s[j] = E::from_float(E::to_float(x[j]) + E::to_float(y[j]));
    return __builtin_bit_cast(u32x2, s);
}

// ONEBAR: -1 as the policy says, 0 / 1 forced.  The matrix phase runs at issue priority 1, as in attn_body_pp2.
// PRE: q arrives multiplied by sm_scale * log2(e) and the S^T accumulators start at minus the row's reference, so the MFMAs deliver the
// exponent argument (no scale-and-shift FMA per score; the scheme of attn_body_pp2's PRE form).
// (Round 4 measured a PRE form with q and k as fp16 carriers and S^T on the f16 MFMA: the plain kernel's distance to the reference's
//  formulation, but no time — 33.8 ms against 32.8 for the bf16 PRE form, plus 0.58 ms for the conversion pass; profiles/r04l_*,
//  r04m_f16qk_kernel_trace.txt.  Removed with the template flag that kept it.)
// attn_m16_tile: one q-tile, described by `ctx` (P::init or, for a workgroup that takes its q-tiles from a queue, P::init_tile).  Every
// wave of the workgroup passes the same number of workgroup barriers whatever its role (leading, lagging, idle: nT + 2 with one
// barrier per tile) and leaves with no LDS-DMA request in flight, so a workgroup may run one q-tile after another: it needs one
// workgroup barrier between two of them (the epilogue of the first reads the stages the second fills).
//
// SPEC (honoured where MSUM is on: bf16, plain form): the overflow test of the max-free softmax runs on every kCheckEvery-th tile only,
// and the q-tile is validated once, after the tile loop.  The per-tile test serves two ends: the reference follows the row maximum, and
// no probability overflows.  The first needs no tile granularity — P is floating point, O and l accumulate in fp32, so a reference that
// lags by up to kCheckEvery - 1 tiles changes the rounding, not the accuracy — and the second is checked where it would show: an
// overflowed probability leaves an infinity or a NaN in the lane's row sums or O accumulators.  After the loop every lane tests them with
// !(|x| < 2^120), the wave votes, lane 0 of a wave that saw one sets a word in LDS behind the stages (smem + attn_m16_lds_bytes() + 8:
// the launch provides 16 bytes there, the caller zeroes the word before the first pass and no pass with check_mask = 0 touches it),
// ONE workgroup barrier follows that every wave passes, idle waves included, and a non-zero word
// makes every wave return true without storing anything (a check point that is about to rescale a large sum by a factor that has
// underflowed to zero makes the sum infinite instead, so that it fails here — see the exact path): the caller then runs the same
// q-tile once more with check_mask = 0 — the test on every tile, the body without SPEC tile for tile, no validation — and that pass stores.  At most one replay per q-tile, no waiting
// on another workgroup; the stages are quiescent at the barrier as they are between two q-tiles of a queue kernel, and no epilogue has
// read them, so the second pass needs no further barrier in front.  `replay_ctr` (or nullptr) counts replayed q-tiles
// (svg_debug_band_replays).  Without SPEC the function returns false.
constexpr int kCheckEvery = 8;
template <typename T, typename P, bool TRACE = false, int ONEBAR = -1, bool PRE = false, bool SPEC = false>
__device__ __forceinline__ bool attn_m16_tile(const typename P::Params& prm, const typename P::Ctx& ctx, char* smem,
                                              int check_mask = kCheckEvery - 1, unsigned* replay_ctr = nullptr) {
    using E = Elt<T>;
    using M = Mfma16<T>;
    using V8 = typename E::v8;
    constexpr int D = 128;
    constexpr int NW = 8;
    constexpr int KS = D / 32;              // 32-wide contraction steps of S^T
    constexpr int NDB = D / 16;             // 16-wide d blocks of O^T
    using Img = KvImage16<D>;               // the K / V image of a stage
    constexpr int NS = 4;                   // LDS stages
    constexpr int kImg = Img::kImg, kStage = Img::kStage;
    constexpr int NP = 2;                   // DMA pieces (16 keys x 64 B) per wave per tensor per tile
    constexpr int kCarry = 8;               // V fragments of the next matrix phase read in the tail of this one (attn_body_pp2: kCarry)
    constexpr int kPF = 8;                  // operand fragments in flight ahead of their MFMAs
    constexpr bool kOneBar = ONEBAR < 0 ? P::kOneBarrier : (ONEBAR != 0);   // one workgroup barrier per tile instead of two (attn_body_pp2: on for the variable-block policy)
    static_assert(P::kRowBlocks == 1 && !P::kPartialOut && !P::kFixup && P::kIntervalMask, "band / variable-block policy");
    // MSUM (bf16, plain form): the row sum on the matrix pipe.  Four extra MFMAs per tile (A = a fragment of ones, B = the
    // P fragment: every accumulator of a lane receives the COMPLETE sum of its query row over the chunk's 32 keys) replace the 32 v_add of
    // the vector phase; the overflow test of the max-free softmax — a probability above the reference by more than 2^kBias — becomes a bit
    // test on the packed bf16 probabilities: with the exponent argument lowered by kBias a probability reaches 2.0 (exponent field >= 128,
    // bit 14 / 30 of the packed word: the OR of all sixteen words shows it, 8 v_or3_b32) exactly when the row sum test of the plain
    // form would be near its 2048.  O and l carry the common factor 2^-kBias, which the final division removes.
    // Measured (profiles/r05a_ab_m16_msum_prio3.txt, same box, HunyuanVideo 720p): 64.1 instead of 65.1 Mcycles per launch, of which the power
    // management returns half as clock (1985 vs 2000 MHz): 32.3 against 32.55 ms; with the sum MFMAs after the chunk's LAST PV step instead of
    // its first the gain is gone (65.4 Mcycles).  fp16 keeps the vector-phase sum: 2^-10 would push small probabilities into fp16's subnormals.
    constexpr bool MSUM = std::is_same_v<T, __bf16> && !PRE;
    constexpr float kBias = MSUM ? 10.f : 0.f;
    constexpr bool kSpec = SPEC && MSUM;
    static_assert(!(SPEC && TRACE) && (kCheckEvery & (kCheckEvery - 1)) == 0, "SPEC: product kernels; a power of two");

    unsigned long long wg_t0 = 0, wg_t2 = 0;   // launch timeline (diagnostics builds, svg_debug_wg_trace): entry, end of the tile loop
    if constexpr (TRACE) wg_t0 = __builtin_amdgcn_s_memtime();
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = wave_id();
    const int g4 = lane >> 4;
    const int n16 = lane & 15;
    const bool lagging = wave >= NW / 2;
    const int nT = ctx.nT;
    // SPEC: tiles with (t & check_mask) == 0 run the overflow test (0 on the replay: every tile); the word the validation votes into
    volatile int* const spec_word = (volatile int*)(smem + attn_m16_lds_bytes() + 8);

    const T* __restrict__ qb = P::q_base(prm, ctx);
    const T* __restrict__ kb_ = P::k_base(prm, ctx);
    const T* __restrict__ vb = P::v_base(prm, ctx);
    const unsigned lds0 = (unsigned)(size_t)smem;

    // ---- DMA bookkeeping: as attn_body_pp2 (a wave's NP pieces per tensor are d-blocks dma_db0 .. of ONE 16-key group) ----
    const int dma_kg = wave / 2;
    const int dma_db0 = (wave % 2) * NP;
    const int krow = 16 * dma_kg + (lane >> 2);
    constexpr bool kCursor = HasRowCursor<P>::value;
    auto cur = [&] {
        if constexpr (kCursor) {
            typename P::RowWalk w;
            P::row_walk_init(prm, ctx, w);
            return w;
        } else {
            typename P::KvCursor c;
            P::kv_cursor_init(prm, ctx, c, krow);
            return c;
        }
    }();
    const unsigned col_v = (unsigned)(dma_db0 * 64 + Img::col_v(lane));            // the source column of BOTH tensors
    const unsigned lds_piece = lds0 + (unsigned)(dma_db0 * (kBN * 64) + dma_kg * 1024);
    // (row strides: 2 D bytes for contiguous heads, H * D or 3 * H * D elements for k / v read in place from a projection's output)
    const unsigned k_rsb = (unsigned)P::k_rs(prm) * 2u, v_rsb = (unsigned)P::v_rs(prm) * 2u;
    int nphys = 0, nnext = 0;
    unsigned req_ko = 0, req_vo = 0;   // row cursor: the byte offsets of the taken row (nphys is not used)
    auto resolve = [&](int t, auto guard_c) {
        if constexpr (kCursor) {   // in place; behind the last tile the cursor stays where it is (nothing requests that row)
            if (!decltype(guard_c)::value || t < nT) P::row_walk_next(prm, cur, nnext, P::tile_key0(ctx, t), krow);
        } else if constexpr (decltype(guard_c)::value) {
            nnext = (t < nT) ? P::kv_phys(prm, ctx, cur, t, krow) : 0;
        } else {
            nnext = P::kv_phys(prm, ctx, cur, t, krow);
        }
    };
    constexpr std::true_type kGuarded{};
    auto take = [&]() {
        if constexpr (kCursor) {
            req_ko = __umul24((unsigned)nnext, k_rsb) + col_v;
            req_vo = __umul24((unsigned)nnext, v_rsb) + col_v;
            asm volatile("" : "+v"(req_ko), "+v"(req_vo));   // formed here, before the cursor moves (P::row_walk_next steps it in place)
        } else {
            nphys = nnext;
        }
    };
    auto dma_piece = [&](int t, auto j_c) {
        constexpr int j = decltype(j_c)::value;
        const unsigned st = __builtin_amdgcn_readfirstlane(lds_piece + (unsigned)((t % NS) * kStage) + j * (kBN * 64));
        const unsigned ko = kCursor ? req_ko : __umul24((unsigned)nphys, k_rsb) + col_v;
        const unsigned vo = kCursor ? req_vo : __umul24((unsigned)nphys, v_rsb) + col_v;
        lds_dma16_kv<kImg>(st, ko, vo, (const char*)kb_ + j * 64, (const char*)vb + j * 64);
    };
    auto dma_issue = [&](int t) {
        dma_piece(t, std::integral_constant<int, 0>{});
        dma_piece(t, std::integral_constant<int, 1>{});
    };
    const int dist = lagging ? 3 : 2;   // tile u + dist is requested in N(u)
    constexpr bool kRun = kCursor && HasTileRun<P>::value;
    int run_lo = 0, run_n = 0;          // tile run of this wave: two scalars of the q-tile
    if constexpr (kRun) {
        P::tile_run(ctx, cur, dist, run_lo, run_n);
        run_lo = __builtin_amdgcn_readfirstlane(run_lo), run_n = __builtin_amdgcn_readfirstlane(run_n);
    }
    for (int t = 0; t < dist; ++t) {
        resolve(t, kGuarded);
        take();
        if (t < nT) dma_issue(t);
    }
    resolve(dist, kGuarded);   // requested in N(0)

    // ---- Q fragments, mask intervals and softmax state of the lane's two query rows ----
    int q_log[2];
    V8 qf[2][KS];
    int m_a0[2], m_b0[2];
    unsigned m_alen[2], m_blen[2];
#pragma unroll
    for (int rb = 0; rb < 2; ++rb) {
        const int row_in_wg = wave * 32 + rb * 16 + n16;
        const int qp = P::q_phys(prm, ctx, row_in_wg);
        q_log[rb] = P::q_logical(ctx, row_in_wg);
        const T* qrow = qb + (size_t)(qp >= 0 ? qp : 0) * P::q_rs(prm) + g4 * 8;
#pragma unroll
        for (int ks = 0; ks < KS; ++ks) qf[rb][ks] = *(const V8*)(qrow + ks * 32);
        P::row_intervals(prm, ctx, q_log[rb], m_a0[rb], m_alen[rb], m_b0[rb], m_blen[rb]);
    }

    const int k_lane = Img::k_lane(g4, n16);
    const int v_lane0 = Img::v_lane0(g4, n16);   // even 16-wide d blocks
    const int v_lane1 = v_lane0 ^ 32;            // odd ones

    float m_run[2] = {-INFINITY, -INFINITY}, m_use[2] = {0.f, 0.f}, l_run[2] = {0.f, 0.f}, psum[2] = {0.f, 0.f};
    float m_sub[2] = {kBias, kBias};                                   // what the exponent argument subtracts: m_use + kBias
    f32x4 acc_l[2] = {{0.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 0.f}};     // MSUM: row sums (every element the same complete sum)
    V8 ones8;
#pragma unroll
    for (int j = 0; j < 8; ++j) ones8[j] = E::from_float(1.f);
    bool force_exact = true;                                           // MSUM: psum_thr < 0
    int spec_mode = -1;                                                // SPEC: -1 while force_exact holds, then check_mask
    f32x4 acc_o[NDB][2];
#pragma unroll
    for (int db = 0; db < NDB; ++db)
#pragma unroll
        for (int rb = 0; rb < 2; ++rb)
#pragma unroll
            for (int r = 0; r < 4; ++r) acc_o[db][rb][r] = 0.f;
    const float c_log2 = prm.scale_log2;
    if constexpr (MSUM) asm volatile("" : "+v"(ones8));

#pragma unroll
    for (int rb = 0; rb < 2; ++rb)
#pragma unroll
        for (int ks = 0; ks < KS; ++ks) asm volatile("" : "+v"(qf[rb][ks]));
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    pp_barrier();
    if (!kOneBar && lagging) pp_barrier();  // waves 4..7 run one phase behind

    const bool idle = !P::wave_active(ctx, wave * 32);

    // per-phase cycle trace (diagnostics builds, svg_debug_pp_trace: the slots of attn_body_pp2 — M, barrier, N, barrier)
    unsigned tr_acc[4] = {0, 0, 0, 0};
    unsigned long long tr_last = 0, tr_first = 0;
    if constexpr (TRACE) tr_first = tr_last = __builtin_amdgcn_s_memtime();
    auto tick = [&](auto slot_c) {
        if constexpr (TRACE) {
            constexpr int slot = decltype(slot_c)::value;
            const unsigned long long now = __builtin_amdgcn_s_memtime();
            tr_acc[slot] += (unsigned)(now - tr_last);
            tr_last = now;
        }
    };

    f32x4 neg_ref[2] = {{0.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 0.f}};   // PRE: minus the reference of the lane's two rows (what the S^T accumulators start from)
    float pre_shift[2] = {0.f, 0.f};                                   // PRE, exact path only: old reference minus new reference
    f32x4 sc[4][2];        // scores [16-key block][row block]: S(t) until the PV steps have consumed it, then S(t + 1) accumulates here
    V8 pf[2][2];           // probabilities [32-key chunk][row block]
    float psum_thr = -1.f; // (wave-uniform) 2048 once every row of the wave has a finite reference; until then every tile takes the exact path

    // operand fragments travel as raw bits
    auto kfrag = [&](const char* st, int kblk, int ks) -> i16x8 { return Img::kfrag(st, k_lane, kblk, ks); };
    auto vfrag = [&](const char* st, int kc, int db) -> i16x8 { return Img::vfrag(st, v_lane0, v_lane1, kc, db); };
    // probabilities of the 32-key chunk kc: the lane's 8 scores per row block (key blocks 2 kc, 2 kc + 1) against the row's reference
    auto probs_impl = [&](int kc, auto shifted_c) {
        constexpr bool shifted = decltype(shifted_c)::value;
#pragma unroll
        for (int rb = 0; rb < 2; ++rb)
#pragma unroll
            for (int h = 0; h < 2; ++h)
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    float p;
                    if constexpr (PRE && shifted) p = __builtin_amdgcn_exp2f(sc[2 * kc + h][rb][r] + pre_shift[rb]);
                    else if constexpr (PRE) p = __builtin_amdgcn_exp2f(sc[2 * kc + h][rb][r]);    // the MFMAs delivered the exponent argument
                    else p = __builtin_amdgcn_exp2f(__builtin_fmaf(sc[2 * kc + h][rb][r], c_log2, -m_sub[rb]));
                    if constexpr (!MSUM) psum[rb] += p;
                    pf[kc][rb][4 * h + r] = E::from_float(p);
                }
    };
    auto probs = [&](int kc) { probs_impl(kc, std::false_type{}); };
    auto stage_resolve_next = [&](int t, auto guard_c) {
        take();
        resolve(t + dist + 1, guard_c);
    };
    auto stage_request = [&](int t) {
        const bool more = t + dist < nT;
        if (more) dma_issue(t + dist);
        if (more) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(2 * NP) : "memory");
        else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    };
    // vector phase of tile t on sc: mask, probabilities, sum check, (rare) exact path, DMA requests, DMA wait
    auto vector_phase = [&](int t, auto guard_c) {
        constexpr bool guard = decltype(guard_c)::value;
        constexpr bool run_form = kRun && !guard;   // (runs lie inside the unguarded loop)
        int tk0 = 0, cls = TILE_FULL;
        if constexpr (run_form) {
            // The per-lane step is common to the tiles inside and outside the run; the scalar decisions — which tile comes next, whether it
            // steps, what this tile's class is — are made outside the run only.  The exact path stays the one-armed branch around an
            // in-place write that row_walk_next has: what it tests is a scalar both ways.
            using R = TileRunOps<P>;
            const bool in_run = (unsigned)(t - run_lo) < (unsigned)run_n;
            take();
            R::step(cur, nnext);
            dma_piece(t + dist, std::integral_constant<int, 0>{});
            bool cheap = true;
            int k_next = 0;
            if (__builtin_expect(in_run, 1)) {
                R::in_run(cur);
            } else {
                k_next = P::tile_key0(ctx, t + dist + 1);
                cheap = R::cheap(cur, k_next);
                tk0 = P::tile_key0(ctx, t);
                cls = P::classify(prm, ctx, tk0, wave * 32);
            }
            if (__builtin_expect(!cheap, 0)) R::exact(prm, cur, nnext, k_next, krow);
        } else {
            stage_resolve_next(t, guard_c);
        }
        const bool more = !guard || t + dist < nT;
        if constexpr (!run_form) {
            if (more) dma_piece(t + dist, std::integral_constant<int, 0>{});
            tk0 = P::tile_key0(ctx, t);
            cls = P::classify(prm, ctx, tk0, wave * 32);
        }
        if (cls != TILE_FULL) {
            const bool part = (cls == TILE_PARTIAL);  // a tile this wave does not need at all is processed fully masked
#pragma unroll
            for (int rb = 0; rb < 2; ++rb) {
                int ka = tk0 + 4 * g4 - m_a0[rb], kb2 = tk0 + 4 * g4 - m_b0[rb];
                asm volatile("" : "+v"(ka), "+v"(kb2));   // opaque: keeps LICM from hoisting the per-element terms out of the loop
#pragma unroll
                for (int b = 0; b < 4; ++b)
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        const int key = 16 * b + r;
                        const bool ok = ((unsigned)(ka + key) < m_alen[rb]) | ((unsigned)(kb2 + key) < m_blen[rb]);
                        sc[b][rb][r] = (part & ok) ? sc[b][rb][r] : -INFINITY;
                    }
            }
        }
        if (more) dma_piece(t + dist, std::integral_constant<int, 1>{});
        psum[0] = 0.f, psum[1] = 0.f;
#pragma unroll
        for (int kc = 0; kc < 2; ++kc) {
            probs(kc);
            asm volatile("" : "+v"(pf[kc][0]), "+v"(pf[kc][1]), "+v"(psum[0]), "+v"(psum[1]));   // stays in this phase
        }
        bool exact;
        if constexpr (MSUM) {
            typedef unsigned u32x4_t __attribute__((ext_vector_type(4)));
            const u32x4_t w0 = __builtin_bit_cast(u32x4_t, pf[0][0]), w1 = __builtin_bit_cast(u32x4_t, pf[0][1]);
            const u32x4_t w2 = __builtin_bit_cast(u32x4_t, pf[1][0]), w3 = __builtin_bit_cast(u32x4_t, pf[1][1]);
            const unsigned o0 = w0[0] | w0[1] | w0[2], o1 = w0[3] | w1[0] | w1[1], o2 = w1[2] | w1[3] | w2[0];   // (v_or3_b32, depth 3)
            const unsigned o3 = w2[1] | w2[2] | w2[3], o4 = w3[0] | w3[1] | w3[2];
            if constexpr (kSpec) {
                exact = spec_mode < 0;
                if (spec_mode >= 0 && (t & spec_mode) == 0) {   // wave-uniform: a scalar branch around the OR chain and the vote
                    const unsigned bits = (o0 | o1 | o2) | (o3 | o4 | w3[3]);
                    exact = __builtin_amdgcn_readfirstlane((int)__any((bits & 0x40004000u) != 0u)) != 0;   // (a scalar on both paths)
                }
            } else {
                const unsigned bits = (o0 | o1 | o2) | (o3 | o4 | w3[3]);
                exact = force_exact || __any((bits & 0x40004000u) != 0u);
            }
        } else {
            exact = !__all(psum[0] + psum[1] <= psum_thr);
        }
        if (exact) {      // exact path (rare; always until every row has a finite reference; also a non-finite sum)
            bool all_finite = true;
            float alpha[2];
#pragma unroll
            for (int rb = 0; rb < 2; ++rb) {
                float mx = vmax3(sc[0][rb][0], sc[0][rb][1], sc[0][rb][2]);
                mx = vmax3(mx, sc[0][rb][3], sc[1][rb][0]);
                mx = vmax3(mx, sc[1][rb][1], sc[1][rb][2]);
                mx = vmax3(mx, sc[1][rb][3], sc[2][rb][0]);
                mx = vmax3(mx, sc[2][rb][1], sc[2][rb][2]);
                mx = vmax3(mx, sc[2][rb][3], sc[3][rb][0]);
                mx = vmax3(mx, sc[3][rb][1], sc[3][rb][2]);
                mx = vmax2(mx, sc[3][rb][3]);
                const float m_prev = m_use[rb];
                mx = quad_group_max(mx);
                if constexpr (PRE) mx += m_prev;   // scores are relative to the reference they were accumulated under
                else mx *= c_log2;
                const float m_new = fmaxf(m_run[rb], mx);
                m_use[rb] = (m_new == -INFINITY) ? m_prev : m_new;
                m_sub[rb] = m_use[rb] + kBias;
                float a = __builtin_amdgcn_exp2f(fminf(m_prev - m_use[rb], 126.f));
                asm volatile("s_nop 1" : "+v"(a));  // v_exp_f32 -> inline-asm consumer: hipcc does not insert the wait state
                // SPEC, first pass: between two check points a sum may grow to 2^120 under a reference that lags, and a new reference
                // 126 or more above the old one makes `a` zero (v_exp_f32 flushes): the rescale would wipe a sum that is NOT negligible
                // beside the new tile's probabilities, the sums would look valid after the loop, and the row would lose keys.  (With the test
                // on every tile a sum stays below 2^7 per tile, and what a zero `a` drops is below 2^-100 of the row.)  A sum of 2^64 and more
                // under a reference that rises by more than 120 is rescaled by infinity instead: the validation then sees the row and the
                // q-tile is replayed.  Below 2^64 the dropped part is under 2^-52 of the new tile's largest probability (2^-10).
                // (No pass with the test on every tile holds such a sum, so the replay needs no exemption.)
                if constexpr (kSpec) a = (m_prev - m_use[rb] < -120.f && !(fabsf(acc_l[rb][0]) < 0x1p64f)) ? INFINITY : a;
                alpha[rb] = a;
                m_run[rb] = m_new;
                all_finite = all_finite && (m_new != -INFINITY);
                l_run[rb] *= a;
                if constexpr (MSUM) {
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        float x = acc_l[rb][r];
                        asm volatile("v_mul_f32 %0, %1, %0" : "+v"(x) : "v"(a));
                        acc_l[rb][r] = x;
                    }
                }
                if constexpr (PRE) {
                    pre_shift[rb] = m_prev - m_use[rb];
                    // what the next S^T accumulators start from.  Rewritten IN PLACE (tied asm operands): as plain assignments hipcc keeps
                    // the old and the new value in two tuples and copies one into the other on the FAST path of every tile
                    const float nm = -m_use[rb];
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        float c = neg_ref[rb][r];
                        asm volatile("v_mov_b32 %0, %1" : "+v"(c) : "v"(nm));
                        neg_ref[rb][r] = c;
                    }
                }
            }
            psum_thr = __all(all_finite) ? 2048.f : -1.f;
            force_exact = !__all(all_finite);
            if constexpr (kSpec) spec_mode = force_exact ? -1 : check_mask;
#pragma unroll
            for (int db = 0; db < NDB; ++db)
#pragma unroll
                for (int rb = 0; rb < 2; ++rb)
#pragma unroll
                    for (int r = 0; r < 4; ++r) {   // in place (tied operands): plain assignments make hipcc keep two register sets for O
                        float x = acc_o[db][rb][r];
                        asm volatile("v_mul_f32 %0, %1, %0" : "+v"(x) : "v"(alpha[rb]));
                        acc_o[db][rb][r] = x;
                    }
            psum[0] = 0.f, psum[1] = 0.f;
#pragma unroll
            for (int kc = 0; kc < 2; ++kc) {
                probs_impl(kc, std::true_type{});
                asm volatile("" : "+v"(pf[kc][0]), "+v"(pf[kc][1]), "+v"(psum[0]), "+v"(psum[1]));
            }
        }
        if (more) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(2 * NP) : "memory");
        else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    };
    // Matrix phase: O^T += V(t)^T P(t)^T (16 fragments, 32 MFMAs), then S(t+1)^T = K(t+1) Q^T (16 fragments, 32 MFMAs).  One step =
    // { LDS read of the fragment kPF steps ahead; the fragment's two MFMAs (row blocks 0 and 1) }, fenced with sched_barrier.
    constexpr int NPV = 2 * NDB;
    constexpr int kMsumAt = 0;         // the d block after whose MFMAs the chunk's two row-sum MFMAs are issued
    i16x8 ring[kPF + 1];
    i16x8 carry[kCarry];
    auto carry_load = [&](int t, int i) { carry[i] = vfrag(smem + (t % NS) * kStage, i / NDB, i % NDB); };
    auto matrix_phase = [&](int t, auto has_next_c) {
        constexpr bool has_next = decltype(has_next_c)::value;
        constexpr int NALL = has_next ? NPV + 4 * KS : NPV;
        const char* stv = smem + (t % NS) * kStage;
        const char* stk = smem + ((t + 1) % NS) * kStage;
        const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
        auto fetch = [&](int i) {  // operand fragment of step i
            if (i >= NALL) return;
            if (i < NPV) {
                ring[i % (kPF + 1)] = vfrag(stv, i / NDB, i % NDB);
            } else {
                const int j = i - NPV;
                ring[i % (kPF + 1)] = kfrag(stk, j & 3, j >> 2);
            }
        };
#pragma unroll
        for (int i = kCarry; i < kPF; ++i) fetch(i);
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int i = 0; i < NALL; ++i) {
            fetch(i + kPF);
            if constexpr (has_next) {   // the last kPF steps have no operand of this phase left to fetch: the next tile's first V fragments
                if (i + kPF >= NALL && i + kPF - NALL < kCarry) carry_load(t + 1, i + kPF - NALL);
            }
            if (i < NPV) {
                const int kc = i / NDB, db = i % NDB;
                const V8 a = __builtin_bit_cast(V8, i < kCarry ? carry[i < kCarry ? i : 0] : ring[i % (kPF + 1)]);
                acc_o[db][0] = M::mfma(a, pf[kc][0], acc_o[db][0]);
                acc_o[db][1] = M::mfma(a, pf[kc][1], acc_o[db][1]);
                if constexpr (MSUM) {
                    if (db == kMsumAt) {
                        acc_l[0] = M::mfma(ones8, pf[kc][0], acc_l[0]);
                        acc_l[1] = M::mfma(ones8, pf[kc][1], acc_l[1]);
                    }
                } else {
                    if (i == NPV - 1) l_run[0] += psum[0], l_run[1] += psum[1];
                }
            } else {
                const int j = i - NPV, ks = j >> 2, b = j & 3;
                const V8 a = __builtin_bit_cast(V8, ring[i % (kPF + 1)]);
                // (PRE, first step: D = A B + neg_ref with neg_ref left where it is.  Its result is read by the next step's MFMA of the same
                //  key block only, as C, same tuple; neg_ref is written on the exact path of a vector phase, a barrier away.)
                if constexpr (PRE) {
                    sc[b][0] = ks == 0 ? M::mfma_keep_c(a, qf[0][ks], neg_ref[0]) : M::mfma(a, qf[0][ks], sc[b][0]);
                    sc[b][1] = ks == 0 ? M::mfma_keep_c(a, qf[1][ks], neg_ref[1]) : M::mfma(a, qf[1][ks], sc[b][1]);
                } else {
                    sc[b][0] = M::mfma(a, qf[0][ks], ks == 0 ? zero : sc[b][0]);
                    sc[b][1] = M::mfma(a, qf[1][ks], ks == 0 ? zero : sc[b][1]);
                }
            }
            __builtin_amdgcn_sched_barrier(0);
        }
        if constexpr (has_next) {
#pragma unroll
            for (int b = 0; b < 4; ++b) asm volatile("" : "+v"(sc[b][0]), "+v"(sc[b][1]));
        }
    };

    // SPEC, first pass: the vote of this wave (`bad`: a lane holds an overflowed sum or accumulator), the barrier, the verdict
    auto spec_replay = [&](bool bad) -> bool {
        if (__any(bad) && lane == 0) *spec_word = 1;
        pp_barrier();
        if (__builtin_amdgcn_readfirstlane(*spec_word) == 0) return false;
        if (replay_ctr && tid == 0) atomicAdd(replay_ctr, 1u);
        return true;
    };

    if (idle) {
        for (int t = 0; t < nT; ++t) {
            if (!kOneBar || lagging) pp_barrier();
            stage_resolve_next(t, kGuarded);
            stage_request(t);
            if (!kOneBar || !lagging) pp_barrier();
        }
        pp_barrier();
        if (!kOneBar && !lagging) pp_barrier();
        if constexpr (kSpec) {
            if (check_mask != 0 && spec_replay(false)) return true;
        }
        P::notify(prm, ctx);
        return false;
    }

    // ---- M(0): only S(0) ----
    if (nT > 0) {
        const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int ks = 0; ks < KS; ++ks)
#pragma unroll
            for (int b = 0; b < 4; ++b) {
                const V8 a = __builtin_bit_cast(V8, kfrag(smem, b, ks));
                sc[b][0] = M::mfma(a, qf[0][ks], ks == 0 ? zero : sc[b][0]);   // (reference 0 so far, also for PRE)
                sc[b][1] = M::mfma(a, qf[1][ks], ks == 0 ? zero : sc[b][1]);
            }
#pragma unroll
        for (int b = 0; b < 4; ++b) asm volatile("" : "+v"(sc[b][0]), "+v"(sc[b][1]));
#pragma unroll
        for (int i = 0; i < kCarry; ++i) carry_load(0, i);
    }
    // (kOneBar: which of the two barriers of a tile a wave keeps is a run-time property of the wave — the skip is a branch inside the asm
    //  block of pp_barrier_if, one copy of the loop.  Leading waves: [N(t), barrier, M(t)]; lagging waves: [barrier, N(t), M(t)].)
    const int bar_n = lagging ? 1 : 0, bar_m = lagging ? 0 : 1;
    const int lag_s = __builtin_amdgcn_readfirstlane(bar_n);   // row-cursor policies: `lagging` as ONE scalar for both barriers (pp_barrier_sel)
    auto tile = [&](int t, auto has_next_c, auto guard_c) {
        tick(std::integral_constant<int, 0>{});
        if constexpr (kOneBar && kCursor) pp_barrier_sel<true>(lag_s);
        else if constexpr (kOneBar) pp_barrier_if(bar_n);
        else pp_barrier();
        tick(std::integral_constant<int, 1>{});
        vector_phase(t, guard_c);
        tick(std::integral_constant<int, 2>{});
        if constexpr (kOneBar && kCursor) pp_barrier_sel<false>(lag_s);
        else if constexpr (kOneBar) pp_barrier_if(bar_m);
        else pp_barrier();
        tick(std::integral_constant<int, 3>{});
        __builtin_amdgcn_s_setprio(1);   // the matrix phase wins the issue arbitration against the partner's vector phase
        matrix_phase(t, has_next_c);
        __builtin_amdgcn_s_setprio(0);
    };
    // steady state: every tile a phase of tile t touches (t + dist + 1 at most) exists; then the guarded tail; then the peeled last tile
    int t = 0;
    for (const int n_main = nT - dist - 1; t < n_main; ++t) tile(t, std::true_type{}, std::false_type{});
    for (; t + 1 < nT; ++t) tile(t, std::true_type{}, kGuarded);
    if (nT > 0) tile(nT - 1, std::false_type{}, kGuarded);
    // the leading waves wait until the lagging waves have read V of the last tile: the epilogue reuses the stages
    pp_barrier();
    if (!kOneBar && !lagging) pp_barrier();
    if constexpr (TRACE) {
        if (blockIdx.x == kPpTraceBlock && lane == 0) {
#pragma unroll
            for (int j = 0; j < 4; ++j) g_pp_trace[wave * 8 + j] = tr_acc[j];
            if (wave == 0) g_pp_trace[64] = (unsigned long long)nT, g_pp_trace[65] = tr_last - tr_first;
        }
        wg_t2 = __builtin_amdgcn_s_memtime();
    }
    if constexpr (kSpec) {
        if (check_mask != 0) {
            bool bad = !(fabsf(acc_l[0][0]) < 0x1p120f) || !(fabsf(acc_l[1][0]) < 0x1p120f);   // (also true of a NaN)
#pragma unroll
            for (int db = 0; db < NDB; ++db)
#pragma unroll
                for (int rb = 0; rb < 2; ++rb)
#pragma unroll
                    for (int r = 0; r < 4; ++r) bad = bad || !(fabsf(acc_o[db][rb][r]) < 0x1p120f);
            if (spec_replay(bad)) return true;
        }
    }

    // ---------------- epilogue: O^T -> LDS -> whole rows ----------------
    constexpr int kEpiStride = D * 2 + 8;
    char* erow = smem + (size_t)(wave * 32) * kEpiStride;
#pragma unroll
    for (int rb = 0; rb < 2; ++rb) {
        const float l_tot = MSUM ? acc_l[rb][0] : quad_group_sum(l_run[rb]);
        const float inv = l_tot > 0.f ? 1.f / l_tot : 0.f;
        if constexpr (HasRowLse<P>::value) {   // every lane of a row's quad group holds m_use and l_tot: the one with g4 == 0 stores
            const int qp = P::q_phys(prm, ctx, wave * 32 + rb * 16 + n16);
            if (g4 == 0 && qp >= 0)
                P::lse_base(prm, ctx)[qp] = l_tot > 0.f ? 0.6931471805599453f * (m_use[rb] + kBias + __builtin_amdgcn_logf(l_tot)) : -INFINITY;
        }
        if constexpr (HasRowO32<P>::value) {   // fp32 rows: the lane stores its four floats of every 16-column block itself
            const int qp = P::q_phys(prm, ctx, wave * 32 + rb * 16 + n16);
            if (qp >= 0) {
                float* const dst = P::o32_base(prm, ctx) + (size_t)qp * D + 4 * g4;
#pragma unroll
                for (int db = 0; db < NDB; ++db) {
                    *(f32x4*)(dst + 16 * db) = o32_values<T, E>(acc_o[db][rb], inv);
                }
            }
            continue;
        }
#pragma unroll
        for (int db = 0; db < NDB; ++db) {
            typename E::v4 o4;
#pragma unroll
            for (int j = 0; j < 4; ++j) o4[j] = E::from_float(acc_o[db][rb][j] * inv);
            *(typename E::v4*)(erow + (rb * 16 + n16) * kEpiStride + (16 * db + 4 * g4) * 2) = o4;
        }
    }
    if constexpr (HasRowO32<P>::value) {   // (no 16-bit row store; the trace stamps below are not built for these policies)
        P::notify(prm, ctx);
        return false;
    }
    __builtin_amdgcn_s_waitcnt(0xc07f);
    __builtin_amdgcn_wave_barrier();
    T* __restrict__ ob = P::o_base(prm, ctx);
    const int o_rs = P::o_rs(prm);
    constexpr int kLanesPerRow = D * 2 / 8;
    constexpr int kRowsPerPass = 64 / kLanesPerRow;
    const int sub = lane / kLanesPerRow;
    const int colb = (lane - sub * kLanesPerRow) * 8;
    int ephys[32 / kRowsPerPass];
#pragma unroll
    for (int i = 0; i < 32 / kRowsPerPass; ++i) ephys[i] = P::q_phys(prm, ctx, wave * 32 + i * kRowsPerPass + sub);
#pragma unroll
    for (int i = 0; i < 32 / kRowsPerPass; ++i) {
        const int rr = i * kRowsPerPass + sub;
        u32x2 val = *(const u32x2*)(erow + rr * kEpiStride + colb);
        if (ephys[i] >= 0) {
            u32x2* const dst = (u32x2*)((char*)(ob + (size_t)ephys[i] * o_rs) + colb);
            // (which lane stores which 8 bytes of o depends on wave, lane and the q-tile only — never on the keys: a lane that adds
            //  here reads back what IT stored in an earlier pass over the same q-tile, program order, no fence; see cross_attn_pair_kernel)
            if constexpr (HasAddOnStore<P>::value) {
                if (P::add_on_store(prm)) val = add_rounded16<T>(*dst, val);
            }
            *dst = val;
        }
    }
    P::notify(prm, ctx);
    if constexpr (TRACE) {   // the four stamps and the hardware ids of attn_body_pp2's timeline, one record per workgroup (wave 0)
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        if (wave == 0 && lane == 0 && blockIdx.x < (unsigned)kWgTraceMax) {
            unsigned long long* w = g_wg_trace + (size_t)blockIdx.x * 6;
            w[0] = wg_t0, w[1] = tr_first, w[2] = wg_t2, w[3] = __builtin_amdgcn_s_memtime();
            w[4] = __builtin_amdgcn_s_getreg((31 << 11) | 4);    // HW_REG_HW_ID
            w[5] = __builtin_amdgcn_s_getreg((31 << 11) | 20);   // HW_REG_XCC_ID
        }
    }
    return false;
}

// the workgroup's one q-tile is the one its dispatch id maps to (P::init); SPEC: and once more if its validation failed
template <typename T, typename P, bool TRACE = false, int ONEBAR = -1, bool PRE = false, bool SPEC = false>
__device__ __forceinline__ void attn_body_m16(const typename P::Params& prm, char* smem, char* policy_lds, unsigned* replay_ctr = nullptr) {
    typename P::Ctx ctx;
    if (!P::init(prm, ctx, policy_lds)) return;
    if constexpr (SPEC && std::is_same_v<T, __bf16> && !PRE) {   // (where attn_m16_tile honours it)
        if (threadIdx.x == 0) *(volatile int*)(smem + attn_m16_lds_bytes() + 8) = 0;   // (ordered by the first barrier of the q-tile)
#pragma nounroll
        for (int check_mask = kCheckEvery - 1;; check_mask = 0)
            if (!attn_m16_tile<T, P, TRACE, ONEBAR, PRE, SPEC>(prm, ctx, smem, check_mask, replay_ctr)) break;
    } else {
        attn_m16_tile<T, P, TRACE, ONEBAR, PRE>(prm, ctx, smem);
    }
}

}  // namespace svg

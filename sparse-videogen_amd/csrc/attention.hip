// SVG1 band (block-sparse) and dense attention for gfx950: the kernels that run the bodies of attn_core.h / attn_m16.h on the band
// policy (band_policy.h), the counter pool of the queue launches, the svg_band_attention* entries, the completion-counter waiters and
// the svg_debug_* trace readers; svg_band_attention_lse (row log-sum-exp output) and svg_band_attention_lse_f32 (fp32 rows) and their
// device-switch and groups forms (include/svg_attn_band_lse_forms.h); their window forms svg_band_window_attention_lse[_f32]
// (include/svg_attn_band_window.h) and their frame-shard forms svg_band_shard_attention_lse[_f32] (include/svg_attn_band_shard.h).
// (One-wave-per-SIMD body: attention_w4.hip; fp8:
// attention_f8.hip; SVG2: attention_varblock.hip.)
#include <algorithm>
#include <atomic>
#include <mutex>

#include "attn_core.h"
#include "attn_m16.h"
#include "band_policy.h"

namespace svg {

// lock-step schedule, NW waves x 32 rows (attn_body): every wave runs QK^T -> softmax -> PV per tile.  The reference schedule of
// the test-suite (variant 1, 4 waves: two workgroups per CU) and the body of the 128-row variable-block kernel and the profiler.
template <typename T, int D, int NW>
__global__ __launch_bounds__(NW * 64, 2) void band_attn_kernel(typename BandPolicy<T, D, NW>::Params prm) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    attn_body<T, D, NW, BandPolicy<T, D, NW>>(prm, smem, nullptr);
}

// two-phase ping-pong schedule, 8 waves x 32 rows (attn_body_pp2): variant 2
// head_dim 64: FOUR waves per SIMD — 128 registers (the LEAN form of the body) and 64 KiB of LDS per workgroup put two workgroups on a
// CU.  At head_dim 64 a tile is 512 cycles of matrix work beside the same 141 vector instructions per wave as at head_dim 128, and one
// wave gets a third of what the vector pipe can take (tools/probe_exp.hip): with two waves per SIMD the matrix pipe is 40 % busy, with
// four 49 % — 18 % fewer cycles per launch; the chip then meets its power limit at head_dim 64 too and gives back part of it: −10.7 % in
// time on CogVideoX-v1.5, bit-identical output (profiles/r04zr_ab_d64_four_waves.txt, r04zs_*).
template <typename T, int D>
__global__ __launch_bounds__(512, (D == 64 ? 4 : 2)) void band_attn_pp2_kernel(typename BandPolicy<T, D, 8>::Params prm) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    attn_body_pp2<T, D, BandPolicy<T, D, 8>, false, 0, false, D == 64>(prm, smem, nullptr);
}
// svg_band_attention_switch at head_dim 64: band_attn_pp2_kernel<T, 64> — four waves per SIMD, the LEAN form of the body — with the
// device-side choice between two parameter blocks in front of it (`flag[0] != 0` selects prm_alt, the dense warm-up mask without the
// layout transformation — the dense / sparse decision of attention_core_logic, hyvideo/attention.py:491-496, without reading the timestep
// back to the host; a one-wave-per-SIMD switch kernel served this head size until the end of round 4)
template <typename T>
__global__ __launch_bounds__(512, 4) void band_attn_pp2_switch64_kernel(typename BandPolicy<T, 64, 8>::Params prm,
                                                                        typename BandPolicy<T, 64, 8>::Params prm_alt,
                                                                        const int32_t* __restrict__ flag) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    if (flag[0] != 0) attn_body_pp2<T, 64, BandPolicy<T, 64, 8>, false, 0, false, true>(prm_alt, smem, nullptr);
    else attn_body_pp2<T, 64, BandPolicy<T, 64, 8>, false, 0, false, true>(prm, smem, nullptr);
}
// Device-side switch between two masks on the pre-scaled two-phase body (svg_band_attention_switch_prescaled): `flag[0] != 0`
// selects prm_alt — the dense warm-up mask without the layout transformation — otherwise prm (see band_attn_pp2_switch64_kernel)
template <typename T, int D>
__global__ __launch_bounds__(512, 2) void band_attn_pp2q_switch_kernel(typename BandPolicy<T, D, 8>::Params prm,
                                                                       typename BandPolicy<T, D, 8>::Params prm_alt,
                                                                       const int32_t* __restrict__ flag) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    if (flag[0] != 0) attn_body_pp2<T, D, BandPolicy<T, D, 8>, false, 0, true>(prm_alt, smem, nullptr);
    else attn_body_pp2<T, D, BandPolicy<T, D, 8>, false, 0, true>(prm, smem, nullptr);
}

// Frozen reference schedule (variant 6; bf16 / D = 128 only): the two-phase body as it stood at the end of round 1 — running row
// maximum with a deferred rescale, one probability step in the shadow of the PV MFMAs, operands fetched at the start of the matrix
// phase.  Kept so that ONE bench run can time it beside the default on the same box (bench.py `same_box_ab`): box-to-box clock
// spread (+-4 %) is as large as a typical schedule gain.
__global__ __launch_bounds__(512, 2) void band_attn_pp2_frozen_kernel(typename BandPolicy<__bf16, 128, 8>::Params prm) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    attn_body_pp2<__bf16, 128, BandPolicy<__bf16, 128, 8>, false, 8>(prm, smem, nullptr);
}
// the two-phase schedule on v_mfma_f32_16x16x32 (attn_m16.h): head_dim 128; variant 8
// (issue priority in the matrix phase, ONE barrier per tile: 32.55 ms against 33.1 with two — profiles/r04g_ab_m16_cfg.txt; the 32x32x16
//  body gained nothing from the single barrier because the clock took it back, this one runs ~300 MHz further from the power limit)
// The plain bf16 forms of this kernel, of the queue kernel and of the device-switched kernel run the overflow test of the max-free
// softmax on every eighth tile and validate the q-tile after its loop (SPEC, attn_m16.h); fp16 and the pre-scaled forms do not.
static __device__ unsigned g_band_replays;   // q-tiles that failed the validation and were replayed (svg_debug_band_replays)
constexpr int kTailLds = 16;                 // bytes behind the stages: the queue's slot (two words), the word of the validation, the block of a per-head queue item
// One template for every form on the static mapping; the policy is the only thing that differs between the instantiations, and each
// instantiation's listing is compared with the one it had as a kernel of its own (tools/asm_diff.py --pair, profiles/kernel_templates_asm_diff.txt).
//   BandPolicy<T, 128, 8>                          svg_band_attention: the plain kernel
//   BandLsePolicy / BandF32Policy                  svg_band_attention_lse[_f32]: the epilogue of attn_m16_tile also stores one fp32 per query
//                                                  row; the fp32 policy stores the rows as fp32, before their rounding, and no 16-bit o
//   BandWindowLsePolicy / BandWindowF32Policy      svg_band_window_attention_lse[_f32]: a row window of q / o / lse and a key window of k / v
//                                                  under the mask at its global coordinates, over the q-tiles of the row window
//   BandShardLsePolicy / BandShardF32Policy        svg_band_shard_attention_lse[_f32]: a frame shard of the rows over a frame shard of the keys,
//                                                  heads in logical order and token-major heads in one launch, the mask at the coordinates the
//                                                  shard maps give, over the q-tiles of the q shard
// The same template arguments of the body for all of them, SPEC and the replay counter included, so o keeps the bits of the plain entry — also
// where a window or two shards are the whole sequence.  A q-tile that fails its validation returns before the epilogue and stores nothing
// (neither o nor lse nor o32); its replay stores them all.
template <typename T, typename Pol>
__global__ __launch_bounds__(512, 2) void band_attn_m16_kernel(typename Pol::Params prm) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    attn_body_m16<T, Pol, false, 1, false, true>(prm, smem, nullptr, &g_band_replays);
}
// pre-scaled q on the 16x16x32 body (PRE form of attn_body_m16)
template <typename T>
__global__ __launch_bounds__(512, 2) void band_attn_m16q_kernel(typename BandPolicy<T, 128, 8>::Params prm) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    attn_body_m16<T, BandPolicy<T, 128, 8>, false, 1, true>(prm, smem, nullptr);
}
// The same two kernels as resident workgroups on a work queue (BandQueue, band_policy.h): min(work items, CUs) workgroups, each
// running one q-tile after another until the queue is dry.  What band_run launches for head_dim 128 when there are more q-tiles
// than compute units, unless the call counts completions (those rely on the head-major order of the static mapping) or no counter
// block is to be had; the device-switched kernel below keeps the static mapping.  Per row the same keys in the same order with the same arithmetic: bit-identical output.
// One template, and so one copy of the loop: the policy (BandPolicy<T, 128, 8>, plain and PRE; BandLsePolicy where svg_band_attention_lse takes
// the queue) is the only thing that differs between the instantiations, and each one's listing is checked as for band_attn_m16_kernel.  The
// policy is an argument of the kernel and the loop is NOT a function the kernels share: with the loop factored out the listings came out
// different.  The fp32 policy has no queue form: its instantiation reserved 36 bytes of scratch per lane, so svg_band_attention_lse_f32 keeps
// the static mapping.
template <typename T, typename Pol, bool PRE = false>
__global__ __launch_bounds__(512, 2) void band_attn_m16_queue_kernel(typename Pol::Params prm, BandQueue qd) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    int* const slot = (int*)(smem + attn_m16_lds_bytes());   // (head, q-tile) of the next work item, from lane 0 to the workgroup
    // SPEC of attn_m16_tile (plain bf16): a q-tile whose validation failed leaves slot[2] = 1 and stores nothing.  Lane 0 then takes no
    // new work item and marks the slot 2 — the same (head, q-tile) once more, with the overflow test on every tile — and after that
    // pass 0 again.  (Waves that still read the verdict of the first pass see 1 or 2, non-zero either way; no wave reads slot[2] between
    // the barrier below and the end of a second pass.)
    constexpr bool kSpec = !PRE && std::is_same_v<T, __bf16>;
    int dry = 0;
    if constexpr (kSpec) {
        if (threadIdx.x == 0) slot[2] = 0;
    }
    for (;;) {
        if (threadIdx.x == 0) {
            bool fresh = true;
            if constexpr (kSpec) {
                fresh = __builtin_amdgcn_readfirstlane(slot[2]) != 1;   // (a scalar: one lane is active here)
                slot[2] = fresh ? 0 : 2;
            }
            if (fresh) {
                const int xcd = __builtin_amdgcn_s_getreg((31 << 11) | 20) & (kNumXCD - 1);   // HW_REG_XCC_ID
                int head = -1, qt = 0;
                const int w = qd.take(xcd, dry);
                if (w >= 0) qd.decode(w, head, qt);
                slot[0] = head, slot[1] = qt;
            }
        }
        // Every wave is through the LDS reads of its last epilogue before any wave requests K / V of the next q-tile; and the slot
        // is not rewritten before every wave has read it: lane 0 comes back here through the barriers of a q-tile (two at least).
        __syncthreads();
        const int head = __builtin_amdgcn_readfirstlane(slot[0]), qt = __builtin_amdgcn_readfirstlane(slot[1]);
        if (head < 0) break;
        typename Pol::Ctx ctx;
        Pol::init_tile(prm, ctx, head, qt);
        if constexpr (kSpec) {
            const int check_mask = __builtin_amdgcn_readfirstlane(slot[2]) == 2 ? 0 : kCheckEvery - 1;
            attn_m16_tile<T, Pol, false, 1, PRE, true>(prm, ctx, smem, check_mask, &g_band_replays);
        } else {
            attn_m16_tile<T, Pol, false, 1, PRE>(prm, ctx, smem);
        }
    }
    if (threadIdx.x == 0) qd.leave(gridDim.x);
}
// Device-side switch between two masks on the 16x16x32 body: `flag[0] != 0` selects prm_alt.  Static mapping over the q-tiles of the
// larger block; SPEC and the replay counter as in band_attn_m16_kernel (not in the PRE form), so either flag value keeps the bits of the
// single-mask kernel.  One template; the policy is the only thing that differs between the instantiations, and each one's listing is
// checked as for band_attn_m16_kernel:
//   BandPolicy<T, 128, 8>, plain and PRE           svg_band_attention_switch[_prescaled] at head_dim 128
//   BandLsePolicy / BandF32Policy                  svg_band_attention_switch_lse[_f32]: lse (and o32) are indexed by the physical q row under the
//                                                  parameter block the flag selects — prm_alt carries no head permutation, so its rows are the logical ones
//   BandShardLsePolicy / BandShardF32Policy        svg_band_shard_attention_switch_lse[_f32] (include/svg_attn_band_shard_switch.h): the alternate
//                                                  mask on the same two shards, every head in logical order (no head flags); o / lse (o32) at
//                                                  the shard row q was read from under either block
template <typename T, typename Pol, bool PRE = false>
__global__ __launch_bounds__(512, 2) void band_attn_m16_switch_kernel(typename Pol::Params prm, typename Pol::Params prm_alt,
                                                                      const int32_t* __restrict__ flag) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    if (flag[0] != 0) attn_body_m16<T, Pol, false, 1, PRE, !PRE>(prm_alt, smem, nullptr, &g_band_replays);
    else attn_body_m16<T, Pol, false, 1, PRE, !PRE>(prm, smem, nullptr, &g_band_replays);
}
// One band per head (svg_band_attention_per_head_lse, include/svg_attn_adaptive_band.h): BandPerHeadLsePolicy (band_policy.h) on the static
// mapping, the template arguments of the body those of band_attn_m16_kernel.  Two parameter blocks that differ in their row
// regions alone — prm: a band that cuts the full rows out, prm_wide: one above S, which does not (band_row_regions) — and the head's band
// picks; the blocks are kernel arguments as they are (a patched copy of one lives in private memory: the selects of kv_schedule index it).
template <typename T>
__global__ __launch_bounds__(512, 2) void band_attn_m16_per_head_kernel(typename BandPerHeadLsePolicy<T>::Params prm,
                                                                        typename BandPerHeadLsePolicy<T>::Params prm_wide) {
    using Pol = BandPerHeadLsePolicy<T>;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    int head, qt;
    if (!Pol::map_block(prm, head, qt)) return;
    if (Pol::per_head_band_of(prm, head) > prm.S) attn_body_m16<T, Pol, false, 1, false, true>(prm_wide, smem, nullptr, &g_band_replays);
    else attn_body_m16<T, Pol, false, 1, false, true>(prm, smem, nullptr, &g_band_replays);
}
// ... with the device switch in front (svg_band_attention_switch_per_head_lse): `flag[0] != 0` runs prm_alt — the alternate mask as it is, no
// band vector and no head flags — on the same grid; per (head, q-tile) the body does what band_attn_m16_switch_kernel's does under that flag
template <typename T>
__global__ __launch_bounds__(512, 2) void band_attn_m16_per_head_switch_kernel(typename BandPerHeadLsePolicy<T>::Params prm,
                                                                               typename BandPerHeadLsePolicy<T>::Params prm_wide,
                                                                               typename BandPerHeadLsePolicy<T>::Params prm_alt,
                                                                               const int32_t* __restrict__ flag) {
    using Pol = BandPerHeadLsePolicy<T>;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    if (flag[0] != 0) {
        attn_body_m16<T, Pol, false, 1, false, true>(prm_alt, smem, nullptr, &g_band_replays);
        return;
    }
    int head, qt;
    if (!Pol::map_block(prm, head, qt)) return;
    if (Pol::per_head_band_of(prm, head) > prm.S) attn_body_m16<T, Pol, false, 1, false, true>(prm_wide, smem, nullptr, &g_band_replays);
    else attn_body_m16<T, Pol, false, 1, false, true>(prm, smem, nullptr, &g_band_replays);
}
// The per-head kernel as resident workgroups on the work queue (svg_band_attention_per_head_queue_lse,
// include/svg_attn_band_per_head_queue.h): the loop, the slot and the replay hand-shake of band_attn_m16_queue_kernel, restated here with the
// policy visible to it for the reason given there.  The queue is the one of prm — the hint's block, built through its BandLsePolicy base — so
// decode() yields (head, index) in prm's numbering, the pairs map_block yields under the static mapping.  A head on the wide block takes the
// index as its q-tile; an index behind its last one is no work, and lane 0 resolves that inside its take loop (one uniform load of the
// head's band, a compare, the next take), so the workgroup only ever sees real work items and the barriers are those of the plain queue
// kernel.  Lane 0 publishes which block the head runs in the slot's free word (0: prm, 1: prm_wide, 2: prm_alt).
// The blocks are kernel arguments as they are, and the q-tile's one is picked BY ADDRESS in the kernarg segment, not by branch: inside the
// loop a copy of the tile body per block keeps every block's scalars live across it — 284 (bf16) / 240 (fp16) bytes of scratch per lane
// here and 496 / 432 with the device switch —, where one body on the block at slot[3] * sizeof(Params) is the plain queue kernel's loop
// with its block read through a pointer: no scratch (profiles/adaptive_band_queue_kernel_stats.txt).  The explicit arguments of a kernel
// lie in its kernarg segment from offset 0 in their order at their natural alignment, so the leading blocks are an array there.
template <typename P>
static __device__ __forceinline__ const P& kernarg_block(int i) {
    static_assert(sizeof(P) % 8 == 0 && alignof(P) == 8, "the leading blocks of the arguments lie back to back");
#if defined(__HIP_DEVICE_COMPILE__)
    return ((const __attribute__((address_space(4))) P*)__builtin_amdgcn_kernarg_segment_ptr())[i];
#else
    const P* const none = nullptr;   // (the host pass only parses the kernels)
    return none[i];
#endif
}
template <typename T>
__global__ __launch_bounds__(512, 2) void band_attn_m16_per_head_queue_kernel(typename BandPerHeadLsePolicy<T>::Params prm,
                                                                              typename BandPerHeadLsePolicy<T>::Params prm_wide,
                                                                              BandQueue qd) {
    using Pol = BandPerHeadLsePolicy<T>;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    int* const slot = (int*)(smem + attn_m16_lds_bytes());   // (head, q-tile) of the next work item, the word of the validation, the block
    constexpr bool kSpec = std::is_same_v<T, __bf16>;
    int dry = 0;
    if constexpr (kSpec) {
        if (threadIdx.x == 0) slot[2] = 0;
    }
    for (;;) {
        if (threadIdx.x == 0) {
            bool fresh = true;
            if constexpr (kSpec) {
                fresh = __builtin_amdgcn_readfirstlane(slot[2]) != 1;   // (a scalar: one lane is active here)
                slot[2] = fresh ? 0 : 2;
            }
            if (fresh) {
                const int xcd = __builtin_amdgcn_s_getreg((31 << 11) | 20) & (kNumXCD - 1);   // HW_REG_XCC_ID
                int head = -1, qt = 0, wide = 0;
                for (;;) {
                    const int w = qd.take(xcd, dry);
                    if (w < 0) {
                        head = -1;
                        break;
                    }
                    qd.decode(w, head, qt);
                    wide = Pol::per_head_band_of(prm, head) > prm.S;
                    if (!wide || qt < prm_wide.nqt) break;   // (else: behind the wide head's last q-tile; prm_wide.nqt <= prm.nqt, checked on the host)
                }
                slot[0] = head, slot[1] = qt, slot[3] = wide;
            }
        }
        __syncthreads();   // (what this barrier orders: band_attn_m16_queue_kernel)
        const int head = __builtin_amdgcn_readfirstlane(slot[0]), qt = __builtin_amdgcn_readfirstlane(slot[1]);
        if (head < 0) break;
        const typename Pol::Params& p = kernarg_block<typename Pol::Params>(__builtin_amdgcn_readfirstlane(slot[3]));
        typename Pol::Ctx ctx;
        Pol::init_tile(p, ctx, head, qt);
        if constexpr (kSpec) {
            const int check_mask = __builtin_amdgcn_readfirstlane(slot[2]) == 2 ? 0 : kCheckEvery - 1;
            attn_m16_tile<T, Pol, false, 1, false, true>(p, ctx, smem, check_mask, &g_band_replays);
        } else {
            attn_m16_tile<T, Pol, false, 1, false>(p, ctx, smem);
        }
    }
    if (threadIdx.x == 0) qd.leave(gridDim.x);
}
// ... with the device switch in front (svg_band_attention_switch_per_head_queue_lse): `flag[0] != 0` selects the alternate mask's queue and
// block for the whole launch — no band vector, no head flags, nothing dropped.  One counter block: one descriptor is live per launch.
template <typename T>
__global__ __launch_bounds__(512, 2) void band_attn_m16_per_head_switch_queue_kernel(typename BandPerHeadLsePolicy<T>::Params prm,
                                                                                     typename BandPerHeadLsePolicy<T>::Params prm_wide,
                                                                                     typename BandPerHeadLsePolicy<T>::Params prm_alt,
                                                                                     const int32_t* __restrict__ flag, BandQueue qd,
                                                                                     BandQueue qd_alt) {
    using Pol = BandPerHeadLsePolicy<T>;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    int* const slot = (int*)(smem + attn_m16_lds_bytes());
    constexpr bool kSpec = std::is_same_v<T, __bf16>;
    int dry = 0;
    if constexpr (kSpec) {
        if (threadIdx.x == 0) slot[2] = 0;
    }
    for (;;) {
        if (threadIdx.x == 0) {
            bool fresh = true;
            if constexpr (kSpec) {
                fresh = __builtin_amdgcn_readfirstlane(slot[2]) != 1;
                slot[2] = fresh ? 0 : 2;
            }
            if (fresh) {
                const int xcd = __builtin_amdgcn_s_getreg((31 << 11) | 20) & (kNumXCD - 1);   // HW_REG_XCC_ID
                int head = -1, qt = 0, sel = 2;
                if (flag[0] != 0) {
                    const int w = qd_alt.take(xcd, dry);
                    if (w >= 0) qd_alt.decode(w, head, qt);
                } else {
                    for (;;) {
                        const int w = qd.take(xcd, dry);
                        if (w < 0) {
                            head = -1;
                            break;
                        }
                        qd.decode(w, head, qt);
                        sel = Pol::per_head_band_of(prm, head) > prm.S;
                        if (!sel || qt < prm_wide.nqt) break;
                    }
                }
                slot[0] = head, slot[1] = qt, slot[3] = sel;
            }
        }
        __syncthreads();
        const int head = __builtin_amdgcn_readfirstlane(slot[0]), qt = __builtin_amdgcn_readfirstlane(slot[1]);
        if (head < 0) break;
        const typename Pol::Params& p = kernarg_block<typename Pol::Params>(__builtin_amdgcn_readfirstlane(slot[3]));
        typename Pol::Ctx ctx;
        Pol::init_tile(p, ctx, head, qt);
        if constexpr (kSpec) {
            const int check_mask = __builtin_amdgcn_readfirstlane(slot[2]) == 2 ? 0 : kCheckEvery - 1;
            attn_m16_tile<T, Pol, false, 1, false, true>(p, ctx, smem, check_mask, &g_band_replays);
        } else {
            attn_m16_tile<T, Pol, false, 1, false>(p, ctx, smem);
        }
    }
    if (threadIdx.x == 0) qd.leave(gridDim.x);
}
// the same for q that carries sm_scale * log2(e) (svg_band_attention_prescaled): no scale-and-shift per score
template <typename T, int D>
__global__ __launch_bounds__(512, 2) void band_attn_pp2q_kernel(typename BandPolicy<T, D, 8>::Params prm) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    attn_body_pp2<T, D, BandPolicy<T, D, 8>, false, 0, true>(prm, smem, nullptr);
}
#ifdef SVG_ABLATIONS
// Diagnostics build only (python sparse-videogen_amd/build.py --ablations): the two-phase kernel with the per-phase cycle trace
// and the launch timeline, and its timing ablations (ABL > 0: results are wrong by construction).  Not in the product library.
template <typename T, int D, int ABL>
__global__ __launch_bounds__(512, 2) void band_attn_pp2_trace_kernel(typename BandPolicy<T, D, 8>::Params prm) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    attn_body_pp2<T, D, BandPolicy<T, D, 8>, true, ABL>(prm, smem, nullptr);
}
template <typename T>   // trace code 9: the 16x16x32 body (attn_m16.h) with the cycle trace — and two barriers per tile (the policy's
                        // default), where the product kernel keeps one: not quite the shipped schedule
__global__ __launch_bounds__(512, 2) void band_attn_m16_trace_kernel(typename BandPolicy<T, 128, 8>::Params prm) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    attn_body_m16<T, BandPolicy<T, 128, 8>, true>(prm, smem, nullptr);
}
template <typename T, int D>   // trace code 3: the pre-scaled-q body (svg_band_attention_prescaled) with the cycle trace
__global__ __launch_bounds__(512, 2) void band_attn_pp2q_trace_kernel(typename BandPolicy<T, D, 8>::Params prm) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    attn_body_pp2<T, D, BandPolicy<T, D, 8>, true, 0, true>(prm, smem, nullptr);
}
#endif

int (*g_trace_reader)(uint64_t*, bool, int) = read_trace_here;   // diagnostics only: the reader of the unit of the last traced launch (attn_core.h)

// Schedules of svg_band_attention (`variant`, include/svg_attn.h).
enum BandSchedule : int { kBandAuto = 0, kBandLockstep4 = 1, kBandPingPong = 2, kBandW4 = 3, kBandFrozen = 6, kBandM16 = 8 };
// default (variant 0): head_dim 128 -> the two-phase schedule on 16x16x32 MFMAs (attn_m16.h, variant 8; profiles/r04f_ab_m16.txt);
// head_dim 64 -> the two-phase 32x32x16 body in its four-waves-per-SIMD (LEAN) form (band_attn_pp2_kernel, variant 2; profiles/r04zr_*).
// Measured alternatives at head_dim 64: the one-wave-per-SIMD body (variant 3, 13.7 - 14.3 against 12.7 - 12.9 ms on CogVideoX-v1.5) and the
// 16x16x32 body at four waves per SIMD (round 5, no gain: profiles/r05b_ab_d64_m16.txt, removed).  Launches that count completions
// (svg_band_attention_notify*) take the same defaults.
static inline int band_default(int D) { return D == 128 ? kBandM16 : kBandPingPong; }

int band_waves_per_tile(int variant) {
    const int v = variant == kBandAuto ? kBandPingPong : variant;
    return v == kBandW4 ? 4 : ((v == kBandPingPong || v == kBandM16) ? 8 : -1);   // waves that report per 256-row q-tile; -1: no counters
}

}  // namespace svg

using namespace svg;

// one wave: spin until every counter has reached `target` (see BandPolicy::Params::done)
__global__ __launch_bounds__(64) void wait_counters_kernel(const int32_t* __restrict__ counters, int n, int target) {
    for (int i = threadIdx.x; i < n; i += 64) {
        while (__hip_atomic_load(counters + i, __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_AGENT) < target) __builtin_amdgcn_s_sleep(32);
    }
}

// the same with a deadline (wall_clock64: the constant 100 MHz counter): a waiter can never hang a stream — when the deadline
// passes it sets *timed_out and returns, and whatever was queued behind it runs on incomplete data, which the caller detects by
// reading the flag (bench.py: after warm-up, then falls back to chunk launches)
__global__ __launch_bounds__(64) void wait_counters_deadline_kernel(const int32_t* __restrict__ counters, int n, int target,
                                                                    long long ticks, int32_t* __restrict__ timed_out) {
    const long long t0 = wall_clock64();
    for (int i = threadIdx.x; i < n; i += 64) {
        while (__hip_atomic_load(counters + i, __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_AGENT) < target) {
            if (wall_clock64() - t0 > ticks) {
                __hip_atomic_store(timed_out, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
                return;
            }
            __builtin_amdgcn_s_sleep(32);
        }
    }
}

// ---- counter blocks of the queue launches (band_queue_block, band_policy.h) ----
namespace {
constexpr int kQueueBlocks = 64;    // streams per device that can hold a block
constexpr int kQueueDevices = 16;
struct QueuePool {
    int device = -1, n_cu = 0, n_used = 0;
    int32_t* base = nullptr;        // kQueueBlocks * kQueueWords zeroed words, never freed (the process ends with them)
    hipStream_t owner[kQueueBlocks];
};
std::mutex g_queue_mu;
QueuePool g_queue_pool[kQueueDevices];
int g_queue_pools = 0;
std::atomic<int> g_queue_cap{0};
}  // namespace

int32_t* svg::band_queue_block(hipStream_t st, int& n_cu) {
    hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
    if (hipStreamIsCapturing(st, &cap) != hipSuccess || cap != hipStreamCaptureStatusNone) {
        (void)hipGetLastError();
        return nullptr;
    }
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess) return nullptr;
    std::lock_guard<std::mutex> lock(g_queue_mu);
    QueuePool* pool = nullptr;
    for (int i = 0; i < g_queue_pools; ++i)
        if (g_queue_pool[i].device == dev) pool = &g_queue_pool[i];
    if (!pool) {
        if (g_queue_pools == kQueueDevices) return nullptr;
        int n = 0;
        void* mem = nullptr;
        const size_t bytes = (size_t)kQueueBlocks * kQueueWords * sizeof(int32_t);
        if (hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || n <= 0 ||
            hipMalloc(&mem, bytes) != hipSuccess) {
            (void)hipGetLastError();
            return nullptr;
        }
        if (hipMemset(mem, 0, bytes) != hipSuccess || hipDeviceSynchronize() != hipSuccess) {
            (void)hipGetLastError();
            (void)hipFree(mem);
            return nullptr;
        }
        pool = &g_queue_pool[g_queue_pools++];
        pool->device = dev, pool->n_cu = n, pool->base = (int32_t*)mem;
    }
    n_cu = pool->n_cu;
    for (int i = 0; i < pool->n_used; ++i)
        if (pool->owner[i] == st) return pool->base + (size_t)i * kQueueWords;
    if (pool->n_used == kQueueBlocks) return nullptr;
    pool->owner[pool->n_used] = st;
    return pool->base + (size_t)(pool->n_used++) * kQueueWords;
}

int svg::band_queue_cap() { return g_queue_cap.load(std::memory_order_relaxed); }

// The sizes a band launch can address (SVG_ERR_UNSUPPORTED beyond them), and the only place that states them.
// (S >= 2^24 ought to be refused here for every form; that changes the contract and gets a pull request of its own.)
static int band_check_size(const BandCall& c) {
    if ((int64_t)c.BH * c.S * c.D >= (1ll << 40)) return SVG_ERR_UNSUPPORTED;
    return check_rows(c.S, c.D);
}

// The queue decision of a launch of `items` work items on `st`: the counter block and the number of resident workgroups, or no block —
// the static mapping — where none is to be had or one round of workgroups covers the launch.
// (a launch of one round has nothing to balance, and a workgroup pays nine atomics to find the queue dry: 0.068 against
//  0.064 ms on the 52 q-tiles of the benchmark's tiny workload)
struct BandQueueLaunch {
    int32_t* block;
    int n_wg;
};
static BandQueueLaunch band_queue_decision(int items, hipStream_t st) {
    int n_cu = 0;
    int32_t* const block = band_queue_block(st, n_cu);
    const int cap = band_queue_cap();
    if (!block || (items <= n_cu && cap == 0)) return {nullptr, 0};
    const int n_wg = std::min(items, n_cu);
    return {block, cap > 0 ? std::min(n_wg, cap) : n_wg};
}

// the alternate call of a device switch: alt_mask, and no head permutation — a shard call keeps perm's geometry (in `pm`), without its flags
static BandCall band_alt_call(const BandCall& c, svg_perm_desc_t& pm) {
    BandCall b = c;
    b.mask = c.alt_mask, b.perm = nullptr;
    if (c.form == kBandShard) pm = *c.perm, pm.head_perm_flag = nullptr, b.perm = &pm;
    return b;
}

// One launch of the 16x16x32 body on policy Pol, for every form that takes it.  The device switch (c.use_alt) gets the blocks of both masks
// (band_alt_call) and runs over the q-tiles of the larger; a single mask goes to the work queue where the form has one and the call does
// not count completions (band_queue_decision), else to the static mapping over its q-tiles.
template <typename T, typename Pol, bool PRE = false>
static int launch_band_m16(const BandCall& c) {
    // (only what is launched is instantiated: the window forms have no device switch; the fp32, window and shard forms have no queue)
    constexpr bool kWindow = std::is_same_v<Pol, BandWindowLsePolicy<T>> || std::is_same_v<Pol, BandWindowF32Policy<T>>;
    constexpr bool kShard = std::is_same_v<Pol, BandShardLsePolicy<T>> || std::is_same_v<Pol, BandShardF32Policy<T>>;
    constexpr bool kQueue = std::is_same_v<Pol, BandPolicy<T, 128, 8>> || std::is_same_v<Pol, BandLsePolicy<T>>;
    auto params = [](const BandCall& b) {
        if constexpr (kWindow) return make_band_window_params<Pol, T>(b);
        else if constexpr (kShard) return make_band_shard_params<Pol, T>(b);
        else return make_band_params<Pol, T>(b);
    };
    const int lds = attn_m16_lds_bytes() + kTailLds;
    const hipStream_t st = c.stream;
    const typename Pol::Params p = params(c);
    if constexpr (!kWindow) {
        if (c.use_alt) {
            svg_perm_desc_t pm;
            const typename Pol::Params b = params(band_alt_call(c, pm));
            return launch_attn(band_attn_m16_switch_kernel<T, Pol, PRE>, dim3(std::max(p.nqt, b.nqt) * p.BH), 512, lds, st, p, b, c.use_alt);
        }
    }
    auto kern = [] {
        if constexpr (PRE) return band_attn_m16q_kernel<T>;
        else return band_attn_m16_kernel<T, Pol>;
    }();
    if constexpr (kQueue) {
        if (const BandQueueLaunch ql = c.done ? BandQueueLaunch{nullptr, 0} : band_queue_decision(p.nqt * p.BH, st); ql.block) {
            BandQueue qd = make_band_queue<Pol>(p);
            qd.ctr = ql.block;
            return launch_attn(band_attn_m16_queue_kernel<T, Pol, PRE>, dim3(ql.n_wg), 512, lds, st, p, qd);
        }
    }
    return launch_attn(kern, dim3(p.nqt * p.BH), 512, lds, st, p);
}

// One band per head (include/svg_attn_adaptive_band.h): the per-head kernels.  The parameter block is built for a band that cuts the full
// rows out (min(mask->band, S)) and once more for one that does not (S + 1); the kernel picks per head, and the policy reads the head's
// band where the block has the mask's.
template <typename T>
static int launch_band_per_head(const BandCall& c) {
    using Pol = BandPerHeadLsePolicy<T>;
    const int S = c.S, BH = c.BH;
    const hipStream_t st = c.stream;
    auto params = [&](const svg_band_mask_t* m, int band_of, const svg_perm_desc_t* pm, const int32_t* band_vec) {
        svg_band_mask_t mm = *m;
        mm.band = band_of;
        BandCall b = c;
        b.mask = &mm, b.perm = pm;
        typename Pol::Params p = make_band_params<Pol, T>(b);
        p.band_vec = band_vec;
        p.map_nqt = p.nqt, p.map_n_heavy = p.n_heavy, p.map_heavy_lo = p.heavy_lo;
        return p;
    };
    const typename Pol::Params p = params(c.mask, std::min(c.mask->band, S), c.perm, c.band);
    typename Pol::Params w = params(c.mask, S + 1, c.perm, c.band);
    if (w.nqt > p.nqt) return SVG_ERR_LAUNCH;   // (fewer cuts never make more q-tiles: band_row_regions)
    w.map_nqt = p.map_nqt, w.map_n_heavy = p.map_n_heavy, w.map_heavy_lo = p.map_heavy_lo;   // one mapping for both blocks
    const int lds = attn_m16_lds_bytes() + kTailLds;
    typename Pol::Params a{};
    if (c.use_alt) a = params(c.alt_mask, c.alt_mask->band, nullptr, nullptr);
    const int items = (c.use_alt ? std::max(p.nqt, a.nqt) : p.nqt) * BH;
    // queue: resident workgroups where a single-mask launch would run them (include/svg_attn_band_per_head_queue.h).  The queues are
    // built through the LSE base of the blocks: the per-head Ctx carries a band kv_schedule would read and no host sets.
    if (const BandQueueLaunch ql = c.queue ? band_queue_decision(items, st) : BandQueueLaunch{nullptr, 0}; ql.block) {
        BandQueue qd = make_band_queue<BandLsePolicy<T>>(p);
        qd.ctr = ql.block;
        if (!c.use_alt) return launch_attn(band_attn_m16_per_head_queue_kernel<T>, dim3(ql.n_wg), 512, lds, st, p, w, qd);
        BandQueue qa = make_band_queue<BandLsePolicy<T>>(a);
        qa.ctr = ql.block;
        return launch_attn(band_attn_m16_per_head_switch_queue_kernel<T>, dim3(ql.n_wg), 512, lds, st, p, w, a, c.use_alt, qd, qa);
    }
    if (!c.use_alt) return launch_attn(band_attn_m16_per_head_kernel<T>, dim3(p.nqt * BH), 512, lds, st, p, w);
    return launch_attn(band_attn_m16_per_head_switch_kernel<T>, dim3(items), 512, lds, st, p, w, a, c.use_alt);
}

// The fp32 entries: o32 travels in the place of o through the null checks and the layout checks of the 16-bit entries.  With a layout q
// stands in and the o member of the layout, which these entries do not read, takes q's strides (`abi` holds that copy, which is the
// layout to check); without one, o32 itself.
static const svg_attn_layout_t* band_f32_stand_in(BandCall& c, svg_attn_layout_t& abi) {
    c.o = c.layout ? const_cast<void*>(c.q) : c.o32;
    if (!c.layout) return nullptr;
    abi = *c.layout, abi.o = abi.q;
    return &abi;
}

static int check_band_shard(const svg_band_shard_t* s, int32_t S, const svg_perm_desc_t* perm) {
    return check_frame_shard(s, S, perm->vid0, perm->num_frame, perm->frame_size);
}
static int check_band_shard_geometry(int32_t S, const svg_perm_desc_t* perm) {
    if (S <= 0 || perm->num_frame <= 0 || perm->frame_size <= 0 || perm->vid0 < 0 ||
        (int64_t)perm->vid0 + (int64_t)perm->num_frame * perm->frame_size > S)
        return SVG_ERR_BAD_ARG;
    return SVG_OK;
}

// The argument checks of every band call, in the order the entry tables pin (tests/test_entry_validation_cpu.py and the per-header tables):
// pointers and counts, what the form adds, the masks, the sizes, the counters, the layout (into c.lay) against the call's Sq / Sk.
static int band_check_call(BandCall& c) {
    svg_attn_layout_t abi;
    const svg_attn_layout_t* const layout = c.o32 ? band_f32_stand_in(c, abi) : c.layout;
    if (c.layout) c.strided = true;
    if (!c.q || !c.k || !c.v || !c.o || !c.mask || c.BH <= 0 || c.S <= 0) return SVG_ERR_BAD_ARG;
    int rc = SVG_OK;
    if (c.form == kBandShard) {   // perm's geometry (checked whether or not it carries flags), the q shard, the k shard
        if (!c.perm || !c.q_shard || !c.k_shard) return SVG_ERR_BAD_ARG;
        rc = check_band_shard_geometry(c.S, c.perm);
        if (rc == SVG_OK) rc = check_band_shard(c.q_shard, c.S, c.perm);
        if (rc == SVG_OK) rc = check_band_shard(c.k_shard, c.S, c.perm);
    } else if (c.form == kBandWindow) {
        if (c.win_Sq <= 0 || c.win_Sk <= 0 || c.q_begin < 0 || c.k_begin < 0 || (int64_t)c.q_begin + c.win_Sq > c.S ||
            (int64_t)c.k_begin + c.win_Sk > c.S)
            return SVG_ERR_BAD_ARG;
    }
    if (rc == SVG_OK) rc = check_band_mask(c.S, c.mask, c.perm);
    // (the window form states its sizes behind its layout and its head size: band_run)
    if (rc == SVG_OK && c.form != kBandWindow) rc = band_check_size(c);
    if (rc == SVG_OK && c.alt_mask) rc = check_band_mask(c.S, c.alt_mask, nullptr);
    if (rc != SVG_OK) return rc;
    if (c.done && (int64_t)c.done_words < (int64_t)c.BH * (c.done_nseg + 1)) return SVG_ERR_WORKSPACE;   // segment counters + one hidden counter per head
    return c.strided ? layout_from_abi(layout, c.BH, c.BH, c.Sq(), c.Sk(), c.D, c.q, c.k, c.v, c.o, c.lay) : (int)SVG_OK;
}

// Every svg_band_attention* entry, after the null checks of its own arguments: validation, then the kernel of the call's form and
// `variant` for (dtype, D).
static int band_run(BandCall c) {
    int rc = band_check_call(c);
    if (rc != SVG_OK) return rc;
    const int32_t BH = c.BH;
    const hipStream_t st = c.stream;
    if (c.lse) {   // the LSE / fp32 forms: the default head_dim-128 body — single mask (queue or static mapping) or device switch
        if (c.D != 128 || c.variant != kBandAuto || c.done || c.prescaled) return SVG_ERR_UNSUPPORTED;
        if (c.form == kBandWindow) {   // key tiles stay aligned to the mask's coordinates; and the sizes, which this form states here
            if (c.k_begin % kBN != 0) return SVG_ERR_UNSUPPORTED;
            if ((rc = band_check_size(c)) != SVG_OK) return rc;
        }
        if (c.o32 && ((size_t)c.o32 & 15) != 0) return SVG_ERR_UNSUPPORTED;   // 16-byte stores
        return dispatch_td(c.dtype, c.D, [&](auto t, auto d) -> int {
            using T = decltype(t);
            if constexpr (decltype(d)::value != 128) {
                return SVG_ERR_UNSUPPORTED;
            } else {   // (the *_f32 entries: c.o is the stand-in of o32 here, the kernel gets no 16-bit o)
                switch (c.form) {
                    case kBandWindow: return c.o32 ? launch_band_m16<T, BandWindowF32Policy<T>>(c) : launch_band_m16<T, BandWindowLsePolicy<T>>(c);
                    case kBandShard: return c.o32 ? launch_band_m16<T, BandShardF32Policy<T>>(c) : launch_band_m16<T, BandShardLsePolicy<T>>(c);
                    case kBandPerHead: return launch_band_per_head<T>(c);
                    default: return c.o32 ? launch_band_m16<T, BandF32Policy<T>>(c) : launch_band_m16<T, BandLsePolicy<T>>(c);
                }
            }
        });
    }
    int variant = c.variant, trace_abl = -1;
    if ((variant & 0xFF) == 32) {   // diagnostics builds: traced one-wave-per-SIMD kernel, bits 8..11 = its timing ablation
        c.trace = true;
        c.trace_abl = (variant >> 8) & 15;
        return run_band_w4(c);
    }
    if (variant & 64) {   // diagnostics builds: bit 6 = traced two-phase kernel, bits 8..11 = its timing ablation
        trace_abl = (variant >> 8) & 15;
        variant = kBandPingPong;
        g_trace_reader = read_trace_here;
    }
    if (variant == kBandAuto) variant = band_default(c.D);
    if (c.done && band_waves_per_tile(variant) < 0) return SVG_ERR_UNSUPPORTED;
    if (c.strided && variant != kBandM16 && variant != kBandPingPong) return SVG_ERR_UNSUPPORTED;   // strided tensors: the two-phase bodies only (see svg_attn_layout_t)
    if (variant == kBandW4) return run_band_w4(c);
    if (variant != kBandLockstep4 && variant != kBandPingPong && variant != kBandFrozen && variant != kBandM16) return SVG_ERR_BAD_ARG;
    return dispatch_td(c.dtype, c.D, [&](auto t, auto d) -> int {
        using T = decltype(t);
        constexpr int DD = decltype(d)::value;
        using Pol = BandPolicy<T, DD, 8>;
        auto launch = [&](auto kern, int lds) {   // 8 waves over the q-tiles of every head
            const typename Pol::Params p = make_band_params<Pol, T>(c);
            return launch_attn(kern, dim3(p.nqt * BH), 512, lds, st, p);
        };
        // a device-switch kernel: the parameters of both masks (the alternate one without the head permutation) and the flag, over
        // the q-tiles of the larger of the two
        auto launch_switch = [&](auto kern, int lds) {
            svg_perm_desc_t pm;
            const typename Pol::Params a = make_band_params<Pol, T>(c), b = make_band_params<Pol, T>(band_alt_call(c, pm));
            return launch_attn(kern, dim3(std::max(a.nqt, b.nqt) * BH), 512, lds, st, a, b, c.use_alt);
        };
        switch (variant) {
            case kBandLockstep4: {
                using Pol4 = BandPolicy<T, DD, 4>;
                const typename Pol4::Params p = make_band_params<Pol4, T>(c);
                return launch_attn(band_attn_kernel<T, DD, 4>, dim3(p.nqt * BH), 256, attn_lds_bytes<DD, 4>(), st, p);
            }
            case kBandPingPong:
#ifdef SVG_ABLATIONS
                if constexpr (DD == 128 && std::is_same<T, __bf16>::value) {
                    switch (trace_abl) {
#define SVG_PP_TRACE(A) case A: return launch(band_attn_pp2_trace_kernel<T, DD, A>, attn_pp2_lds_bytes<DD>());
                        SVG_PP_TRACE(0) SVG_PP_TRACE(1) SVG_PP_TRACE(2) SVG_PP_TRACE(4) SVG_PP_TRACE(5) SVG_PP_TRACE(6) SVG_PP_TRACE(7) SVG_PP_TRACE(8)
#undef SVG_PP_TRACE
                        case -1: break;
                        case 3: return launch(band_attn_pp2q_trace_kernel<T, DD>, attn_pp2_lds_bytes<DD>());
                        case 9: return launch(band_attn_m16_trace_kernel<T>, attn_m16_lds_bytes());
                        default: return SVG_ERR_UNSUPPORTED;
                    }
                }
#endif
                if (trace_abl >= 0) return SVG_ERR_UNSUPPORTED;   // the trace / ablation kernels exist in -DSVG_ABLATIONS builds only
                if (c.use_alt) {
                    if (c.prescaled) return launch_switch(band_attn_pp2q_switch_kernel<T, DD>, attn_pp2_lds_bytes<DD>());
                    if constexpr (DD == 64) return launch_switch(band_attn_pp2_switch64_kernel<T>, attn_pp2_lds_bytes<64>());
                    return SVG_ERR_UNSUPPORTED;
                }
                return launch(c.prescaled ? band_attn_pp2q_kernel<T, DD> : band_attn_pp2_kernel<T, DD>, attn_pp2_lds_bytes<DD>());
            case kBandFrozen:   // bf16 / head_dim 128 only
                if constexpr (DD == 128 && std::is_same<T, __bf16>::value) {
                    if (c.done || c.prescaled) return SVG_ERR_UNSUPPORTED;
                    return launch(band_attn_pp2_frozen_kernel, attn_pp2_lds_bytes<128>());
                }
                return SVG_ERR_UNSUPPORTED;
            default:   // kBandM16: two-phase body on 16x16x32 MFMAs (attn_m16.h), head_dim 128; PRE forms for a q that carries the scale
                // (switch, work queue — the static mapping where the call counts completions or no counter block is to be had: launch_band_m16)
                if constexpr (DD == 128) {
                    return c.prescaled ? launch_band_m16<T, Pol, true>(c) : launch_band_m16<T, Pol>(c);
                }
                return SVG_ERR_UNSUPPORTED;
        }
    });
}

// a call without tensors, for the parameter blocks the host walks (launch geometry, queue order, the svg_debug_* entries)
static BandCall band_shape_call(int32_t BH, int32_t S, const svg_band_mask_t* mask, const svg_perm_desc_t* perm) {
    return BandCall{nullptr, nullptr, nullptr, nullptr, BH, S, 128, SVG_DTYPE_BF16, 1.f, mask, perm};
}

extern "C" int svg_band_attention(const void* q, const void* k, const void* v, void* o, int32_t BH, int32_t S, int32_t D,
                                  int32_t dtype, float sm_scale, const svg_band_mask_t* mask,
                                  const svg_perm_desc_t* perm, int32_t variant, void* stream) {
    return band_run(BandCall{q, k, v, o, BH, S, D, dtype, sm_scale, mask, perm, nullptr, (hipStream_t)stream, variant});
}

extern "C" int svg_band_attention_strided(const void* q, const void* k, const void* v, void* o, int32_t BH, int32_t S, int32_t D,
                                          int32_t dtype, float sm_scale, const svg_band_mask_t* mask, const svg_perm_desc_t* perm,
                                          const svg_attn_layout_t* layout, void* stream) {
    BandCall c{q, k, v, o, BH, S, D, dtype, sm_scale, mask, perm, layout, (hipStream_t)stream};
    c.strided = true;   // (a null layout is refused where the layout is checked)
    return band_run(c);
}

extern "C" int svg_band_attention_lse(const void* q, const void* k, const void* v, void* o, float* lse, int32_t BH, int32_t S, int32_t D,
                                      int32_t dtype, float sm_scale, const svg_band_mask_t* mask, const svg_perm_desc_t* perm,
                                      const svg_attn_layout_t* layout, void* stream) {
    if (!lse) return SVG_ERR_BAD_ARG;
    BandCall c{q, k, v, o, BH, S, D, dtype, sm_scale, mask, perm, layout, (hipStream_t)stream};
    c.lse = lse;
    return band_run(c);
}

extern "C" int svg_band_attention_lse_f32(const void* q, const void* k, const void* v, float* o32, float* lse, int32_t BH, int32_t S,
                                          int32_t D, int32_t dtype, float sm_scale, const svg_band_mask_t* mask,
                                          const svg_perm_desc_t* perm, const svg_attn_layout_t* layout, void* stream) {
    if (!o32 || !lse) return SVG_ERR_BAD_ARG;
    BandCall c{q, k, v, nullptr, BH, S, D, dtype, sm_scale, mask, perm, layout, (hipStream_t)stream};
    c.lse = lse, c.o32 = o32;
    return band_run(c);
}

// The window entries (include/svg_attn_band_window.h): the LSE / fp32 forms over a row window and a key window, on the static mapping.
extern "C" int svg_band_window_attention_lse(const void* q, const void* k, const void* v, void* o, float* lse, int32_t BH, int32_t S,
                                             int32_t q_begin, int32_t Sq, int32_t k_begin, int32_t Sk, int32_t D, int32_t dtype,
                                             float sm_scale, const svg_band_mask_t* mask, const svg_attn_layout_t* layout, void* stream) {
    if (!o || !lse) return SVG_ERR_BAD_ARG;
    BandCall c{q, k, v, o, BH, S, D, dtype, sm_scale, mask, nullptr, layout, (hipStream_t)stream};
    c.lse = lse, c.form = kBandWindow, c.q_begin = q_begin, c.win_Sq = Sq, c.k_begin = k_begin, c.win_Sk = Sk;
    return band_run(c);
}

extern "C" int svg_band_window_attention_lse_f32(const void* q, const void* k, const void* v, float* o32, float* lse, int32_t BH, int32_t S,
                                                 int32_t q_begin, int32_t Sq, int32_t k_begin, int32_t Sk, int32_t D, int32_t dtype,
                                                 float sm_scale, const svg_band_mask_t* mask, const svg_attn_layout_t* layout,
                                                 void* stream) {
    if (!o32 || !lse) return SVG_ERR_BAD_ARG;
    BandCall c{q, k, v, nullptr, BH, S, D, dtype, sm_scale, mask, nullptr, layout, (hipStream_t)stream};
    c.lse = lse, c.o32 = o32, c.form = kBandWindow, c.q_begin = q_begin, c.win_Sq = Sq, c.k_begin = k_begin, c.win_Sk = Sk;
    return band_run(c);
}

// The shard entries (include/svg_attn_band_shard.h) and their device switch (include/svg_attn_band_shard_switch.h): perm's geometry and the
// two shards are checked with the call (band_check_call); alt_mask and use_alt_flag join the first NULL check, alt_mask is checked against S
// where every switch entry's is.
extern "C" int svg_band_shard_attention_lse(const void* q, const void* k, const void* v, void* o, float* lse, int32_t BH, int32_t S, int32_t D,
                                            int32_t dtype, float sm_scale, const svg_band_mask_t* mask, const svg_perm_desc_t* perm,
                                            const svg_band_shard_t* q_shard, const svg_band_shard_t* k_shard,
                                            const svg_attn_layout_t* layout, void* stream) {
    if (!lse) return SVG_ERR_BAD_ARG;
    BandCall c{q, k, v, o, BH, S, D, dtype, sm_scale, mask, perm, layout, (hipStream_t)stream};
    c.lse = lse, c.form = kBandShard, c.q_shard = q_shard, c.k_shard = k_shard;
    return band_run(c);
}

extern "C" int svg_band_shard_attention_lse_f32(const void* q, const void* k, const void* v, float* o32, float* lse, int32_t BH, int32_t S,
                                                int32_t D, int32_t dtype, float sm_scale, const svg_band_mask_t* mask,
                                                const svg_perm_desc_t* perm, const svg_band_shard_t* q_shard,
                                                const svg_band_shard_t* k_shard, const svg_attn_layout_t* layout, void* stream) {
    if (!o32 || !lse) return SVG_ERR_BAD_ARG;
    BandCall c{q, k, v, nullptr, BH, S, D, dtype, sm_scale, mask, perm, layout, (hipStream_t)stream};
    c.lse = lse, c.o32 = o32, c.form = kBandShard, c.q_shard = q_shard, c.k_shard = k_shard;
    return band_run(c);
}

extern "C" int svg_band_shard_attention_switch_lse(const void* q, const void* k, const void* v, void* o, float* lse, int32_t BH, int32_t S,
                                                   int32_t D, int32_t dtype, float sm_scale, const svg_band_mask_t* mask,
                                                   const svg_perm_desc_t* perm, const svg_band_mask_t* alt_mask, const int32_t* use_alt_flag,
                                                   const svg_band_shard_t* q_shard, const svg_band_shard_t* k_shard,
                                                   const svg_attn_layout_t* layout, void* stream) {
    if (!lse || !alt_mask || !use_alt_flag) return SVG_ERR_BAD_ARG;
    BandCall c{q, k, v, o, BH, S, D, dtype, sm_scale, mask, perm, layout, (hipStream_t)stream};
    c.lse = lse, c.form = kBandShard, c.q_shard = q_shard, c.k_shard = k_shard, c.alt_mask = alt_mask, c.use_alt = use_alt_flag;
    return band_run(c);
}

extern "C" int svg_band_shard_attention_switch_lse_f32(const void* q, const void* k, const void* v, float* o32, float* lse, int32_t BH,
                                                       int32_t S, int32_t D, int32_t dtype, float sm_scale, const svg_band_mask_t* mask,
                                                       const svg_perm_desc_t* perm, const svg_band_mask_t* alt_mask,
                                                       const int32_t* use_alt_flag, const svg_band_shard_t* q_shard,
                                                       const svg_band_shard_t* k_shard, const svg_attn_layout_t* layout, void* stream) {
    if (!o32 || !lse || !alt_mask || !use_alt_flag) return SVG_ERR_BAD_ARG;
    BandCall c{q, k, v, nullptr, BH, S, D, dtype, sm_scale, mask, perm, layout, (hipStream_t)stream};
    c.lse = lse, c.o32 = o32, c.form = kBandShard, c.q_shard = q_shard, c.k_shard = k_shard, c.alt_mask = alt_mask, c.use_alt = use_alt_flag;
    return band_run(c);
}

extern "C" int32_t svg_debug_band_shard_map(const svg_perm_desc_t* perm, int32_t S, const svg_band_shard_t* shard, int32_t token_major,
                                            const int32_t* x, int32_t n, int32_t* g_out, int32_t* ginv_out) {
    if (!perm || !shard || !x || n < 0 || check_band_shard_geometry(S, perm) != SVG_OK || check_band_shard(shard, S, perm) != SVG_OK) return -1;
    const BandShardMap m = svg::make_band_shard_map(*shard, perm->vid0, perm->num_frame, perm->frame_size);
    for (int i = 0; i < n; ++i) {
        if (g_out) g_out[i] = m.g(perm->vid0, perm->num_frame, perm->frame_size, token_major != 0, x[i]);
        if (ginv_out) ginv_out[i] = m.ginv(perm->vid0, perm->num_frame, perm->frame_size, token_major != 0, x[i]);
    }
    return n;
}

// (head_dim 128: the PRE form of the 16x16x32 body — 33.0 - 33.3 ms against 33.6 - 34.2 for the 32x32x16 one, same box, profiles/r04k_ab_m16_prescaled.txt)
extern "C" int svg_band_attention_prescaled(const void* q_scaled, const void* k, const void* v, void* o, int32_t BH, int32_t S,
                                            int32_t D, int32_t dtype, const svg_band_mask_t* mask, const svg_perm_desc_t* perm,
                                            void* stream) {
    BandCall c{q_scaled, k, v, o, BH, S, D, dtype, 1.f, mask, perm, nullptr, (hipStream_t)stream};
    c.prescaled = true;
    return band_run(c);
}

extern "C" int32_t svg_band_attention_notify_target(int32_t S, const svg_band_mask_t* mask) {
    if (!mask || S <= 0) return -1;
    using Pol = svg::BandPolicy<__bf16, 128, 8>;
    const auto p = svg::make_band_params<Pol, __bf16>(band_shape_call(1, S, mask, nullptr));
    return p.nqt * band_waves_per_tile(kBandAuto);   // every wave of every q-tile of a head reports once
}

extern "C" int32_t svg_band_attention_notify_layout(int32_t S, const svg_band_mask_t* mask, int32_t nseg, int32_t* row_bounds,
                                                    int32_t* targets) {
    if (!mask || S <= 0 || nseg <= 0 || !row_bounds || !targets) return -1;
    using Pol = svg::BandPolicy<__bf16, 128, 8>;   // (q-tiles are 256 rows in every schedule that counts)
    BandCall c = band_shape_call(1, S, mask, nullptr);
    c.done_nseg = nseg;
    const auto p = svg::make_band_params<Pol, __bf16>(c);
    auto tile_row = [&](int t) {   // first row of q-tile t (row order), S behind the last tile
        if (t >= p.nqt) return S;
        int r = 0;
        for (int i = 1; i < 4; ++i)
            if (t >= p.reg_t0[i]) r = i;
        return p.reg_lo[r] + (t - p.reg_t0[r]) * Pol::BM;
    };
    for (int sgm = 0; sgm < p.done_nseg; ++sgm) {
        const int t_lo = sgm * p.done_tps, t_hi = (sgm == p.done_nseg - 1) ? p.nqt : std::min(p.nqt, (sgm + 1) * p.done_tps);
        row_bounds[sgm] = tile_row(t_lo);
        targets[sgm] = (t_hi - t_lo) * band_waves_per_tile(kBandAuto);
    }
    row_bounds[p.done_nseg] = S;
    return p.done_nseg;   // segments actually used (<= nseg)
}

extern "C" int svg_band_attention_notify(const void* q, const void* k, const void* v, void* o, int32_t BH, int32_t S, int32_t D,
                                         int32_t dtype, float sm_scale, const svg_band_mask_t* mask, const svg_perm_desc_t* perm,
                                         int32_t* done_per_head, int32_t done_words, void* stream) {
    return svg_band_attention_notify_seg(q, k, v, o, BH, S, D, dtype, sm_scale, mask, perm, done_per_head, done_words, 1, stream);
}

extern "C" int svg_band_attention_notify_seg(const void* q, const void* k, const void* v, void* o, int32_t BH, int32_t S, int32_t D,
                                             int32_t dtype, float sm_scale, const svg_band_mask_t* mask,
                                             const svg_perm_desc_t* perm, int32_t* done, int32_t done_words, int32_t nseg,
                                             void* stream) {
    if (!done || nseg <= 0) return SVG_ERR_BAD_ARG;
    BandCall c{q, k, v, o, BH, S, D, dtype, sm_scale, mask, perm, nullptr, (hipStream_t)stream};
    c.done = done, c.done_words = done_words, c.done_nseg = nseg;
    return band_run(c);
}

extern "C" int svg_band_attention_prescaled_notify_seg(const void* q_scaled, const void* k, const void* v, void* o, int32_t BH,
                                                       int32_t S, int32_t D, int32_t dtype, const svg_band_mask_t* mask,
                                                       const svg_perm_desc_t* perm, int32_t* done, int32_t done_words, int32_t nseg,
                                                       void* stream) {
    if (!done || nseg <= 0) return SVG_ERR_BAD_ARG;
    BandCall c{q_scaled, k, v, o, BH, S, D, dtype, 1.f, mask, perm, nullptr, (hipStream_t)stream};
    c.done = done, c.done_words = done_words, c.done_nseg = nseg, c.prescaled = true;
    return band_run(c);
}

extern "C" int svg_wait_counters(const int32_t* counters, int32_t n, int32_t target, void* stream) {
    if (!counters || n <= 0) return SVG_ERR_BAD_ARG;
    hipLaunchKernelGGL(wait_counters_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, counters, n, target);
    return launch_status();
}

extern "C" int svg_wait_counters_deadline(const int32_t* counters, int32_t n, int32_t target, int32_t timeout_ms,
                                          int32_t* timed_out, void* stream) {
    if (!counters || n <= 0 || timeout_ms <= 0 || !timed_out) return SVG_ERR_BAD_ARG;
    hipLaunchKernelGGL(wait_counters_deadline_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, counters, n, target,
                       (long long)timeout_ms * 100000LL, timed_out);
    return launch_status();
}

// the device switch runs on the default schedule of the head size: the 16x16x32 body at head_dim 128 (attn_m16.h), the LEAN 32x32x16
// one at 64 (band_attn_pp2_kernel<T, 64>); strided tensors as in svg_band_attention_strided
extern "C" int svg_band_attention_switch(const void* q, const void* k, const void* v, void* o, int32_t BH, int32_t S, int32_t D,
                                         int32_t dtype, float sm_scale, const svg_band_mask_t* mask, const svg_perm_desc_t* perm,
                                         const svg_band_mask_t* alt_mask, const int32_t* use_alt_flag, void* stream) {
    if (!alt_mask || !use_alt_flag) return SVG_ERR_BAD_ARG;
    BandCall c{q, k, v, o, BH, S, D, dtype, sm_scale, mask, perm, nullptr, (hipStream_t)stream};
    c.alt_mask = alt_mask, c.use_alt = use_alt_flag;
    return band_run(c);
}

extern "C" int svg_band_attention_switch_strided(const void* q, const void* k, const void* v, void* o, int32_t BH, int32_t S, int32_t D,
                                                 int32_t dtype, float sm_scale, const svg_band_mask_t* mask, const svg_perm_desc_t* perm,
                                                 const svg_band_mask_t* alt_mask, const int32_t* use_alt_flag,
                                                 const svg_attn_layout_t* layout, void* stream) {
    if (!layout || !alt_mask || !use_alt_flag) return SVG_ERR_BAD_ARG;
    BandCall c{q, k, v, o, BH, S, D, dtype, sm_scale, mask, perm, layout, (hipStream_t)stream};
    c.alt_mask = alt_mask, c.use_alt = use_alt_flag;
    return band_run(c);
}

extern "C" int svg_band_attention_switch_prescaled(const void* q_scaled, const void* k, const void* v, void* o, int32_t BH, int32_t S,
                                                   int32_t D, int32_t dtype, const svg_band_mask_t* mask, const svg_perm_desc_t* perm,
                                                   const svg_band_mask_t* alt_mask, const int32_t* use_alt_flag, void* stream) {
    if (!alt_mask || !use_alt_flag) return SVG_ERR_BAD_ARG;
    BandCall c{q_scaled, k, v, o, BH, S, D, dtype, 1.f, mask, perm, nullptr, (hipStream_t)stream};
    c.alt_mask = alt_mask, c.use_alt = use_alt_flag, c.prescaled = true;
    return band_run(c);
}

// LSE / fp32 forms of the device switch (include/svg_attn_band_lse_forms.h)
extern "C" int svg_band_attention_switch_lse(const void* q, const void* k, const void* v, void* o, float* lse, int32_t BH, int32_t S,
                                             int32_t D, int32_t dtype, float sm_scale, const svg_band_mask_t* mask,
                                             const svg_perm_desc_t* perm, const svg_band_mask_t* alt_mask, const int32_t* use_alt_flag,
                                             const svg_attn_layout_t* layout, void* stream) {
    if (!lse || !alt_mask || !use_alt_flag) return SVG_ERR_BAD_ARG;
    BandCall c{q, k, v, o, BH, S, D, dtype, sm_scale, mask, perm, layout, (hipStream_t)stream};
    c.lse = lse, c.alt_mask = alt_mask, c.use_alt = use_alt_flag;
    return band_run(c);
}

extern "C" int svg_band_attention_switch_lse_f32(const void* q, const void* k, const void* v, float* o32, float* lse, int32_t BH, int32_t S,
                                                 int32_t D, int32_t dtype, float sm_scale, const svg_band_mask_t* mask,
                                                 const svg_perm_desc_t* perm, const svg_band_mask_t* alt_mask,
                                                 const int32_t* use_alt_flag, const svg_attn_layout_t* layout, void* stream) {
    if (!o32 || !lse || !alt_mask || !use_alt_flag) return SVG_ERR_BAD_ARG;
    BandCall c{q, k, v, nullptr, BH, S, D, dtype, sm_scale, mask, perm, layout, (hipStream_t)stream};
    c.lse = lse, c.o32 = o32, c.alt_mask = alt_mask, c.use_alt = use_alt_flag;
    return band_run(c);
}

// One band per head (include/svg_attn_adaptive_band.h, include/svg_attn_band_per_head_queue.h): the checks of
// svg_band_attention[_switch]_lse in their order, then launch_band_per_head.
extern "C" int svg_band_attention_per_head_lse(const void* q, const void* k, const void* v, void* o, float* lse, int32_t BH, int32_t S,
                                               int32_t D, int32_t dtype, float sm_scale, const svg_band_mask_t* mask, const int32_t* band,
                                               const svg_perm_desc_t* perm, const svg_attn_layout_t* layout, void* stream) {
    if (!lse || !band) return SVG_ERR_BAD_ARG;
    BandCall c{q, k, v, o, BH, S, D, dtype, sm_scale, mask, perm, layout, (hipStream_t)stream};
    c.lse = lse, c.form = kBandPerHead, c.band = band;
    return band_run(c);
}

extern "C" int svg_band_attention_switch_per_head_lse(const void* q, const void* k, const void* v, void* o, float* lse, int32_t BH, int32_t S,
                                                      int32_t D, int32_t dtype, float sm_scale, const svg_band_mask_t* mask,
                                                      const svg_band_mask_t* alt_mask, const int32_t* use_alt, const int32_t* band,
                                                      const svg_perm_desc_t* perm, const svg_attn_layout_t* layout, void* stream) {
    if (!lse || !band || !alt_mask || !use_alt) return SVG_ERR_BAD_ARG;
    BandCall c{q, k, v, o, BH, S, D, dtype, sm_scale, mask, perm, layout, (hipStream_t)stream};
    c.lse = lse, c.form = kBandPerHead, c.band = band, c.alt_mask = alt_mask, c.use_alt = use_alt;
    return band_run(c);
}

extern "C" int svg_band_attention_per_head_queue_lse(const void* q, const void* k, const void* v, void* o, float* lse, int32_t BH, int32_t S,
                                                     int32_t D, int32_t dtype, float sm_scale, const svg_band_mask_t* mask,
                                                     const int32_t* band, const svg_perm_desc_t* perm, const svg_attn_layout_t* layout,
                                                     void* stream) {
    if (!lse || !band) return SVG_ERR_BAD_ARG;
    BandCall c{q, k, v, o, BH, S, D, dtype, sm_scale, mask, perm, layout, (hipStream_t)stream};
    c.lse = lse, c.form = kBandPerHead, c.band = band, c.queue = true;
    return band_run(c);
}

extern "C" int svg_band_attention_switch_per_head_queue_lse(const void* q, const void* k, const void* v, void* o, float* lse, int32_t BH,
                                                            int32_t S, int32_t D, int32_t dtype, float sm_scale, const svg_band_mask_t* mask,
                                                            const svg_band_mask_t* alt_mask, const int32_t* use_alt, const int32_t* band,
                                                            const svg_perm_desc_t* perm, const svg_attn_layout_t* layout, void* stream) {
    if (!lse || !band || !alt_mask || !use_alt) return SVG_ERR_BAD_ARG;
    BandCall c{q, k, v, o, BH, S, D, dtype, sm_scale, mask, perm, layout, (hipStream_t)stream};
    c.lse = lse, c.form = kBandPerHead, c.band = band, c.alt_mask = alt_mask, c.use_alt = use_alt, c.queue = true;
    return band_run(c);
}

// svg_band_groups_attention: the heads of one call in groups of consecutive heads, each under a mask (and an alternate mask) of its
// own — the videos of a batch whose text lengths differ.  Every group is checked before the first launches; the launches are those of
// the single-mask entry the arguments select, one pass through band_run per group.  (One launch per group and not a mask per head
// inside one launch: DESIGN §3.1.3.)
// The call of the group of `heads` heads behind `h0` heads of call `c`: tensor bases (byte offsets in 64 bits; 16-bit elements; a null o —
// the fp32 forms — stays null), lse and o32 as contiguous [BH, S] / [BH, S, D] fp32 whatever the layout, and the head-permutation flags (in `pm`).
static BandCall band_group_at(const BandCall& c, int64_t h0, int32_t heads, svg_perm_desc_t& pm) {
    auto at = [](const void* p, int64_t elements) -> const void* { return p ? (const char*)p + elements * 2 : nullptr; };
    BandCall g = c;
    g.BH = heads;
    if (c.layout) {   // whole videos: the base moves by batch strides
        const int64_t b0 = h0 / c.layout->heads_per_batch;
        g.q = at(c.q, b0 * c.layout->q.batch), g.k = at(c.k, b0 * c.layout->k.batch), g.v = at(c.v, b0 * c.layout->v.batch);
        g.o = (void*)at(c.o, b0 * c.layout->o.batch);
    } else {
        const int64_t off = h0 * (int64_t)c.S * c.D;
        g.q = at(c.q, off), g.k = at(c.k, off), g.v = at(c.v, off), g.o = (void*)at(c.o, off);
    }
    if (c.lse) g.lse = c.lse + (size_t)h0 * (size_t)c.S;
    if (c.o32) g.o32 = c.o32 + (size_t)h0 * (size_t)c.S * (size_t)c.D;
    if (c.perm) {
        pm = *c.perm, g.perm = &pm;
        if (pm.head_perm_flag) pm.head_perm_flag += h0;
    }
    return g;
}

// every groups entry, with the call of all heads in `c` (c.use_alt with alt_masks, or neither)
static int band_groups_run(BandCall c, const svg_band_mask_t* masks, const svg_band_mask_t* alt_masks, const int32_t* group_heads,
                           int32_t n_groups) {
    if (!c.q || !c.k || !c.v || !(c.o32 ? (void*)c.o32 : c.o) || !masks || !group_heads || n_groups < 1 || c.BH <= 0 || c.S <= 0)
        return SVG_ERR_BAD_ARG;
    if ((alt_masks != nullptr) != (c.use_alt != nullptr)) return SVG_ERR_BAD_ARG;
    int64_t heads = 0;
    for (int g = 0; g < n_groups; ++g) {
        if (group_heads[g] < 1) return SVG_ERR_BAD_ARG;
        if (c.layout && (c.layout->heads_per_batch <= 0 || group_heads[g] % c.layout->heads_per_batch != 0)) return SVG_ERR_BAD_ARG;
        heads += group_heads[g];
    }
    if (heads != c.BH) return SVG_ERR_BAD_ARG;
    if (c.prescaled) c.sm_scale = 1.f;
    svg_perm_desc_t pm;
    auto group = [&](int g, int64_t h0) {
        BandCall gc = band_group_at(c, h0, group_heads[g], pm);
        gc.mask = masks + g, gc.alt_mask = alt_masks ? alt_masks + g : nullptr;
        return gc;
    };
    // what the single-mask entries check, for every group, before anything is launched
    int64_t h0 = 0;
    for (int g = 0; g < n_groups; h0 += group_heads[g++]) {
        BandCall gc = group(g, h0);
        if (const int rc = band_check_call(gc); rc != SVG_OK) return rc;
    }
    if (c.prescaled && c.layout) return SVG_ERR_UNSUPPORTED;   // (no single-mask entry takes a pre-scaled q with a layout)
    if (const int rc = dispatch_td(c.dtype, c.D, [](auto, auto) { return (int)SVG_OK; }); rc != SVG_OK) return rc;
    if (c.lse && (c.D != 128 || ((size_t)c.o32 & 15) != 0)) return SVG_ERR_UNSUPPORTED;
    h0 = 0;
    for (int g = 0; g < n_groups; h0 += group_heads[g++])
        if (const int rc = band_run(group(g, h0)); rc != SVG_OK) return rc;   // (a failed launch: SVG_ERR_LAUNCH)
    return SVG_OK;
}

extern "C" int svg_band_groups_attention(const void* q, const void* k, const void* v, void* o, int32_t BH, int32_t S, int32_t D,
                                         int32_t dtype, float sm_scale, const svg_band_mask_t* masks, const svg_band_mask_t* alt_masks,
                                         const int32_t* group_heads, int32_t n_groups, const svg_perm_desc_t* perm,
                                         const int32_t* use_alt_flag, int32_t q_prescaled, const svg_attn_layout_t* layout,
                                         void* stream) {
    BandCall c{q, k, v, o, BH, S, D, dtype, sm_scale, nullptr, perm, layout, (hipStream_t)stream};
    c.use_alt = use_alt_flag, c.prescaled = q_prescaled != 0;
    return band_groups_run(c, masks, alt_masks, group_heads, n_groups);
}

extern "C" int svg_band_groups_attention_lse(const void* q, const void* k, const void* v, void* o, float* lse, int32_t BH, int32_t S,
                                             int32_t D, int32_t dtype, float sm_scale, const svg_band_mask_t* masks,
                                             const svg_band_mask_t* alt_masks, const int32_t* group_heads, int32_t n_groups,
                                             const svg_perm_desc_t* perm, const int32_t* use_alt_flag, const svg_attn_layout_t* layout,
                                             void* stream) {
    if (!lse) return SVG_ERR_BAD_ARG;
    BandCall c{q, k, v, o, BH, S, D, dtype, sm_scale, nullptr, perm, layout, (hipStream_t)stream};
    c.lse = lse, c.use_alt = use_alt_flag;
    return band_groups_run(c, masks, alt_masks, group_heads, n_groups);
}

extern "C" int svg_band_groups_attention_lse_f32(const void* q, const void* k, const void* v, float* o32, float* lse, int32_t BH, int32_t S,
                                                 int32_t D, int32_t dtype, float sm_scale, const svg_band_mask_t* masks,
                                                 const svg_band_mask_t* alt_masks, const int32_t* group_heads, int32_t n_groups,
                                                 const svg_perm_desc_t* perm, const int32_t* use_alt_flag,
                                                 const svg_attn_layout_t* layout, void* stream) {
    if (!o32 || !lse) return SVG_ERR_BAD_ARG;
    BandCall c{q, k, v, nullptr, BH, S, D, dtype, sm_scale, nullptr, perm, layout, (hipStream_t)stream};
    c.lse = lse, c.o32 = o32, c.use_alt = use_alt_flag;
    return band_groups_run(c, masks, alt_masks, group_heads, n_groups);
}

extern "C" int32_t svg_band_queue_order(int32_t BH, int32_t S, const svg_band_mask_t* mask, int32_t* out, int32_t out_words) {
    if (!mask || BH <= 0 || S <= 0 || check_band_mask(S, mask, nullptr) != SVG_OK) return -1;
    using Pol = svg::BandPolicy<__bf16, 128, 8>;
    const auto p = svg::make_band_params<Pol, __bf16>(band_shape_call(BH, S, mask, nullptr));
    const BandQueue qd = svg::make_band_queue<Pol>(p);
    if (!out) return qd.n_items;
    int n = 0;
    for (int x = 0; x <= kNumXCD; ++x)   // the eight lists, then the tail
        for (unsigned i = 0;; ++i) {
            const int w = x < kNumXCD ? qd.item(x, i) : qd.tail_item(i);
            if (w < 0) break;
            if (3 * (n + 1) > out_words) return -1;
            int head, qt;
            qd.decode(w, head, qt);
            Pol::Ctx c;
            Pol::kv_schedule(p, c, qt);
            out[3 * n] = x, out[3 * n + 1] = head * p.nqt + qt, out[3 * n + 2] = c.nT;
            ++n;
        }
    return n;
}

// the order of the per-head queue launches on the host (include/svg_attn_band_per_head_queue.h): the blocks and queues launch_band_per_head builds,
// walked list by list, with the drop lane 0 of the kernels resolves
extern "C" int32_t svg_band_per_head_queue_order(int32_t BH, int32_t S, const svg_band_mask_t* mask, const svg_band_mask_t* alt_mask,
                                                 int32_t use_alt, const int32_t* band, int32_t* out, int32_t out_words) {
    if (!mask || !band || BH <= 0 || S <= 0 || check_band_mask(S, mask, nullptr) != SVG_OK) return -1;
    if (alt_mask && check_band_mask(S, alt_mask, nullptr) != SVG_OK) return -1;
    if (use_alt && !alt_mask) return -1;
    using Pol = svg::BandLsePolicy<__bf16>;
    auto params = [&](const svg_band_mask_t* m, int band_of) {
        svg_band_mask_t mm = *m;
        mm.band = band_of;
        return svg::make_band_params<Pol, __bf16>(band_shape_call(BH, S, &mm, nullptr));
    };
    const auto p = use_alt ? params(alt_mask, alt_mask->band) : params(mask, std::min(mask->band, S));
    const auto w = params(mask, S + 1);
    if (!use_alt && w.nqt > p.nqt) return -1;
    const BandQueue qd = svg::make_band_queue<Pol>(p);
    if (!out) return qd.n_items;
    int n = 0;
    for (int x = 0; x <= kNumXCD; ++x)   // the eight lists, then the tail
        for (unsigned i = 0;; ++i) {
            const int item = x < kNumXCD ? qd.item(x, i) : qd.tail_item(i);
            if (item < 0) break;
            if (4 * (int64_t)(n + 1) > out_words) return -1;
            int head, qt;
            qd.decode(item, head, qt);
            const bool wide = !use_alt && std::min(std::max(band[head], 1), S + 1) > S;
            out[4 * n] = x, out[4 * n + 1] = head, out[4 * n + 2] = wide && qt >= w.nqt ? -1 : qt, out[4 * n + 3] = use_alt ? 2 : (wide ? 1 : 0);
            ++n;
        }
    return n;
}

extern "C" int svg_debug_band_queue_cap(int32_t max_workgroups) {
    if (max_workgroups < 0) return SVG_ERR_BAD_ARG;
    g_queue_cap.store(max_workgroups, std::memory_order_relaxed);
    return SVG_OK;
}

extern "C" int64_t svg_debug_band_replays(int32_t reset) {
    unsigned n = 0;
    if (hipDeviceSynchronize() != hipSuccess || hipMemcpyFromSymbol(&n, HIP_SYMBOL(g_band_replays), sizeof n) != hipSuccess) return -1;
    const unsigned zero = 0;
    if (reset && hipMemcpyToSymbol(HIP_SYMBOL(g_band_replays), &zero, sizeof zero) != hipSuccess) return -1;
    return (int64_t)n;
}

// the row cursor of the 16x16x32 band body walked on the host, with the parameters a launch would build (see include/svg_attn.h)
extern "C" int32_t svg_debug_band_row_cursor(int32_t S, int32_t vid0, int32_t num_frame, int32_t frame_size, int32_t token_major,
                                             const int32_t* k0, int32_t n, int32_t* out, int32_t out_words, int32_t* cheap) {
    using Pol = svg::BandPolicy<__bf16, 128, 8>;
    if (S <= 0 || n < 0 || !k0 || !out || (int64_t)out_words < (int64_t)n * kBN) return -1;
    const svg_band_mask_t mask{S, S, 0, 0, 0, 0};
    const int64_t flag = 1;   // (never read: the builder only asks whether the call names token-major heads)
    const svg_perm_desc_t perm{&flag, vid0, num_frame, frame_size};
    if (check_band_mask(S, &mask, &perm) != SVG_OK) return -1;
    const Pol::Params p = svg::make_band_params<Pol, __bf16>(band_shape_call(1, S, &mask, &perm));
    Pol::Ctx c{};
    c.perm = token_major != 0;
    for (int row = 0; row < kBN; ++row) {   // one lane's walk over the tiles, as the kernel does it
        Pol::RowWalk w;
        Pol::row_walk_init(p, c, w);
        int phys = 0;
        for (int i = 0; i < n; ++i) {
            Pol::RowWalk probe = w;
            if (cheap) cheap[i] = Pol::row_walk_cheap(probe, k0[i]) ? 1 : 0;
            Pol::row_walk_next(p, w, phys, k0[i], row);
            out[(size_t)i * kBN + row] = phys;
        }
    }
    return n;
}

// the tile run of one wave of one q-tile of the 16x16x32 band body and the walk that uses it, on the host with the parameters a launch would
// build and the functions the kernel calls (see include/svg_attn.h)
extern "C" int32_t svg_debug_band_tile_run(int32_t S, const svg_band_mask_t* mask, int32_t vid0, int32_t num_frame, int32_t frame_size,
                                           int32_t token_major, int32_t qt, int32_t wave, int32_t dist, int32_t* out4, int32_t* tiles,
                                           int32_t tiles_words, int32_t* rows, int32_t rows_words) {
    using Pol = svg::BandPolicy<__bf16, 128, 8>;
    if (S <= 0 || !mask || !out4 || wave < 0 || wave >= 8 || dist < 1 || dist > 8 || qt < 0) return -1;
    if (num_frame <= 0 && token_major) return -1;
    const int64_t flag = 1;   // (never read: the builder only asks whether the call names token-major heads)
    const svg_perm_desc_t perm{&flag, vid0, num_frame, frame_size};
    const svg_perm_desc_t* pd = num_frame > 0 ? &perm : nullptr;
    if (check_band_mask(S, mask, pd) != SVG_OK) return -1;
    const Pol::Params p = svg::make_band_params<Pol, __bf16>(band_shape_call(1, S, mask, pd));
    if (qt >= p.nqt) return -1;
    Pol::Ctx c{};
    c.perm = token_major != 0;
    Pol::kv_schedule(p, c, qt);
    Pol::wave_fast_interval(p, c, wave, c.fk_lo, c.fk_hi);
    const int nT = c.nT;
    if ((tiles && (int64_t)tiles_words < (int64_t)nT * 4) || (rows && (int64_t)rows_words < (int64_t)nT * kBN)) return -1;
    Pol::RowWalk w0;
    Pol::row_walk_init(p, c, w0);
    int run_lo = 0, run_n = 0;
    Pol::tile_run(c, w0, dist, run_lo, run_n);
    out4[0] = run_lo, out4[1] = run_n, out4[2] = nT, out4[3] = p.nqt;
    if (tiles) {   // per tile, with the generic functions: first key, FULL by the fast-path interval, follows its predecessor, N(t)'s tile steps
        for (int t = 0; t < nT; ++t) {
            const int k0 = Pol::tile_key0(c, t);
            tiles[4 * t] = k0;
            tiles[4 * t + 1] = Pol::fast_full(c, k0) ? 1 : 0;
            tiles[4 * t + 2] = (t > 0 && k0 == Pol::tile_key0(c, t - 1) + kBN) ? 1 : 0;
            int cheap = 0;
            if (t + dist + 1 < nT) {
                Pol::RowWalk probe = w0;
                probe.prev_k0 = Pol::tile_key0(c, t + dist);   // the latest resolved tile when N(t) runs
                cheap = Pol::row_walk_cheap(probe, Pol::tile_key0(c, t + dist + 1)) ? 1 : 0;
            }
            tiles[4 * t + 3] = cheap;
        }
    }
    if (rows) {   // one lane's walk per row of a tile, in the kernel's order: tiles 0 .. dist in front of the loop, tile t + dist + 1 in N(t)
        for (int row = 0; row < kBN; ++row) {
            Pol::RowWalk w = w0;
            int phys = 0;
            for (int t = 0; t <= dist && t < nT; ++t) {
                Pol::row_walk_next(p, w, phys, Pol::tile_key0(c, t), row);
                rows[(size_t)t * kBN + row] = phys;
            }
            for (int t = 0; t + dist + 1 < nT; ++t) {   // (all of these lie in the unguarded loop; the guarded tail resolves nothing)
                Pol::row_walk_step(w, phys);
                if ((unsigned)(t - run_lo) < (unsigned)run_n) Pol::row_walk_in_run(w);
                else {   // (as attn_m16_tile spells it)
                    const int k_next = Pol::tile_key0(c, t + dist + 1);
                    if (!Pol::row_walk_cheap(w, k_next)) Pol::row_walk_exact(p, w, phys, k_next, row);
                }
                rows[(size_t)(t + dist + 1) * kBN + row] = phys;
            }
        }
    }
    return nT;
}

// the traces of the last traced launch (diagnostics builds; SVG_ERR_UNSUPPORTED otherwise)
extern "C" int svg_debug_wg_trace(uint64_t* out, int n_workgroups) { return g_trace_reader(out, true, n_workgroups); }
extern "C" int svg_debug_pp_trace(uint64_t* out104) { return g_trace_reader(out104, false, 0); }

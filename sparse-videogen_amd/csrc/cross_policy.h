// Cross-attention policy for attn_m16_tile (attn_m16.h): Sq query rows over ONE dense segment of Skv keys starting at key 0, Sq != Skv
// allowed — the text / image-token attention of the Wan and Cosmos blocks (svg_cross_attention in svg_attn.h).  No row permutation, no
// mask but the end of the key set: only the ragged last key tile takes the per-element path.  Modelled on BandPolicy (band_policy.h).
// Windowed form (svg_cross_attention_keyrange): the segment is [begin, end) of the head's video, read from two device arrays — a text
// key-padding mask.  Logical key tile t is key tile t0 + t with t0 = begin / 64, so a left-padded window walks no masked tile; the (at
// most two) edge tiles take the per-element path; nT == 0 for an empty window, whose rows come out as zeros.  The plain form's members are
// empty bases and compile-time branches: its kernel is the one it was.
// LSE form (svg_cross_attention_lse, CrossLsePolicy below): either of the two plus one fp32 per query row, the log-sum-exp of its scores.
// fp32 form (svg_cross_attention_lse_f32, CrossF32Policy below): the LSE form with its rows stored as fp32, before the 16-bit rounding.
#pragma once
#include "attn_core.h"

namespace svg {

template <bool Windowed>
struct CrossWindowArgs {};
template <>
struct CrossWindowArgs<true> {
    const int* kv_begin;   // [BH / heads_per_window] device; nullptr: all zeros
    const int* kv_end;     // [BH / heads_per_window] device
    int heads_per_window;
};
template <bool Windowed>
struct CrossWindowCtx {};
template <>
struct CrossWindowCtx<true> {
    int kbegin, kend, t0;  // the window clamped to 0 <= kbegin <= kend <= Skv; its first key tile
};

template <typename T, bool Windowed = false>
struct CrossPolicy : LayoutAccess<CrossPolicy<T, Windowed>> {
    static constexpr int kHeadDim = 128;
    static constexpr bool kFixup = false;
    static constexpr bool kPartialOut = false;
    static constexpr bool kIntervalMask = true;   // row_intervals() describes the mask (two-phase body)
    static constexpr bool kFastPartial = false;
    static constexpr bool kOneBarrier = false;    // as BandPolicy; the kernel forces one barrier per tile as band_attn_m16_kernel does
    static constexpr int kRowBlocks = 1;
    static constexpr int kWR = 32;                // rows per wave
    static constexpr int BM = 8 * kWR;            // rows per q-tile

    struct Params : CrossWindowArgs<Windowed> {
        const T* q;
        const T* k;
        const T* v;
        T* o;
        int Sq, Skv, BH, nqt;
        float scale_log2;
        AttnLayout lay;   // strides of q, k, v, o (contiguous [BH, Sq, D] / [BH, Skv, D] unless the caller passed a layout)
    };
    struct Ctx : CrossWindowCtx<Windowed> {
        int head, qt, q0, q_end, nT;
    };
    struct KvCursor {};

    // work item w of a launch -> (head, q-tile), head-major
    static __device__ __forceinline__ void init_tile(const Params& p, Ctx& c, int head, int qt) {
        c.head = head, c.qt = qt;
        c.q0 = qt * BM;
        c.q_end = min(c.q0 + BM, p.Sq);
        if constexpr (Windowed) {
            // wave-uniform loads (head comes from the workgroup id), moved to scalar registers: the window, and with it nT, stay scalar
            const int w = head / p.heads_per_window;
            const int e = min(max(__builtin_amdgcn_readfirstlane(p.kv_end[w]), 0), p.Skv);
            const int b = min(max(p.kv_begin ? __builtin_amdgcn_readfirstlane(p.kv_begin[w]) : 0, 0), e);
            c.kbegin = b, c.kend = e;
            c.t0 = b / kBN;
            c.nT = e > b ? (e - 1) / kBN - c.t0 + 1 : 0;
        } else {
            c.nT = (p.Skv + kBN - 1) / kBN;
        }
    }

    static __device__ __forceinline__ int q_logical(const Ctx& c, int row) { return c.q0 + row; }
    static __device__ __forceinline__ bool wave_active(const Ctx& c, int wrow0) { return c.q0 + wrow0 < c.q_end; }
    static __device__ __forceinline__ int q_phys(const Params&, const Ctx& c, int row) {
        const int l = c.q0 + row;
        return l < c.q_end ? l : -1;
    }
    static __device__ __forceinline__ int tile_key0(const Ctx& c, int t) {
        if constexpr (Windowed) return (c.t0 + t) * kBN;
        else return t * kBN;
    }
    static __device__ __forceinline__ void kv_cursor_init(const Params&, const Ctx&, KvCursor&, int) {}
    // rows at or behind Skv are never read: their lanes fetch row 0, and row_intervals masks what they deliver
    // (windowed: rows outside [kbegin, kend) likewise — their lanes fetch row kbegin, a row of the window: nT > 0 only if it has one)
    static __device__ __forceinline__ int kv_phys(const Params& p, const Ctx& c, KvCursor&, int t, int row) {
        if constexpr (Windowed) {
            const int l = (c.t0 + t) * kBN + row;
            return (l >= c.kbegin && l < c.kend) ? l : c.kbegin;
        } else {
            const int l = t * kBN + row;
            return l < p.Skv ? l : 0;
        }
    }
    // wave-uniform: every key of the tile at key k0 exists
    static __device__ __forceinline__ bool fast_full(const Params& p, int k0) { return k0 + kBN <= p.Skv; }
    static __device__ __forceinline__ int classify(const Params& p, const Ctx& c, int k0, int wrow0) {
        if constexpr (Windowed) {   // full only if the tile lies wholly inside the window
            if (k0 >= c.kbegin && k0 + kBN <= c.kend) return TILE_FULL;
        } else {
            if (fast_full(p, k0)) return TILE_FULL;
        }
        return wave_active(c, wrow0) ? TILE_PARTIAL : TILE_SKIP;
    }
    // the keys of a row: [0, Skv) — windowed: [kbegin, kend) — no second interval
    static __device__ __forceinline__ void row_intervals(const Params& p, const Ctx& c, int, int& a0, unsigned& alen, int& b0, unsigned& blen) {
        if constexpr (Windowed) a0 = c.kbegin, alen = (unsigned)(c.kend - c.kbegin);
        else a0 = 0, alen = (unsigned)p.Skv;
        b0 = 0, blen = 0u;
    }
    static __device__ __forceinline__ float score_fixup(const Params&, float s) { return s; }
    static __device__ __forceinline__ void notify(const Params&, const Ctx&) {}
};

// LSE form (svg_cross_attention_lse): the plain or windowed policy plus the row log-sum-exp (attn_m16.h: HasRowLse, switched on by
// lse_base below) — what a caller needs to merge results computed over parts of the keys (svg_merge_attention_states).  lse is a
// contiguous fp32 [BH, Sq] whatever the layout of q / o: it is small, and the merge reads it linearly.
template <typename T, bool Windowed = false>
struct CrossLsePolicy : CrossPolicy<T, Windowed> {
    using Base = CrossPolicy<T, Windowed>;
    struct Params : Base::Params {
        float* lse;   // [BH, Sq]
    };
    static __device__ __forceinline__ float* lse_base(const Params& p, const typename Base::Ctx& c) { return p.lse + (size_t)c.head * (size_t)p.Sq; }
};

// fp32 form (svg_cross_attention_lse_f32): the LSE policy plus the rows before their rounding (attn_m16.h: HasRowO32, switched on by
// o32_base below) — a part for svg_merge_attention_states_f32, whose rounding is then the only one.  o32 is a contiguous fp32 [BH, Sq, 128]
// whatever the layout of q; Params::o is not used.
template <typename T, bool Windowed = false>
struct CrossF32Policy : CrossLsePolicy<T, Windowed> {
    using Base = CrossLsePolicy<T, Windowed>;
    struct Params : Base::Params {
        float* o32;   // [BH, Sq, 128]
    };
    static __device__ __forceinline__ float* o32_base(const Params& p, const typename Base::Ctx& c) {
        return p.o32 + (size_t)c.head * (size_t)p.Sq * 128;
    }
};

// Pair form (svg_cross_attention_pair): the plain policy run twice per q-tile, over key set A and then over key set B, the second pass
// adding its rounded rows to what the first stored (attn_m16.h: add-on-store, switched on by add_on_store below).  The kernel hands
// attn_m16_tile one Params per pass — the plain Params of that pass's key set plus the flag — so every member above serves both.
template <typename T>
struct CrossPairPolicy : CrossPolicy<T, false> {
    using Base = CrossPolicy<T, false>;
    struct Params : Base::Params {
        int add_to_o;   // 0: store the rows (pass A); 1: add them to the rows in o (pass B)
    };
    static __device__ __forceinline__ bool add_on_store(const Params& p) { return p.add_to_o != 0; }
};
// what the pair kernel takes: the plain Params of key set A, and of key set B whatever differs — its tensors, its length and its strides
// (the batch stride of a [B, Skv, H * D] projection view depends on Skv: one AttnLayout cannot describe both sets)
template <typename T>
struct CrossPairArgs {
    typename CrossPolicy<T, false>::Params a;
    const T* k_b;
    const T* v_b;
    int Skv_b, hpb_kv_b;
    long long k_bs_b, k_hs_b, v_bs_b, v_hs_b;
    int k_rs_b, v_rs_b;
};

}  // namespace svg

/*
 * svg_attn.h — C ABI of libsvgattn.so, the MI355X (gfx950) sparse-attention engine that sits behind the
 * attention-processor / operator API of svg-project/Sparse-VideoGen.
 *
 * Every entry point is `extern "C"`, takes raw device pointers + sizes + an opaque hipStream_t (as void*),
 * launches asynchronously on that stream, never allocates, never synchronises, never throws.  The return
 * value is 0 on success or a negative SVG_ERR_* code (svg_strerror() gives text).  Tensors are owned by the
 * caller.  "ref:" lines cite the reference interface (path:line under the Sparse-VideoGen tree) that the
 * entry point replaces; INTEGRATION.md shows the Python-side binding a maintainer would add.
 *
 * Layout conventions (same as the reference): Q/K/V/O are contiguous [cfg*H, S, D] ("BH, S, D"), element
 * type bf16 or fp16 (dtype code), D in {64, 128}.  Token order along S is the model's: Hunyuan/Wan/Cosmos
 * video tokens first (frame-major, idx = f*P + p) then text; CogVideoX text first.
 */
#ifndef SVG_ATTN_H_
#define SVG_ATTN_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SVG_DTYPE_BF16 0
#define SVG_DTYPE_F16 1
#define SVG_DTYPE_F32 2   /* only where an entry point says so (block glue: fp32 LayerNorm outputs, fp32 weights) */

#define SVG_OK 0
#define SVG_ERR_BAD_ARG (-1)       /* null pointer, negative size, inconsistent geometry          */
#define SVG_ERR_UNSUPPORTED (-2)   /* head_dim / dtype / size outside what the kernels implement  */
#define SVG_ERR_WORKSPACE (-3)     /* caller-provided workspace too small                          */
#define SVG_ERR_LAUNCH (-4)        /* hipLaunchKernel / attribute call failed (see svg_last_hip_error) */

/* ABI version of this header: bumped whenever an existing entry point's signature or a struct layout changes (new entry points do
 * not bump it).  A binding compares svg_abi_version() of the library it loaded with the SVG_ABI_VERSION it was written against and
 * refuses to call into a mismatch (svg/_native.py load()).  4: round 4 (svg_band_attention_notify* carry `done_words`). */
#define SVG_ABI_VERSION 4
int svg_abi_version(void);

const char* svg_strerror(int code);
int svg_last_hip_error(void);          /* raw hipError_t of the last failing launch in this thread */
const char* svg_build_info(void);      /* "libsvgattn gfx950 <date> ..."                           */

/* ------------------------------------------------------------------------------------------------
 * Layout transformation ("placement").
 * ref: svg/models/hyvideo/placement.py:124-153 (hunyuan_sparse_head_placement),
 *      svg/models/hyvideo/placement.py:360-387 (hunyuan_hidden_states_placement),
 *      svg/models/cog/placement.py:80-82 (text-first variant), svg/models/wan/placement.py (ctx = 0).
 * For every (cfg, head) with best_mask_idx != 0 ("temporal head") video row f*P+p moves to p*F+f
 * (forward) or p*F+f moves to f*P+p (inverse); text rows and "spatial" heads are copied unchanged.
 * best_mask_idx: device int64 [BH].  text_first = 0: text is the last `context_length` rows
 * (Hunyuan/Wan), 1: the first `context_length` rows (CogVideoX).  n_tensors in {1,2,3}: the same
 * transformation is applied to up to three tensors in one launch (Q,K,V).
 * ---------------------------------------------------------------------------------------------- */
int svg_head_placement(const void* const* src, void* const* dst, int32_t n_tensors, const int64_t* best_mask_idx,
                       int32_t BH, int32_t S, int32_t D, int32_t dtype, int32_t context_length, int32_t num_frame,
                       int32_t frame_size, int32_t text_first, int32_t inverse, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Token permutation (gather) and inverse permutation (scatter) of rows.
 * ref: svg/kernels/triton/permute.py:12-43,82-128 (Y[bh,s,:] = X[bh, idx[bh,s], :])
 *      svg/kernels/triton/permute.py:46-75,131-170 (Y[bh, idx[bh,s], :] = X[bh,s,:])
 * idx: device int32 [BH, S].
 * ---------------------------------------------------------------------------------------------- */
int svg_permute_rows(const void* x, const int32_t* idx, void* y, int32_t BH, int32_t S, int32_t D, int32_t dtype,
                     void* stream);
int svg_inverse_permute_rows(const void* x, const int32_t* idx, void* y, int32_t BH, int32_t S, int32_t D,
                             int32_t dtype, void* stream);

/* Stable argsort of cluster labels (counting sort): sorted_idx[b, :] = argsort(labels[b, :], stable),
 * counts[b, k] = |{n : labels[b,n] == k}|.  This fixes the tie order the reference leaves unspecified
 * (torch.argsort without stable=True, ref: svg/kernels/triton/permute.py:113, svg/kmeans_utils.py:396).
 * labels: device int32 [B, N] with values in [0, K); sorted_idx: int32 [B, N]; counts: int32 [B, K] (may be NULL).
 * workspace: svg_argsort_workspace_bytes(B, N, K) bytes of device scratch. */
size_t svg_argsort_workspace_bytes(int32_t B, int32_t N, int32_t K);
int svg_argsort_labels(const int32_t* labels, int32_t* sorted_idx, int32_t* counts, int32_t B, int32_t N, int32_t K,
                       void* workspace, size_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------------------------------
 * SVG1 block-sparse attention (and the dense baseline) — one analytic mask family.
 * ref: flex_attention(q, k, v, block_mask) at svg/models/hyvideo/attention.py:401-403 with the mask_mod of
 *      svg/models/hyvideo/utils.py:20-44, svg/models/wan/utils.py:25-41, svg/models/cog/utils.py:30-46;
 *      dense: flash_attn_varlen_func with cu_seqlens [0, valid, S], svg/models/hyvideo/attention.py:452-470.
 * allowed(q, k) = (q < real_len && k < real_len &&
 *                  (|q - k| < band || colfull_lo <= k < colfull_hi || rowfull_lo <= q < rowfull_hi))
 *              || (q >= real_len && k >= real_len)
 *   Hunyuan : real_len = V + prompt_len, band = floor(w*P/128)*128, colfull = rowfull = [V, real_len)
 *   Wan     : real_len = S, band = ceil(w*P/128)*128 + 1 (the reference uses <=), colfull = [0, P), rowfull = {}
 *   Cog     : real_len = S, band = floor(w*P/128)*128, colfull = [0, Lp (+P if sink)), rowfull = [0, Lp)
 *   dense   : band = S + 1 (two segments when real_len < S, i.e. cu_seqlens [0, real_len, S])
 * Rows with no allowed key produce zeros.  The mask is evaluated element-wise on band-edge tiles, exactly as
 * flex_attention applies mask_mod inside partial blocks.
 * Sizes (every svg_band_attention* entry): S < 2^24 and S * D * 2 < 2^32 (the LDS-DMA requests carry 32-bit byte offsets per head and
 * compute a row's offset with a 24-bit multiply), BH * S * D < 2^40; larger calls return SVG_ERR_UNSUPPORTED.
 *
 * Fused layout transformation: when head_perm_flag != NULL, heads with head_perm_flag[bh] != 0 are processed
 * in token-major order *without* materialising the permuted tensors: logical row i (< perm_V, offset by
 * perm_vid0) is read from / written to physical row vid0 + (i%F)*P + i/F.  The mask is in logical order.
 * This equals placement -> attention -> inverse placement of the reference (attention.py:514-520).
 * ---------------------------------------------------------------------------------------------- */
typedef struct svg_band_mask {
    int32_t real_len;
    int32_t band;
    int32_t colfull_lo, colfull_hi;
    int32_t rowfull_lo, rowfull_hi;
} svg_band_mask_t;

typedef struct svg_perm_desc {
    const int64_t* head_perm_flag; /* device int64 [BH] (best_mask_idx) or NULL                 */
    int32_t vid0;                  /* first video row (0 text-last, context_length text-first)  */
    int32_t num_frame;             /* F                                                          */
    int32_t frame_size;            /* P                                                          */
} svg_perm_desc_t;

/* variant: 0 = default (= 8 at head_dim 128; = 2 at head_dim 64, where the two-phase body runs four waves per SIMD — two workgroups per CU).  All schedules produce the same result up to rounding.
 *   1 = lock-step, 4 waves x 32 query rows, 128-row q-tiles, two workgroups per CU (register-staged K/V) — the plain schedule
 *       the test-suite uses as the in-library reference;
 *   2 = two-phase ping-pong, 8 waves x 32 rows: the two waves that share a SIMD alternate a matrix phase (PV of tile t + QK^T
 *       of tile t+1, operands streamed from LDS) and a vector phase (softmax without a running maximum, LDS-DMA requests), always
 *       in opposite phases;
 *   3 = one wave per SIMD, 4 waves x 64 rows, O and Q in the AGPR half of the register file, softmax / LDS reads / LDS-DMA
 *       requests software-pipelined into the gaps between the wave's own MFMAs, one barrier per tile (csrc/attn_w4.h).
 *   8 = the two-phase schedule of 2 on v_mfma_f32_16x16x32 instead of 32x32x16 (head_dim 128 only; csrc/attn_m16.h): the 16-bit
 *       attention kernels run at the chip's power limit, and the 16x16x32 shape does the same FLOPs with half the accumulator
 *       traffic — the matrix pipe alone is granted 2.15 GHz instead of 1.75 on changing operands (profiles/r04c_energy_table.txt).
 *   6 = frozen reference schedule (bf16, D = 128 only): the two-phase body with the round-1 softmax (running maximum, deferred
 *       rescale) and operand fetch, kept so that a bench run can time it beside the default on the same box.
 * Any other value: SVG_ERR_BAD_ARG.  Builds with -DSVG_ABLATIONS (diagnostics, never the product library) additionally accept
 * 32: variant 3 with the per-phase cycle trace (svg_debug_pp_trace), and
 * 64 | (abl << 8): variant 2 with the per-phase cycle trace / launch timeline (svg_debug_pp_trace, svg_debug_wg_trace) and its
 * timing-only ablations abl = 1..7 (wrong results by construction); the product library returns SVG_ERR_UNSUPPORTED for them. */
int svg_band_attention(const void* q, const void* k, const void* v, void* o, int32_t BH, int32_t S, int32_t D,
                       int32_t dtype, float sm_scale, const svg_band_mask_t* mask, const svg_perm_desc_t* perm,
                       int32_t variant, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Strided tensors: attention straight out of / into the projection layout.
 * ref: the reference's processors build q, k, v as `proj(x).unflatten(2, (heads, -1)).transpose(1, 2)` and hand the result back as
 *      `hidden_states.transpose(1, 2).flatten(2, 3)` (svg/models/wan/attention.py:123-125,168-170, hyvideo/attention.py:83-85,202) —
 *      flex_attention / flash-attn take the strided VIEWS, and what they cannot take is copied: one transpose copy per tensor and
 *      layer (V in, O out: 2 x 2 x S x H x D x 2 bytes that carry no arithmetic).
 * A tensor here is a [B, H, S, D] view whose last dimension is contiguous; strides are in ELEMENTS.  Head index bh = b * H + h with
 * H = heads_per_batch (k / v of svg_varblock_attention_strided: kv_heads_per_batch).  The contiguous [BH, S, D] layout of every other
 * entry point is { batch = H * S * D, head = S * D, row = D }; the projection layout [B, S, H * D] is { S * H * D, D, H * D }; a slice
 * of a fused QKV projection [B, S, 3 * H * D] is { 3 * S * H * D, D, 3 * H * D } behind a base pointer moved to the slice.
 * Requirements: base pointers and row strides multiples of 16 bytes; S * row stride * 2 < 2^32 for k and v (their LDS-DMA requests
 * carry 32-bit byte offsets per head), row strides < 2^23 elements.  The default schedules only — the two-phase bodies: 16x16x32 at
 * head_dim 128, 32x32x16 at head_dim 64 (variant 0 of svg_band_attention, the default of svg_varblock_attention on block-rows large
 * enough for it; svg_sample_mse: its second form, bf16); anything else returns SVG_ERR_UNSUPPORTED and the caller copies, as the
 * reference does.  Results are bit-identical to the contiguous call on the same values (tests/test_gpu_strided.py).
 * ---------------------------------------------------------------------------------------------- */
typedef struct svg_tensor_strides {
    int64_t batch, head, row;          /* element strides of a [B, H, S, D] view, stride(D) == 1 */
} svg_tensor_strides_t;

typedef struct svg_attn_layout {
    int32_t heads_per_batch;           /* H of q / o (and of k / v unless kv_heads_per_batch says otherwise) */
    int32_t kv_heads_per_batch;        /* 0: = heads_per_batch */
    svg_tensor_strides_t q, k, v, o;
} svg_attn_layout_t;

int svg_band_attention_strided(const void* q, const void* k, const void* v, void* o, int32_t BH, int32_t S, int32_t D,
                               int32_t dtype, float sm_scale, const svg_band_mask_t* mask, const svg_perm_desc_t* perm,
                               const svg_attn_layout_t* layout, void* stream);

/* svg_band_attention for a q that already carries the softmax scale: q_scaled = q * sm_scale * log2(e), rounded ONCE to the 16-bit
 * type by whoever produced q (svg_qk_norm_rope* with q_scale — the processors' prologue — so no second rounding happens on that
 * path).  The kernel then starts its score accumulators at minus the row's softmax reference and the MFMAs deliver the exponent
 * argument directly: one FMA per score less on the vector pipe (the PRE form of the default two-phase schedule: on 16x16x32 MFMAs at
 * D = 128, on 32x32x16 at D = 64).  Same mask / perm semantics and the same result as svg_band_attention(q, ..., sm_scale) up to the
 * rounding of q_scaled — which is the catch: the scores come from round(c * q) instead of c * round(q), a second 2^-9 perturbation on
 * bf16 (2.8e-3 ... 6.4e-3 rel. L2 to the reference's formulation where svg_band_attention holds 1.9 - 2.3e-3; fp16: 3.5e-4 ... 8e-4 vs
 * 2.4 - 2.9e-4).  It is what flex_attention calls its PRESCALE_QK kernel option ("about 20% more numerical error, but slightly faster");
 * the reference runs flex_attention with the default, PRESCALE_QK = False (svg/models/hyvideo/attention.py:401-403), and so do the
 * processors of this package unless `prescale_q` is switched on. */
int svg_band_attention_prescaled(const void* q_scaled, const void* k, const void* v, void* o, int32_t BH, int32_t S, int32_t D,
                                 int32_t dtype, const svg_band_mask_t* mask, const svg_perm_desc_t* perm, void* stream);

/* svg_band_attention_switch (device-side dense / sparse switch, below) for a pre-scaled q. */
int svg_band_attention_switch_prescaled(const void* q_scaled, const void* k, const void* v, void* o, int32_t BH, int32_t S, int32_t D,
                                        int32_t dtype, const svg_band_mask_t* mask, const svg_perm_desc_t* perm,
                                        const svg_band_mask_t* alt_mask, const int32_t* use_alt_flag, void* stream);

/* ------------------------------------------------------------------------------------------------
 * SVG2 variable-block sparse attention.
 * ref: dynamic_block_sparse_fwd_flashinfer, svg/kmeans_utils.py:1319-1392 (VariableBlockSparseAttentionWrapper
 *      plan/run, patch assets/patches/modifications.patch:18-78); semantics = dynamic_block_sparse_fwd_torch,
 *      svg/kmeans_utils.py:902-995: query rows of block-row i attend exactly the kv rows of block-cols j with
 *      block_map[h, i, j]; blocks are consecutive ranges of sizes q_sizes[h, :], k_sizes[h, :]; rows with no
 *      active key (and rows of empty blocks) give zeros.
 * q/o: [Hq, Sq, D], k/v: [Hkv, Skv, D] (Hq % Hkv == 0: GQA group shares map/sizes of its kv head).
 * block_map: device uint8/bool [Hkv, QB, KB]; q_sizes int32 [Hkv, QB]; k_sizes int32 [Hkv, KB].  KB <= 4032 (the compacted key-block list of a
 * block-row lives in LDS beside the K / V stages; more returns SVG_ERR_UNSUPPORTED).  Sq and Skv < 2^24, Sq * D * 2 and Skv * D * 2
 * < 2^32 (every svg_varblock_attention* entry, as for svg_band_attention), otherwise SVG_ERR_UNSUPPORTED.
 * Fused token permutation: q_row_idx (int32 [Hq, Sq]) / kv_row_idx (int32 [Hkv, Skv]) map a *permuted* position
 * to the physical row of q,o / k,v (the `sorted_indices` of permute_tensor_by_labels); NULL = tensors are
 * already permuted.  With both given the call equals permute(q,k,v) -> attention -> inverse_permute(o)
 * (ref: svg/models/hyvideo/attention.py:651-653,778-783).
 * variant: -1 = auto (what the Python layer passes), 0 = 128-row q tiles (4 waves, two workgroups per CU), 1 = 256-row q tiles
 * (8 waves, lock-step), 2 = mixed (full 256-row tiles on 8 waves, the rest of each block-row on 128-row tiles; two launches),
 * 3 = 256-row q tiles with the two-phase ping-pong body of svg_band_attention (waves without query rows idle), workgroups
 * launched longest-first inside every kv head (device-side counting sort on the active keys of the block-rows), and REMAINDER
 * PACKING: the ragged last tiles of two block-rows of a kv head that fit into one tile and share many key blocks (a device-side
 * matching on the map's bitmap rows) run as ONE tile that walks the common key blocks once — exact: a row sees its own block-row's
 * keys only (two key intervals per row); 6 = variant 3 without the packing (the default of round 2);
 * 4 = the same kernel in block-row order (A/B measurements); 5 = variant 3 recording the launch timeline (svg_debug_wg_trace);
 * at head_dim 128 the two-phase body of 3 .. 7 runs on 16x16x32 MFMAs (csrc/attn_m16.h) — 8 = 3 naming that body, 9 = 3 forcing the
 * 32x32x16 body (A/B);
 * 7 = similarity order: block-rows with (nearly) the same active key blocks are neighbours of a device-built nearest-neighbour
 * chain and consecutive workgroups go to the same XCD so that they meet in its L2 (maps whose bitmap does not fit the chain
 * kernel's 64 KiB of LDS — QB * (KB / 32 + 4) words — fall back to 3).  Measured at Wan 2.1 720p (profiles/r03b_pmc_svg2_*):
 * L2 hit rate 48 % instead of 31 %, 90 GB instead of 119 GB between L2 and the fabric, kernel time unchanged, chain kernel
 * 0.7 - 1.0 ms — kept for the traffic it saves when the fabric is shared (multi-GPU exchange), not the default.
 * ---------------------------------------------------------------------------------------------- */
size_t svg_varblock_workspace_bytes(int32_t Hq, int32_t Hkv, int32_t QB, int32_t KB, int32_t Sq);
int svg_varblock_attention(const void* q, const void* k, const void* v, void* o, int32_t Hq, int32_t Hkv, int32_t Sq,
                           int32_t Skv, int32_t D, int32_t dtype, float sm_scale, const uint8_t* block_map,
                           const int32_t* q_sizes, const int32_t* k_sizes, int32_t QB, int32_t KB,
                           const int32_t* q_row_idx, const int32_t* kv_row_idx, void* workspace,
                           size_t workspace_bytes, int32_t variant, void* stream);
/* svg_varblock_attention (variant -1) on strided q, k, v, o: svg_attn_layout_t above; heads_per_batch counts q heads,
 * kv_heads_per_batch kv heads (0: heads_per_batch * Hkv / Hq).  Block-rows large enough for the default (two-phase) body
 * (Sq >= 160 * QB), otherwise SVG_ERR_UNSUPPORTED. */
int svg_varblock_attention_strided(const void* q, const void* k, const void* v, void* o, int32_t Hq, int32_t Hkv, int32_t Sq,
                                   int32_t Skv, int32_t D, int32_t dtype, float sm_scale, const uint8_t* block_map,
                                   const int32_t* q_sizes, const int32_t* k_sizes, int32_t QB, int32_t KB,
                                   const int32_t* q_row_idx, const int32_t* kv_row_idx, void* workspace,
                                   size_t workspace_bytes, const svg_attn_layout_t* layout, void* stream);

/* Dense attention of Sq query rows over Skv keys (Sq != Skv allowed): softmax(q k^T * sm_scale) v per head.
 * ref: the cross-attention branch of the Wan / Cosmos processors, F.scaled_dot_product_attention with attn_mask None
 *      (svg/models/wan/attention.py:174-188,198-201, svg/models/cosmos/attention.py:104-107).
 * head_dim 128, bf16 / fp16 (the two-phase 16x16x32 body of csrc/attn_m16.h on csrc/cross_policy.h: resident workgroups over the
 * 256-row q-tiles of every head, no workspace, no planning pass); anything else SVG_ERR_UNSUPPORTED, and the caller keeps its own
 * dense path.  Sq and Skv < 2^24, the key / value rows of one head within 2^32 bytes, BH * Sq * D < 2^40.  Key rows at or behind Skv
 * are never read.  layout: svg_attn_layout_t above (q / o described with Sq rows, k / v with Skv), faults reported as by the
 * *_strided entries; results are bit-identical to the contiguous call on the same values. */
int svg_cross_attention(const void* q, const void* k, const void* v, void* o, int32_t BH, int32_t Sq, int32_t Skv, int32_t D,
                        int32_t dtype, float sm_scale, const svg_attn_layout_t* layout /* NULL: contiguous [BH,Sq,D] / [BH,Skv,D] */,
                        void* stream);
/* svg_cross_attention over one key window per group of heads — a text key-padding mask, a batch of prompts of different lengths:
 * heads [w * heads_per_window, (w + 1) * heads_per_window) attend to the keys [kv_begin[w], kv_end[w]) only.
 * ref: the same branch with the bool [B, 1, 1, S_text] mask the Cosmos transformer builds (svg/models/cosmos/custom_models.py:85-86,
 *      cosmos/attention.py:104-110), for masks whose True entries are one contiguous run per video.
 * kv_begin, kv_end: DEVICE int32 arrays of BH / heads_per_window entries; kv_begin NULL: all zeros.  kv_end NULL, heads_per_window <= 0 or
 * BH % heads_per_window != 0: SVG_ERR_BAD_ARG; every check of svg_cross_attention applies, all on the host before any launch.  The window
 * VALUES are device data: the host does not read or validate them, the kernel clamps them to 0 <= begin <= end <= Skv.  Key rows
 * outside a window are never read (a NaN in a padded embedding cannot reach the output) and not paid for: a window costs the 64-key
 * tiles it touches.  An empty window gives zeros in every output row of its heads.  For kv_begin a multiple of 64 the result is
 * bit-identical to svg_cross_attention on the key rows [kv_begin, kv_end) alone. */
int svg_cross_attention_keyrange(const void* q, const void* k, const void* v, void* o, int32_t BH, int32_t Sq, int32_t Skv, int32_t D,
                                 int32_t dtype, float sm_scale, const int32_t* kv_begin, const int32_t* kv_end,
                                 int32_t heads_per_window, const svg_attn_layout_t* layout, void* stream);
/* svg_cross_attention over TWO key sets in one launch, the results added: o = T(float(T(o_a)) + float(T(o_b))) with o_x =
 * softmax(q k_x^T * sm_scale) v_x — each branch normalised and rounded to the 16-bit type on its own, then one fp32 add and one
 * conversion, what torch's add of two 16-bit tensors does: bit-identical to svg_cross_attention(q, k_a, v_a) + svg_cross_attention(q,
 * k_b, v_b) followed by that add.
 * ref: the text and the CLIP image branch of a Wan I2V block and the `hidden_states + hidden_states_img` behind them
 *      (svg/models/wan/attention.py:174-188,198-201,210-229).
 * Per q-tile the kernel stores T(o_a), then runs set B and adds on the final store: q is read twice and o written twice by one launch,
 * no workspace, no atomics.  o MUST NOT OVERLAP q, k_a, v_a, k_b or v_b: q is read again after the first store to o.
 * layout describes q, o and set A (k_a, v_a with Skv_a rows); of layout_b ONLY the k and v strides are read — they describe k_b, v_b
 * with Skv_b rows; heads per batch are those of `layout`.  Either may be NULL: contiguous ([BH, Sq, D], [BH, Skv_x, D]).  Every check of
 * svg_cross_attention applies to both sets, all on the host before any launch: a NULL pointer or a non-positive size SVG_ERR_BAD_ARG,
 * D != 128 or rows the kernels cannot address SVG_ERR_UNSUPPORTED, layout faults as by the *_strided entries.  Key rows at or behind a
 * set's Skv are never read. */
int svg_cross_attention_pair(const void* q, const void* k_a, const void* v_a, const void* k_b, const void* v_b, void* o, int32_t BH,
                             int32_t Sq, int32_t Skv_a, int32_t Skv_b, int32_t D, int32_t dtype, float sm_scale,
                             const svg_attn_layout_t* layout, const svg_attn_layout_t* layout_b, void* stream);
/* svg_cross_attention (kv_end NULL) or svg_cross_attention_keyrange (kv_end given) that also returns the softmax state of every query
 * row: lse[bh, s] = log sum_j exp(sm_scale * q[bh, s] . k[bh, j]) over the keys the row attends to, natural logarithm, fp32, CONTIGUOUS
 * [BH, Sq] whatever the layout of q / o.  With it a result computed over a part of the keys can be combined with others later
 * (svg_merge_attention_states below): dense attention with the keys sharded over GPUs, a ring of key shards.
 * ref: flashinfer's `run(..., return_lse=True)` + `flashinfer.merge_state`, svg/kernels/ops/attention_ops.py:178-188; the
 *      context-parallel dense attention of svg/models/wan_orig/distributed/xdit_context_parallel.py:120-169 (xfuser ring / Ulysses).
 * o has the bits of the entry without lse (same kernel body; the epilogue stores one more fp32 per row).  A row without keys (an empty
 * window) has lse = -inf and o = 0.  lse NULL: SVG_ERR_BAD_ARG; kv_end given with heads_per_window <= 0 or BH % heads_per_window != 0:
 * SVG_ERR_BAD_ARG (kv_end NULL: kv_begin and heads_per_window are ignored); every other check is that of svg_cross_attention, all on the
 * host before any launch.  Band and variable-block attention: include/svg_attn_sparse_lse.h (included at the end of this file); the pair entry
 * does not return lse. */
int svg_cross_attention_lse(const void* q, const void* k, const void* v, void* o, float* lse, int32_t BH, int32_t Sq, int32_t Skv, int32_t D,
                            int32_t dtype, float sm_scale, const int32_t* kv_begin, const int32_t* kv_end /* NULL: all keys */,
                            int32_t heads_per_window, const svg_attn_layout_t* layout, void* stream);
/* N-way merge of attention states: n_parts partial results of the SAME query rows over disjoint parts of the keys — o_parts[i] 16-bit
 * contiguous [BH, Sq, D], lse_parts[i] fp32 contiguous [BH, Sq] (svg_cross_attention_lse) — combined into the result over all the keys.
 * Per row, in fp32, parts in index order: m = max_i lse_i, w_i = exp(lse_i - m), o = sum_i w_i o_i / sum_i w_i rounded once to the 16-bit
 * type, lse = m + log sum_i w_i.  A part with lse_i = -inf (or whose weight underflows to zero) contributes nothing and its o_i is not
 * looked at; all parts -inf: o = 0, lse = -inf; n_parts == 1 copies the bits.
 * ref: flashinfer.merge_state, svg/kernels/ops/attention_ops.py:178-188; the step merge of the ring attention behind
 *      svg/models/wan_orig/distributed/xdit_context_parallel.py:120-169.
 * 1 <= n_parts <= 8 (the pointers travel by value in the kernel arguments; all parts in ONE pass because a chain of pairwise merges
 * rounds every intermediate o to 16 bits — 3.8e-3 instead of 2.35e-3 rel. L2 at 8 bf16 parts): anything else SVG_ERR_BAD_ARG, as are a
 * NULL o_parts / lse_parts / o, a NULL among the first n_parts entries of either array (HOST arrays of DEVICE pointers, as
 * svg_head_placement takes them) and a non-positive size.  D other than 64 / 128, a dtype other than bf16 / fp16, rows the attention
 * kernels cannot address (Sq >= 2^24, BH * Sq * D >= 2^40) or a part / o not 16-byte aligned: SVG_ERR_UNSUPPORTED.  lse (merged, [BH, Sq])
 * may be NULL.  layout: NULL for a contiguous o; otherwise ONLY heads_per_batch and the o strides are read (token-major o for the output
 * projection), with the checks of the *_strided entries.  o must not overlap a part. */
int svg_merge_attention_states(const void* const* o_parts, const float* const* lse_parts, int32_t n_parts, void* o, float* lse /* may be NULL */,
                               int32_t BH, int32_t Sq, int32_t D, int32_t dtype, const svg_attn_layout_t* layout /* o strides only; NULL: contiguous */,
                               void* stream);
/* svg_cross_attention_lse that hands out every row BEFORE its rounding: o32 fp32 CONTIGUOUS [BH, Sq, D] whatever the layout of q, the value
 * the 16-bit store of svg_cross_attention_lse rounds (o32 rounded to nearest even IS that o, bit for bit, and lse is bit-identical; fp16: where that store
 * rounded the exact product past what the fp32 product would round to, o32 is one fp32 step off acc * inv, about 3e-5 of the elements).  No 16-bit o
 * is written.  A part for svg_merge_attention_states_f32 below: the merge's rounding is then the only one between the accumulators and the
 * merged result, so a result computed in parts meets the tolerance of one call over all keys.  Twice the output bytes of the 16-bit form.
 * ref: flashinfer's run(..., return_lse=True) + merge_state, svg/kernels/ops/attention_ops.py:178-188 (whose parts are 16-bit).
 * Plain (kv_end NULL) and key-window forms as in svg_cross_attention_lse.  o32 or lse NULL: SVG_ERR_BAD_ARG; o32 not 16-byte aligned:
 * SVG_ERR_UNSUPPORTED; every other check is that of svg_cross_attention_lse (D other than 128: SVG_ERR_UNSUPPORTED), all on the host before
 * any launch.  layout describes q, k and v; its o member is not read.  A row without keys has o32 = 0 and lse = -inf.  Band and
 * variable-block attention: include/svg_attn_f32_parts.h (included at the end of this file). */
int svg_cross_attention_lse_f32(const void* q, const void* k, const void* v, float* o32, float* lse, int32_t BH, int32_t Sq, int32_t Skv,
                                int32_t D, int32_t dtype, float sm_scale, const int32_t* kv_begin, const int32_t* kv_end /* NULL: all keys */,
                                int32_t heads_per_window, const svg_attn_layout_t* layout, void* stream);
/* svg_merge_attention_states over fp32 parts: o_parts[i] fp32 contiguous [BH, Sq, D] as the *_lse_f32 entries write them, lse_parts[i] as
 * there.  The same statement, visiting order and rules for -inf / underflowing parts; the parts enter the fp32 arithmetic as they are and
 * the result is rounded ONCE to `dtype` (bf16 / fp16, the type of o).  n_parts == 1 rounds the part (the bits of the 16-bit attention
 * entry).  Every check and code of svg_merge_attention_states: 1 <= n_parts <= 8, D 64 / 128, parts and o 16-byte aligned, layout read for
 * heads_per_batch and the o strides only.  Reads twice the bytes per part. */
int svg_merge_attention_states_f32(const float* const* o_parts, const float* const* lse_parts, int32_t n_parts, void* o, float* lse /* may be NULL */,
                                   int32_t BH, int32_t Sq, int32_t D, int32_t dtype /* of o */,
                                   const svg_attn_layout_t* layout /* o strides only; NULL: contiguous */, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Online profiler (SVG1): mean-squared error of the two candidate masks on sampled query rows.
 * ref: sample_mse, svg/models/hyvideo/attention.py:376-399 (wan :211-234, cog :120-145) with the profiling masks
 *      of get_attention_mask, svg/models/hyvideo/utils.py:47-93 (wan/utils.py:63-110, cog/utils.py:61-88),
 *      evaluated analytically instead of from two materialised [10000, S] fp32 masks.
 * rows: device int64 [R] sampled query rows (R <= 64 multiple-of-anything; padded internally).  S < 2^24 (every svg_sample_mse* entry,
 * as for svg_band_attention), otherwise SVG_ERR_UNSUPPORTED.
 * profile mask (block = 128): |floor(x/128) - floor(y/128)| < band_blocks with x, y the row / column index in
 * frame-major order (mask 0, "spatial") or in token-major order (mask 1, "temporal"); the per-model quirks of
 * the reference masks (Wan sink columns, Cog's un-offset spatial band and text-less temporal mask) are expressed
 * through svg_profile_variant_t.  A sampled row whose mask admits no key yields NaN like the reference's softmax
 * over all -inf.  out_mse: device float [2, BH].
 * Numerics (csrc/profiler.hip, second form): one score tile serves the dense rows and both masks — the masked softmaxes use
 * the dense rows' running maximum as their reference (exact in real arithmetic; a masked row loses keys that score more than
 * 129 (bf16; fp16: 27) in logit below the row's overall maximum), and a row's denominator is the sum of the probabilities as
 * the numerator sees them (rounded to the input dtype).  The rows are processed in the order of their coordinate under mask 1;
 * the result does not depend on the order they are passed in (up to fp32 summation order over rows).
 * workspace: svg_sample_mse_workspace_bytes(BH, R, D, S).
 * ---------------------------------------------------------------------------------------------- */
typedef struct svg_profile_variant {
    int32_t coord;        /* 0: indices as stored (frame-major); 1: token-major (p*F + f) inside the video range */
    int32_t origin;       /* subtracted from the coordinate before blocking                                    */
    int32_t span;         /* band domain: 0 <= x - origin < span                                               */
    int32_t band_blocks;  /* |floor(x/128) - floor(y/128)| < band_blocks                                       */
    int32_t sink_cols;    /* keys with y < sink_cols always visible (Wan first-frame sink), in variant coords  */
    int32_t text_lo, text_hi; /* rows / cols in [text_lo, text_hi) are all-ones (empty when lo >= hi)          */
} svg_profile_variant_t;

typedef struct svg_profile_desc {
    int32_t vid0;         /* first video row                                   */
    int32_t num_frame;    /* F                                                 */
    int32_t frame_size;   /* P                                                 */
    int32_t emulate_bf16; /* 1: round scores / outputs to the input dtype like the reference's bf16 torch ops */
    svg_profile_variant_t variant[2]; /* [0] "spatial" mask, [1] "temporal" mask */
} svg_profile_desc_t;

size_t svg_sample_mse_workspace_bytes(int32_t BH, int32_t R, int32_t D, int32_t S);
int svg_sample_mse(const void* q, const void* k, const void* v, const int64_t* rows, int32_t R, int32_t BH, int32_t S,
                   int32_t D, int32_t dtype, float sm_scale, const svg_profile_desc_t* prof, float* out_mse,
                   void* workspace, size_t workspace_bytes, void* stream);
/* svg_sample_mse[_flagged] on strided q, k, v (svg_attn_layout_t above; layout->o is ignored).  skip_flag: NULL, or the device flag
 * of svg_sample_mse_flagged.  bf16 only (the second form of the kernel); fp16 with row strides other than D: SVG_ERR_UNSUPPORTED. */
int svg_sample_mse_strided(const void* q, const void* k, const void* v, const int64_t* rows, int32_t R, int32_t BH, int32_t S,
                           int32_t D, int32_t dtype, float sm_scale, const svg_profile_desc_t* prof, float* out_mse,
                           void* workspace, size_t workspace_bytes, const int32_t* skip_flag, const svg_attn_layout_t* layout,
                           void* stream);

/* ------------------------------------------------------------------------------------------------
 * flash-kmeans (Euclidean Lloyd iterations, batched over heads).
 * ref: batch_kmeans_Euclid, svg/kmeans_utils.py:684-733; assign kernel :464-554; sorted centroid update
 *      :258-322,375-421.  One call = one Lloyd iteration, entirely on device:
 *   labels[b,n]   = argmin_k max(0, xsq[b,n] + csq[b,k] - 2 <x[b,n], c[b,k]>)   (lowest index wins ties)
 *   c_new[b,k]    = mean of assigned points (fp32 accumulate, deterministic order), old centroid if empty
 *   counts[b,k]   = cluster sizes;  sorted_idx = stable argsort(labels);  shift[b] = max_k ||c_new - c||
 * x: [B, N, D]; centroids_in/out: [B, K, D] (same dtype as x); labels int32 [B, N]; counts int32 [B, K];
 * sorted_idx int32 [B, N]; shift float [B].  xsq float [B, N] is the reference's `x_sq` (svg_kmeans_xsq; constant over
 * iterations, ref :704) and MAY BE NULL: the kernel assigns by argmax_k (<x, c_k> - |c_k|^2 / 2), which has the same arg-min as
 * the distance form and never reads |x|^2 — pass it only if you compute it anyway.
 * ---------------------------------------------------------------------------------------------- */
int svg_kmeans_xsq(const void* x, float* xsq, int32_t B, int32_t N, int32_t D, int32_t dtype, void* stream);
size_t svg_kmeans_workspace_bytes(int32_t B, int32_t N, int32_t K, int32_t D);
int svg_kmeans_iter(const void* x, const float* xsq, const void* centroids_in, void* centroids_out, int32_t* labels,
                    int32_t* counts, int32_t* sorted_idx, float* shift, int32_t B, int32_t N, int32_t K, int32_t D,
                    int32_t dtype, void* workspace, size_t workspace_bytes, void* stream);

/* The whole Lloyd loop of batch_kmeans_Euclid (ref: svg/kmeans_utils.py:684-733) as ONE call, launches only — no host
 * synchronisation: max_iters x (svg_kmeans_iter into scratch + a commit kernel that applies the reference's stopping rule on the
 * device).  Iteration `it` assigns with the current centroids and computes new ones; while the loop has not stopped its labels /
 * sizes / stable sorted indices are the result; if the largest centre shift (over all batches) is < tol the loop stops THERE and the
 * OLD centroids are the result (:723-724), otherwise the new centroids become current — without convergence the returned centroids
 * are one update ahead of the returned labels, exactly like the reference.  Later iterations still run (no read-back decides how
 * many to launch) but cannot change the result.  n_iters: device int32, the iterations the reference's loop would have run.
 * c_init [B, K, D] is not written; c_work_a / c_work_b [B, K, D] are scratch; centroids_out [B, K, D]; labels / sorted_idx int32
 * [B, N]; counts int32 [B, K].  Replaces ~10 framework micro-launches per iteration of the host-driven loop. */
/* The two halves of svg_kmeans_iter as entry points of their own (host plumbing added at the end of round 3; the kernels are the ones
 * svg_kmeans_iter launches): ref euclid_assign_triton svg/kmeans_utils.py:562-627 and triton_centroid_update_sorted_euclid :375-421.
 * workspace: svg_kmeans_workspace_bytes(B, N, K, D).  labels int32 [B, N]; counts int32 [B, K]; sorted_idx int32 [B, N]; shift float [B]. */
int svg_kmeans_assign(const void* x, const void* centroids, int32_t* labels, int32_t B, int32_t N, int32_t K, int32_t D, int32_t dtype,
                      void* workspace, size_t workspace_bytes, void* stream);
int svg_kmeans_update(const void* x, const int32_t* labels, const void* centroids_in, void* centroids_out, int32_t* counts,
                      int32_t* sorted_idx, float* shift, int32_t B, int32_t N, int32_t K, int32_t D, int32_t dtype, void* workspace,
                      size_t workspace_bytes, void* stream);
size_t svg_kmeans_loop_workspace_bytes(int32_t B, int32_t N, int32_t K, int32_t D);
int svg_kmeans_loop(const void* x, const float* xsq, const void* c_init, void* c_work_a, void* c_work_b, int32_t* labels,
                    int32_t* counts, int32_t* sorted_idx, void* centroids_out, int32_t* n_iters, int32_t B, int32_t N, int32_t K,
                    int32_t D, int32_t dtype, int32_t max_iters, float tol, void* workspace, size_t workspace_bytes, void* stream);
/* svg_kmeans_loop on an x whose batches are `x_batch_stride` elements apart (rows of a batch contiguous, stride D): the video tokens of a
 * [H, S, D] tensor with text tokens behind them — `q[:, :V]` — without the copy the reference makes (`query[:, :, :-context_length, :]`
 * materialised by its Triton kernels' `.contiguous()`, svg/models/hyvideo/attention.py:592-599).  x_batch_stride >= N * D, a multiple of
 * 8, x 16-byte aligned; no xsq argument (the assignment does not read |x|^2).  Same result as svg_kmeans_loop on the copy. */
int svg_kmeans_loop_strided(const void* x, int64_t x_batch_stride, const void* c_init, void* c_work_a, void* c_work_b, int32_t* labels,
                            int32_t* counts, int32_t* sorted_idx, void* centroids_out, int32_t* n_iters, int32_t B, int32_t N,
                            int32_t K, int32_t D, int32_t dtype, int32_t max_iters, float tol, void* workspace,
                            size_t workspace_bytes, void* stream);
/* svg_kmeans_loop[_strided] with one stopping rule per GROUP of batches: the B batches form G = B / group groups of `group` consecutive
 * batches (B % group == 0, group >= 1, otherwise SVG_ERR_BAD_ARG), e.g. the H heads of each video of a [cfg, H] batch.  Group g (batches
 * [g * group, (g + 1) * group)) follows the rule of svg_kmeans_loop on its own batches only: it stops once the largest shift of ITS batches
 * is < tol (a NaN shift never converges), and then keeps the labels / sizes / sorted indices of that iteration and the OLD centroids;
 * another group's shifts never change its result.  n_iters: device int32 [G], the iterations each group's loop would have run.
 * workspace: svg_kmeans_loop_grouped_workspace_bytes(B, N, K, D, group) (0 for a bad group).  With group == B the result is
 * bit-identical to svg_kmeans_loop[_strided], which are these entry points with group = B (and the same workspace size). */
size_t svg_kmeans_loop_grouped_workspace_bytes(int32_t B, int32_t N, int32_t K, int32_t D, int32_t group);
int svg_kmeans_loop_grouped(const void* x, const float* xsq, const void* c_init, void* c_work_a, void* c_work_b, int32_t* labels,
                            int32_t* counts, int32_t* sorted_idx, void* centroids_out, int32_t* n_iters, int32_t B, int32_t N, int32_t K,
                            int32_t D, int32_t dtype, int32_t group, int32_t max_iters, float tol, void* workspace, size_t workspace_bytes,
                            void* stream);
int svg_kmeans_loop_grouped_strided(const void* x, int64_t x_batch_stride, const void* c_init, void* c_work_a, void* c_work_b,
                                    int32_t* labels, int32_t* counts, int32_t* sorted_idx, void* centroids_out, int32_t* n_iters, int32_t B,
                                    int32_t N, int32_t K, int32_t D, int32_t dtype, int32_t group, int32_t max_iters, float tol,
                                    void* workspace, size_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Top-p block selection.
 * ref: identify_dynamic_map + weighted_softmax, svg/kmeans_utils.py:852-896.
 * qc: [BH, QC, D], kc: [BH, KC, D] (dtype), k_sizes int32 [BH, KC]; out_map uint8 [BH, QC, KC].
 * Ties in the descending sort are broken towards the lower cluster index (stable sort).
 * ---------------------------------------------------------------------------------------------- */
int svg_identify_dynamic_map(const void* qc, const void* kc, const int32_t* k_sizes, uint8_t* out_map, int32_t BH,
                             int32_t QC, int32_t KC, int32_t D, int32_t dtype, float top_p, int32_t preserve_length,
                             void* stream);

/* Uniform-block (BSR) front end of the variable-block kernel — the reference's alternative backend
 * (flashinfer.BlockSparseAttentionWrapper plan/run + text merge, svg/kernels/ops/attention_ops.py:107-197, wan variant
 * attention_ops_wan.py): expands (indptr [MB + 1], indices) over MB x NB blocks of row_block x col_block tokens into the dense
 * map [heads, MB + 1, NB + 1] and the size arrays [heads, MB + 1] / [heads, NB + 1] that svg_varblock_attention takes; block-row 0
 * / block-column 0 hold the len_text text tokens (text first) and are always active: video rows see their BSR blocks and all
 * text, text rows see everything — the merge_state of the reference in one kernel. */
int svg_bsr_to_block_map(const int32_t* indptr, const int32_t* indices, int32_t MB, int32_t NB, int32_t row_block,
                         int32_t col_block, int32_t len_text, int32_t heads, uint8_t* block_map, int32_t* q_sizes,
                         int32_t* k_sizes, void* stream);

/* density of a dynamic map, ref: density_calculation, svg/kmeans_utils.py:13-31.  out: float [BH] */
int svg_map_density(const uint8_t* block_map, const int32_t* q_sizes, const int32_t* k_sizes, float* out, int32_t BH,
                    int32_t QB, int32_t KB, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Pre-attention prologue: in-place QK normalisation over head_dim and rotary embedding.
 * ref: the reference's only native extension, svg/kernels/csrc/ops.h:19-260, bound as `_kernels` in
 *      svg/kernels/csrc/ops.cu and called from svg/models/hyvideo/attention.py:162-188, wan/attention.py:45-48,
 *      cog/attention.py:23-34.  Tensors are contiguous [bsz, H, S, D] (norm-only entry points: [m, n] rows), D (n) in
 *      {32, 64, 128, 256}, bf16 or fp16; weights / biases have the tensor dtype; cos / sin tables are fp32.
 * Semantics (pinned by the torch references of the reference's tests, svg/kernels/test/test_*.py):
 *   rms_norm:   y = w * T(x * rsqrt(mean(x^2) + eps))    fp32 statistics, rounded to T before AND after the weight
 *   layer_norm: y = T((x - mean) * rsqrt(var + 1e-5) * w + b)     fp32, biased variance
 *   rope cos/sin ("interleaved pairs"): out = T(x * cos + rotate(x) * sin) in fp32, rotate(x)[2i] = -x[2i+1],
 *               rotate(x)[2i+1] = x[2i]; cos, sin: [S - len_text_prompt, D]
 *   rope complex: (x[2i] + i x[2i+1]) * (real + i imag) in fp64; real, imag: [S - len_text_prompt, D / 2]
 *   rope half-split (rope_kind 3 of the fused entry points below; diffusers apply_rotary_emb(use_real_unbind_dim=-2), ref:
 *               svg/models/cosmos/attention.py:61-66): channel i pairs with i + D/2.  out = T(x * cos + rotate(x) * sin) in fp32, every
 *               product rounded before the add, rotate(x)[i] = -x[i + D/2], rotate(x)[i + D/2] = x[i] for i < D/2; cos, sin:
 *               [rope_hi - rope_lo, D], ALL D columns are read (cos[:, i] need not equal cos[:, i + D/2])
 *   the first (`cossin`, `complex`) or the last (`txtlast`) len_text_prompt positions are left untouched.
 * ---------------------------------------------------------------------------------------------- */
int svg_rms_norm_forward(void* x, const void* weight, int64_t m, int32_t n, int32_t dtype, float eps, void* stream);
int svg_layer_norm_forward(void* x, const void* weight, const void* bias, int64_t m, int32_t n, int32_t dtype,
                           void* stream);
int svg_apply_qk_rope_inplace_cossin(void* q, void* k, const float* cos_cache, const float* sin_cache, int32_t bsz,
                                     int32_t Hq, int32_t Hkv, int32_t S, int32_t D, int32_t dtype, int32_t len_text_prompt,
                                     void* stream);
int svg_apply_qk_rope_inplace_cossin_txtlast(void* q, void* k, const float* cos_cache, const float* sin_cache,
                                             int32_t bsz, int32_t Hq, int32_t Hkv, int32_t S, int32_t D, int32_t dtype,
                                             int32_t len_text_prompt, void* stream);
int svg_apply_qk_rope_inplace_cossin_complex(void* q, void* k, const float* freqs_real, const float* freqs_imag,
                                             int32_t bsz, int32_t Hq, int32_t Hkv, int32_t S, int32_t D, int32_t dtype,
                                             int32_t len_text_prompt, void* stream);
/* Fused form: normalisation (norm_kind 0 none / 1 rms / 2 layer) followed by rotary embedding (rope_kind 0 none / 1 cos-sin /
 * 2 complex / 3 half-split) of positions [rope_lo, rope_hi) with table row (position - rope_lo), ONE pass over q and k (either may be
 * NULL).  Bit-identical to the corresponding sequence of the entry points above (the intermediate rounding is kept); kind 3 is
 * bit-identical to the norm followed by torch's `(x.float() * cos + rotate(x).float() * sin).to(T)`.
 * rope_kind 3 exists on svg_qk_norm_rope, svg_qk_norm_rope_transpose and their _qscale forms only: svg_qk_norm_rope_transpose_joint and
 * svg_rmsnorm_rope_transpose return SVG_ERR_BAD_ARG for it.  SVG_ERR_BAD_ARG: a norm kind outside 0..2, a rope kind outside 0..3, a rope
 * kind != 0 with a NULL table or a range outside [0, S]; SVG_ERR_UNSUPPORTED: D outside {32, 64, 128, 256} — decided before any launch. */
int svg_qk_norm_rope(void* q, void* k, int32_t bsz, int32_t Hq, int32_t Hkv, int32_t S, int32_t D, int32_t dtype,
                     int32_t norm_kind, const void* q_weight, const void* q_bias, const void* k_weight, const void* k_bias,
                     float eps, int32_t rope_kind, const float* cos_or_real, const float* sin_or_imag, int32_t rope_lo,
                     int32_t rope_hi, void* stream);

/* The same pass reading the projection output in token-major layout [bsz, S, H, D] and writing head-major [bsz, H, S, D]:
 * replaces `x.unflatten(2, (heads, -1)).transpose(1, 2)` + contiguous copy + norm + norm + rope
 * (ref: svg/models/hyvideo/attention.py:268-286) by one read and one write per element.  norm_kind = rope_kind = 0 is a plain
 * transpose (use it for V: pass it as q_in / q_out with k_in = NULL). */
int svg_qk_norm_rope_transpose(const void* q_in, const void* k_in, void* q_out, void* k_out, int32_t bsz, int32_t Hq,
                               int32_t Hkv, int32_t S, int32_t D, int32_t dtype, int32_t norm_kind, const void* q_weight,
                               const void* q_bias, const void* k_weight, const void* k_bias, float eps, int32_t rope_kind,
                               const float* cos_or_real, const float* sin_or_imag, int32_t rope_lo, int32_t rope_hi,
                               void* stream);

/* The two fused passes with a factor folded into the LAST rounding of q: q_out = round(q_scale * (norm + RoPE result in fp32)); k is
 * not touched by it.  q_scale = sm_scale * log2(e) produces the q that svg_band_attention_prescaled expects without a second
 * rounding of the rotated positions (positions outside [rope_lo, rope_hi) — the 256 text tokens of Hunyuan — were rounded by the
 * norm already and are rounded again).  q_scale = 1 is bit-identical to the plain entry points; q_scale <= 0: SVG_ERR_BAD_ARG. */
int svg_qk_norm_rope_qscale(void* q, void* k, int32_t bsz, int32_t Hq, int32_t Hkv, int32_t S, int32_t D, int32_t dtype,
                            int32_t norm_kind, const void* q_weight, const void* q_bias, const void* k_weight, const void* k_bias,
                            float eps, int32_t rope_kind, const float* cos_or_real, const float* sin_or_imag, int32_t rope_lo,
                            int32_t rope_hi, float q_scale, void* stream);
int svg_qk_norm_rope_transpose_qscale(const void* q_in, const void* k_in, void* q_out, void* k_out, int32_t bsz, int32_t Hq,
                                      int32_t Hkv, int32_t S, int32_t D, int32_t dtype, int32_t norm_kind, const void* q_weight,
                                      const void* q_bias, const void* k_weight, const void* k_bias, float eps, int32_t rope_kind,
                                      const float* cos_or_real, const float* sin_or_imag, int32_t rope_lo, int32_t rope_hi,
                                      float q_scale, void* stream);

/* Joint (MMDiT) form of svg_qk_norm_rope_transpose: two streams with their own projections and norms meet in ONE sequence.  Segment i
 * fills joint rows [sum(rows[0..i)), sum(rows[0..i])) of the head-major outputs [bsz, H, sum(rows), D] from its own token-major sources
 * [bsz, rows, H * D] with its own norm (norm_kind / weights / eps as in svg_qk_norm_rope, weights and biases of the tensor dtype, NULL =
 * ones / zeros); RoPE applies to JOINT positions [rope_lo, rope_hi) with table row (position - rope_lo); q_scale folds into the last
 * rounding of q as in svg_qk_norm_rope_transpose_qscale; v is a plain transpose.  One launch; n_seg 1 or 2.
 * Bit-identical to svg_qk_norm_rope_transpose_qscale per segment (with the rope rows that fall into it) plus the plain transpose of v,
 * concatenated along the rows.
 * ref: replaces the text-stream projection transposes, norm_added_q / norm_added_k and the three `torch.cat` of
 *      svg/models/hyvideo/attention.py:288-306 (get_encoder_condition_and_concat), after the video stream's :268-286.
 * Any output may be NULL (that tensor is not produced); every segment with rows > 0 supplies exactly the inputs whose outputs are given
 * (a segment with rows = 0 reads nothing and may pass NULL).  SVG_ERR_BAD_ARG: n_seg outside {1, 2}, an input without its output or the
 * reverse, an input equal to an output, rows < 0, a total of 0 or above INT32_MAX / (H * D), a norm / rope kind outside 0..2, a RoPE
 * range outside [0, total], q_scale <= 0.  SVG_ERR_UNSUPPORTED: D outside {32, 64, 128, 256}, a dtype other than bf16 / fp16. */
typedef struct svg_prologue_segment {
    const void* q_in;                  /* token-major [bsz, rows, H * D] of this stream */
    const void* k_in;
    const void* v_in;
    int32_t rows;
    int32_t norm_kind;                 /* 0 none / 1 rms / 2 layer, as svg_qk_norm_rope */
    const void* q_weight;
    const void* q_bias;
    const void* k_weight;
    const void* k_bias;
    float eps;
} svg_prologue_segment_t;

int svg_qk_norm_rope_transpose_joint(const svg_prologue_segment_t* seg, int32_t n_seg, void* q_out, void* k_out, void* v_out,
                                     int32_t bsz, int32_t H, int32_t D, int32_t dtype, int32_t rope_kind, const float* cos_or_real,
                                     const float* sin_or_imag, int32_t rope_lo, int32_t rope_hi, float q_scale, void* stream);

/* The Wan 2.1 prologue in ONE pass (round 6): RMSNorm across ALL heads in the reference's Triton form (svg_rmsnorm_forward's arithmetic over
 * the H * D row) -> rotary embedding of positions [rope_lo, rope_hi) -> head-major transpose for q and k, and the plain transpose of v, in one
 * launch.  Replaces, bit for bit, svg_rmsnorm_forward(q), svg_rmsnorm_forward(k), svg_qk_norm_rope_transpose(q, k, norm 0, rope), the transpose
 * of v — i.e. the reference's get_qk_norm (triton_rmsnorm_forward) + get_transpose_qkv (three `.transpose(1, 2).contiguous()`) +
 * get_rotary_emb (_kernels.apply_qk_rope_inplace_cossin_complex): svg/models/wan/attention.py:99-148.  q_in / k_in / v_in: token-major
 * [bsz, S, H * D] (any of them may be NULL); outputs head-major [bsz, H, S, D]; weights [H * D] of w_dtype or NULL; H * D <= 8192;
 * q_scale as in svg_qk_norm_rope_qscale. */
int svg_rmsnorm_rope_transpose(const void* q_in, const void* k_in, const void* v_in, void* q_out, void* k_out, void* v_out, int32_t bsz,
                               int32_t H, int32_t S, int32_t D, int32_t dtype, const void* q_weight, const void* k_weight,
                               int32_t w_dtype, float eps, int32_t rope_kind, const float* cos_or_real, const float* sin_or_imag,
                               int32_t rope_lo, int32_t rope_hi, float q_scale, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Transformer-block glue of the Wan blocks, rows of [M, N], N % 8 == 0, N <= 8192; dtypes per tensor
 * (SVG_DTYPE_BF16 / F16 / F32); scale, shift, gate are fp32 [M / rows_per_batch, N] (one row per batch element).
 * ref: triton_layernorm_forward svg/kernels/triton/layernorm.py:204-216 (fp32 statistics; the reference writes fp32),
 *      triton_modulate_shift_forward svg/kernels/triton/modulate.py:45-85      y = x * (1 + scale) + shift,
 *      triton_modulate_gate_residual_forward modulate.py:125-164               y = residual + x * gate,
 *      call sites svg/models/wan/custom_models.py:37-111.
 * svg_layernorm_modulate_forward fuses the first two (one read, one write of the 16-bit hidden states instead of
 * read 2 + write 4 + read 4 + write 2 bytes per element); weight / bias NULL = no affine, scale / shift NULL = no modulate.
 * ---------------------------------------------------------------------------------------------- */
int svg_layernorm_forward(const void* x, void* y, const void* weight, const void* bias, int64_t M, int32_t N, int32_t x_dtype,
                          int32_t y_dtype, int32_t w_dtype, float eps, void* stream);
int svg_modulate_shift_forward(const void* x, void* y, const float* scale, const float* shift, int64_t M, int32_t N,
                               int64_t rows_per_batch, int32_t x_dtype, int32_t y_dtype, void* stream);
int svg_modulate_gate_residual_forward(const void* residual, const void* x, const float* gate, void* y, int64_t M, int32_t N,
                                       int64_t rows_per_batch, int32_t r_dtype, int32_t x_dtype, int32_t y_dtype,
                                       void* stream);
int svg_layernorm_modulate_forward(const void* x, void* y, const void* weight, const void* bias, const float* scale,
                                   const float* shift, int64_t M, int32_t N, int64_t rows_per_batch, int32_t x_dtype,
                                   int32_t y_dtype, int32_t w_dtype, float eps, void* stream);
/* RMSNorm of the rows as the reference's TRITON kernel computes it — y = T(x * rsqrt(mean(x^2) + eps) * w), fp32, ONE rounding —:
 * ref: triton_rmsnorm_forward svg/kernels/triton/rmsnorm.py:51-105, the q / k normalisation across all heads of the reference's Wan
 * processors (svg/models/wan/attention.py:105-120).  (svg_rms_norm_forward above is the CUDA extension's form, rounded before the
 * weight like diffusers' RMSNorm; the two differ by at most one ulp of T.)  weight may be NULL. */
int svg_rmsnorm_forward(const void* x, void* y, const void* weight, int64_t M, int32_t N, int32_t x_dtype, int32_t y_dtype,
                        int32_t w_dtype, float eps, void* stream);
/* The same two with `reference_padding`.  0: as above — diffusers' FP32LayerNorm, the branch the reference's kernels replace
 * (svg/models/wan/custom_models.py:44-47).  != 0: the variance of the reference's Triton kernels AS THEY ARE: they load a row
 * zero-padded to N2 = next_power_of_2(N) and the padding takes part in the variance, var' = var + (N2 - N) / N * mean^2
 * (svg/kernels/triton/layernorm.py:35-41, :134-140; found by executing the kernels with Triton's interpreter,
 * tests/test_triton_golden.py).  For a maintainer who needs the reference's ENABLE_FAST_KERNEL numbers rather than LayerNorm's;
 * no difference when N is a power of two or the row mean is 0. */
int svg_layernorm_forward_ex(const void* x, void* y, const void* weight, const void* bias, int64_t M, int32_t N, int32_t x_dtype,
                             int32_t y_dtype, int32_t w_dtype, float eps, int32_t reference_padding, void* stream);
int svg_layernorm_modulate_forward_ex(const void* x, void* y, const void* weight, const void* bias, const float* scale,
                                      const float* shift, int64_t M, int32_t N, int64_t rows_per_batch, int32_t x_dtype,
                                      int32_t y_dtype, int32_t w_dtype, float eps, int32_t reference_padding, void* stream);

/* Device-side dense / sparse switch.  The reference decides per layer on the host,
 * `timestep[0] > first_times_fp` (svg/models/hyvideo/attention.py:491-496), which reads the GPU tensor back in every layer-call.
 * Here the caller turns that comparison into a device flag (one torch op, no synchronisation) and both kernels read it:
 *   svg_band_attention_switch: use_alt_flag[0] != 0 -> attention under alt_mask (the dense warm-up mask) without the layout
 *       transformation of `perm`; otherwise exactly svg_band_attention(mask, perm).  Two-phase kernel only (variant 0).
 *   svg_sample_mse_flagged: skip_flag[0] != 0 -> every kernel of the call returns at once (out_mse is left untouched: the
 *       profiler's result is not used on a dense step); skip_flag == NULL -> svg_sample_mse. */
int svg_band_attention_switch(const void* q, const void* k, const void* v, void* o, int32_t BH, int32_t S, int32_t D,
                              int32_t dtype, float sm_scale, const svg_band_mask_t* mask, const svg_perm_desc_t* perm,
                              const svg_band_mask_t* alt_mask, const int32_t* use_alt_flag, void* stream);
/* svg_band_attention_switch on strided tensors (svg_attn_layout_t above). */
int svg_band_attention_switch_strided(const void* q, const void* k, const void* v, void* o, int32_t BH, int32_t S, int32_t D,
                                      int32_t dtype, float sm_scale, const svg_band_mask_t* mask, const svg_perm_desc_t* perm,
                                      const svg_band_mask_t* alt_mask, const int32_t* use_alt_flag,
                                      const svg_attn_layout_t* layout, void* stream);
int svg_sample_mse_flagged(const void* q, const void* k, const void* v, const int64_t* rows, int32_t R, int32_t BH, int32_t S,
                           int32_t D, int32_t dtype, float sm_scale, const svg_profile_desc_t* prof, float* out_mse,
                           void* workspace, size_t workspace_bytes, const int32_t* skip_flag, void* stream);

/* Band attention over groups of heads, each under a mask of its own: the videos of a batch whose text lengths differ (HunyuanVideo keeps
 * its padded text inside the self-attention sequence, so a list of prompts of different lengths is a list of different masks; the
 * reference sums the lengths over the batch, svg/models/hyvideo/attention.py:308-316, and runs one mask).
 * Group g is the group_heads[g] consecutive heads behind those of groups 0..g-1 (group_heads: HOST memory, n_groups entries, read before
 * the call returns); it runs under masks[g], and under alt_masks[g] when use_alt_flag[0] != 0 on the device.  The result is, bit for bit,
 * one call per group — on that group's heads, with perm->head_perm_flag and the tensor bases advanced to the group's first head, byte
 * offsets in 64 bits — of the single-mask entry the arguments select:
 *   alt_masks == NULL: svg_band_attention (variant 0); with layout: svg_band_attention_strided; q_prescaled != 0 (sm_scale is then
 *       ignored): svg_band_attention_prescaled;
 *   alt_masks != NULL: svg_band_attention_switch, _switch_strided, _switch_prescaled.
 * They are launches on `stream`, one group after the other, and not a mask per head inside one launch.  n_groups == 1 is
 * the single-mask entry itself.  No completion counters: the notify forms stay single-mask.
 * ALL groups are checked on the host before the first launch.  SVG_ERR_BAD_ARG: a NULL tensor, masks or group_heads; n_groups < 1; a
 * group_heads[g] < 1 or a sum other than BH; alt_masks without use_alt_flag or the reverse; a mask or alternate mask of any group that
 * the single-mask entries refuse; with layout, a group that is not a whole number of videos (group_heads[g] % heads_per_batch != 0: a
 * group's base moves by batch strides).  SVG_ERR_UNSUPPORTED: what the single-mask entries do not have — a dtype / head_dim outside
 * bf16, fp16 x 64, 128, rows they cannot address, a layout they refuse, a pre-scaled q with a layout. */
int svg_band_groups_attention(const void* q, const void* k, const void* v, void* o, int32_t BH, int32_t S, int32_t D, int32_t dtype,
                              float sm_scale, const svg_band_mask_t* masks, const svg_band_mask_t* alt_masks,
                              const int32_t* group_heads, int32_t n_groups, const svg_perm_desc_t* perm,
                              const int32_t* use_alt_flag, int32_t q_prescaled, const svg_attn_layout_t* layout, void* stream);

/* fp8 (OCP e4m3) QK^T and PV for the same mask family (BASELINE.json configs[4]; the reference has NO fp8 attention —
 * /root/reference/README.md:117 "[ ] Support FP8 attention" — so there is no interface to cite: this entry point is
 * svg_band_attention with a workspace).  q, k, v, o are the 16-bit tensors of svg_band_attention (D = 128 only); the call runs
 * (1) a per-head absolute-maximum pass, (2) a quantise pass that writes q, k (row-major) and V^T (per 64-key tile) as e4m3 in
 * LOGICAL token order — the head placement of `perm` is applied there — scaled by 448 / amax of the head, and (3) the attention
 * kernel on v_mfma_scale_f32_32x32x64_f8f6f4 with fp32 softmax; probabilities are e4m3 (x 2^8), the output is written in the
 * input dtype at the physical rows (inverse placement fused).  Accuracy is a property of fp8, not of this kernel: see
 * tests/test_gpu_fp8.py for the measured distance to the fp32 oracle and to the 16-bit path.
 * workspace: svg_band_attention_fp8_workspace_bytes(BH, S, D) bytes of device memory (3 * BH * ceil64(S) * D + a few words). */
size_t svg_band_attention_fp8_workspace_bytes(int32_t BH, int32_t S, int32_t D);
int svg_band_attention_fp8(const void* q, const void* k, const void* v, void* o, int32_t BH, int32_t S, int32_t D, int32_t dtype,
                           float sm_scale, const svg_band_mask_t* mask, const svg_perm_desc_t* perm, void* workspace,
                           size_t workspace_bytes, void* stream);
/* The two halves of svg_band_attention_fp8 on their own (same arguments): stage 1 = passes (1) + (2) into the workspace, stage 2 =
 * the attention kernel on a workspace that stage 1 has filled for the same BH, S and perm — for callers that time or overlap the
 * pre-pass separately. */
int svg_band_attention_fp8_stage(const void* q, const void* k, const void* v, void* o, int32_t BH, int32_t S, int32_t D, int32_t dtype,
                                 float sm_scale, const svg_band_mask_t* mask, const svg_perm_desc_t* perm, void* workspace,
                                 size_t workspace_bytes, int32_t stage, void* stream);

/* svg_varblock_attention with e4m3 QK^T / PV — BASELINE.json configs[4] as named (SVG2 with fp8 on the CDNA4 fp8 MFMA; no
 * reference implementation, see svg_band_attention_fp8).  Same arguments as svg_varblock_attention (D = 128; the default schedule:
 * 256-row q tiles in longest-first order); q, k, v are quantised per head (x 448 / amax) in their original row order inside the call
 * and the kernel gathers rows through the block map's run list and q_row_idx / kv_row_idx exactly like the 16-bit kernel; V^T
 * fragments come from ds_read_b64_tr_b8.  workspace: svg_varblock_attention_fp8_workspace_bytes(...) bytes. */
size_t svg_varblock_attention_fp8_workspace_bytes(int32_t Hq, int32_t Hkv, int32_t QB, int32_t KB, int32_t Sq, int32_t Skv, int32_t D);
int svg_varblock_attention_fp8(const void* q, const void* k, const void* v, void* o, int32_t Hq, int32_t Hkv, int32_t Sq, int32_t Skv,
                               int32_t D, int32_t dtype, float sm_scale, const uint8_t* block_map, const int32_t* q_sizes,
                               const int32_t* k_sizes, int32_t QB, int32_t KB, const int32_t* q_row_idx, const int32_t* kv_row_idx,
                               void* workspace, size_t workspace_bytes, void* stream);

/* Exchange overlapped with ONE launch (multi-GPU, SURVEY §8 e).  svg_band_attention_notify = svg_band_attention (variant 0) that
 * also counts completions: every wave adds 1 to done_per_head[h] (int32 [2 * BH], zeroed by the caller; the second half is
 * scratch of the library) after its last store of head h, so done_per_head[h] == svg_band_attention_notify_target(S, mask)
 * means head h of `o` is complete and visible.  The launch is
 * head-major, so heads complete in order; svg_wait_counters enqueues a one-wave kernel on another stream that returns once
 * `n` counters have reached `target` — the all-gather of those heads goes behind it and runs while the launch is still working
 * on the next heads (no chunked launches: at N = 8 three launches of one head cost 5.7 ms, one launch of three heads 4.9 ms). */
int32_t svg_band_attention_notify_target(int32_t S, const svg_band_mask_t* mask);
/* done_words: the number of int32 words the caller allocated at `done_per_head` / `done` — the entry points cannot see the size
 * of a device buffer, and the hidden per-head counters behind the segment counters made the requirement grow once (round 2): a
 * buffer smaller than BH * (nseg + 1) words returns SVG_ERR_WORKSPACE instead of being written out of bounds. */
int svg_band_attention_notify(const void* q, const void* k, const void* v, void* o, int32_t BH, int32_t S, int32_t D,
                              int32_t dtype, float sm_scale, const svg_band_mask_t* mask, const svg_perm_desc_t* perm,
                              int32_t* done_per_head, int32_t done_words, void* stream);
int svg_wait_counters(const int32_t* counters, int32_t n, int32_t target, void* stream);
/* svg_wait_counters with a deadline: the one-wave kernel gives up `timeout_ms` after it started, stores 1 to timed_out[0] (int32
 * in device or pinned host memory, zeroed by the caller) and returns — a waiter of this kind cannot hang its stream whatever
 * happens to the launch it watches; what was queued behind it then runs on incomplete rows, so the caller must read the flag
 * before trusting the exchange (bench.py does after warm-up and falls back to one launch per chunk of heads). */
int svg_wait_counters_deadline(const int32_t* counters, int32_t n, int32_t target, int32_t timeout_ms, int32_t* timed_out,
                               void* stream);
/* The same with several counters per head.  svg_band_attention_notify_layout fills row_bounds[0 .. n] and targets[0 .. n) for this
 * S / mask and returns n <= nseg, the number of segments used; pass that n as `nseg` of svg_band_attention_notify_seg together
 * with done = int32 [BH * (n + 1)], zeroed by the caller (counter (h, s) at done[h * n + s]; the last BH words are scratch of
 * the library).  Contract: done[h * n + s] >= targets[s]  =>  the PHYSICAL rows [row_bounds[s], row_bounds[s + 1]) of head h of
 * `o` are complete and visible.  Segments are cut in q-tile (logical row) order; a head that runs with the fused layout
 * permutation (perm->head_perm_flag[h] != 0) writes the rows of a logical segment to every frame, so its segments are all
 * released together when the head is complete — the contract holds for both kinds of head without the host knowing which
 * is which (best_mask_idx is device data). */
int32_t svg_band_attention_notify_layout(int32_t S, const svg_band_mask_t* mask, int32_t nseg, int32_t* row_bounds, int32_t* targets);
int svg_band_attention_notify_seg(const void* q, const void* k, const void* v, void* o, int32_t BH, int32_t S, int32_t D,
                                  int32_t dtype, float sm_scale, const svg_band_mask_t* mask, const svg_perm_desc_t* perm,
                                  int32_t* done, int32_t done_words, int32_t nseg, void* stream);
/* svg_band_attention_notify_seg for a pre-scaled q (see svg_band_attention_prescaled): same counters, layout and targets. */
int svg_band_attention_prescaled_notify_seg(const void* q_scaled, const void* k, const void* v, void* o, int32_t BH, int32_t S,
                                            int32_t D, int32_t dtype, const svg_band_mask_t* mask, const svg_perm_desc_t* perm,
                                            int32_t* done, int32_t done_words, int32_t nseg, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Work order of the band kernels at head_dim 128 (default schedule; csrc/band_policy.h, BandQueue).
 * With more q-tiles (over all heads) than compute units, svg_band_attention, _strided and _prescaled launch one resident workgroup
 * per compute unit, and the workgroups take (head, q-tile) pairs from a queue: text-row q-tiles first, then the full-length band q-tiles, the shortened band-edge q-tiles
 * last and longest first; every XCD works through a list of its own (32 neighbouring q-tiles at a time) and, when that is dry,
 * through the others'; the shortest q-tiles of all heads, one per compute unit, form a tail that is handed out chip-wide one at a
 * time, longest first.  The counters of the queue live in a pool the LIBRARY owns — no workspace argument: one block per (device,
 * stream), allocated (hipMalloc, once per device, synchronising) at the first such call on a device and never freed; a launch
 * leaves its block zeroed, so back-to-back calls need nothing from the host.  A stream that is being captured into a graph, the
 * 65th stream of a device, and every call that counts completions (svg_band_attention_notify*: consumers rely on heads finishing
 * in order) or switches masks on the device (svg_band_attention_switch*) run the static mapping — one workgroup per q-tile, head
 * after head.  Outputs are bit-identical either way.  (A stream destroyed while its last band launch is still running must not
 * have its handle reused for another band launch before that one has finished: the two would share a block.)
 *
 * svg_band_queue_order: the lists, on the host (no GPU needed).  out == NULL: returns the number of work items (BH * q-tiles per
 * head).  Otherwise writes, list after list (XCD 0 .. 7, then the tail as list 8) and in the order a list hands them out, one triple per work item
 * { list, head * tiles_per_head + q-tile (row order), key tiles of the q-tile } and returns the number of triples; -1: bad
 * arguments or out_words < 3 * work items.
 * svg_debug_band_queue_cap: at most max_workgroups resident workgroups per queue launch from now on, and the queue also for
 * launches of fewer q-tiles than compute units (0: no cap) — tests of the queue's independence of how many workgroups are resident.
 * svg_debug_band_replays: the bf16 band kernels at head_dim 128 test for an overflowing probability on every eighth key tile and
 * validate a q-tile's sums after its loop; a q-tile that fails is computed once more with the test on every tile.  Synchronises the
 * current device and returns how many q-tiles were replayed on it since the library was loaded or the counter was last reset
 * (reset != 0 zeroes it after reading); -1: a HIP error.
 * svg_debug_band_row_cursor: the row cursor of the 16x16x32 band kernels, walked on the host (no GPU needed).  For a head over S rows
 * whose video rows are [vid0, vid0 + num_frame * frame_size), token-major (token_major != 0) or contiguous, the key tiles with first
 * keys k0[0 .. n) are resolved in this order as a wave of the kernel resolves them — a tile that follows the latest one by 64 keys and
 * lies wholly inside the range takes the stepped form, every other tile the division — and out[64 * i + r] receives the physical row of
 * row r of tile i (0 for rows behind S); cheap (or NULL) receives per tile whether the stepped form was taken.  Returns n; -1: bad
 * arguments or out_words < 64 * n.
 * svg_debug_band_tile_run: the tile run of the 16x16x32 band kernels, on the host (no GPU needed).  For wave `wave` (0 .. 7) of q-tile qt
 * (row order) of a head over S rows under `mask` — video rows [vid0, vid0 + num_frame * frame_size), token-major or contiguous;
 * num_frame = 0: no video — and a request distance dist (2 for the leading, 3 for the lagging waves of the kernel), out4 receives
 * { run_lo, run_n, key tiles of the q-tile, q-tiles per head }: the key tiles [run_lo, run_lo + run_n) are the ones whose vector phase
 * makes no per-tile decision — the tile is unmasked by the wave's fast-path interval and follows its predecessor by 64 keys, and the
 * tile that phase resolves, dist + 1 further, lies in the same segment and takes the stepped form of the row cursor.  tiles (or NULL)
 * receives four words per key tile, each evaluated with the per-tile functions the kernel uses outside a run: { first key, unmasked by
 * the fast-path interval, follows its predecessor by 64 keys, the tile dist + 1 further exists and takes the stepped form }.  rows (or
 * NULL) receives rows[64 * t + r], the physical row of row r of key tile t as the kernel's walk — run form inside the run — resolves
 * it.  Returns the number of key tiles; -1: bad arguments, tiles_words < 4 * tiles or rows_words < 64 * tiles. */
int32_t svg_debug_band_tile_run(int32_t S, const svg_band_mask_t* mask, int32_t vid0, int32_t num_frame, int32_t frame_size,
                                int32_t token_major, int32_t qt, int32_t wave, int32_t dist, int32_t* out4, int32_t* tiles,
                                int32_t tiles_words, int32_t* rows, int32_t rows_words);
int32_t svg_band_queue_order(int32_t BH, int32_t S, const svg_band_mask_t* mask, int32_t* out, int32_t out_words);
int svg_debug_band_queue_cap(int32_t max_workgroups);
int64_t svg_debug_band_replays(int32_t reset);
int32_t svg_debug_band_row_cursor(int32_t S, int32_t vid0, int32_t num_frame, int32_t frame_size, int32_t token_major,
                                  const int32_t* k0, int32_t n, int32_t* out, int32_t out_words, int32_t* cheap);

/* Diagnostics (not part of the reference's interface; -DSVG_ABLATIONS builds, otherwise SVG_ERR_UNSUPPORTED): cycle trace of
 * the two-phase attention schedule.  After a svg_band_attention call with variant 64 (bf16, D = 128) and a synchronised
 * stream, copies 104 counters to the host: out[8 * wave + i] = s_memtime ticks wave `wave` of one workgroup spent in
 *   variant 64: i = 0..3  [matrix phase, barrier, vector phase, barrier]
 *   variant 32: i = 0..3  [phase A up to the barrier, wait + barrier, rest of A, phase B]   (waves 0..3)
 * out[64] = KV tiles of that workgroup, out[65] = ticks of its tile loop. */
int svg_debug_pp_trace(uint64_t* out104);

/* Shader-clock probe (measurement aid of bench.py, product library): a one-wave kernel on `stream` that sleeps until
 * stop_flag[0] != 0 (int32 in device or pinned host memory, written by a later memset / copy on ANOTHER stream) or max_ms have
 * passed, then stores { shader-clock ticks (s_memtime), 100 MHz ticks } elapsed to out2[0..1]: the sustained shader clock of
 * the span is 100 MHz * out2[0] / out2[1]. */
int svg_debug_clock_probe(const int32_t* stop_flag, uint64_t* out2, int32_t max_ms, void* stream);

/* Launch timeline of the same traced kernel (variant 64): for each of the first n_workgroups (<= 16384) workgroups
 * out[6 * b + ..] = [s_memtime at entry, at the start of the tile loop, at its end, after the last store of O, HW_ID, XCC_ID]. */
int svg_debug_wg_trace(uint64_t* out, int32_t n_workgroups);

#ifdef __cplusplus
}
#endif

/* the row log-sum-exp forms of band and variable-block attention: declared in a header of their own, part of this interface */
#include "svg_attn_sparse_lse.h"
/* ... and their fp32-row forms (parts for svg_merge_attention_states_f32), likewise */
#include "svg_attn_f32_parts.h"
/* ... and the LSE / fp32 forms of the device-switch and groups launches of band attention, likewise */
#include "svg_attn_band_lse_forms.h"
/* ... and band attention over a row window and a key window of the mask (token-sharded and key-partitioned callers), likewise */
#include "svg_attn_band_window.h"
/* ... and band attention of a frame shard of the rows over a frame shard of the keys, token-major heads included, likewise */
#include "svg_attn_band_shard.h"
/* ... and the device switch between two masks of that shard form (the sparse and the dense warm-up steps of a processor), likewise */
#include "svg_attn_band_shard_switch.h"
/* ... and the pack / unpack layouts of the token-shard exchanges as one batched strided copy, likewise */
#include "svg_attn_shard_exchange.h"
/* ... and the quality probe: dense attention of a few sampled query rows, fp32 rows and row log-sum-exp, likewise */
#include "svg_attn_sample_rows.h"
/* ... and the Lloyd loop of svg_kmeans_loop_grouped in steps, the group maxima handed out and taken back (head-sharded callers), likewise */
#include "svg_attn_kmeans_stepped.h"
/* ... and flash-kmeans with an e4m3 assignment: the centre, the assignment and the Lloyd loop that uses it for its first iterations, likewise */
#include "svg_attn_kmeans_e4m3.h"
/* ... and SVG2's centroid tail: the means of the key clusters and the attention state over the clusters a block map leaves out, likewise */
#include "svg_attn_centroid_tail.h"
/* ... and the per-head band launch below and its device switch as resident workgroups on the work queue, with the order on the host, likewise */
#include "svg_attn_band_per_head_queue.h"
/* ... and SVG1's per-head band width: band attention from a device vector of bands, its device switch and the controller step, likewise */
#include "svg_attn_adaptive_band.h"
/* ... and SVG2's per-head top-p: the block map from a device vector of thresholds, the K-only probe and the controller step, likewise */
#include "svg_attn_adaptive_top_p.h"
/* ... and the online profiler on frame shards: a partial per key shard and the combine over the partials, likewise */
#include "svg_attn_profile_shard.h"
#endif /* SVG_ATTN_H_ */

// SVG2 variable-block attention with the row log-sum-exp, and with fp32 rows, from the bodies `variant = -1` picks besides the 16x16x32
// one (include/svg_attn_varblock_lse_auto.h): the lock-step body on 128-row q-tiles (attn_body, four waves; head_dim 128 and 64) and the
// 32x32x16 two-phase body at head_dim 64 (attn_body_pp2), on VarblockLsePolicyOf / VarblockF32PolicyOf (varblock_policy.h).  The entries,
// the plan and the launch order are attention_varblock.hip's (run_varblock calls the two launches below with the plain call's parameters).
// A translation unit of its own: the kernels of attention_varblock.hip keep their listings, and this one is compiled without packed fp32
// instructions (build.py NO_PACKED_FP32).  What the 16-bit rows round and how is written out in pp2_row16_values (attn_core.h), so o keeps
// the bits of the plain kernels whatever this unit's flags are.
#include "attn_core.h"
#include "varblock_policy.h"

namespace svg {

// 128-row q-tiles, two workgroups per CU as varblock_attn_kernel<T, D, 4>; LDS: the two K/V stages (the fp32 form stages its rows in all
// of them: 4 waves x 32 rows x D x 4 bytes), then the policy's run list.
template <typename T, int D, typename Pol>
__global__ __launch_bounds__(4 * 64, 2) void varblock_attn_lse_kernel(typename Pol::Params prm) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    attn_body<T, D, 4, Pol>(prm, smem, smem + attn_lds_bytes<D, 4>());
}

// 256-row q-tiles at head_dim 64, as varblock_attn_pp2_kernel<T, 64>; the fp32 form stages 8 waves x 32 rows x 256 bytes in the stages
template <typename T, typename Pol>
__global__ __launch_bounds__(512, 2) void varblock_attn_pp2_lse_d64_kernel(typename Pol::Params prm) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    attn_body_pp2<T, 64, Pol>(prm, smem, smem + attn_pp2_lds_bytes<64>());
}

// the plain call's parameter block in the policy's: plus lse, and o32 in the place of the 16-bit o
template <typename Pol, typename Base>
static typename Pol::Params with_state(const Base& p, float* lse, float* o32) {
    typename Pol::Params px;
    static_cast<Base&>(px) = p;
    px.lse = lse;
    if constexpr (HasRowO32<Pol>::value) px.o32 = o32, px.o = nullptr;
    return px;
}

template <typename T, int D>
int launch_varblock_lockstep_lse(const typename VarblockPolicy<T, D, 4>::Params& p, float* lse, float* o32, dim3 grid, int lds_policy,
                                 hipStream_t st) {
    using Lse = VarblockLsePolicyOf<T, D, 4>;
    using F32 = VarblockF32PolicyOf<T, D, 4>;
    const int lds = attn_lds_bytes<D, 4>() + lds_policy;
    if (o32) return launch_attn(varblock_attn_lse_kernel<T, D, F32>, grid, 4 * 64, lds, st, with_state<F32>(p, lse, o32));
    return launch_attn(varblock_attn_lse_kernel<T, D, Lse>, grid, 4 * 64, lds, st, with_state<Lse>(p, lse, nullptr));
}

template <typename T>
int launch_varblock_pp2_lse_d64(const typename VarblockPolicy<T, 64, 8>::Params& p, float* lse, float* o32, dim3 grid, int lds_policy,
                                hipStream_t st) {
    using Lse = VarblockLsePolicyOf<T, 64, 8>;
    using F32 = VarblockF32PolicyOf<T, 64, 8>;
    const int lds = attn_pp2_lds_bytes<64>() + lds_policy;
    if (o32) return launch_attn(varblock_attn_pp2_lse_d64_kernel<T, F32>, grid, 512, lds, st, with_state<F32>(p, lse, o32));
    return launch_attn(varblock_attn_pp2_lse_d64_kernel<T, Lse>, grid, 512, lds, st, with_state<Lse>(p, lse, nullptr));
}

template int launch_varblock_lockstep_lse<__bf16, 128>(const VarblockPolicy<__bf16, 128, 4>::Params&, float*, float*, dim3, int, hipStream_t);
template int launch_varblock_lockstep_lse<__bf16, 64>(const VarblockPolicy<__bf16, 64, 4>::Params&, float*, float*, dim3, int, hipStream_t);
template int launch_varblock_lockstep_lse<_Float16, 128>(const VarblockPolicy<_Float16, 128, 4>::Params&, float*, float*, dim3, int, hipStream_t);
template int launch_varblock_lockstep_lse<_Float16, 64>(const VarblockPolicy<_Float16, 64, 4>::Params&, float*, float*, dim3, int, hipStream_t);
template int launch_varblock_pp2_lse_d64<__bf16>(const VarblockPolicy<__bf16, 64, 8>::Params&, float*, float*, dim3, int, hipStream_t);
template int launch_varblock_pp2_lse_d64<_Float16>(const VarblockPolicy<_Float16, 64, 8>::Params&, float*, float*, dim3, int, hipStream_t);

}  // namespace svg

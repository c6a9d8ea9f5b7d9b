// flash-kmeans by direction (include/svg_attn_kmeans_metric.h): the centroid update of the cosine and dot-product metrics and the
// initial normalisation of the cosine loop.  ref: triton_centroid_update_cosine, svg/kmeans_utils.py:143-190 (sums by atomics, then
// `sums / counts`, `.to(x.dtype)`, F.normalize) and batch_kmeans_Cosine :769.  The assignment of both metrics is the bias-free form of
// kmeans_assign_kernel and the loop is kmeans_loop_run on a record with a metric: both in csrc/kmeans.hip.
// This file is built with IEEE arithmetic (build.py STRICT_FP: no fast-math, no contraction; correctly rounded sqrt and division):
// every norm and quotient below is what the float64 statement of tests/test_gpu_kmeans_metric.py rounds, and scaling a row by a power
// of two scales its weight by the inverse power exactly.
#include <algorithm>

#include "kmeans_metric.h"

extern "C" int svg_argsort_labels(const int32_t* labels, int32_t* sorted_idx, int32_t* counts, int32_t B, int32_t N, int32_t K,
                                  void* workspace, size_t workspace_bytes, void* stream);

namespace svg {

// max(n, 1e-12) that keeps a NaN norm, as torch's clamp_min does (fmaxf would drop it)
__device__ __forceinline__ float norm_floor(float n) { return n < 1e-12f ? 1e-12f : n; }

// |row|^2 of a row held by LPR consecutive lanes, 8 elements each, in every one of them.  The order is fixed: a lane's eight squares
// ascending, then the lanes pairwise by exchange — li ^ 1, li ^ 2, li ^ 4 (, li ^ 8): both partners of a step add the same two numbers, so
// all lanes of the row end on the same bits.  No LDS, no barrier; the lanes of a row always take the same branches.
template <int LPR>
__device__ __forceinline__ float row_sumsq(const float (&f)[8]) {
    float ss = f[0] * f[0];
#pragma unroll
    for (int j = 1; j < 8; ++j) ss += f[j] * f[j];
#pragma unroll
    for (int o = 1; o < LPR; o <<= 1) ss += __shfl_xor(ss, o);
    return ss;
}

// acc += w x for the lane's eight elements of one row; kUnitRows: w = 1 / max(|x|, 1e-12) from the registers that hold the row (no
// |x|^2 pass over x, no [B, N] weight buffer), the product rounded to fp32 and then added; otherwise w = 1
template <typename T, int LPR, bool kUnitRows>
__device__ __forceinline__ void sphere_add_row(float (&acc)[8], const typename Elt<T>::v8& v) {
    float f[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) f[j] = Elt<T>::to_float(v[j]);
    if constexpr (kUnitRows) {
        const float w = 1.f / norm_floor(sqrtf(row_sumsq<LPR>(f)));
#pragma unroll
        for (int j = 0; j < 8; ++j) acc[j] += w * f[j];
    } else {
#pragma unroll
        for (int j = 0; j < 8; ++j) acc[j] += f[j];
    }
}

// ---- weighted, normalising centroid update: the work split of kmeans_update_kernel (csrc/kmeans.hip) — grid = (groups, B), block = 256 =
// 16 row slots x 16 lanes (D = 128) / 32 x 8 (D = 64), a workgroup walks clusters k = blockIdx.x, + gridDim.x, ... of its batch, four rows
// per slot in flight, the next cluster's count, offset and first indices fetched while the current one is summed.  A slot adds its rows
// slot, slot + SLOTS, ... in that order whichever path loads them, the slots are added 0, 1, ... per channel.
// Epilogue, per cluster: the D threads that hold m (the mean, or the old centroid of an empty cluster, ROUNDED to T) reduce |m|^2 over
// the workgroup (wave_sum: exchange steps 32, 16, ..., 1; then the waves' words nrm[0] + nrm[1] + nrm[2] + nrm[3]), divide, round, store, and
// form the shift from the value they stored.
template <typename T, int D, bool kUnitRows>
__global__ __launch_bounds__(256) void kmeans_update_sphere_kernel(const T* __restrict__ x, const T* __restrict__ c_old,
                                                                   T* __restrict__ c_new, const int32_t* __restrict__ sorted_idx,
                                                                   const int32_t* __restrict__ offsets /* [B][nchunks][K], chunk 0 */,
                                                                   const int32_t* __restrict__ counts, float* __restrict__ shift, int N,
                                                                   int K, size_t off_batch_stride, long long x_bs) {
    constexpr int LPR = D / 8;
    constexpr int SLOTS = 256 / LPR;
    __shared__ float red[SLOTS][D + 4];
    __shared__ float nrm[4], dsq[4];
    const int b = blockIdx.y, tid = threadIdx.x;
    const int slot = tid / LPR, li = tid - slot * LPR;
    const T* xb = x + (size_t)b * (size_t)x_bs;
    const int32_t* sidx_b = sorted_idx + (size_t)b * N;
    using V8 = typename Elt<T>::v8;
    int k = blockIdx.x;
    if (k >= K) return;
    int cnt = counts[(size_t)b * K + k];
    int start = offsets[(size_t)b * off_batch_stride + k];
    int pre[4];     // the slot's first four row indices of the cluster (rows slot, slot + SLOTS, ...)
#pragma unroll
    for (int u = 0; u < 4; ++u) pre[u] = (slot + u * SLOTS < cnt) ? sidx_b[start + slot + u * SLOTS] : 0;
    for (;;) {
        const int kn = k + (int)gridDim.x;
        int cnt_n = 0, start_n = 0;
        if (kn < K) {
            cnt_n = counts[(size_t)b * K + kn];
            start_n = offsets[(size_t)b * off_batch_stride + kn];
        }
        const int32_t* sidx = sidx_b + start;
        float acc[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) acc[j] = 0.f;
        int r = slot;
        if (r + 3 * SLOTS < cnt) {     // the first batch of four: its indices are here already
            V8 v[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) v[u] = *(const V8*)(xb + (size_t)pre[u] * D + li * 8);
#pragma unroll
            for (int u = 0; u < 4; ++u) sphere_add_row<T, LPR, kUnitRows>(acc, v[u]);
            r += 4 * SLOTS;
            for (; r + 3 * SLOTS < cnt; r += 4 * SLOTS) {
                int row[4];
#pragma unroll
                for (int u = 0; u < 4; ++u) row[u] = sidx[r + u * SLOTS];
#pragma unroll
                for (int u = 0; u < 4; ++u) v[u] = *(const V8*)(xb + (size_t)row[u] * D + li * 8);
#pragma unroll
                for (int u = 0; u < 4; ++u) sphere_add_row<T, LPR, kUnitRows>(acc, v[u]);
            }
            for (; r < cnt; r += SLOTS) sphere_add_row<T, LPR, kUnitRows>(acc, *(const V8*)(xb + (size_t)sidx[r] * D + li * 8));
        } else {                       // at most three rows for this slot, all of them prefetched
            V8 v[3];
#pragma unroll
            for (int u = 0; u < 3; ++u)
                if (slot + u * SLOTS < cnt) v[u] = *(const V8*)(xb + (size_t)pre[u] * D + li * 8);
#pragma unroll
            for (int u = 0; u < 3; ++u)
                if (slot + u * SLOTS < cnt) sphere_add_row<T, LPR, kUnitRows>(acc, v[u]);
        }
        // the next cluster's first indices: in flight during the reduction below
        if (kn < K) {
#pragma unroll
            for (int u = 0; u < 4; ++u) pre[u] = (slot + u * SLOTS < cnt_n) ? sidx_b[start_n + slot + u * SLOTS] : 0;
        }
#pragma unroll
        for (int j = 0; j < 8; ++j) red[slot][li * 8 + j] = acc[j];
        __syncthreads();                                                   // (1) red is complete
        float mf = 0.f, oldv = 0.f;
        const size_t o = ((size_t)b * K + k) * D + (tid < D ? tid : 0);
        if (tid < D) {
            float s = 0.f;
            for (int sl = 0; sl < SLOTS; ++sl) s += red[sl][tid];          // fixed order -> deterministic
            const T old = c_old[o];
            oldv = Elt<T>::to_float(old);
            // ref: svg/kmeans_utils.py:180-188 sums / clamp(count, 1), an empty cluster takes the old centroid, cast to x.dtype
            mf = Elt<T>::to_float(cnt > 0 ? Elt<T>::from_float(s / (float)cnt) : old);
        }
        const float msq = wave_sum(mf * mf);                               // (threads at or behind D add zeros)
        if ((tid & 63) == 0) nrm[tid >> 6] = msq;
        __syncthreads();                                                   // (2) nrm is complete
        float d2 = 0.f;
        if (tid < D) {
            const float den = norm_floor(sqrtf(nrm[0] + nrm[1] + nrm[2] + nrm[3]));   // ref :189 F.normalize(centroids, p=2, dim=-1)
            const T nv = Elt<T>::from_float(mf / den);
            c_new[o] = nv;
            const float df = Elt<T>::to_float(Elt<T>::from_float(Elt<T>::to_float(nv) - oldv));   // the shift of kmeans_update_kernel
            d2 = df * df;
        }
        d2 = wave_sum(d2);
        if ((tid & 63) == 0) dsq[tid >> 6] = d2;
        __syncthreads();                                                   // (3) dsq is complete
        if (tid == 0) {
            const float nr = sqrtf(dsq[0] + dsq[1] + dsq[2] + dsq[3]);
            // (the NaN rule of kmeans_update_kernel: non-negative floats and the canonical NaN order like ints)
            atomicMax((int*)(shift + b), nr != nr ? 0x7FC00000 : __float_as_int(nr));
        }
        if (kn >= K) break;
        k = kn, cnt = cnt_n, start = start_n;
        // Reuse of red / nrm / dsq by the next cluster, three barriers per cluster (one more than kmeans_update_kernel: the norm has to be
        // known before the value whose shift is taken exists):
        //   red: read between (1) and (2); its next writer stands behind (3) of this cluster, so every thread has passed (2);
        //   nrm: read between (2) and (3); its next writer stands behind (1) of the next cluster, so every thread has passed (3);
        //   dsq: read by tid 0 behind (3), before tid 0 arrives at (1) of the next cluster; its next writer stands behind (2) of the
        //        next cluster, which tid 0 has then passed as well.
    }
}

// c[r] -> the unit row c[r] / max(|c[r]|, 1e-12), rounded once (batch_kmeans_Cosine's F.normalize of the initial centroids, ref :769):
// 16 / 8 lanes per row, |c|^2 by row_sumsq
template <typename T, int D>
__global__ __launch_bounds__(256) void kmeans_unit_rows_kernel(const T* __restrict__ c, T* __restrict__ out, long long rows) {
    constexpr int LPR = D / 8, RPB = 256 / LPR;
    using V8 = typename Elt<T>::v8;
    const int sub = threadIdx.x / LPR, li = threadIdx.x - sub * LPR;
    // (whole passes of the workgroup: the lanes of a row leave the loop together)
    for (long long r = (long long)blockIdx.x * RPB + sub; r < rows; r += (long long)gridDim.x * RPB) {
        const V8 v = *(const V8*)(c + r * D + li * 8);
        float f[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) f[j] = Elt<T>::to_float(v[j]);
        const float den = norm_floor(sqrtf(row_sumsq<LPR>(f)));
        V8 w;
#pragma unroll
        for (int j = 0; j < 8; ++j) w[j] = Elt<T>::from_float(f[j] / den);
        *(V8*)(out + r * D + li * 8) = w;
    }
}

// (instead of a memset node: the loop may be captured into a graph)
__global__ __launch_bounds__(256) void kmeans_clear_shift_kernel(float* __restrict__ shift, int B) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i < B) shift[i] = 0.f;
}

int run_kmeans_update_metric(const KmeansCall& a, const KmeansStep& s) {
    const int B = a.B, N = a.N, K = a.K;
    if (const int rc = svg_argsort_labels(s.labels, s.sorted_idx, s.counts, B, N, K, s.ws.sort, s.ws.sort_bytes, (void*)a.st); rc) return rc;
    hipLaunchKernelGGL(kmeans_clear_shift_kernel, dim3((B + 255) / 256), dim3(256), 0, a.st, s.shift, B);
    const int nchunks = (N + 1023) / 1024;
    const int groups = std::max(1, std::min(K, (3 * kNumCU + B - 1) / B));   // (the workgroups per batch of kmeans_update_kernel)
    return dispatch_td(a.dtype, a.D, [&](auto t, auto d) {
        using T = decltype(t);
        constexpr int DD = decltype(d)::value;
        auto launch = [&](auto kern) {
            hipLaunchKernelGGL(kern, dim3(groups, B), dim3(256), 0, a.st, (const T*)a.x, (const T*)s.c_in, (T*)s.c_out, s.sorted_idx,
                               (const int32_t*)s.ws.sort, s.counts, s.shift, N, K, (size_t)nchunks * K, a.x_bs);
        };
        if (a.metric == SVG_KMEANS_COSINE)
            launch(kmeans_update_sphere_kernel<T, DD, true>);
        else
            launch(kmeans_update_sphere_kernel<T, DD, false>);
        return launch_status();
    });
}

int run_kmeans_unit_rows(const KmeansCall& a, void* out) {
    const long long rows = (long long)a.B * a.K;
    return dispatch_td(a.dtype, a.D, [&](auto t, auto d) {
        using T = decltype(t);
        constexpr int DD = decltype(d)::value;
        constexpr int RPB = 256 / (DD / 8);
        hipLaunchKernelGGL((kmeans_unit_rows_kernel<T, DD>), dim3((unsigned)std::min<long long>(2048, (rows + RPB - 1) / RPB)), dim3(256), 0, a.st,
                           (const T*)a.c_init, (T*)out, rows);
        return launch_status();
    });
}

}  // namespace svg

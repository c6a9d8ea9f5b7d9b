// flash-kmeans for gfx950: one Lloyd iteration of batched Euclidean k-means, entirely on device.
// ref: batch_kmeans_Euclid / _euclid_iter, svg/kmeans_utils.py:629-643,684-733
//      assign kernel  _euclid_assign_kernel             svg/kmeans_utils.py:464-554
//      centroid update (sorted, chunked)                svg/kmeans_utils.py:258-322,375-421
//
//   assign : S^T[c][n] = <C[c], X[n]> on MFMA 32x32x16 (A = centroid tile from LDS, B = point fragments in
//            registers, exactly the S^T half of attn_core.h), dist = max(0, xsq[n] + csq[c] - 2 S), running
//            (min, argmin) per lane, lowest index wins exact ties like the reference's strict '<' across chunks and
//            first-index argmin inside a chunk.  The N x K distance matrix is never materialised.
//   update : stable counting sort of the labels (permute.hip) -> every cluster is a contiguous run of
//            sorted_idx; one workgroup per (batch, cluster) gathers its rows and reduces them in a FIXED order
//            (fp32), so centroids are bit-reproducible run to run (the reference's atomics are not).
#include <algorithm>

#include "attn_f8.h"

extern "C" size_t svg_argsort_workspace_bytes(int32_t B, int32_t N, int32_t K);
extern "C" int svg_argsort_labels(const int32_t* labels, int32_t* sorted_idx, int32_t* counts, int32_t B, int32_t N,
                                  int32_t K, void* workspace, size_t workspace_bytes, void* stream);

namespace svg {

// ---- ||x||^2 exactly like the reference: (x**2) rounded to the input dtype, summed in fp32, rounded to dtype ----
// ref: svg/kmeans_utils.py:704 `x_sq = (x**2).sum(dim=-1)` on a bf16 tensor, :512 cast to fp32 in the kernel
template <typename T>
__global__ __launch_bounds__(256) void xsq_kernel(const T* __restrict__ x, float* __restrict__ xsq, long long rows, int D) {
    const int lpr = D / 8;                       // lanes per row (8 elements = 16 B each)
    const int rpb = 256 / lpr;                   // rows per block pass
    const int sub = threadIdx.x / lpr, li = threadIdx.x - sub * lpr;
    for (long long r = (long long)blockIdx.x * rpb + sub; r < rows; r += (long long)gridDim.x * rpb) {
        const typename Elt<T>::v8 v = *(const typename Elt<T>::v8*)(x + r * D + li * 8);
        float s = 0.f;
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const float f = Elt<T>::to_float(v[j]);
            s += Elt<T>::to_float(Elt<T>::from_float(f * f));
        }
        for (int o = lpr >> 1; o >= 1; o >>= 1) s += __shfl_xor(s, o);
        if (li == 0) xsq[r] = Elt<T>::to_float(Elt<T>::from_float(s));
    }
}

// ---- ||c||^2: products rounded to the input dtype, fp32 sum (ref: svg/kmeans_utils.py:531) ----
template <typename T>
__global__ __launch_bounds__(256) void csq_kernel(const T* __restrict__ c, float* __restrict__ csq, long long rows, int D) {
    const int lpr = D / 8;
    const int rpb = 256 / lpr;
    const int sub = threadIdx.x / lpr, li = threadIdx.x - sub * lpr;
    for (long long r = (long long)blockIdx.x * rpb + sub; r < rows; r += (long long)gridDim.x * rpb) {
        const typename Elt<T>::v8 v = *(const typename Elt<T>::v8*)(c + r * D + li * 8);
        float s = 0.f;
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const float f = Elt<T>::to_float(v[j]);
            s += Elt<T>::to_float(Elt<T>::from_float(f * f));
        }
        for (int o = lpr >> 1; o >= 1; o >>= 1) s += __shfl_xor(s, o);
        if (li == 0) csq[r] = s;
    }
}

#ifdef SVG_KMEANS_TRACE
static __device__ unsigned long long g_km_trace[8 * 8];   // diagnostics build: per wave of workgroup (7, 0): cycles in { init, mfma, epilogue, stage, barrier }, tiles
#endif
// ---- assignment: grid = (ceil(N / (NW*32)), B), block = NW*64 ----
template <typename T, int D, int NW>
__global__ __launch_bounds__(NW * 64, 2) void kmeans_assign_kernel(const T* __restrict__ x, const T* __restrict__ cent,
                                                                    const float* __restrict__ xsq,
                                                                    const float* __restrict__ csq, int32_t* __restrict__ labels,
                                                                    int N, int K, long long x_bs /* elements between the batches of x */) {
    using E = Elt<T>;
    using V8 = typename E::v8;
    using L = LdsLayout<D>;
    constexpr int NT = NW * 64;
    constexpr int KS = D / 16;
    constexpr int NCH = (kBN * L::kCPR) / NT;
    constexpr int kStage = L::kKBytes + kBN * 4;  // centroid tile + its 64 squared norms
    extern __shared__ __attribute__((aligned(16))) char smem[];

    const int b = blockIdx.y;
    const int tid = threadIdx.x, lane = tid & 63, wave = wave_id();
    const int g = lane >> 5, ql = lane & 31;
    const int n = blockIdx.x * (NW * 32) + wave * 32 + ql;
    const T* xb = x + (size_t)b * (size_t)x_bs;
    const T* cb = cent + (size_t)b * K * D;
    const float* csqb = csq + (size_t)b * K;

    V8 xf[KS];
    {
        const T* xrow = xb + (size_t)(n < N ? n : 0) * D + g * 8;
#pragma unroll
        for (int ks = 0; ks < KS; ++ks) xf[ks] = *(const V8*)(xrow + ks * 16);
    }
    (void)xsq;   // |x|^2 does not change the argmin; the parameter stays for the callers that keep the distance form

    int srow[NCH], scol[NCH], k_dst[NCH];
#pragma unroll
    for (int i = 0; i < NCH; ++i) {
        const int id = tid + i * NT;
        srow[i] = id / L::kCPR;
        scol[i] = id - srow[i] * L::kCPR;
        k_dst[i] = L::k_off(srow[i], scol[i]);
    }
    u32x4 creg[NCH];
    float sreg = 0.f;
    bool sreg_ok = false;
    const int nT = (K + kBN - 1) / kBN;
    auto issue = [&](int t) {
#pragma unroll
        for (int i = 0; i < NCH; ++i) {
            const int c = t * kBN + srow[i];
            creg[i] = *(const u32x4*)(cb + (size_t)(c < K ? c : 0) * D + scol[i] * 8);
        }
        if (tid < kBN) {   // |c|^2, RAW: the multiply sits in write() — used here it makes hipcc wait (vmcnt(0)) for the loads it has just issued
            const int c = t * kBN + tid;
            sreg = csqb[c < K ? c : 0];
            sreg_ok = c < K;
        }
    };
    auto write = [&](int buf) {
        char* base = smem + buf * kStage;
#pragma unroll
        for (int i = 0; i < NCH; ++i) *(u32x4*)(base + k_dst[i]) = creg[i];
        // -|c|^2 / 2 (the accumulator's start value, see below); centroids behind K can never win
        if (tid < kBN) *(float*)(base + L::kKBytes + tid * 4) = sreg_ok ? -0.5f * sreg : -INFINITY;
    };

    issue(0);
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) asm volatile("" : "+v"(xf[ks]));
    write(0);
    if (nT > 1) issue(1);
    __syncthreads();

    const int ksw0 = (D == 128) ? (ql & 15) : ((ql >> 1) & 7);
    // argmin_c |x - c|^2 = argmax_c (x.c - |c|^2 / 2): the accumulators start at -|c|^2 / 2, so an element of the epilogue is a
    // compare and two selects (the distance form — fma, clamp, bounds test, compare, two selects — made this kernel VALU-bound:
    // 192 VALU against 16 MFMAs per tile).  Ties keep the lowest index, like argmin.
    // Round 5 (profiles/r05r_kmeans_assign_trace.txt, r05j_ab_kmeans_assign.txt; labels bit-identical throughout).  The per-phase trace (-DSVG_KMEANS_TRACE) found
    // the MFMA phase at 1050 - 1240 cycles for 512 of matrix work (one fragment pair in flight) and the loads of tile t + 2 waited out in the iteration that
    // issued them (the -|c|^2 / 2 multiply consumed its load at once): both fixed below — 3040 -> 2640 cycles per tile, 0.55 -> 0.525 ms per call.  What bounds
    // the kernel now is the arg-max epilogue: per SIMD and tile four waves need 2048 cycles of matrix pipe and ~4000 of vector issue (3 VALU per score).
    // Measured and removed: a second score set (168 registers: slower), a half-tile pipeline, 128-centroid stages (no gain: neither overlap nor the
    // barrier was the problem).
    float best = -INFINITY;
    int best_idx = 0;
#ifdef SVG_KMEANS_TRACE
    unsigned long long tr[5] = {0, 0, 0, 0, 0}, tl = __builtin_amdgcn_s_memtime();
#define KM_TICK(i) { const unsigned long long now_ = __builtin_amdgcn_s_memtime(); tr[i] += now_ - tl; tl = now_; }
#else
#define KM_TICK(i)
#endif
    for (int t = 0; t < nT; ++t) {
        const int buf = t & 1;
        const char* kbuf = smem + buf * kStage;
        const float* h_t = (const float*)(kbuf + L::kKBytes);
        f32x16 s[2];
#pragma unroll
        for (int bb = 0; bb < 2; ++bb)
#pragma unroll
            for (int rq = 0; rq < 4; ++rq) {
                const f32x4 h4 = *(const f32x4*)(h_t + 32 * bb + 8 * rq + 4 * g);
#pragma unroll
                for (int j = 0; j < 4; ++j) s[bb][rq * 4 + j] = h4[j];
            }
        float tb;
        int ti;
        KM_TICK(0)
        // centroid fragments two k-steps ahead of their MFMAs (hipcc's own schedule kept ONE pair in flight and waited for it in front of
        // every MFMA: 1050 - 1240 cycles for 512 cycles of matrix work per tile, profiles/r05r_kmeans_assign_trace.txt)
        constexpr int kAhead = 2;
        V8 af[kAhead + 1][2];
        auto afetch = [&](int ks) {
            const int cch = ((2 * ks + g) ^ ksw0) << 4;
#pragma unroll
            for (int bb = 0; bb < 2; ++bb) af[ks % (kAhead + 1)][bb] = *(const V8*)(kbuf + (32 * bb + ql) * L::kRowBytes + cch);
        };
#pragma unroll
        for (int ks = 0; ks < kAhead; ++ks) afetch(ks);
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int ks = 0; ks < KS; ++ks) {
            if (ks + kAhead < KS) afetch(ks + kAhead);
#pragma unroll
            for (int bb = 0; bb < 2; ++bb) s[bb] = E::mfma(af[ks % (kAhead + 1)][bb], xf[ks], s[bb]);
            __builtin_amdgcn_sched_barrier(0);
        }
#ifdef SVG_KMEANS_TRACE
        asm volatile("" : "+v"(s[0]), "+v"(s[1]));
#endif
        KM_TICK(1)
        // four independent chains of eight elements (ascending index inside a chain), merged in index order with the same strict compare:
        // the result of the one 32-step chain — lowest index wins ties — at a quarter of its dependent latency (3 dependent VALU per step:
        // 665 - 860 cycles per tile in the trace)
        float cb_[4];
        int ci_[4];
#pragma unroll
        for (int ch = 0; ch < 4; ++ch) {
            const int bb = ch >> 1, r0 = (ch & 1) * 8;
            cb_[ch] = s[bb][r0];
            ci_[ch] = 32 * bb + 8 * (r0 >> 2) + (r0 & 3) + 4 * g;
#pragma unroll
            for (int r = r0 + 1; r < r0 + 8; ++r) {
                const int c = 32 * bb + 8 * (r >> 2) + (r & 3);   // + 4 g: tile-local centroid index, ascending in (bb, r)
                const bool upd = s[bb][r] > cb_[ch];
                cb_[ch] = upd ? s[bb][r] : cb_[ch];
                ci_[ch] = upd ? c + 4 * g : ci_[ch];
            }
        }
        tb = cb_[0];
        ti = ci_[0];
#pragma unroll
        for (int ch = 1; ch < 4; ++ch) {
            const bool upd = cb_[ch] > tb;
            tb = upd ? cb_[ch] : tb;
            ti = upd ? ci_[ch] : ti;
        }
        const bool upd = tb > best;
        best = upd ? tb : best;
        best_idx = upd ? t * kBN + ti : best_idx;
#ifdef SVG_KMEANS_TRACE
        asm volatile("" : "+v"(best), "+v"(best_idx));
#endif
        KM_TICK(2)
        if (t + 1 < nT) write(buf ^ 1);
        if (t + 2 < nT) issue(t + 2);
        KM_TICK(3)
        __syncthreads();
        KM_TICK(4)
    }
#ifdef SVG_KMEANS_TRACE
    if (blockIdx.x == 7 && blockIdx.y == 0 && lane == 0) {
        for (int i = 0; i < 5; ++i) g_km_trace[wave * 8 + i] = tr[i];
        g_km_trace[wave * 8 + 5] = (unsigned long long)nT;
    }
#endif
    // the two lanes of a point cover disjoint centroid subsets: merge, lowest index wins ties
    const float ob = __shfl_xor(best, 32);
    const int oi = __shfl_xor(best_idx, 32);
    if (ob > best || (ob == best && oi < best_idx)) best = ob, best_idx = oi;
    if (g == 0 && n < N) labels[(size_t)b * N + n] = best_idx;
}

// ---- centroid update: grid = (groups, B), block = 256 = 16 row slots x 16 lanes (D = 128) / 32 x 8 (D = 64); a workgroup walks clusters
// k = blockIdx.x, + gridDim.x, ... of its batch.  (Until round 5 one workgroup per cluster: at K = 1000 that is 40000 workgroups of ~75 rows whose
// lifetime is three dependent latencies — count / offset, row indices, rows — 0.36 ms per call at Wan 720p where the K = 300 side, HBM-bound, takes
// 0.16.  Now the next cluster's count, offset and first four row indices per slot are fetched while the current one is summed.  The order of every
// sum is unchanged: the same bits.)
template <typename T, int D>
__global__ __launch_bounds__(256) void kmeans_update_kernel(const T* __restrict__ x, const T* __restrict__ c_old,
                                                            T* __restrict__ c_new, const int32_t* __restrict__ sorted_idx,
                                                            const int32_t* __restrict__ offsets /* [B][nchunks][K], chunk 0 */,
                                                            const int32_t* __restrict__ counts, float* __restrict__ shift,
                                                            int N, int K, size_t off_batch_stride, long long x_bs) {
    constexpr int LPR = D / 8;
    constexpr int SLOTS = 256 / LPR;
    __shared__ float red[SLOTS][D + 4];
    __shared__ float nrm[4];
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
        // four rows of a slot in flight (index loads, then row loads); summed in the order a one-row loop sums them
        int r = slot;
        {
#pragma clang fp reassociate(off)
            if (r + 3 * SLOTS < cnt) {     // the first batch: its indices are here already
                V8 v[4];
#pragma unroll
                for (int u = 0; u < 4; ++u) v[u] = *(const V8*)(xb + (size_t)pre[u] * D + li * 8);
#pragma unroll
                for (int u = 0; u < 4; ++u)
#pragma unroll
                    for (int j = 0; j < 8; ++j) acc[j] += Elt<T>::to_float(v[u][j]);
                r += 4 * SLOTS;
                for (; r + 3 * SLOTS < cnt; r += 4 * SLOTS) {
                    int row[4];
#pragma unroll
                    for (int u = 0; u < 4; ++u) row[u] = sidx[r + u * SLOTS];
#pragma unroll
                    for (int u = 0; u < 4; ++u) v[u] = *(const V8*)(xb + (size_t)row[u] * D + li * 8);
#pragma unroll
                    for (int u = 0; u < 4; ++u)
#pragma unroll
                        for (int j = 0; j < 8; ++j) acc[j] += Elt<T>::to_float(v[u][j]);
                }
                for (; r < cnt; r += SLOTS) {
                    const V8 w = *(const V8*)(xb + (size_t)sidx[r] * D + li * 8);
#pragma unroll
                    for (int j = 0; j < 8; ++j) acc[j] += Elt<T>::to_float(w[j]);
                }
            } else {                       // at most three rows for this slot, all of them prefetched
                V8 v[3];
#pragma unroll
                for (int u = 0; u < 3; ++u)
                    if (slot + u * SLOTS < cnt) v[u] = *(const V8*)(xb + (size_t)pre[u] * D + li * 8);
#pragma unroll
                for (int u = 0; u < 3; ++u)
                    if (slot + u * SLOTS < cnt) {
#pragma unroll
                        for (int j = 0; j < 8; ++j) acc[j] += Elt<T>::to_float(v[u][j]);
                    }
            }
        }
        // the next cluster's first indices: in flight during the reduction below
        if (kn < K) {
#pragma unroll
            for (int u = 0; u < 4; ++u) pre[u] = (slot + u * SLOTS < cnt_n) ? sidx_b[start_n + slot + u * SLOTS] : 0;
        }
#pragma unroll
        for (int j = 0; j < 8; ++j) red[slot][li * 8 + j] = acc[j];
        __syncthreads();
        float d2 = 0.f;
        if (tid < D) {
            float s = 0.f;
            for (int sl = 0; sl < SLOTS; ++sl) s += red[sl][tid];  // fixed order -> deterministic
            const size_t o = ((size_t)b * K + k) * D + tid;
            const float oldv = Elt<T>::to_float(c_old[o]);
            // ref: svg/kmeans_utils.py:416-421 sums / clamp(count,1), empty cluster keeps the old centroid, cast to x.dtype
            const T nv = cnt > 0 ? Elt<T>::from_float(s / (float)cnt) : c_old[o];
            c_new[o] = nv;
            const float df = Elt<T>::to_float(Elt<T>::from_float(Elt<T>::to_float(nv) - oldv));
            d2 = df * df;
        }
        d2 = wave_sum(d2);
        if ((tid & 63) == 0) nrm[tid >> 6] = d2;
        __syncthreads();
        if (tid == 0) {
            const float nr = sqrtf(nrm[0] + nrm[1] + nrm[2] + nrm[3]);
            // non-negative floats order like ints, and so does a NaN whose sign bit is clear — above all of them; one whose sign bit is set
            // (it keeps the sign of the input's) is a negative int and would lose against the 0 the shift starts from: the canonical NaN
            atomicMax((int*)(shift + b), nr != nr ? 0x7FC00000 : __float_as_int(nr));
        }
        if (kn >= K) break;
        k = kn, cnt = cnt_n, start = start_n;
        // (red / nrm of this cluster are read before the barriers above; the next writes to red come after the second one, the next write to
        //  nrm after the next cluster's first barrier: tid 0 has read nrm by then only if it passed that barrier too — it has: same barrier)
    }
}

// the two halves of an iteration (the reference's euclid_assign_triton / triton_centroid_update_sorted_euclid, svg/kmeans_utils.py:562-627,
// 375-421) as host functions of their own: svg_kmeans_iter runs one after the other, svg_kmeans_assign / svg_kmeans_update expose them
template <typename T, int D>
static int run_kmeans_assign(const void* x, const float* xsq, const void* c_in, int32_t* labels, int B, int N, int K, void* ws,
                             hipStream_t st, long long x_bs) {
    constexpr int NW = 8;
    float* csq = (float*)ws;
    hipLaunchKernelGGL((csq_kernel<T>), dim3(std::min<long long>(2048, ((long long)B * K + 15) / 16)), dim3(256), 0, st,
                       (const T*)c_in, csq, (long long)B * K, D);
    constexpr int lds = 2 * (LdsLayout<D>::kKBytes + kBN * 4);
    auto kern = kmeans_assign_kernel<T, D, NW>;
    hipLaunchKernelGGL(kern, dim3((N + NW * 32 - 1) / (NW * 32), B), dim3(NW * 64), lds, st, (const T*)x, (const T*)c_in, xsq,
                       csq, labels, N, K, x_bs);
    return launch_status();
}

template <typename T, int D>
static int run_kmeans_update(const void* x, const void* c_in, void* c_out, const int32_t* labels, int32_t* counts, int32_t* sorted_idx,
                             float* shift, int B, int N, int K, void* ws, hipStream_t st, long long x_bs) {
    const size_t csq_bytes = ((size_t)B * K * sizeof(float) + 255) / 256 * 256;
    char* sort_ws = (char*)ws + csq_bytes;
    const size_t sort_bytes = svg_argsort_workspace_bytes(B, N, K);
    int rc = svg_argsort_labels(labels, sorted_idx, counts, B, N, K, sort_ws, sort_bytes, (void*)st);
    if (rc) return rc;
    (void)hipMemsetAsync(shift, 0, (size_t)B * sizeof(float), st);
    const int nchunks = (N + 1023) / 1024;
    // workgroups per batch: three per CU over the whole launch.  Measured at Wan 720p (40 heads, K = 300 and 1000 on two streams, the 2-iteration
    // stage): 6 per head 3.49 ms, 8 3.27, 12 3.14, 16 3.05, 20 3.02, 26 3.13, 32 3.17, 52 3.22, 100 3.36, one per cluster 3.37; the kernel of
    // round 4 (one workgroup per cluster, no prefetch) 3.39 (profiles/r05zw_kmeans_update_groups.txt).
    const int groups = std::max(1, std::min(K, (3 * kNumCU + B - 1) / B));
    hipLaunchKernelGGL((kmeans_update_kernel<T, D>), dim3(groups, B), dim3(256), 0, st, (const T*)x, (const T*)c_in, (T*)c_out,
                       sorted_idx, (const int32_t*)sort_ws, counts, shift, N, K, (size_t)nchunks * K, x_bs);
    return launch_status();
}

template <typename T, int D>
static int run_kmeans_iter(const void* x, const float* xsq, const void* c_in, void* c_out, int32_t* labels, int32_t* counts,
                           int32_t* sorted_idx, float* shift, int B, int N, int K, void* ws, size_t ws_bytes,
                           hipStream_t st, long long x_bs) {
    (void)ws_bytes;
    if (const int rc = run_kmeans_assign<T, D>(x, xsq, c_in, labels, B, N, K, ws, st, x_bs); rc != SVG_OK) return rc;
    return run_kmeans_update<T, D>(x, c_in, c_out, labels, counts, sorted_idx, shift, B, N, K, ws, st, x_bs);
}

// ---- the Lloyd loop on the device (svg_kmeans_loop[_grouped]): commit of one iteration's result under the reference's stopping rule ----
// The B batches form G stopping groups of `group` consecutive batches each (svg_kmeans_loop: one group of all B).  State words, G of
// each kind: state[0 .. 2G): "the reference's loop has left" before iteration `it` (ping-pong by iteration parity: every thread of the
// commit kernel reads the flags of the iteration before, one thread per group writes the flag for the next), state[2G + g]: n_iters of
// group g, state[3G + g]: which centroid buffer holds group g's result (0 initial, 1 / 2 the two work buffers).  With G = 1 this is the
// layout of the ungrouped loop: [flag0, flag1, n_iters, selector].
// kGivenMaxima = false: `shift` is the float [B] of the iteration and the group maxima are reduced here (svg_kmeans_loop*);
// true: `shift` is the float [G] of group maxima the caller hands in (svg_kmeans_stepped_commit: a collective may have sat between the
// iteration and this launch) — the same rule, `conv = !(m != m) && m < tol`, applied to it.
template <bool kGivenMaxima>
__global__ __launch_bounds__(256) void kmeans_commit_kernel(const int32_t* __restrict__ labels, const int32_t* __restrict__ sorted_idx,
                                                            const int32_t* __restrict__ counts, int32_t* __restrict__ labels_r,
                                                            int32_t* __restrict__ sorted_r, int32_t* __restrict__ counts_r,
                                                            const float* __restrict__ shift, int32_t* __restrict__ state, long long gn,
                                                            long long gk, int group, float tol, int it, int sel_cur, int sel_out) {
    const int G = gridDim.y, gy = blockIdx.y;   // blockIdx.y: the group whose rows this workgroup copies
    const int32_t* stopped_in = state + (it & 1) * G;
    if (stopped_in[gy] == 0) {   // ref svg/kmeans_utils.py:716-733: the labels / sizes of the iteration a group's loop is in are its result
        const long long n0 = gy * gn, k0 = gy * gk;
        for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < gn; i += (long long)gridDim.x * 256) {
            labels_r[n0 + i] = labels[n0 + i];
            sorted_r[n0 + i] = sorted_idx[n0 + i];
        }
        for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < gk; i += (long long)gridDim.x * 256) counts_r[k0 + i] = counts[k0 + i];
    }
    if (blockIdx.x == 0 && gy == 0) {   // the stopping rule, one wave per group (waves take groups w, w + 4, ...)
        const int lane = threadIdx.x & 63;
        for (int g = threadIdx.x >> 6; g < G; g += 4) {
            float mx = 0.f;
            bool nan = false;   // fmaxf drops a NaN operand; the reference's `shift.max()` propagates it, and `NaN < tol` is False (:723)
            if constexpr (kGivenMaxima) {
                mx = shift[g];
                nan = mx != mx;
            } else {
                for (int b = g * group + lane; b < (g + 1) * group; b += 64) {
                    const float sft = shift[b];
                    nan |= sft != sft;
                    mx = fmaxf(mx, sft);
                }
                mx = wave_max(mx);
                nan = __builtin_amdgcn_ballot_w64(nan) != 0ull;
            }
            if (lane == 0) {
                const bool stopped = stopped_in[g] != 0;
                const bool conv = !nan && mx < tol;   // `center_shift < tol` (:723): a NaN shift never converges, the loop runs to max_iters
                if (!stopped) {
                    state[2 * G + g] += 1;
                    state[3 * G + g] = conv ? sel_cur : sel_out;   // converged: the OLD centroids are returned; otherwise the new ones become current
                }
                state[((it + 1) & 1) * G + g] = (stopped || conv) ? 1 : 0;
            }
        }
    }
}
// maxima[g] = the largest shift of group g's batches, a NaN among them propagated as torch.max propagates it (the stepped loop: what
// kmeans_commit_kernel<false> reduces for itself, written out so that the caller can reduce it further).  One wave per group.
__global__ __launch_bounds__(256) void kmeans_group_maxima_kernel(const float* __restrict__ shift, float* __restrict__ maxima, int G, int group) {
    const int lane = threadIdx.x & 63;
    for (int g = blockIdx.x * 4 + (threadIdx.x >> 6); g < G; g += gridDim.x * 4) {
        float mx = 0.f;
        bool nan = false;
        for (int b = g * group + lane; b < (g + 1) * group; b += 64) {
            const float sft = shift[b];
            nan |= sft != sft;
            mx = fmaxf(mx, sft);
        }
        mx = wave_max(mx);
        nan = __builtin_amdgcn_ballot_w64(nan) != 0ull;
        if (lane == 0) maxima[g] = nan ? __builtin_nanf("") : mx;
    }
}
template <typename T>
__global__ __launch_bounds__(256) void kmeans_select_kernel(const T* __restrict__ c0, const T* __restrict__ c1, const T* __restrict__ c2,
                                                            T* __restrict__ out, const int32_t* __restrict__ sel_g, long long group_n8) {
    const int sel = sel_g[blockIdx.y];   // blockIdx.y: the group (its rows are group_n8 8-element vectors)
    const T* src = sel == 0 ? c0 : (sel == 1 ? c1 : c2);
    using V8 = typename Elt<T>::v8;
    const long long o = blockIdx.y * group_n8;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < group_n8; i += (long long)gridDim.x * 256)
        ((V8*)out)[o + i] = ((const V8*)src)[o + i];
}


// =====================================================================================================================================
// e4m3 assignment (include/svg_attn_kmeans_e4m3.h): the scores of kmeans_assign_kernel on v_mfma_scale_f32_32x32x64_f8f6f4 — 4 MFMAs per
// 64-centroid tile in place of 16, at twice the 16-bit rate per MFMA cycle.  Per batch, with a centre mu[128] (fp32; the caller's, or the
// channel mean of the loop's initial centroids — |x - c|^2 does not depend on it, it only keeps a common offset out of the 3-bit mantissa):
//   a row r = x_n - mu or c_k - mu (fp32) is quantised with a power-of-two scale of its own, e = f8_row_exponent(max_d |r_d|),
//   q(r)_d = e4m3_rne(r_d 2^e), and stands for q(r) 2^-e: the exponents travel as the instruction's E8M0 block scales (a lane's 32 bytes are
//   one block: half a row), so  s_k = fp32 sum_d q(x - mu)_d q(c_k - mu)_d 2^-(e_x + e_k) - csq'_k / 2,  csq'_k the fp32 |c_k - mu|^2 of the
//   UNquantised row.  The label is the lowest index of the maximum, through the epilogue of kmeans_assign_kernel.
// Points are centred and quantised in registers when a workgroup loads them (the two lanes of a point share the row maximum); centroids
// by a pre-pass per call into an image [B, K, 128] + scale bytes + csq' (they are read by every workgroup of the batch).
// =====================================================================================================================================
// mu[b][d] = mean_k c[b][k][d] in fp32: grid = B, block = 256 = 16 row slots x 16 lanes, the slots' partial sums added in a fixed order
template <typename T>
__global__ __launch_bounds__(256) void kmeans_centre_kernel(const T* __restrict__ c, float* __restrict__ mu, int K) {
    constexpr int D = 128, LPR = D / 8, SLOTS = 256 / LPR;
    __shared__ float red[SLOTS][D + 4];
    using V8 = typename Elt<T>::v8;
    const int b = blockIdx.x, tid = threadIdx.x, slot = tid / LPR, li = tid - slot * LPR;
    const T* cb = c + (size_t)b * K * D;
    float acc[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) acc[j] = 0.f;
    for (int k = slot; k < K; k += SLOTS) {
        const V8 v = *(const V8*)(cb + (size_t)k * D + li * 8);
#pragma unroll
        for (int j = 0; j < 8; ++j) acc[j] += Elt<T>::to_float(v[j]);
    }
#pragma unroll
    for (int j = 0; j < 8; ++j) red[slot][li * 8 + j] = acc[j];
    __syncthreads();
    if (tid < D) {
        float s = 0.f;
        for (int sl = 0; sl < SLOTS; ++sl) s += red[sl][tid];
        mu[(size_t)b * D + tid] = s / (float)K;
    }
}

// the centroid pre-pass of one e4m3 assignment: c8 [B, K, 128] e4m3, cscale int32 [B, K] (the E8M0 byte 127 - e), csq float [B, K]
// (|c - mu|^2 of the unquantised row).  16 lanes per row, 8 channels each.
template <typename T>
__global__ __launch_bounds__(256) void kmeans_e4m3_centroids_kernel(const T* __restrict__ c, const float* __restrict__ mu /* [B, 128] or NULL */,
                                                                    uint8_t* __restrict__ c8, int32_t* __restrict__ cscale,
                                                                    float* __restrict__ csq, int K, long long rows) {
    constexpr int D = 128;
    using V8 = typename Elt<T>::v8;
    const int sub = threadIdx.x >> 4, li = threadIdx.x & 15;
    for (long long r = (long long)blockIdx.x * 16 + sub; r < rows; r += (long long)gridDim.x * 16) {
        const V8 v = *(const V8*)(c + r * D + li * 8);
        f32x4 m0 = {0.f, 0.f, 0.f, 0.f}, m1 = m0;
        if (mu) {
            const float* mp = mu + (r / K) * D + li * 8;
            m0 = *(const f32x4*)mp, m1 = *(const f32x4*)(mp + 4);
        }
        float d[8], s = 0.f, mx = 0.f;
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            d[j] = Elt<T>::to_float(v[j]) - (j < 4 ? m0[j] : m1[j - 4]);
            s += d[j] * d[j];
            mx = fmaxf(mx, fabsf(d[j]));
        }
#pragma unroll
        for (int o = 8; o >= 1; o >>= 1) s += __shfl_xor(s, o), mx = fmaxf(mx, __shfl_xor(mx, o));
        const int e = f8_row_exponent(mx);
        *(u32x2*)(c8 + r * D + li * 8) = u32x2{f8_pack4(ldexpf(d[0], e), ldexpf(d[1], e), ldexpf(d[2], e), ldexpf(d[3], e)),
                                               f8_pack4(ldexpf(d[4], e), ldexpf(d[5], e), ldexpf(d[6], e), ldexpf(d[7], e))};
        if (li == 0) cscale[r] = 127 - e, csq[r] = s;
    }
}

// ---- e4m3 assignment: grid = (ceil(N / 256), B), block = 512: the staging, double buffer and arg-max of kmeans_assign_kernel<T, 128, 8> ----
// LDS stage: the tile's centroid image [64][128] bytes in the K layout of attn_f8.h (f8_k_off), its 64 start values -csq' / 2 (-inf behind K)
// and its 64 scale words.  Operands: A = centroid row 32 bb + ql, bytes [64 ks + 32 g, +32), B = the point's bytes of the same channels.
template <typename T>
__global__ __launch_bounds__(512, 2) void kmeans_assign_e4m3_kernel(const T* __restrict__ x, const float* __restrict__ mu,
                                                                    const uint8_t* __restrict__ c8, const int32_t* __restrict__ cscale,
                                                                    const float* __restrict__ csq, int32_t* __restrict__ labels, int N, int K,
                                                                    long long x_bs /* elements between the batches of x */) {
    using E = Elt<T>;
    using V8 = typename E::v8;
    constexpr int D = 128, NW = 8, KS = D / 64;
    constexpr int kKBytes = kBN * D;                   // one byte per element
    constexpr int kStage = kKBytes + kBN * 4 + kBN * 4;
    static_assert(kBN * (D / 16) == NW * 64, "one 16-byte chunk of a centroid tile per thread");
    extern __shared__ __attribute__((aligned(16))) char smem[];

    const int b = blockIdx.y;
    const int tid = threadIdx.x, lane = tid & 63, wave = wave_id();
    const int g = lane >> 5, ql = lane & 31;
    const int n = blockIdx.x * (NW * 32) + wave * 32 + ql;
    const T* xb = x + (size_t)b * (size_t)x_bs;
    const uint8_t* c8b = c8 + (size_t)b * K * D;
    const float* csqb = csq + (size_t)b * K;
    const int32_t* cscb = cscale + (size_t)b * K;

    // the point: channels [64 ks + 32 g, +32) centred in fp32, the row maximum from both lanes, quantised in place
    i32x8 xf[KS];
    int x_scale;
    {
        const T* xrow = xb + (size_t)(n < N ? n : 0) * D + g * 32;
        const float* mub = mu ? mu + (size_t)b * D + g * 32 : nullptr;
        float r[KS][32], mx = 0.f;
#pragma unroll
        for (int ks = 0; ks < KS; ++ks)
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                const V8 v = *(const V8*)(xrow + ks * 64 + c * 8);
                f32x4 m0 = {0.f, 0.f, 0.f, 0.f}, m1 = m0;
                if (mub) m0 = *(const f32x4*)(mub + ks * 64 + c * 8), m1 = *(const f32x4*)(mub + ks * 64 + c * 8 + 4);
#pragma unroll
                for (int j = 0; j < 8; ++j) {
                    const float d = E::to_float(v[j]) - (j < 4 ? m0[j] : m1[j - 4]);
                    r[ks][c * 8 + j] = d;
                    mx = fmaxf(mx, fabsf(d));
                }
            }
        mx = fmaxf(mx, __shfl_xor(mx, 32));
        const int e = f8_row_exponent(mx);
#pragma unroll
        for (int ks = 0; ks < KS; ++ks)
#pragma unroll
            for (int w = 0; w < 8; ++w)
                xf[ks][w] = (int)f8_pack4(ldexpf(r[ks][4 * w], e), ldexpf(r[ks][4 * w + 1], e), ldexpf(r[ks][4 * w + 2], e),
                                          ldexpf(r[ks][4 * w + 3], e));
        x_scale = f8_row_scale_word(e);
    }

    const int srow = tid >> 3, scol = tid & 7;
    const int k_dst = f8_k_off(srow, scol);
    u32x4 creg;
    float sreg = 0.f;
    int ereg = 0;
    bool sreg_ok = false;
    const int nT = (K + kBN - 1) / kBN;
    auto issue = [&](int t) {
        const int c = t * kBN + srow;
        creg = *(const u32x4*)(c8b + (size_t)(c < K ? c : 0) * D + scol * 16);
        if (tid < kBN) {   // (used in write() only, like kmeans_assign_kernel's |c|^2)
            const int ck = t * kBN + tid;
            sreg = csqb[ck < K ? ck : 0];
            ereg = cscb[ck < K ? ck : 0];
            sreg_ok = ck < K;
        }
    };
    auto write = [&](int buf) {
        char* base = smem + buf * kStage;
        *(u32x4*)(base + k_dst) = creg;
        if (tid < kBN) {
            *(float*)(base + kKBytes + tid * 4) = sreg_ok ? -0.5f * sreg : -INFINITY;   // centroids behind K can never win
            *(int*)(base + kKBytes + kBN * 4 + tid * 4) = ereg * 0x01010101;
        }
    };

    issue(0);
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) asm volatile("" : "+v"(xf[ks]));
    write(0);
    if (nT > 1) issue(1);
    __syncthreads();

    const int ksw = (ql >> 1) & 7;
    float best = -INFINITY;
    int best_idx = 0;
    for (int t = 0; t < nT; ++t) {
        const int buf = t & 1;
        const char* kbuf = smem + buf * kStage;
        const float* h_t = (const float*)(kbuf + kKBytes);
        const int* e_t = (const int*)(kbuf + kKBytes + kBN * 4);
        f32x16 s[2];
        int c_scale[2];
#pragma unroll
        for (int bb = 0; bb < 2; ++bb) {
#pragma unroll
            for (int rq = 0; rq < 4; ++rq) {
                const f32x4 h4 = *(const f32x4*)(h_t + 32 * bb + 8 * rq + 4 * g);
#pragma unroll
                for (int j = 0; j < 4; ++j) s[bb][rq * 4 + j] = h4[j];
            }
            c_scale[bb] = e_t[32 * bb + ql];
        }
        i32x8 af[KS][2];
#pragma unroll
        for (int ks = 0; ks < KS; ++ks)
#pragma unroll
            for (int bb = 0; bb < 2; ++bb) {
                const char* rowp = kbuf + (32 * bb + ql) * D;
                const u32x4 lo = *(const u32x4*)(rowp + (((4 * ks + 2 * g) ^ ksw) << 4));
                const u32x4 hi = *(const u32x4*)(rowp + (((4 * ks + 2 * g + 1) ^ ksw) << 4));
                af[ks][bb] = i32x8{(int)lo[0], (int)lo[1], (int)lo[2], (int)lo[3], (int)hi[0], (int)hi[1], (int)hi[2], (int)hi[3]};
            }
#pragma unroll
        for (int ks = 0; ks < KS; ++ks)
#pragma unroll
            for (int bb = 0; bb < 2; ++bb)
                s[bb] = __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(af[ks][bb], xf[ks], s[bb], 0, 0, 0, c_scale[bb], 0, x_scale);
        // the arg-max of kmeans_assign_kernel: four chains of eight registers, merged in index order with the same strict compare
        float cb_[4];
        int ci_[4];
#pragma unroll
        for (int ch = 0; ch < 4; ++ch) {
            const int bb = ch >> 1, r0 = (ch & 1) * 8;
            cb_[ch] = s[bb][r0];
            ci_[ch] = 32 * bb + 8 * (r0 >> 2) + (r0 & 3) + 4 * g;
#pragma unroll
            for (int r = r0 + 1; r < r0 + 8; ++r) {
                const int c = 32 * bb + 8 * (r >> 2) + (r & 3);
                const bool upd = s[bb][r] > cb_[ch];
                cb_[ch] = upd ? s[bb][r] : cb_[ch];
                ci_[ch] = upd ? c + 4 * g : ci_[ch];
            }
        }
        float tb = cb_[0];
        int ti = ci_[0];
#pragma unroll
        for (int ch = 1; ch < 4; ++ch) {
            const bool upd = cb_[ch] > tb;
            tb = upd ? cb_[ch] : tb;
            ti = upd ? ci_[ch] : ti;
        }
        const bool upd = tb > best;
        best = upd ? tb : best;
        best_idx = upd ? t * kBN + ti : best_idx;
        if (t + 1 < nT) write(buf ^ 1);
        if (t + 2 < nT) issue(t + 2);
        __syncthreads();
    }
    // the two lanes of a point cover disjoint centroid subsets: merge, lowest index wins ties
    const float ob = __shfl_xor(best, 32);
    const int oi = __shfl_xor(best_idx, 32);
    if (ob > best || (ob == best && oi < best_idx)) best = ob, best_idx = oi;
    if (g == 0 && n < N) labels[(size_t)b * N + n] = best_idx;
}

}  // namespace svg

using namespace svg;

#ifdef SVG_KMEANS_TRACE
extern "C" int svg_debug_kmeans_trace(uint64_t* out64) {
    return hipMemcpyFromSymbol(out64, HIP_SYMBOL(g_km_trace), sizeof(uint64_t) * 64) == hipSuccess ? SVG_OK : SVG_ERR_LAUNCH;
}
#endif

extern "C" int svg_kmeans_xsq(const void* x, float* xsq, int32_t B, int32_t N, int32_t D, int32_t dtype, void* stream) {
    if (!x || !xsq || B <= 0 || N <= 0) return SVG_ERR_BAD_ARG;
    if (D != 64 && D != 128) return SVG_ERR_UNSUPPORTED;
    const long long rows = (long long)B * N;
    const int rpb = 256 / (D / 8);
    dim3 grid((unsigned)std::min<long long>(4096, (rows + rpb - 1) / rpb));
    if (dtype == SVG_DTYPE_BF16)
        hipLaunchKernelGGL((xsq_kernel<__bf16>), grid, dim3(256), 0, (hipStream_t)stream, (const __bf16*)x, xsq, rows, D);
    else if (dtype == SVG_DTYPE_F16)
        hipLaunchKernelGGL((xsq_kernel<_Float16>), grid, dim3(256), 0, (hipStream_t)stream, (const _Float16*)x, xsq, rows, D);
    else
        return SVG_ERR_UNSUPPORTED;
    return launch_status();
}

extern "C" size_t svg_kmeans_workspace_bytes(int32_t B, int32_t N, int32_t K, int32_t D) {
    (void)D;
    if (B <= 0 || N <= 0 || K <= 0) return 0;
    const size_t csq_bytes = ((size_t)B * K * sizeof(float) + 255) / 256 * 256;
    return csq_bytes + svg_argsort_workspace_bytes(B, N, K);
}

// one Lloyd iteration on x whose batches are x_bs elements apart (rows contiguous inside a batch): svg_kmeans_iter (x_bs = N * D) and the
// iterations of svg_kmeans_loop[_strided]
static int kmeans_iter_impl(const void* x, long long x_bs, const float* xsq, const void* centroids_in, void* centroids_out,
                            int32_t* labels, int32_t* counts, int32_t* sorted_idx, float* shift, int32_t B, int32_t N,
                            int32_t K, int32_t D, int32_t dtype, void* workspace, size_t workspace_bytes, void* stream) {
    // (xsq may be NULL: the argmax form of the assignment does not use |x|^2 — see kmeans_assign_kernel; the parameter stays in the
    //  signature because the reference's distance form carries it, svg/kmeans_utils.py:704)
    if (!x || !centroids_in || !centroids_out || !labels || !counts || !sorted_idx || !shift || !workspace)
        return SVG_ERR_BAD_ARG;
    if (B <= 0 || N <= 0 || K <= 0) return SVG_ERR_BAD_ARG;
    if (K > 8192) return SVG_ERR_UNSUPPORTED;
    if (workspace_bytes < svg_kmeans_workspace_bytes(B, N, K, D)) return SVG_ERR_WORKSPACE;
    hipStream_t st = (hipStream_t)stream;
    if (dtype == SVG_DTYPE_BF16) {
        if (D == 128)
            return run_kmeans_iter<__bf16, 128>(x, xsq, centroids_in, centroids_out, labels, counts, sorted_idx, shift, B, N,
                                                K, workspace, workspace_bytes, st, x_bs);
        if (D == 64)
            return run_kmeans_iter<__bf16, 64>(x, xsq, centroids_in, centroids_out, labels, counts, sorted_idx, shift, B, N, K,
                                               workspace, workspace_bytes, st, x_bs);
    } else if (dtype == SVG_DTYPE_F16) {
        if (D == 128)
            return run_kmeans_iter<_Float16, 128>(x, xsq, centroids_in, centroids_out, labels, counts, sorted_idx, shift, B, N,
                                                  K, workspace, workspace_bytes, st, x_bs);
        if (D == 64)
            return run_kmeans_iter<_Float16, 64>(x, xsq, centroids_in, centroids_out, labels, counts, sorted_idx, shift, B, N,
                                                 K, workspace, workspace_bytes, st, x_bs);
    }
    return SVG_ERR_UNSUPPORTED;
}

extern "C" int svg_kmeans_iter(const void* x, const float* xsq, const void* centroids_in, void* centroids_out,
                               int32_t* labels, int32_t* counts, int32_t* sorted_idx, float* shift, int32_t B, int32_t N,
                               int32_t K, int32_t D, int32_t dtype, void* workspace, size_t workspace_bytes, void* stream) {
    return kmeans_iter_impl(x, (long long)N * D, xsq, centroids_in, centroids_out, labels, counts, sorted_idx, shift, B, N, K, D, dtype,
                            workspace, workspace_bytes, stream);
}

#define SVG_KM_DISPATCH(CALL)                                                                  \
    if (dtype == SVG_DTYPE_BF16) {                                                             \
        if (D == 128) return CALL(__bf16, 128);                                                \
        if (D == 64) return CALL(__bf16, 64);                                                  \
    } else if (dtype == SVG_DTYPE_F16) {                                                       \
        if (D == 128) return CALL(_Float16, 128);                                              \
        if (D == 64) return CALL(_Float16, 64);                                                \
    }                                                                                          \
    return SVG_ERR_UNSUPPORTED;

// labels[b, n] = argmin_k |x[b, n] - centroids[b, k]|^2 (lowest index on ties): the assignment half of svg_kmeans_iter on its own.
extern "C" int svg_kmeans_assign(const void* x, const void* centroids, int32_t* labels, int32_t B, int32_t N, int32_t K, int32_t D,
                                 int32_t dtype, void* workspace, size_t workspace_bytes, void* stream) {
    if (!x || !centroids || !labels || !workspace || B <= 0 || N <= 0 || K <= 0) return SVG_ERR_BAD_ARG;
    if (K > 8192) return SVG_ERR_UNSUPPORTED;
    if (workspace_bytes < svg_kmeans_workspace_bytes(B, N, K, D)) return SVG_ERR_WORKSPACE;
    hipStream_t st = (hipStream_t)stream;
#define SVG_KM_ASSIGN(T, DD) run_kmeans_assign<T, DD>(x, nullptr, centroids, labels, B, N, K, workspace, st, (long long)N * DD)
    SVG_KM_DISPATCH(SVG_KM_ASSIGN)
#undef SVG_KM_ASSIGN
}

// The update half on GIVEN labels: stable sort of the labels, per-cluster fp32 means in a fixed order, empty clusters keep
// centroids_in, shift[b] = the largest centre movement (as svg_kmeans_iter).
extern "C" int svg_kmeans_update(const void* x, const int32_t* labels, const void* centroids_in, void* centroids_out, int32_t* counts,
                                 int32_t* sorted_idx, float* shift, int32_t B, int32_t N, int32_t K, int32_t D, int32_t dtype,
                                 void* workspace, size_t workspace_bytes, void* stream) {
    if (!x || !labels || !centroids_in || !centroids_out || !counts || !sorted_idx || !shift || !workspace) return SVG_ERR_BAD_ARG;
    if (B <= 0 || N <= 0 || K <= 0) return SVG_ERR_BAD_ARG;
    if (K > 8192) return SVG_ERR_UNSUPPORTED;
    if (workspace_bytes < svg_kmeans_workspace_bytes(B, N, K, D)) return SVG_ERR_WORKSPACE;
    hipStream_t st = (hipStream_t)stream;
#define SVG_KM_UPDATE(T, DD) run_kmeans_update<T, DD>(x, centroids_in, centroids_out, labels, counts, sorted_idx, shift, B, N, K, workspace, st, (long long)N * DD)
    SVG_KM_DISPATCH(SVG_KM_UPDATE)
#undef SVG_KM_UPDATE
}
#undef SVG_KM_DISPATCH

// scratch of svg_kmeans_loop_grouped: per-iteration scratch of svg_kmeans_iter + scratch labels / sorted indices / counts / shift of one
// iteration + 4 state words per stopping group (one 256-byte block for up to 16 groups: the ungrouped loop's size)
extern "C" size_t svg_kmeans_loop_grouped_workspace_bytes(int32_t B, int32_t N, int32_t K, int32_t D, int32_t group) {
    const size_t it = svg_kmeans_workspace_bytes(B, N, K, D);
    if (it == 0 || group <= 0 || B % group != 0) return 0;
    const size_t a = ((size_t)B * N * 4 + 255) / 256 * 256, c = ((size_t)B * K * 4 + 255) / 256 * 256, sh = ((size_t)B * 4 + 255) / 256 * 256;
    const size_t st = ((size_t)(B / group) * 4 * sizeof(int32_t) + 255) / 256 * 256;
    return (it + 255) / 256 * 256 + 2 * a + c + sh + st;
}

extern "C" size_t svg_kmeans_loop_workspace_bytes(int32_t B, int32_t N, int32_t K, int32_t D) {
    return B > 0 ? svg_kmeans_loop_grouped_workspace_bytes(B, N, K, D, B) : 0;
}

// ---- the host steps of the Lloyd loop, shared by svg_kmeans_loop* (all of them in one call) and svg_kmeans_stepped_* (one per call) ----
// scratch of one loop: the per-iteration scratch of svg_kmeans_iter, one iteration's labels / sorted indices / counts / shift, the state words
struct KmeansLoopScratch {
    void* it_ws;
    size_t it_bytes;
    int32_t *t_labels, *t_sorted, *t_counts;
    float* t_shift;
    int32_t* state;
};
static size_t kmeans_state_bytes(int G) { return ((size_t)G * 4 * sizeof(int32_t) + 255) / 256 * 256; }
// state_first = false: the layout of svg_kmeans_loop_grouped_workspace_bytes (state words last); true: the stepped entries' (state words
// first: svg_kmeans_stepped_finish has no N and finds them there)
static KmeansLoopScratch kmeans_loop_scratch(void* workspace, int B, int N, int K, int D, int G, bool state_first) {
    KmeansLoopScratch s;
    s.it_bytes = (svg_kmeans_workspace_bytes(B, N, K, D) + 255) / 256 * 256;
    const size_t a = ((size_t)B * N * 4 + 255) / 256 * 256, c = ((size_t)B * K * 4 + 255) / 256 * 256, sh = ((size_t)B * 4 + 255) / 256 * 256;
    char* w = (char*)workspace + (state_first ? kmeans_state_bytes(G) : 0);
    s.it_ws = w;
    s.t_labels = (int32_t*)(w + s.it_bytes);
    s.t_sorted = (int32_t*)(w + s.it_bytes + a);
    s.t_counts = (int32_t*)(w + s.it_bytes + 2 * a);
    s.t_shift = (float*)(w + s.it_bytes + 2 * a + c);
    s.state = state_first ? (int32_t*)workspace : (int32_t*)(w + s.it_bytes + 2 * a + c + sh);
    return s;
}

// iteration `it` into the scratch: it == 0 clears the state words and reads c_init, writing c_work_a; odd iterations write c_work_b
static int kmeans_loop_iterate(const KmeansLoopScratch& s, const void* x, long long x_bs, const float* xsq, const void* c_init, void* c_work_a,
                               void* c_work_b, int it, int B, int N, int K, int D, int dtype, int G, void* stream) {
    if (it == 0 && hipMemsetAsync(s.state, 0, (size_t)4 * G * sizeof(int32_t), (hipStream_t)stream) != hipSuccess) return SVG_ERR_LAUNCH;
    const void* cur = it == 0 ? c_init : ((it & 1) ? c_work_a : c_work_b);
    void* out = (it & 1) ? c_work_b : c_work_a;
    return kmeans_iter_impl(x, x_bs, xsq, cur, out, s.t_labels, s.t_counts, s.t_sorted, s.t_shift, B, N, K, D, dtype, s.it_ws, s.it_bytes, stream);
}

// the commit of iteration `it`; maxima == NULL: the group maxima are reduced from the scratch shift inside the kernel
static void kmeans_loop_commit(const KmeansLoopScratch& s, const float* maxima, int32_t* labels, int32_t* counts, int32_t* sorted_idx, int it,
                               float tol, int B, int N, int K, int group, hipStream_t st) {
    const int G = B / group;
    const int sel_cur = it == 0 ? 0 : ((it & 1) ? 1 : 2), sel_out = (it & 1) ? 2 : 1;   // 0 initial, 1 / 2 the two work buffers
    const long long gn = (long long)group * N, gk = (long long)group * K;
    // (G = 1: the grid of the ungrouped loop; more groups share about as many workgroups, a stopped group's return at once)
    const dim3 grid((unsigned)std::min<long long>((2048 + G - 1) / G, (gn + 255) / 256), (unsigned)G);
    if (maxima)
        hipLaunchKernelGGL(kmeans_commit_kernel<true>, grid, dim3(256), 0, st, s.t_labels, s.t_sorted, s.t_counts, labels, sorted_idx, counts,
                           maxima, s.state, gn, gk, group, tol, it, sel_cur, sel_out);
    else
        hipLaunchKernelGGL(kmeans_commit_kernel<false>, grid, dim3(256), 0, st, s.t_labels, s.t_sorted, s.t_counts, labels, sorted_idx, counts,
                           s.t_shift, s.state, gn, gk, group, tol, it, sel_cur, sel_out);
}

// every group's centroids from the buffer its selector names, and the n_iters words
static int kmeans_loop_finish(const KmeansLoopScratch& s, const void* c_init, const void* c_work_a, const void* c_work_b, void* centroids_out,
                              int32_t* n_iters, int B, int K, int D, int dtype, int group, hipStream_t st) {
    const int G = B / group;
    const long long gn8 = (long long)group * K * D / 8;
    const dim3 g2((unsigned)std::min<long long>((1024 + G - 1) / G, (gn8 + 255) / 256), (unsigned)G);
    if (dtype == SVG_DTYPE_BF16)
        hipLaunchKernelGGL((kmeans_select_kernel<__bf16>), g2, dim3(256), 0, st, (const __bf16*)c_init, (const __bf16*)c_work_a,
                           (const __bf16*)c_work_b, (__bf16*)centroids_out, s.state + 3 * G, gn8);
    else
        hipLaunchKernelGGL((kmeans_select_kernel<_Float16>), g2, dim3(256), 0, st, (const _Float16*)c_init, (const _Float16*)c_work_a,
                           (const _Float16*)c_work_b, (_Float16*)centroids_out, s.state + 3 * G, gn8);
    if (hipMemcpyAsync(n_iters, s.state + 2 * G, (size_t)G * sizeof(int32_t), hipMemcpyDeviceToDevice, st) != hipSuccess) return SVG_ERR_LAUNCH;
    return launch_status();
}

// svg_kmeans_loop (x_bs = N * D, group = B), svg_kmeans_loop_strided (group = B) and their grouped forms
static int kmeans_loop_impl(const void* x, long long x_bs, const float* xsq, const void* c_init, void* c_work_a, void* c_work_b, int32_t* labels,
                            int32_t* counts, int32_t* sorted_idx, void* centroids_out, int32_t* n_iters, int32_t B, int32_t N,
                            int32_t K, int32_t D, int32_t dtype, int32_t group, int32_t max_iters, float tol, void* workspace,
                            size_t workspace_bytes, void* stream) {
    if (!x || !c_init || !c_work_a || !c_work_b || !labels || !counts || !sorted_idx || !centroids_out || !n_iters || !workspace)
        return SVG_ERR_BAD_ARG;   // (xsq may be NULL, see svg_kmeans_iter)
    if (B <= 0 || N <= 0 || K <= 0 || max_iters <= 0 || group <= 0 || B % group != 0) return SVG_ERR_BAD_ARG;
    if (K > 8192 || (D != 64 && D != 128) || (dtype != SVG_DTYPE_BF16 && dtype != SVG_DTYPE_F16)) return SVG_ERR_UNSUPPORTED;
    if (workspace_bytes < svg_kmeans_loop_grouped_workspace_bytes(B, N, K, D, group)) return SVG_ERR_WORKSPACE;
    if (c_init == c_work_a || c_init == c_work_b || c_work_a == c_work_b || centroids_out == c_work_a || centroids_out == c_work_b)
        return SVG_ERR_BAD_ARG;
    hipStream_t st = (hipStream_t)stream;
    const int G = B / group;
    const KmeansLoopScratch s = kmeans_loop_scratch(workspace, B, N, K, D, G, false);
    for (int it = 0; it < max_iters; ++it) {
        if (const int rc = kmeans_loop_iterate(s, x, x_bs, xsq, c_init, c_work_a, c_work_b, it, B, N, K, D, dtype, G, stream); rc != SVG_OK) return rc;
        kmeans_loop_commit(s, nullptr, labels, counts, sorted_idx, it, tol, B, N, K, group, st);
    }
    return kmeans_loop_finish(s, c_init, c_work_a, c_work_b, centroids_out, n_iters, B, K, D, dtype, group, st);
}

static int check_strided(const void* x, int64_t x_batch_stride, int32_t N, int32_t D) {
    if (x_batch_stride < (int64_t)N * D) return SVG_ERR_BAD_ARG;
    if (x_batch_stride % 8 != 0 || ((size_t)x & 15) != 0) return SVG_ERR_UNSUPPORTED;
    return SVG_OK;
}

extern "C" int svg_kmeans_loop(const void* x, const float* xsq, const void* c_init, void* c_work_a, void* c_work_b, int32_t* labels,
                               int32_t* counts, int32_t* sorted_idx, void* centroids_out, int32_t* n_iters, int32_t B, int32_t N,
                               int32_t K, int32_t D, int32_t dtype, int32_t max_iters, float tol, void* workspace,
                               size_t workspace_bytes, void* stream) {
    return kmeans_loop_impl(x, (long long)N * D, xsq, c_init, c_work_a, c_work_b, labels, counts, sorted_idx, centroids_out, n_iters, B, N, K, D,
                            dtype, B, max_iters, tol, workspace, workspace_bytes, stream);
}

extern "C" int svg_kmeans_loop_strided(const void* x, int64_t x_batch_stride, const void* c_init, void* c_work_a, void* c_work_b,
                                       int32_t* labels, int32_t* counts, int32_t* sorted_idx, void* centroids_out, int32_t* n_iters,
                                       int32_t B, int32_t N, int32_t K, int32_t D, int32_t dtype, int32_t max_iters, float tol,
                                       void* workspace, size_t workspace_bytes, void* stream) {
    if (const int rc = check_strided(x, x_batch_stride, N, D); rc != SVG_OK) return rc;
    return kmeans_loop_impl(x, (long long)x_batch_stride, nullptr, c_init, c_work_a, c_work_b, labels, counts, sorted_idx, centroids_out, n_iters,
                            B, N, K, D, dtype, B, max_iters, tol, workspace, workspace_bytes, stream);
}

extern "C" int svg_kmeans_loop_grouped(const void* x, const float* xsq, const void* c_init, void* c_work_a, void* c_work_b, int32_t* labels,
                                       int32_t* counts, int32_t* sorted_idx, void* centroids_out, int32_t* n_iters, int32_t B, int32_t N,
                                       int32_t K, int32_t D, int32_t dtype, int32_t group, int32_t max_iters, float tol, void* workspace,
                                       size_t workspace_bytes, void* stream) {
    return kmeans_loop_impl(x, (long long)N * D, xsq, c_init, c_work_a, c_work_b, labels, counts, sorted_idx, centroids_out, n_iters, B, N, K, D,
                            dtype, group, max_iters, tol, workspace, workspace_bytes, stream);
}

extern "C" int svg_kmeans_loop_grouped_strided(const void* x, int64_t x_batch_stride, const void* c_init, void* c_work_a, void* c_work_b,
                                               int32_t* labels, int32_t* counts, int32_t* sorted_idx, void* centroids_out, int32_t* n_iters,
                                               int32_t B, int32_t N, int32_t K, int32_t D, int32_t dtype, int32_t group, int32_t max_iters,
                                               float tol, void* workspace, size_t workspace_bytes, void* stream) {
    if (const int rc = check_strided(x, x_batch_stride, N, D); rc != SVG_OK) return rc;
    return kmeans_loop_impl(x, (long long)x_batch_stride, nullptr, c_init, c_work_a, c_work_b, labels, counts, sorted_idx, centroids_out, n_iters,
                            B, N, K, D, dtype, group, max_iters, tol, workspace, workspace_bytes, stream);
}

// ---- the Lloyd loop in steps (include/svg_attn_kmeans_stepped.h): the host steps above, one per call, with the group maxima handed out
// by iterate and taken back by commit ----
extern "C" size_t svg_kmeans_stepped_workspace_bytes(int32_t B, int32_t N, int32_t K, int32_t D, int32_t group) {
    if (K > 8192 || (D != 64 && D != 128)) return 0;
    return svg_kmeans_loop_grouped_workspace_bytes(B, N, K, D, group);   // (the same blocks, the state words in front)
}

extern "C" int svg_kmeans_stepped_iterate(const void* x, int64_t x_batch_stride, const void* c_init, void* c_work_a, void* c_work_b, int32_t it,
                                          float* maxima, int32_t B, int32_t N, int32_t K, int32_t D, int32_t dtype, int32_t group,
                                          void* workspace, size_t workspace_bytes, void* stream) {
    if (!x || !c_init || !c_work_a || !c_work_b || !maxima || !workspace) return SVG_ERR_BAD_ARG;
    if (B <= 0 || N <= 0 || K <= 0 || group <= 0 || B % group != 0 || it < 0) return SVG_ERR_BAD_ARG;
    if (K > 8192 || (D != 64 && D != 128) || (dtype != SVG_DTYPE_BF16 && dtype != SVG_DTYPE_F16)) return SVG_ERR_UNSUPPORTED;
    if (workspace_bytes < svg_kmeans_stepped_workspace_bytes(B, N, K, D, group)) return SVG_ERR_WORKSPACE;
    if (c_init == c_work_a || c_init == c_work_b || c_work_a == c_work_b) return SVG_ERR_BAD_ARG;
    if (const int rc = check_strided(x, x_batch_stride, N, D); rc != SVG_OK) return rc;
    const int G = B / group;
    const KmeansLoopScratch s = kmeans_loop_scratch(workspace, B, N, K, D, G, true);
    if (const int rc = kmeans_loop_iterate(s, x, (long long)x_batch_stride, nullptr, c_init, c_work_a, c_work_b, it, B, N, K, D, dtype, G, stream);
        rc != SVG_OK)
        return rc;
    hipLaunchKernelGGL(kmeans_group_maxima_kernel, dim3((unsigned)std::min(256, (G + 3) / 4)), dim3(256), 0, (hipStream_t)stream, s.t_shift, maxima,
                       G, (int)group);
    return launch_status();
}

extern "C" int svg_kmeans_stepped_commit(const float* maxima, int32_t* labels, int32_t* counts, int32_t* sorted_idx, int32_t it, float tol, int32_t B,
                                         int32_t N, int32_t K, int32_t group, void* workspace, size_t workspace_bytes, void* stream) {
    if (!maxima || !labels || !counts || !sorted_idx || !workspace) return SVG_ERR_BAD_ARG;
    if (B <= 0 || N <= 0 || K <= 0 || group <= 0 || B % group != 0 || it < 0) return SVG_ERR_BAD_ARG;
    if (K > 8192) return SVG_ERR_UNSUPPORTED;
    // (no head_dim here: none of the blocks' sizes depends on it)
    if (workspace_bytes < svg_kmeans_stepped_workspace_bytes(B, N, K, 128, group)) return SVG_ERR_WORKSPACE;
    const KmeansLoopScratch s = kmeans_loop_scratch(workspace, B, N, K, 128, B / group, true);
    kmeans_loop_commit(s, maxima, labels, counts, sorted_idx, it, tol, B, N, K, group, (hipStream_t)stream);
    return launch_status();
}

extern "C" int svg_kmeans_stepped_finish(const void* c_init, const void* c_work_a, const void* c_work_b, void* centroids_out, int32_t* n_iters,
                                         int32_t B, int32_t K, int32_t D, int32_t dtype, int32_t group, void* workspace, size_t workspace_bytes,
                                         void* stream) {
    if (!c_init || !c_work_a || !c_work_b || !centroids_out || !n_iters || !workspace) return SVG_ERR_BAD_ARG;
    if (B <= 0 || K <= 0 || group <= 0 || B % group != 0) return SVG_ERR_BAD_ARG;
    if (K > 8192 || (D != 64 && D != 128) || (dtype != SVG_DTYPE_BF16 && dtype != SVG_DTYPE_F16)) return SVG_ERR_UNSUPPORTED;
    // (no N here: the smallest workspace an iterate of these B, K, D, group took — the state words finish reads lie in front of it)
    if (workspace_bytes < svg_kmeans_stepped_workspace_bytes(B, 1, K, D, group)) return SVG_ERR_WORKSPACE;
    if (c_init == c_work_a || c_init == c_work_b || c_work_a == c_work_b || centroids_out == c_work_a || centroids_out == c_work_b)
        return SVG_ERR_BAD_ARG;
    const KmeansLoopScratch s = kmeans_loop_scratch(workspace, B, 1, K, D, B / group, true);
    return kmeans_loop_finish(s, c_init, c_work_a, c_work_b, centroids_out, n_iters, B, K, D, dtype, group, (hipStream_t)stream);
}

// ---- the e4m3 assignment and the Lloyd loop that uses it for its first iterations (include/svg_attn_kmeans_e4m3.h) ----
// scratch of one e4m3 assignment: the centroid image, its scale bytes (one int32 each) and csq'
struct KmeansE4m3Scratch {
    uint8_t* c8;
    int32_t* cscale;
    float* csq;
};
static size_t kmeans_e4m3_image_bytes(int B, int K) { return ((size_t)B * K * 128 + 255) / 256 * 256; }
static size_t kmeans_e4m3_row_bytes(int B, int K) { return ((size_t)B * K * 4 + 255) / 256 * 256; }
static size_t kmeans_e4m3_mu_bytes(int B) { return ((size_t)B * 128 * sizeof(float) + 255) / 256 * 256; }
static KmeansE4m3Scratch kmeans_e4m3_scratch(void* w, int B, int K) {
    KmeansE4m3Scratch s;
    s.c8 = (uint8_t*)w;
    s.cscale = (int32_t*)((char*)w + kmeans_e4m3_image_bytes(B, K));
    s.csq = (float*)((char*)w + kmeans_e4m3_image_bytes(B, K) + kmeans_e4m3_row_bytes(B, K));
    return s;
}

template <typename T>
static int run_kmeans_assign_e4m3(const void* x, const float* mu, const void* c_in, int32_t* labels, int B, int N, int K,
                                  const KmeansE4m3Scratch& s, hipStream_t st, long long x_bs) {
    const long long rows = (long long)B * K;
    hipLaunchKernelGGL((kmeans_e4m3_centroids_kernel<T>), dim3((unsigned)std::min<long long>(2048, (rows + 15) / 16)), dim3(256), 0, st,
                       (const T*)c_in, mu, s.c8, s.cscale, s.csq, K, rows);
    constexpr int lds = 2 * (kBN * 128 + kBN * 8);
    hipLaunchKernelGGL((kmeans_assign_e4m3_kernel<T>), dim3((N + 255) / 256, B), dim3(512), lds, st, (const T*)x, mu, s.c8, s.cscale, s.csq,
                       labels, N, K, x_bs);
    return launch_status();
}

static bool kmeans_e4m3_covers(int32_t K, int32_t D, int32_t dtype) {
    return K <= 8192 && D == 128 && (dtype == SVG_DTYPE_BF16 || dtype == SVG_DTYPE_F16);
}

extern "C" int svg_kmeans_centre(const void* centroids, float* mu, int32_t B, int32_t K, int32_t D, int32_t dtype, void* stream) {
    if (!centroids || !mu || B <= 0 || K <= 0) return SVG_ERR_BAD_ARG;
    if (!kmeans_e4m3_covers(K, D, dtype)) return SVG_ERR_UNSUPPORTED;
    if (dtype == SVG_DTYPE_BF16)
        hipLaunchKernelGGL((kmeans_centre_kernel<__bf16>), dim3(B), dim3(256), 0, (hipStream_t)stream, (const __bf16*)centroids, mu, K);
    else
        hipLaunchKernelGGL((kmeans_centre_kernel<_Float16>), dim3(B), dim3(256), 0, (hipStream_t)stream, (const _Float16*)centroids, mu, K);
    return launch_status();
}

extern "C" size_t svg_kmeans_assign_e4m3_workspace_bytes(int32_t B, int32_t N, int32_t K, int32_t D) {
    if (B <= 0 || N <= 0 || K <= 0 || K > 8192 || D != 128) return 0;
    return kmeans_e4m3_image_bytes(B, K) + 2 * kmeans_e4m3_row_bytes(B, K);
}

extern "C" int svg_kmeans_assign_e4m3(const void* x, const void* centroids, const float* mu, int32_t* labels, int32_t B, int32_t N, int32_t K,
                                      int32_t D, int32_t dtype, void* workspace, size_t workspace_bytes, void* stream) {
    if (!x || !centroids || !labels || !workspace || B <= 0 || N <= 0 || K <= 0) return SVG_ERR_BAD_ARG;   // (mu may be NULL: zeros)
    if (!kmeans_e4m3_covers(K, D, dtype)) return SVG_ERR_UNSUPPORTED;
    if (workspace_bytes < svg_kmeans_assign_e4m3_workspace_bytes(B, N, K, D)) return SVG_ERR_WORKSPACE;
    if ((((size_t)x | (size_t)mu) & 15) != 0) return SVG_ERR_UNSUPPORTED;   // (16-byte loads of rows and of mu)
    const KmeansE4m3Scratch s = kmeans_e4m3_scratch(workspace, B, K);
    if (dtype == SVG_DTYPE_BF16)
        return run_kmeans_assign_e4m3<__bf16>(x, mu, centroids, labels, B, N, K, s, (hipStream_t)stream, (long long)N * D);
    return run_kmeans_assign_e4m3<_Float16>(x, mu, centroids, labels, B, N, K, s, (hipStream_t)stream, (long long)N * D);
}

// the blocks of svg_kmeans_loop_grouped_workspace_bytes in front (fp8_iters = 0 IS svg_kmeans_loop_grouped_strided on them), then mu and
// the scratch of one e4m3 assignment
extern "C" size_t svg_kmeans_loop_e4m3_workspace_bytes(int32_t B, int32_t N, int32_t K, int32_t D, int32_t group) {
    const size_t loop = svg_kmeans_loop_grouped_workspace_bytes(B, N, K, D, group);
    if (loop == 0 || K > 8192 || D != 128) return 0;
    return (loop + 255) / 256 * 256 + kmeans_e4m3_mu_bytes(B) + svg_kmeans_assign_e4m3_workspace_bytes(B, N, K, D);
}

extern "C" int svg_kmeans_loop_e4m3(const void* x, int64_t x_batch_stride, const void* c_init, void* c_work_a, void* c_work_b, int32_t* labels,
                                    int32_t* counts, int32_t* sorted_idx, void* centroids_out, int32_t* n_iters, int32_t B, int32_t N,
                                    int32_t K, int32_t D, int32_t dtype, int32_t group, int32_t max_iters, float tol, int32_t fp8_iters,
                                    void* workspace, size_t workspace_bytes, void* stream) {
    if (!x || !c_init || !c_work_a || !c_work_b || !labels || !counts || !sorted_idx || !centroids_out || !n_iters || !workspace)
        return SVG_ERR_BAD_ARG;
    if (B <= 0 || N <= 0 || K <= 0 || max_iters <= 0 || group <= 0 || B % group != 0 || fp8_iters < 0 || fp8_iters > max_iters)
        return SVG_ERR_BAD_ARG;
    if (!kmeans_e4m3_covers(K, D, dtype)) return SVG_ERR_UNSUPPORTED;
    if (workspace_bytes < svg_kmeans_loop_e4m3_workspace_bytes(B, N, K, D, group)) return SVG_ERR_WORKSPACE;
    if (c_init == c_work_a || c_init == c_work_b || c_work_a == c_work_b || centroids_out == c_work_a || centroids_out == c_work_b)
        return SVG_ERR_BAD_ARG;
    if (const int rc = check_strided(x, x_batch_stride, N, D); rc != SVG_OK) return rc;
    const long long x_bs = (long long)x_batch_stride;
    if (fp8_iters == 0)   // today's loop, call for call
        return kmeans_loop_impl(x, x_bs, nullptr, c_init, c_work_a, c_work_b, labels, counts, sorted_idx, centroids_out, n_iters, B, N, K, D, dtype,
                                group, max_iters, tol, workspace, workspace_bytes, stream);
    hipStream_t st = (hipStream_t)stream;
    const int G = B / group;
    const KmeansLoopScratch s = kmeans_loop_scratch(workspace, B, N, K, D, G, false);
    char* extra = (char*)workspace + (svg_kmeans_loop_grouped_workspace_bytes(B, N, K, D, group) + 255) / 256 * 256;
    float* mu = (float*)extra;
    const KmeansE4m3Scratch es = kmeans_e4m3_scratch(extra + kmeans_e4m3_mu_bytes(B), B, K);
    if (const int rc = svg_kmeans_centre(c_init, mu, B, K, D, dtype, stream); rc != SVG_OK) return rc;
    if (hipMemsetAsync(s.state, 0, (size_t)4 * G * sizeof(int32_t), st) != hipSuccess) return SVG_ERR_LAUNCH;
    for (int it = 0; it < max_iters; ++it) {
        if (it < fp8_iters) {   // the centroids rotate as in kmeans_loop_iterate; the update, sort and commit are the 16-bit loop's
            const void* cur = it == 0 ? c_init : ((it & 1) ? c_work_a : c_work_b);
            void* out = (it & 1) ? c_work_b : c_work_a;
            int rc;
            if (dtype == SVG_DTYPE_BF16) {
                rc = run_kmeans_assign_e4m3<__bf16>(x, mu, cur, s.t_labels, B, N, K, es, st, x_bs);
                if (rc == SVG_OK) rc = run_kmeans_update<__bf16, 128>(x, cur, out, s.t_labels, s.t_counts, s.t_sorted, s.t_shift, B, N, K, s.it_ws, st, x_bs);
            } else {
                rc = run_kmeans_assign_e4m3<_Float16>(x, mu, cur, s.t_labels, B, N, K, es, st, x_bs);
                if (rc == SVG_OK) rc = run_kmeans_update<_Float16, 128>(x, cur, out, s.t_labels, s.t_counts, s.t_sorted, s.t_shift, B, N, K, s.it_ws, st, x_bs);
            }
            if (rc != SVG_OK) return rc;
            // an e4m3 iteration never stops a group: a shift is >= 0 or NaN, so nothing is below a tol of -1
            kmeans_loop_commit(s, nullptr, labels, counts, sorted_idx, it, -1.f, B, N, K, group, st);
        } else {
            if (const int rc = kmeans_loop_iterate(s, x, x_bs, nullptr, c_init, c_work_a, c_work_b, it, B, N, K, D, dtype, G, stream); rc != SVG_OK)
                return rc;
            kmeans_loop_commit(s, nullptr, labels, counts, sorted_idx, it, tol, B, N, K, group, st);
        }
    }
    return kmeans_loop_finish(s, c_init, c_work_a, c_work_b, centroids_out, n_iters, B, K, D, dtype, group, st);
}

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
#include "kmeans_metric.h"

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
// kBias = false is the assignment of the cosine and dot-product metrics (include/svg_attn_kmeans_metric.h): argmax_c <x, c>.  The
// accumulators start at 0 (-inf behind K), so |c|^2 is neither computed, loaded nor staged: a stage is the centroid tile alone.
template <typename T, int D, int NW, bool kBias = true>
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
    constexpr int kStage = L::kKBytes + (kBias ? kBN * 4 : 0);  // centroid tile + its 64 squared norms
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
        if (kBias && tid < kBN) {   // |c|^2, RAW: the multiply sits in write() — used here it makes hipcc wait (vmcnt(0)) for the loads it has just issued
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
        if (kBias && tid < kBN) *(float*)(base + L::kKBytes + tid * 4) = sreg_ok ? -0.5f * sreg : -INFINITY;
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
        if constexpr (kBias) {
#pragma unroll
            for (int bb = 0; bb < 2; ++bb)
#pragma unroll
                for (int rq = 0; rq < 4; ++rq) {
                    const f32x4 h4 = *(const f32x4*)(h_t + 32 * bb + 8 * rq + 4 * g);
#pragma unroll
                    for (int j = 0; j < 4; ++j) s[bb][rq * 4 + j] = h4[j];
                }
        } else {
            // no bias: the scores start at 0.  Only the last tile can have centroids behind K, and the test is uniform over the workgroup:
            // register r of block bb is the tile's centroid 32 bb + 8 (r >> 2) + (r & 3) + 4 g
            const bool partial = K - t * kBN < kBN;
            const int left = K - t * kBN - 4 * g;
#pragma unroll
            for (int bb = 0; bb < 2; ++bb)
#pragma unroll
                for (int r = 0; r < 16; ++r) s[bb][r] = (partial && 32 * bb + 8 * (r >> 2) + (r & 3) >= left) ? -INFINITY : 0.f;
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
// (kBias = false: the metrics' assignment — no csq_kernel launch, `ws` is not touched)
template <typename T, int D, bool kBias>
static int run_kmeans_assign(const KmeansCall& a, const KmeansStep& s) {
    constexpr int NW = 8;
    if constexpr (kBias)
        hipLaunchKernelGGL((csq_kernel<T>), dim3(std::min<long long>(2048, ((long long)a.B * a.K + 15) / 16)), dim3(256), 0, a.st,
                           (const T*)s.c_in, s.ws.csq, (long long)a.B * a.K, D);
    constexpr int lds = 2 * (LdsLayout<D>::kKBytes + (kBias ? kBN * 4 : 0));
    auto kern = kmeans_assign_kernel<T, D, NW, kBias>;
    hipLaunchKernelGGL(kern, dim3((a.N + NW * 32 - 1) / (NW * 32), a.B), dim3(NW * 64), lds, a.st, (const T*)a.x, (const T*)s.c_in, a.xsq,
                       s.ws.csq, s.labels, a.N, a.K, a.x_bs);
    return launch_status();
}

template <typename T, int D>
static int run_kmeans_update(const KmeansCall& a, const KmeansStep& s) {
    const int B = a.B, N = a.N, K = a.K;
    int rc = svg_argsort_labels(s.labels, s.sorted_idx, s.counts, B, N, K, s.ws.sort, s.ws.sort_bytes, (void*)a.st);
    if (rc) return rc;
    (void)hipMemsetAsync(s.shift, 0, (size_t)B * sizeof(float), a.st);
    const int nchunks = (N + 1023) / 1024;
    // workgroups per batch: three per CU over the whole launch.  Measured at Wan 720p (40 heads, K = 300 and 1000 on two streams, the 2-iteration
    // stage): 6 per head 3.49 ms, 8 3.27, 12 3.14, 16 3.05, 20 3.02, 26 3.13, 32 3.17, 52 3.22, 100 3.36, one per cluster 3.37; the kernel of
    // round 4 (one workgroup per cluster, no prefetch) 3.39 (profiles/r05zw_kmeans_update_groups.txt).
    const int groups = std::max(1, std::min(K, (3 * kNumCU + B - 1) / B));
    hipLaunchKernelGGL((kmeans_update_kernel<T, D>), dim3(groups, B), dim3(256), 0, a.st, (const T*)a.x, (const T*)s.c_in, (T*)s.c_out,
                       s.sorted_idx, (const int32_t*)s.ws.sort, s.counts, s.shift, N, K, (size_t)nchunks * K, a.x_bs);
    return launch_status();
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

template <typename T>
static int run_kmeans_assign_e4m3(const KmeansCall& a, const KmeansStep& s) {
    const long long rows = (long long)a.B * a.K;
    hipLaunchKernelGGL((kmeans_e4m3_centroids_kernel<T>), dim3((unsigned)std::min<long long>(2048, (rows + 15) / 16)), dim3(256), 0, a.st,
                       (const T*)s.c_in, s.mu, s.e4m3.c8, s.e4m3.cscale, s.e4m3.csq, a.K, rows);
    constexpr int lds = 2 * (kBN * 128 + kBN * 8);
    hipLaunchKernelGGL((kmeans_assign_e4m3_kernel<T>), dim3((a.N + 255) / 256, a.B), dim3(512), lds, a.st, (const T*)a.x, s.mu, s.e4m3.c8,
                       s.e4m3.cscale, s.e4m3.csq, s.labels, a.N, a.K, a.x_bs);
    return launch_status();
}

}  // namespace svg

using namespace svg;

#ifdef SVG_KMEANS_TRACE
extern "C" int svg_debug_kmeans_trace(uint64_t* out64) {
    return hipMemcpyFromSymbol(out64, HIP_SYMBOL(g_km_trace), sizeof(uint64_t) * 64) == hipSuccess ? SVG_OK : SVG_ERR_LAUNCH;
}
#endif

// ---- the call record (csrc/kmeans_metric.h) as the entries fill it ----
static KmeansCall kmeans_shape(int32_t B, int32_t N, int32_t K, int32_t D, int32_t group) {
    KmeansCall a;
    a.B = B, a.N = N, a.K = K, a.D = D, a.group = group, a.x_bs = (long long)N * D;
    return a;
}
static KmeansCall kmeans_call(KmeansCall a, int32_t dtype, void* workspace, size_t workspace_bytes, void* stream) {
    a.dtype = dtype, a.workspace = workspace, a.workspace_bytes = workspace_bytes, a.st = (hipStream_t)stream;
    return a;
}

// ---- the checks, each written once.  An entry lists the ones it applies in the order its header documents; the first that fails is the
// return code (all of them are host arithmetic on the record: none touches memory or launches) ----
static int first_failure(std::initializer_list<int> rcs) {
    for (const int rc : rcs)
        if (rc != SVG_OK) return rc;
    return SVG_OK;
}
static int need(bool ok, int rc) { return ok ? SVG_OK : rc; }
static int check_pointers(std::initializer_list<const void*> required) {
    for (const void* p : required)
        if (!p) return SVG_ERR_BAD_ARG;
    return SVG_OK;
}
static int check_positive(std::initializer_list<int32_t> sizes) {
    for (const int32_t n : sizes)
        if (n <= 0) return SVG_ERR_BAD_ARG;
    return SVG_OK;
}
static int check_group(const KmeansCall& a) { return need(a.group > 0 && a.B % a.group == 0, SVG_ERR_BAD_ARG); }
static int check_metric(const KmeansCall& a) { return need(a.metric == SVG_KMEANS_COSINE || a.metric == SVG_KMEANS_DOT, SVG_ERR_BAD_ARG); }
// the covered (K, D, dtype): the e4m3 entries are head_dim 128 only
static int check_K(int32_t K) { return K > 8192 ? SVG_ERR_UNSUPPORTED : SVG_OK; }
static int check_D(int32_t D) { return D != 64 && D != 128 ? SVG_ERR_UNSUPPORTED : SVG_OK; }
static int check_dtype(int32_t dtype) { return need(dtype == SVG_DTYPE_BF16 || dtype == SVG_DTYPE_F16, SVG_ERR_UNSUPPORTED); }
static int check_covers(const KmeansCall& a) { return first_failure({check_K(a.K), check_D(a.D), check_dtype(a.dtype)}); }
static int check_e4m3_covers(const KmeansCall& a) { return first_failure({check_K(a.K), need(a.D == 128, SVG_ERR_UNSUPPORTED), check_dtype(a.dtype)}); }
static int check_workspace(const KmeansCall& a, size_t bytes) { return need(a.workspace_bytes >= bytes, SVG_ERR_WORKSPACE); }
// the three centroid buffers are distinct and the result is neither work buffer (an entry without centroids_out leaves it NULL; the work
// buffers are required pointers)
static int check_alias(const KmeansCall& a) {
    return need(a.c_init != a.c_work_a && a.c_init != a.c_work_b && a.c_work_a != a.c_work_b && a.centroids_out != a.c_work_a &&
                    a.centroids_out != a.c_work_b, SVG_ERR_BAD_ARG);
}
static int check_strided(const KmeansCall& a) {
    if (a.x_bs < (long long)a.N * a.D) return SVG_ERR_BAD_ARG;
    if (a.x_bs % 8 != 0 || ((size_t)a.x & 15) != 0) return SVG_ERR_UNSUPPORTED;
    return SVG_OK;
}
static int check_loop_pointers(const KmeansCall& a) {   // (xsq may be NULL, see KmeansCall)
    return check_pointers({a.x, a.c_init, a.c_work_a, a.c_work_b, a.labels, a.counts, a.sorted_idx, a.centroids_out, a.n_iters, a.workspace});
}
static int check_loop_sizes(const KmeansCall& a) { return first_failure({check_positive({a.B, a.N, a.K, a.max_iters}), check_group(a)}); }

// ---- the workspace layouts: one function per kind yields the byte count (from a record without a workspace: the *_workspace_bytes
// entries) and the block pointers.  Every block starts on a multiple of 256 bytes. ----
struct Blocks {   // hands out consecutive 256-byte-rounded blocks from `base` (integer arithmetic: base may be 0)
    uintptr_t base;
    size_t off = 0;
    void* take(size_t n) {
        void* p = (void*)(base + off);
        off += up256(n);
        return p;
    }
};
// bytes = 0 where a size is not positive
static KmeansIterWs kmeans_iter_ws(const KmeansCall& a, void* base) {
    KmeansIterWs w{};
    if (a.B <= 0 || a.N <= 0 || a.K <= 0) return w;
    Blocks b{(uintptr_t)base};
    w.csq = (float*)b.take((size_t)a.B * a.K * sizeof(float));
    w.sort = b.take(0);
    w.sort_bytes = svg_argsort_workspace_bytes(a.B, a.N, a.K);
    w.bytes = b.off + w.sort_bytes;
    return w;
}
static KmeansE4m3Ws kmeans_e4m3_ws(const KmeansCall& a, void* base) {
    Blocks b{(uintptr_t)base};
    const size_t row = (size_t)a.B * a.K * 4;
    KmeansE4m3Ws w;
    w.c8 = (uint8_t*)b.take((size_t)a.B * a.K * 128);
    w.cscale = (int32_t*)b.take(row);
    w.csq = (float*)b.take(row);
    w.bytes = b.off;
    return w;
}
// scratch of one loop: the per-iteration scratch of svg_kmeans_iter, one iteration's labels / sorted indices / counts / shift and 4 state
// words per stopping group (one 256-byte block for up to 16 groups: the ungrouped loop's size).
//   kLoopStateLast : the layout of svg_kmeans_loop_grouped_workspace_bytes
//   kLoopStateFirst: the stepped entries' (the same blocks, the state words in front: svg_kmeans_stepped_finish has no N and finds them there)
//   kLoopE4m3      : kLoopStateLast (fp8_iters = 0 IS svg_kmeans_loop_grouped_strided on it), then mu and the scratch of one e4m3 assignment
//   kLoopMetric    : kLoopStateLast, then the unit rows of c_init (cosine; the dot metric leaves them unused)
enum KmeansLoopKind { kLoopStateLast, kLoopStateFirst, kLoopE4m3, kLoopMetric };
struct KmeansLoopWs {
    KmeansIterWs it;
    int32_t *t_labels, *t_sorted, *t_counts;
    float* t_shift;
    int32_t* state;
    float* mu;
    KmeansE4m3Ws e4m3;
    void* c_unit;
    size_t bytes;   // 0: no loop of these sizes and this group
};
static KmeansLoopWs kmeans_loop_ws(const KmeansCall& a, KmeansLoopKind kind) {
    KmeansLoopWs w{};
    const size_t it_bytes = kmeans_iter_ws(a, nullptr).bytes;
    if (it_bytes == 0 || a.group <= 0 || a.B % a.group != 0) return w;
    Blocks b{(uintptr_t)a.workspace};
    const size_t rows = (size_t)a.B * a.N * 4, state = (size_t)(a.B / a.group) * 4 * sizeof(int32_t);
    if (kind == kLoopStateFirst) w.state = (int32_t*)b.take(state);
    w.it = kmeans_iter_ws(a, b.take(it_bytes));
    w.t_labels = (int32_t*)b.take(rows);
    w.t_sorted = (int32_t*)b.take(rows);
    w.t_counts = (int32_t*)b.take((size_t)a.B * a.K * 4);
    w.t_shift = (float*)b.take((size_t)a.B * 4);
    if (kind != kLoopStateFirst) w.state = (int32_t*)b.take(state);
    if (kind == kLoopE4m3) {
        w.mu = (float*)b.take((size_t)a.B * 128 * sizeof(float));
        w.e4m3 = kmeans_e4m3_ws(a, b.take(0));
        b.off += w.e4m3.bytes;
    }
    if (kind == kLoopMetric) w.c_unit = b.take((size_t)a.B * a.K * a.D * 2);
    w.bytes = b.off;
    return w;
}

// ---- one iteration: an assignment (Euclidean with the |c|^2 bias, bias-free for the metrics, or e4m3) followed by an update
// (kmeans_update_kernel, or kmeans_update_sphere_kernel of csrc/kmeans_metric.hip for the metrics) ----
static int kmeans_assign(const KmeansCall& a, const KmeansStep& s) {
    return dispatch_td(a.dtype, a.D, [&](auto t, auto d) {
        using T = decltype(t);
        constexpr int D = decltype(d)::value;
        return a.metric == SVG_KMEANS_EUCLID ? run_kmeans_assign<T, D, true>(a, s) : run_kmeans_assign<T, D, false>(a, s);
    });
}
static int kmeans_assign_e4m3(const KmeansCall& a, const KmeansStep& s) {
    return dispatch_td(a.dtype, a.D, [&](auto t, auto) { return run_kmeans_assign_e4m3<decltype(t)>(a, s); });
}
static int kmeans_update(const KmeansCall& a, const KmeansStep& s) {
    if (a.metric != SVG_KMEANS_EUCLID) return run_kmeans_update_metric(a, s);
    return dispatch_td(a.dtype, a.D, [&](auto t, auto d) { return run_kmeans_update<decltype(t), decltype(d)::value>(a, s); });
}
// iteration `it` of the record: the first a.fp8_iters iterations assign with the e4m3 scores
static int kmeans_iteration(const KmeansCall& a, const KmeansStep& s, int it) {
    if (const int rc = it < a.fp8_iters ? kmeans_assign_e4m3(a, s) : kmeans_assign(a, s); rc != SVG_OK) return rc;
    return kmeans_update(a, s);
}
static int kmeans_centre(const KmeansCall& a, float* mu) {   // mu = the channel mean of a.c_init
    return dispatch_td(a.dtype, a.D, [&](auto t, auto) {
        using T = decltype(t);
        hipLaunchKernelGGL((kmeans_centre_kernel<T>), dim3(a.B), dim3(256), 0, a.st, (const T*)a.c_init, mu, a.K);
        return launch_status();
    });
}

// ---- the host steps of the Lloyd loop, shared by svg_kmeans_loop* (all of them in one call) and svg_kmeans_stepped_* (one per call) ----
// iteration `it` into the scratch: it == 0 clears the state words and reads c_init, writing c_work_a; odd iterations write c_work_b
static int kmeans_loop_iterate(const KmeansCall& a, const KmeansLoopWs& w, int it) {
    const int G = a.B / a.group;
    if (it == 0 && hipMemsetAsync(w.state, 0, (size_t)4 * G * sizeof(int32_t), a.st) != hipSuccess) return SVG_ERR_LAUNCH;
    const void* cur = it == 0 ? a.c_init : ((it & 1) ? a.c_work_a : a.c_work_b);
    void* out = (it & 1) ? a.c_work_b : a.c_work_a;
    return kmeans_iteration(a, KmeansStep{cur, out, w.t_labels, w.t_counts, w.t_sorted, w.t_shift, w.it, w.mu, w.e4m3}, it);
}

// the commit of iteration `it`; a.maxima == NULL: the group maxima are reduced from the scratch shift inside the kernel
static void kmeans_loop_commit(const KmeansCall& a, const KmeansLoopWs& w, int it, float tol) {
    const int group = a.group, G = a.B / group;
    const int sel_cur = it == 0 ? 0 : ((it & 1) ? 1 : 2), sel_out = (it & 1) ? 2 : 1;   // 0 initial, 1 / 2 the two work buffers
    const long long gn = (long long)group * a.N, gk = (long long)group * a.K;
    // (G = 1: the grid of the ungrouped loop; more groups share about as many workgroups, a stopped group's return at once)
    const dim3 grid((unsigned)std::min<long long>((2048 + G - 1) / G, (gn + 255) / 256), (unsigned)G);
    if (a.maxima)
        hipLaunchKernelGGL(kmeans_commit_kernel<true>, grid, dim3(256), 0, a.st, w.t_labels, w.t_sorted, w.t_counts, a.labels, a.sorted_idx,
                           a.counts, a.maxima, w.state, gn, gk, group, tol, it, sel_cur, sel_out);
    else
        hipLaunchKernelGGL(kmeans_commit_kernel<false>, grid, dim3(256), 0, a.st, w.t_labels, w.t_sorted, w.t_counts, a.labels, a.sorted_idx,
                           a.counts, w.t_shift, w.state, gn, gk, group, tol, it, sel_cur, sel_out);
}

// every group's centroids from the buffer its selector names, and the n_iters words
static int kmeans_loop_finish(const KmeansCall& a, const KmeansLoopWs& w) {
    const int G = a.B / a.group;
    const long long gn8 = (long long)a.group * a.K * a.D / 8;
    const dim3 g2((unsigned)std::min<long long>((1024 + G - 1) / G, (gn8 + 255) / 256), (unsigned)G);
    const int rc = dispatch_td(a.dtype, a.D, [&](auto t, auto) {
        using T = decltype(t);
        hipLaunchKernelGGL((kmeans_select_kernel<T>), g2, dim3(256), 0, a.st, (const T*)a.c_init, (const T*)a.c_work_a, (const T*)a.c_work_b,
                           (T*)a.centroids_out, w.state + 3 * G, gn8);
        return SVG_OK;
    });
    if (rc != SVG_OK) return rc;
    if (hipMemcpyAsync(a.n_iters, w.state + 2 * G, (size_t)G * sizeof(int32_t), hipMemcpyDeviceToDevice, a.st) != hipSuccess) return SVG_ERR_LAUNCH;
    return launch_status();
}

// The loop driver of svg_kmeans_loop*, svg_kmeans_loop_e4m3 and svg_kmeans_loop_metric on a checked record: state clear -> iterate ->
// commit -> ... -> finish.
static int kmeans_loop_run(KmeansCall a, const KmeansLoopWs& w) {
    if (a.metric == SVG_KMEANS_COSINE) {
        // the unit rows of c_init, behind the blocks of the Euclidean loop: from here on they ARE the initial centroids (selector 0), so a
        // group that converges at once returns them, and c_init is never written
        if (const int rc = run_kmeans_unit_rows(a, w.c_unit); rc != SVG_OK) return rc;
        a.c_init = w.c_unit;
    }
    if (a.fp8_iters > 0)   // (fp8_iters = 0: svg_kmeans_loop_grouped_strided, call for call)
        if (const int rc = kmeans_centre(a, w.mu); rc != SVG_OK) return rc;
    for (int it = 0; it < a.max_iters; ++it) {
        if (const int rc = kmeans_loop_iterate(a, w, it); rc != SVG_OK) return rc;
        // an e4m3 iteration never stops a group: a shift is >= 0 or NaN, so nothing is below a tol of -1
        kmeans_loop_commit(a, w, it, it < a.fp8_iters ? -1.f : a.tol);
    }
    return kmeans_loop_finish(a, w);
}

// ---- the entries ----
extern "C" int svg_kmeans_xsq(const void* x, float* xsq, int32_t B, int32_t N, int32_t D, int32_t dtype, void* stream) {
    if (const int rc = first_failure({check_pointers({x, xsq}), check_positive({B, N}), check_D(D)}); rc != SVG_OK) return rc;
    const long long rows = (long long)B * N;
    const int rpb = 256 / (D / 8);
    dim3 grid((unsigned)std::min<long long>(4096, (rows + rpb - 1) / rpb));
    return dispatch_td(dtype, D, [&](auto t, auto) {
        using T = decltype(t);
        hipLaunchKernelGGL((xsq_kernel<T>), grid, dim3(256), 0, (hipStream_t)stream, (const T*)x, xsq, rows, D);
        return launch_status();
    });
}

extern "C" size_t svg_kmeans_workspace_bytes(int32_t B, int32_t N, int32_t K, int32_t D) {
    return kmeans_iter_ws(kmeans_shape(B, N, K, D, B), nullptr).bytes;
}

// One Lloyd iteration.  The workspace is sized before the (dtype, head_dim) pair is looked at: an uncovered pair is the dispatch's answer.
extern "C" int svg_kmeans_iter(const void* x, const float* xsq, const void* centroids_in, void* centroids_out,
                               int32_t* labels, int32_t* counts, int32_t* sorted_idx, float* shift, int32_t B, int32_t N,
                               int32_t K, int32_t D, int32_t dtype, void* workspace, size_t workspace_bytes, void* stream) {
    KmeansCall a = kmeans_call(kmeans_shape(B, N, K, D, B), dtype, workspace, workspace_bytes, stream);
    a.x = x, a.xsq = xsq;
    const KmeansIterWs ws = kmeans_iter_ws(a, workspace);
    const int rc = first_failure({check_pointers({x, centroids_in, centroids_out, labels, counts, sorted_idx, shift, workspace}),
                                  check_positive({B, N, K}), check_K(K), check_workspace(a, ws.bytes)});
    return rc != SVG_OK ? rc : kmeans_iteration(a, KmeansStep{centroids_in, centroids_out, labels, counts, sorted_idx, shift, ws}, 0);
}

// labels[b, n] = argmin_k |x[b, n] - centroids[b, k]|^2 (lowest index on ties): the assignment half of svg_kmeans_iter on its own.
extern "C" int svg_kmeans_assign(const void* x, const void* centroids, int32_t* labels, int32_t B, int32_t N, int32_t K, int32_t D,
                                 int32_t dtype, void* workspace, size_t workspace_bytes, void* stream) {
    KmeansCall a = kmeans_call(kmeans_shape(B, N, K, D, B), dtype, workspace, workspace_bytes, stream);
    a.x = x;
    const KmeansIterWs ws = kmeans_iter_ws(a, workspace);
    const int rc = first_failure({check_pointers({x, centroids, labels, workspace}), check_positive({B, N, K}), check_K(K), check_workspace(a, ws.bytes)});
    return rc != SVG_OK ? rc : kmeans_assign(a, KmeansStep{centroids, nullptr, labels, nullptr, nullptr, nullptr, ws});
}

// The update half on GIVEN labels: stable sort of the labels, per-cluster fp32 means in a fixed order, empty clusters keep
// centroids_in, shift[b] = the largest centre movement (as svg_kmeans_iter).
extern "C" int svg_kmeans_update(const void* x, const int32_t* labels, const void* centroids_in, void* centroids_out, int32_t* counts,
                                 int32_t* sorted_idx, float* shift, int32_t B, int32_t N, int32_t K, int32_t D, int32_t dtype,
                                 void* workspace, size_t workspace_bytes, void* stream) {
    KmeansCall a = kmeans_call(kmeans_shape(B, N, K, D, B), dtype, workspace, workspace_bytes, stream);
    a.x = x;
    const KmeansIterWs ws = kmeans_iter_ws(a, workspace);
    const int rc = first_failure({check_pointers({x, labels, centroids_in, centroids_out, counts, sorted_idx, shift, workspace}),
                                  check_positive({B, N, K}), check_K(K), check_workspace(a, ws.bytes)});
    // (the step's labels are only read by an update)
    return rc != SVG_OK ? rc : kmeans_update(a, KmeansStep{centroids_in, centroids_out, const_cast<int32_t*>(labels), counts, sorted_idx, shift, ws});
}

extern "C" size_t svg_kmeans_loop_grouped_workspace_bytes(int32_t B, int32_t N, int32_t K, int32_t D, int32_t group) {
    return kmeans_loop_ws(kmeans_shape(B, N, K, D, group), kLoopStateLast).bytes;
}

extern "C" size_t svg_kmeans_loop_workspace_bytes(int32_t B, int32_t N, int32_t K, int32_t D) {
    return B > 0 ? svg_kmeans_loop_grouped_workspace_bytes(B, N, K, D, B) : 0;
}

// the record of a loop entry: the part every loop entry takes (x_bs and xsq, metric, fp8_iters are the entry's)
static KmeansCall kmeans_loop_call(KmeansCall a, const void* x, const void* const (&cents)[4], int32_t* const (&outs)[4]) {
    a.x = x, a.c_init = cents[0], a.c_work_a = const_cast<void*>(cents[1]), a.c_work_b = const_cast<void*>(cents[2]);
    a.centroids_out = const_cast<void*>(cents[3]);
    a.labels = outs[0], a.counts = outs[1], a.sorted_idx = outs[2], a.n_iters = outs[3];
    return a;
}

extern "C" int svg_kmeans_loop_grouped(const void* x, const float* xsq, const void* c_init, void* c_work_a, void* c_work_b, int32_t* labels,
                                       int32_t* counts, int32_t* sorted_idx, void* centroids_out, int32_t* n_iters, int32_t B, int32_t N,
                                       int32_t K, int32_t D, int32_t dtype, int32_t group, int32_t max_iters, float tol, void* workspace,
                                       size_t workspace_bytes, void* stream) {
    KmeansCall a = kmeans_loop_call(kmeans_call(kmeans_shape(B, N, K, D, group), dtype, workspace, workspace_bytes, stream), x,
                                    {c_init, c_work_a, c_work_b, centroids_out}, {labels, counts, sorted_idx, n_iters});
    a.xsq = xsq, a.max_iters = max_iters, a.tol = tol;
    const KmeansLoopWs w = kmeans_loop_ws(a, kLoopStateLast);
    const int rc = first_failure({check_loop_pointers(a), check_loop_sizes(a), check_covers(a), check_workspace(a, w.bytes), check_alias(a)});
    return rc != SVG_OK ? rc : kmeans_loop_run(a, w);
}

extern "C" int svg_kmeans_loop_grouped_strided(const void* x, int64_t x_batch_stride, const void* c_init, void* c_work_a, void* c_work_b,
                                               int32_t* labels, int32_t* counts, int32_t* sorted_idx, void* centroids_out, int32_t* n_iters,
                                               int32_t B, int32_t N, int32_t K, int32_t D, int32_t dtype, int32_t group, int32_t max_iters,
                                               float tol, void* workspace, size_t workspace_bytes, void* stream) {
    KmeansCall a = kmeans_loop_call(kmeans_call(kmeans_shape(B, N, K, D, group), dtype, workspace, workspace_bytes, stream), x,
                                    {c_init, c_work_a, c_work_b, centroids_out}, {labels, counts, sorted_idx, n_iters});
    a.x_bs = (long long)x_batch_stride, a.max_iters = max_iters, a.tol = tol;
    const KmeansLoopWs w = kmeans_loop_ws(a, kLoopStateLast);
    const int rc = first_failure({check_strided(a), check_loop_pointers(a), check_loop_sizes(a), check_covers(a), check_workspace(a, w.bytes),
                                  check_alias(a)});
    return rc != SVG_OK ? rc : kmeans_loop_run(a, w);
}

// svg_kmeans_loop and svg_kmeans_loop_strided: one stopping group of all B batches
extern "C" int svg_kmeans_loop(const void* x, const float* xsq, const void* c_init, void* c_work_a, void* c_work_b, int32_t* labels,
                               int32_t* counts, int32_t* sorted_idx, void* centroids_out, int32_t* n_iters, int32_t B, int32_t N,
                               int32_t K, int32_t D, int32_t dtype, int32_t max_iters, float tol, void* workspace,
                               size_t workspace_bytes, void* stream) {
    return svg_kmeans_loop_grouped(x, xsq, c_init, c_work_a, c_work_b, labels, counts, sorted_idx, centroids_out, n_iters, B, N, K, D, dtype, B,
                                   max_iters, tol, workspace, workspace_bytes, stream);
}

extern "C" int svg_kmeans_loop_strided(const void* x, int64_t x_batch_stride, const void* c_init, void* c_work_a, void* c_work_b,
                                       int32_t* labels, int32_t* counts, int32_t* sorted_idx, void* centroids_out, int32_t* n_iters,
                                       int32_t B, int32_t N, int32_t K, int32_t D, int32_t dtype, int32_t max_iters, float tol,
                                       void* workspace, size_t workspace_bytes, void* stream) {
    return svg_kmeans_loop_grouped_strided(x, x_batch_stride, c_init, c_work_a, c_work_b, labels, counts, sorted_idx, centroids_out, n_iters, B, N,
                                           K, D, dtype, B, max_iters, tol, workspace, workspace_bytes, stream);
}

// ---- the Lloyd loop in steps (include/svg_attn_kmeans_stepped.h): the host steps above, one per call, with the group maxima handed out
// by iterate and taken back by commit ----
extern "C" size_t svg_kmeans_stepped_workspace_bytes(int32_t B, int32_t N, int32_t K, int32_t D, int32_t group) {
    if (first_failure({check_K(K), check_D(D)}) != SVG_OK) return 0;
    return kmeans_loop_ws(kmeans_shape(B, N, K, D, group), kLoopStateFirst).bytes;
}

extern "C" int svg_kmeans_stepped_iterate(const void* x, int64_t x_batch_stride, const void* c_init, void* c_work_a, void* c_work_b, int32_t it,
                                          float* maxima, int32_t B, int32_t N, int32_t K, int32_t D, int32_t dtype, int32_t group,
                                          void* workspace, size_t workspace_bytes, void* stream) {
    KmeansCall a = kmeans_call(kmeans_shape(B, N, K, D, group), dtype, workspace, workspace_bytes, stream);
    a.x = x, a.x_bs = (long long)x_batch_stride, a.c_init = c_init, a.c_work_a = c_work_a, a.c_work_b = c_work_b;
    const KmeansLoopWs w = kmeans_loop_ws(a, kLoopStateFirst);
    const int rc = first_failure({check_pointers({x, c_init, c_work_a, c_work_b, maxima, workspace}), check_positive({B, N, K}), check_group(a),
                                  need(it >= 0, SVG_ERR_BAD_ARG), check_covers(a), check_workspace(a, w.bytes), check_alias(a), check_strided(a)});
    if (rc != SVG_OK) return rc;
    if (const int rc2 = kmeans_loop_iterate(a, w, it); rc2 != SVG_OK) return rc2;
    const int G = B / group;
    hipLaunchKernelGGL(kmeans_group_maxima_kernel, dim3((unsigned)std::min(256, (G + 3) / 4)), dim3(256), 0, a.st, w.t_shift, maxima, G, (int)group);
    return launch_status();
}

extern "C" int svg_kmeans_stepped_commit(const float* maxima, int32_t* labels, int32_t* counts, int32_t* sorted_idx, int32_t it, float tol, int32_t B,
                                         int32_t N, int32_t K, int32_t group, void* workspace, size_t workspace_bytes, void* stream) {
    // (no head_dim here: none of the blocks' sizes depends on it — the record carries 128)
    KmeansCall a = kmeans_call(kmeans_shape(B, N, K, 128, group), 0, workspace, workspace_bytes, stream);
    a.maxima = maxima, a.labels = labels, a.counts = counts, a.sorted_idx = sorted_idx;
    const KmeansLoopWs w = kmeans_loop_ws(a, kLoopStateFirst);
    const int rc = first_failure({check_pointers({maxima, labels, counts, sorted_idx, workspace}), check_positive({B, N, K}), check_group(a),
                                  need(it >= 0, SVG_ERR_BAD_ARG), check_K(K), check_workspace(a, w.bytes)});
    if (rc != SVG_OK) return rc;
    kmeans_loop_commit(a, w, it, tol);
    return launch_status();
}

extern "C" int svg_kmeans_stepped_finish(const void* c_init, const void* c_work_a, const void* c_work_b, void* centroids_out, int32_t* n_iters,
                                         int32_t B, int32_t K, int32_t D, int32_t dtype, int32_t group, void* workspace, size_t workspace_bytes,
                                         void* stream) {
    // (no N here: the record carries 1 — the smallest workspace an iterate of these B, K, D, group took; the state words finish reads lie
    //  in front of it)
    KmeansCall a = kmeans_call(kmeans_shape(B, 1, K, D, group), dtype, workspace, workspace_bytes, stream);
    a.c_init = c_init, a.c_work_a = const_cast<void*>(c_work_a), a.c_work_b = const_cast<void*>(c_work_b);   // (read only here)
    a.centroids_out = centroids_out, a.n_iters = n_iters;
    const KmeansLoopWs w = kmeans_loop_ws(a, kLoopStateFirst);
    const int rc = first_failure({check_pointers({c_init, c_work_a, c_work_b, centroids_out, n_iters, workspace}), check_positive({B, K}),
                                  check_group(a), check_covers(a), check_workspace(a, w.bytes), check_alias(a)});
    return rc != SVG_OK ? rc : kmeans_loop_finish(a, w);
}

// ---- the e4m3 assignment and the Lloyd loop that uses it for its first iterations (include/svg_attn_kmeans_e4m3.h) ----
extern "C" int svg_kmeans_centre(const void* centroids, float* mu, int32_t B, int32_t K, int32_t D, int32_t dtype, void* stream) {
    KmeansCall a = kmeans_call(kmeans_shape(B, 1, K, D, B), dtype, nullptr, 0, stream);
    a.c_init = centroids;
    const int rc = first_failure({check_pointers({centroids, mu}), check_positive({B, K}), check_e4m3_covers(a)});
    return rc != SVG_OK ? rc : kmeans_centre(a, mu);
}

extern "C" size_t svg_kmeans_assign_e4m3_workspace_bytes(int32_t B, int32_t N, int32_t K, int32_t D) {
    if (check_positive({B, N, K}) != SVG_OK || check_K(K) != SVG_OK || D != 128) return 0;
    return kmeans_e4m3_ws(kmeans_shape(B, N, K, D, B), nullptr).bytes;
}

extern "C" int svg_kmeans_assign_e4m3(const void* x, const void* centroids, const float* mu, int32_t* labels, int32_t B, int32_t N, int32_t K,
                                      int32_t D, int32_t dtype, void* workspace, size_t workspace_bytes, void* stream) {
    KmeansCall a = kmeans_call(kmeans_shape(B, N, K, D, B), dtype, workspace, workspace_bytes, stream);
    a.x = x;
    KmeansStep s{};
    s.c_in = centroids, s.labels = labels, s.mu = mu, s.e4m3 = kmeans_e4m3_ws(a, workspace);   // (mu may be NULL: zeros)
    const int rc = first_failure({check_pointers({x, centroids, labels, workspace}), check_positive({B, N, K}), check_e4m3_covers(a),
                                  check_workspace(a, s.e4m3.bytes),
                                  need((((size_t)x | (size_t)mu) & 15) == 0, SVG_ERR_UNSUPPORTED)});   // (16-byte loads of rows and of mu)
    return rc != SVG_OK ? rc : kmeans_assign_e4m3(a, s);
}

extern "C" size_t svg_kmeans_loop_e4m3_workspace_bytes(int32_t B, int32_t N, int32_t K, int32_t D, int32_t group) {
    if (check_K(K) != SVG_OK || D != 128) return 0;
    return kmeans_loop_ws(kmeans_shape(B, N, K, D, group), kLoopE4m3).bytes;
}

extern "C" int svg_kmeans_loop_e4m3(const void* x, int64_t x_batch_stride, const void* c_init, void* c_work_a, void* c_work_b, int32_t* labels,
                                    int32_t* counts, int32_t* sorted_idx, void* centroids_out, int32_t* n_iters, int32_t B, int32_t N,
                                    int32_t K, int32_t D, int32_t dtype, int32_t group, int32_t max_iters, float tol, int32_t fp8_iters,
                                    void* workspace, size_t workspace_bytes, void* stream) {
    KmeansCall a = kmeans_loop_call(kmeans_call(kmeans_shape(B, N, K, D, group), dtype, workspace, workspace_bytes, stream), x,
                                    {c_init, c_work_a, c_work_b, centroids_out}, {labels, counts, sorted_idx, n_iters});
    a.x_bs = (long long)x_batch_stride, a.max_iters = max_iters, a.tol = tol, a.fp8_iters = fp8_iters;
    const KmeansLoopWs w = kmeans_loop_ws(a, kLoopE4m3);
    const int rc = first_failure({check_loop_pointers(a), check_loop_sizes(a), need(fp8_iters >= 0 && fp8_iters <= max_iters, SVG_ERR_BAD_ARG),
                                  check_e4m3_covers(a), check_workspace(a, w.bytes), check_alias(a), check_strided(a)});
    return rc != SVG_OK ? rc : kmeans_loop_run(a, w);
}

// ---- the cosine and dot-product metrics (include/svg_attn_kmeans_metric.h): the bias-free assignment, the update of
// csrc/kmeans_metric.hip, and the loop driver with a metric ----
extern "C" int svg_kmeans_assign_metric(const void* x, const void* centroids, int32_t* labels, int32_t B, int32_t N, int32_t K, int32_t D,
                                        int32_t dtype, int32_t metric, void* workspace, size_t workspace_bytes, void* stream) {
    KmeansCall a = kmeans_call(kmeans_shape(B, N, K, D, B), dtype, workspace, workspace_bytes, stream);
    a.x = x, a.metric = metric;
    const KmeansIterWs ws = kmeans_iter_ws(a, workspace);
    const int rc = first_failure({check_pointers({x, centroids, labels, workspace}), check_positive({B, N, K}), check_metric(a), check_covers(a),
                                  check_workspace(a, ws.bytes)});
    return rc != SVG_OK ? rc : kmeans_assign(a, KmeansStep{centroids, nullptr, labels, nullptr, nullptr, nullptr, ws});
}

extern "C" int svg_kmeans_update_metric(const void* x, const int32_t* labels, const void* centroids_in, void* centroids_out, int32_t* counts,
                                        int32_t* sorted_idx, float* shift, int32_t B, int32_t N, int32_t K, int32_t D, int32_t dtype,
                                        int32_t metric, void* workspace, size_t workspace_bytes, void* stream) {
    KmeansCall a = kmeans_call(kmeans_shape(B, N, K, D, B), dtype, workspace, workspace_bytes, stream);
    a.x = x, a.metric = metric;
    const KmeansIterWs ws = kmeans_iter_ws(a, workspace);
    const int rc = first_failure({check_pointers({x, labels, centroids_in, centroids_out, counts, sorted_idx, shift, workspace}),
                                  check_positive({B, N, K}), check_metric(a), check_covers(a), check_workspace(a, ws.bytes)});
    return rc != SVG_OK ? rc : kmeans_update(a, KmeansStep{centroids_in, centroids_out, const_cast<int32_t*>(labels), counts, sorted_idx, shift, ws});
}

extern "C" size_t svg_kmeans_loop_metric_workspace_bytes(int32_t B, int32_t N, int32_t K, int32_t D, int32_t group) {
    if (first_failure({check_K(K), check_D(D)}) != SVG_OK) return 0;
    return kmeans_loop_ws(kmeans_shape(B, N, K, D, group), kLoopMetric).bytes;
}

extern "C" int svg_kmeans_loop_metric(const void* x, int64_t x_batch_stride, const void* c_init, void* c_work_a, void* c_work_b, int32_t* labels,
                                      int32_t* counts, int32_t* sorted_idx, void* centroids_out, int32_t* n_iters, int32_t B, int32_t N,
                                      int32_t K, int32_t D, int32_t dtype, int32_t metric, int32_t group, int32_t max_iters, float tol,
                                      void* workspace, size_t workspace_bytes, void* stream) {
    KmeansCall a = kmeans_loop_call(kmeans_call(kmeans_shape(B, N, K, D, group), dtype, workspace, workspace_bytes, stream), x,
                                    {c_init, c_work_a, c_work_b, centroids_out}, {labels, counts, sorted_idx, n_iters});
    a.x_bs = (long long)x_batch_stride, a.metric = metric, a.max_iters = max_iters, a.tol = tol;
    const KmeansLoopWs w = kmeans_loop_ws(a, kLoopMetric);
    const int rc = first_failure({check_loop_pointers(a), check_loop_sizes(a), check_metric(a), check_covers(a), check_workspace(a, w.bytes),
                                  check_alias(a), check_strided(a)});
    return rc != SVG_OK ? rc : kmeans_loop_run(a, w);
}

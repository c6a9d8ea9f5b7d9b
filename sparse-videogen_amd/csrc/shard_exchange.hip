// svg_copy_boxes (include/svg_attn_shard_exchange.h): the pack / unpack layouts either side of the two all-to-all exchanges of a token-sharded
// layer-call as ONE batched strided copy of rows of D 16-bit elements.  HBM-bound: every lane moves 16-byte chunks, kCopyUnroll loads in
// flight before the first store; no LDS.
//
// Work unit: a TILE of kRows consecutive rows along extent[2] of one (i0, i1) of one box of one tensor.  A tile's tensor, box, i0, i1 and
// first row are the same for the whole workgroup, so the search through the launch's segments and the two divisions run on the scalar
// unit from the kernel arguments; a lane's own arithmetic is one row index, a bound test and one 64-bit multiply-add per address.  A
// lane's chunks of one pass are neighbours in the row (kD / 8 lanes cover a row of 128 or 256 bytes: whole cache lines on both sides).
#include "svg_common.h"

namespace svg {

constexpr int kCopyThreads = 256;
constexpr int kCopyUnroll = 4;                                                   // 16-byte loads of a lane in flight
constexpr int kCopyMaxSegs = SVG_COPY_MAX_TENSORS * SVG_COPY_MAX_BOXES;          // (tensor, box) pairs of one launch
constexpr int kCopyMaxGrid = 2048;                                               // 256 CUs x 8 workgroups; the rest by grid stride

struct CopyArgs {
    const char* src[SVG_COPY_MAX_TENSORS];
    char* dst[SVG_COPY_MAX_TENSORS];
    svg_copy_box_t box[SVG_COPY_MAX_BOXES];
    uint32_t seg_end[kCopyMaxSegs];      // tiles of segments 0..s, cumulative; segments without a tile are not listed
    uint8_t seg_tensor[kCopyMaxSegs], seg_box[kCopyMaxSegs];
    uint32_t total;                      // seg_end[n_seg - 1]
};

template <int kD>
constexpr int copy_tile_rows() {
    return kCopyThreads * kCopyUnroll / (kD / 8);
}

template <int kD>
__global__ __launch_bounds__(kCopyThreads) void copy_boxes_kernel(const CopyArgs a) {
    constexpr int kCpr = kD / 8;                     // 16-byte chunks of a row
    constexpr int kPass = kCopyThreads / kCpr;       // rows one pass of the workgroup covers
    constexpr int kRows = copy_tile_rows<kD>();
    const int row_in_pass = (int)threadIdx.x / kCpr;
    const int chunk_bytes = ((int)threadIdx.x % kCpr) * 16;
    for (uint32_t tile = blockIdx.x; tile < a.total; tile += gridDim.x) {
        // uniform: the segment of this tile, then (i0, i1, first row) inside its box
        int s = 0;
        while (tile >= a.seg_end[s]) ++s;            // (tile < total = the last listed seg_end: s stays inside the list)
        const uint32_t u = tile - (s ? a.seg_end[s - 1] : 0u);
        const int t = a.seg_tensor[s];
        const svg_copy_box_t& b = a.box[a.seg_box[s]];
        const uint32_t n1 = (uint32_t)b.extent[1], n2 = (uint32_t)b.extent[2];
        const uint32_t tiles2 = (n2 + kRows - 1) / kRows;
        const uint32_t outer = u / tiles2;
        const uint32_t r0 = (u - outer * tiles2) * kRows;
        const uint32_t i0 = outer / n1, i1 = outer - i0 * n1;
        const char* const sp = a.src[t] + 2 * (b.src_offset + (int64_t)i0 * b.src_stride[0] + (int64_t)i1 * b.src_stride[1]);
        char* const dp = a.dst[t] + 2 * (b.dst_offset + (int64_t)i0 * b.dst_stride[0] + (int64_t)i1 * b.dst_stride[1]);
        const int64_t ss = 2 * b.src_stride[2], ds = 2 * b.dst_stride[2];
        u32x4 v[kCopyUnroll];
#pragma unroll
        for (int j = 0; j < kCopyUnroll; ++j) {
            const uint32_t r = r0 + j * kPass + row_in_pass;
            if (r < n2) v[j] = *(const u32x4*)(sp + (int64_t)r * ss + chunk_bytes);
        }
#pragma unroll
        for (int j = 0; j < kCopyUnroll; ++j) {
            const uint32_t r = r0 + j * kPass + row_in_pass;
            if (r < n2) *(u32x4*)(dp + (int64_t)r * ds + chunk_bytes) = v[j];
        }
    }
}

}  // namespace svg

using namespace svg;

extern "C" int svg_copy_boxes(const svg_copy_tensor_t* tensors, int32_t n_tensors, const svg_copy_box_t* boxes, int32_t n_boxes, int32_t D,
                              int32_t dtype, void* stream) {
    if (!tensors || !boxes || n_tensors < 1 || n_tensors > SVG_COPY_MAX_TENSORS || n_boxes < 1 || n_boxes > SVG_COPY_MAX_BOXES)
        return SVG_ERR_BAD_ARG;
    for (int t = 0; t < n_tensors; ++t) {
        const svg_copy_tensor_t& x = tensors[t];
        if (!x.src || !x.dst || x.box_begin < 0 || x.box_count < 0 || x.box_begin > n_boxes || x.box_count > n_boxes - x.box_begin)
            return SVG_ERR_BAD_ARG;
    }
    for (int i = 0; i < n_boxes; ++i) {
        const svg_copy_box_t& b = boxes[i];
        if (b.src_offset < 0 || b.dst_offset < 0) return SVG_ERR_BAD_ARG;
        for (int d = 0; d < 3; ++d)
            if (b.extent[d] < 0 || b.src_stride[d] < 0 || b.dst_stride[d] < 0) return SVG_ERR_BAD_ARG;
    }
    for (int t = 0; t < n_tensors; ++t)
        if (tensors[t].src == tensors[t].dst) return SVG_ERR_BAD_ARG;
    if (D != 64 && D != 128) return SVG_ERR_UNSUPPORTED;
    if (dtype != SVG_DTYPE_BF16 && dtype != SVG_DTYPE_F16) return SVG_ERR_UNSUPPORTED;
    for (int t = 0; t < n_tensors; ++t)
        if ((((size_t)tensors[t].src) | ((size_t)tensors[t].dst)) & 15) return SVG_ERR_UNSUPPORTED;
    constexpr int64_t kMaxElems = 1ll << 40;
    for (int i = 0; i < n_boxes; ++i) {
        const svg_copy_box_t& b = boxes[i];
        if (((b.src_offset | b.dst_offset) & 7) || b.src_offset >= kMaxElems || b.dst_offset >= kMaxElems) return SVG_ERR_UNSUPPORTED;
        for (int d = 0; d < 3; ++d)
            if (((b.src_stride[d] | b.dst_stride[d]) & 7) || b.src_stride[d] >= kMaxElems || b.dst_stride[d] >= kMaxElems)
                return SVG_ERR_UNSUPPORTED;
    }
    // the segments: (tensor, box) pairs with at least one tile, and their cumulative tile counts
    const int rows_per_tile = D == 64 ? copy_tile_rows<64>() : copy_tile_rows<128>();
    CopyArgs a{};
    int n_seg = 0;
    int64_t total = 0;
    for (int t = 0; t < n_tensors; ++t) {
        a.src[t] = (const char*)tensors[t].src;
        a.dst[t] = (char*)tensors[t].dst;
        for (int i = tensors[t].box_begin; i < tensors[t].box_begin + tensors[t].box_count; ++i) {
            const svg_copy_box_t& b = boxes[i];
            const int64_t tiles = (int64_t)b.extent[0] * b.extent[1] * (((int64_t)b.extent[2] + rows_per_tile - 1) / rows_per_tile);
            if (tiles == 0) continue;
            total += tiles;
            if (total > 0x7fffffffll) return SVG_ERR_UNSUPPORTED;
            a.seg_end[n_seg] = (uint32_t)total;
            a.seg_tensor[n_seg] = (uint8_t)t;
            a.seg_box[n_seg] = (uint8_t)i;
            ++n_seg;
        }
    }
    if (total == 0) return SVG_OK;   // every box empty: nothing to copy, no launch
    for (int i = 0; i < n_boxes; ++i) a.box[i] = boxes[i];
    a.total = (uint32_t)total;
    const unsigned grid = (unsigned)(total < kCopyMaxGrid ? total : kCopyMaxGrid);
    if (D == 64) hipLaunchKernelGGL(copy_boxes_kernel<64>, dim3(grid), dim3(kCopyThreads), 0, (hipStream_t)stream, a);
    else hipLaunchKernelGGL(copy_boxes_kernel<128>, dim3(grid), dim3(kCopyThreads), 0, (hipStream_t)stream, a);
    return launch_status();
}

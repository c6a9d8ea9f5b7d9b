/* The exchange layouts of token-shard mode as ONE batched strided copy: part of the C ABI of libsvgattn (include/svg_attn.h includes this file
 * at its end; the error codes and conventions are the ones documented there, SVG_ABI_VERSION is unchanged).  A header of its own for the
 * reason include/svg_attn_sparse_lse.h gives; the validation table of the entry is tests/test_token_shards_cpu.py, and svg/_native.py binds
 * it from SHARD_EXCHANGE_SIGNATURES. */
#ifndef SVG_ATTN_SHARD_EXCHANGE_H_
#define SVG_ATTN_SHARD_EXCHANGE_H_
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SVG_COPY_MAX_TENSORS 3
#define SVG_COPY_MAX_BOXES 16

/* One box: extent[0] * extent[1] * extent[2] rows of D contiguous 16-bit elements.  Row (i0, i1, i2) is read at
 *   src + src_offset + i0 * src_stride[0] + i1 * src_stride[1] + i2 * src_stride[2]
 * and written at the same expression of the dst_* members; offsets and strides in ELEMENTS.  The kernel's tiles run along extent[2]:
 * give the longest extent (the rows of a shard) there. */
typedef struct {
    int64_t src_offset, dst_offset;
    int32_t extent[3];
    int32_t reserved;        /* 0 */
    int64_t src_stride[3], dst_stride[3];
} svg_copy_box_t;

/* One tensor of a launch: its two base pointers and the boxes [box_begin, box_begin + box_count) of the launch's list it copies — q, k and
 * v of one layer-call share the boxes of a layout; a v that is a view of a fused projection brings boxes (source strides) of its own. */
typedef struct {
    const void* src;
    void* dst;
    int32_t box_begin, box_count;
} svg_copy_tensor_t;

/* svg_copy_boxes: every box of every tensor in ONE launch — the pack and unpack steps either side of the two all-to-all exchanges of a
 * token-sharded layer-call (svg/distributed.py run_token_sharded; the builders of the four layouts are in svg/_native.py), which are
 * otherwise `world` strided copies per tensor.  The descriptors travel in the kernel arguments: no device table, no host-to-device copy,
 * nothing is allocated or synchronised.  HBM-bound: 16-byte loads and stores, the grid flattened over the row tiles of all boxes of all
 * tensors, bounded, with a grid-stride loop; no LDS.  Boxes may not overlap in the destination, and no source row may be a destination
 * row of the same launch (the caller's business: the order of the copies is not defined).
 * A box with a zero extent copies nothing; nothing outside the boxes' destination rows is written.
 * Return codes, all decided on the host before any launch, in this order:
 *   SVG_ERR_BAD_ARG      tensors or boxes NULL, n_tensors outside 1..SVG_COPY_MAX_TENSORS, n_boxes outside 1..SVG_COPY_MAX_BOXES, a tensor
 *                        with a NULL src or dst or with [box_begin, box_begin + box_count) outside [0, n_boxes], a negative extent,
 *                        stride or offset;
 *   SVG_ERR_BAD_ARG      src == dst for a tensor;
 *   SVG_ERR_UNSUPPORTED  D not in {64, 128}, a dtype other than bf16 / fp16, a base pointer, an offset or a stride that is not 16-byte
 *                        aligned (8 elements), an offset or a stride of 2^40 elements or more, more than 2^31 - 1 row tiles in all. */
int svg_copy_boxes(const svg_copy_tensor_t* tensors, int32_t n_tensors, const svg_copy_box_t* boxes, int32_t n_boxes, int32_t D, int32_t dtype,
                   void* stream);

#ifdef __cplusplus
}
#endif
#endif /* SVG_ATTN_SHARD_EXCHANGE_H_ */

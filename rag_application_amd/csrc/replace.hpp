// Host-side launch prototypes of replace.hip (libhx, gfx950): upsert by an existing id.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace hx {

// ---- replace.hip: upsert by an existing id (hx_replace_rows, hx_payload_replace*) -------------------------------------
// dst row rows[i] = src row i, i < count (row_bytes a multiple of 16; one 4-byte value per row for _u32).  src and dst are
// different allocations and the rows unique: one launch per array.
void launch_scatter_rows16(const void* src, void* dst, int64_t row_bytes, const uint32_t* rows, int64_t count,
                           hipStream_t st);
void launch_scatter_u32(const void* src, void* dst, const uint32_t* rows, int64_t count, hipStream_t st);
// map[rows[i] - f] = i for rows[i] in [f, f + docs) (the caller fills map[0, docs) with 0xFFFFFFFF = not replaced)
void launch_splice_map(const uint32_t* rows, int64_t count, int64_t f, int64_t docs, uint32_t* map, hipStream_t st);
// CSR splice over the m documents from f on (indptr = the stored offsets at document f, new_indptr = the batch's):
// len[j] = the batch vector's length where map[j] names one, the old length otherwise; the segmented copy to idx2 / val2
// at off[j] (off = exclusive prefix of len) reads a replaced document from new_idx / new_val and any other from idx /
// val, with the min / max of the copied weights merged into mm[0] / mm[1] (orderable u32, as launch_minmax_f32)
void launch_csr_splice_len(const int64_t* indptr, const uint32_t* map, const int64_t* new_indptr, int64_t m, int64_t* len,
                           hipStream_t st);
void launch_csr_splice(const int64_t* indptr, const uint32_t* map, const int64_t* new_indptr, const int64_t* off, int64_t m,
                       const int32_t* idx, const float* val, const int32_t* new_idx, const float* new_val, int32_t* idx2,
                       float* val2, uint32_t* mm, hipStream_t st);
// the same segmented copy for one 4-byte element plane of a payload list column
void launch_csr_splice_u32(const int64_t* indptr, const uint32_t* map, const int64_t* new_indptr, const int64_t* off,
                           int64_t m, const uint32_t* src, const uint32_t* new_src, uint32_t* dst, hipStream_t st);

}  // namespace hx

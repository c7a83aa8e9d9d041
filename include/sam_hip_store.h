/* sam_hip_store.h -- batches gathered by index from region features that stay resident in device memory.  An extension of the
 * model's ABI: additive (sam_abi_version() stays what it was), declared here and in no other header; a C caller includes this file, which includes
 * sam_hip.h.  Same conventions as there.
 *
 * The store keeps the rows of all images back to back (CSR): image g owns rows row_off[g] .. row_off[g + 1] - 1 of every row matrix of its group
 * (row_off int64 [n_images + 1]; total_rows = the row count of the matrices).  A batch is sample_idx int32 [B]: question indices when image_of (int32
 * [n_questions], the image of every question) is given, else image indices (image_of NULL; n_questions is then the index range and must equal n_images).
 *
 * Part descriptors are HOST arrays of int64 words, read before the launch and passed by value (at most 8 parts per call):
 *   sam_store_gather_ragged: 5 words per part  {src, ld_src_bytes, dst, ld_dst_bytes, row_bytes}
 *   sam_store_gather_fixed:  6 words per part  {src, ld_src_bytes, dst, ld_dst_bytes, row_bytes, key}      key 0: row = the question, 1: row = its image
 * src / dst are device addresses, the strides are in BYTES (>= row_bytes >= 1); a row is copied as bytes, whatever its element type: with 16-byte
 * accesses when both addresses and both strides are multiples of 16, with 4-byte accesses when they are multiples of 4, byte by byte otherwise, and
 * the bytes of a row past the last whole access byte by byte.  Source addressing is 64-bit throughout.
 *
 * sam_store_gather_ragged writes the ragged batch sam_ragged_expand reads, one launch per token group:
 *   for sample b: q = sample_idx[b], g = image_of ? image_of[q] : q, lo = row_off[g], hi = row_off[g + 1],
 *                 cnt = min(max(hi - lo, 0), n_max)                      -- only the first n_max rows are kept
 *   counts_out[b] = cnt; destination row off(b) + i (off = the exclusive prefix sum of the counts of the samples in front) of every part receives
 *   source row lo + i for i < cnt, as long as off(b) + i < cap_rows.  Destination rows at or past the total are not written.
 *   Nothing read from device memory is trusted:
 *     q outside [0, n_questions) or g outside [0, n_images):  cnt = 0, status[b] |= 1
 *     [lo, lo + cnt) not inside [0, total_rows]:                the range is cut to its part inside (cnt shrinks, lo moves to 0), status[b] |= 2
 *   status int32 [B] is only ever OR-ed into: zero it before the first call.  B >= 1, n_max >= 1, B * n_max < 2^31, n_parts in [1, 8], cap_rows >= 1.
 *
 * sam_store_gather_fixed copies one row per sample and part: row q (key 0) or row g (key 1) of src to row b of dst.  A sample whose q is out of range
 * (key 1: or whose g is) gets a row of zero bytes and status[b] |= 1.  B >= 1, n_parts in [1, 8].
 *
 * One wave per (destination row, part), four waves per 256-thread block, no atomics, no workspace, nothing read back by the host. */
#ifndef SAM_HIP_STORE_H
#define SAM_HIP_STORE_H
#include "sam_hip.h"
#ifdef __cplusplus
extern "C" {
#endif

int sam_store_gather_ragged(const int32_t* sample_idx, int B, const int32_t* image_of, int n_questions, const int64_t* row_off, int n_images,
                            int64_t total_rows, int n_max, const int64_t* parts, int n_parts, int32_t* counts_out, int32_t* status, int cap_rows,
                            void* stream);
int sam_store_gather_fixed(const int32_t* sample_idx, int B, const int32_t* image_of, int n_questions, int n_images, const int64_t* parts, int n_parts,
                           int32_t* status, void* stream);

#ifdef __cplusplus
}
#endif
#endif

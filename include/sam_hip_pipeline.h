/* sam_hip_pipeline.h -- entry points of libsam_hip.so that replace work of the reference's DATASET, not of its model: tensors the reference
 * precomputes on the host, caches on disk and ships with every batch are derived here, on the device, from inputs the step already holds.
 *
 * The second public header of the library.  sam_hip.h is the model's ABI (versioned by sam_abi_version()); this header adds entry points next to
 * it without touching that ABI.  Same conventions: plain C, every function returns 0 or a SAM_ERR_* code of sam_hip.h with a message in
 * sam_last_error(), arguments are checked before any device call, launches go to the caller's stream and nothing synchronises, no workspace,
 * no atomics.  The declarations use the spellings sam_hip.h uses (the ctypes binding is derived from both headers by one parser).
 */
#ifndef SAM_HIP_PIPELINE_H
#define SAM_HIP_PIPELINE_H
#include "sam_hip.h"
#include "sam_hip_text.h"     /* the entry points that start from the OCR tokens' text (sam_phoc_from_text) */
#ifdef __cplusplus
extern "C" {
#endif

/* ---- spatial allow bits straight from the batch's boxes, one launch ----
 * The reference builds the spatial graph of a sample in Python (sam/spatial_utils.py:92-218: covers / inside / IoU >= 0.5 / eight direction
 * sectors within a distance limit / self), broadcasts it to a multi-hot [n, n, 12] tensor (:33-52), composes the context's neighbouring sectors
 * (sam/datasets/textvqa_dataset.py:378-409), pickles the result and ships int8 [B,150,150,12] per context with every batch; the model turns it
 * into additive masks per layer (sam/sa_m4c.py:470-552) and min-combines them with the attention mask (:568).
 * This entry point goes from the boxes to the allow bits of sam_mask_bits_spatial with no [B,n,n,12] tensor anywhere.
 *
 * CONTRACT, by equivalence: for every accepted argument set `out` equals, bit for bit and in all NW words of every row (words past N read 0),
 *     sam_mask_bits_spatial(base, adj, B, N, NW, T, n_obj + n_ocr, 12, H, quadrant_bits, out)
 *     with adj = sam_spatial_relation_tensor(float64(cat(obj[..., :4], ocr[..., :4])), B, n_obj + n_ocr, context, distance_threshold).
 * Both kernels are compiled from one copy of the pair classification (csrc/spatial_pair.h); the equality is checked bit for bit by the tests, pairs
 * on sector boundaries included.  fp32 -> f64 is exact, and the dataset's own f64 boxes hold fp32 values, so fp32 device boxes (the batch's pad_obj_bboxes / pad_ocr_bboxes, row stride 5) reproduce the reference's graph.  A padding
 * row is an all-zero box, as in the reference.
 *
 * base u32 [B,1,N,NW] as for sam_mask_bits_spatial; obj_boxes [B, n_obj, ld_obj] and ocr_boxes [B, n_ocr, ld_ocr] (element strides ld >= 4,
 * normalised xyxy in columns 0..3; n_obj > 0 -- a batch without an object group is refused --; ocr_boxes may be NULL with n_ocr = 0);
 * boxes_f64: 0 = fp32 rows, 1 = float64 rows; the sequence is T text rows | n_obj | n_ocr | decoder rows, T + n_obj + n_ocr <= N <= 32 * NW; context in {1,3,5,7,9}; H >= 12 heads (heads >= 12 carry no
 * spatial restriction); quadrant_bits as for sam_mask_bits_spatial (legal ids 1,2,4,7,8,9); out u32 [B,H,N,NW].
 * One wave per (batch, query) row; only object / OCR rows do box arithmetic (float64, one key per lane). */
int sam_mask_bits_from_boxes(const uint32_t* base, const void* obj_boxes, int64_t ld_obj, int n_obj, const void* ocr_boxes, int64_t ld_ocr, int n_ocr,
                             int boxes_f64, int B, int N, int NW, int T, int H, int context, double distance_threshold, unsigned quadrant_bits,
                             uint32_t* out, void* stream);

#ifdef __cplusplus
}
#endif
#endif

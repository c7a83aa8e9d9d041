/* sam_hip_aux_targets.h -- what the spatial aux heads' loss reads (sam_hip_aux_loss.h: codes, valid), in ONE launch from what a batch ships: the
 * 12-channel relation tensor spatial_adj_matrices["1"] and the two padding masks.  An extension of the model's ABI: additive (sam_abi_version() stays
 * what it was), declared here and in no other header; a C caller includes this file, which includes sam_hip.h.  Same conventions as there.
 *
 * sam_aux_targets:
 *   rel        int8 [B, n, n, 12] contiguous, any byte alignment; NULL: only `valid` is written (a batch that builds its codes from boxes,
 *              sam_relation_codes_from_boxes) and `codes` is not touched (it may be NULL too)
 *   obj_mask   [B, n_obj], ocr_mask [B, n_ocr]: integer or bool elements of mask_elem_bytes (1, 4 or 8) bytes each, unit column stride, row strides
 *              ld_obj / ld_ocr in ELEMENTS, pointers aligned to the element size.  An element is valid iff any of its bits is set.  ocr_mask may
 *              be NULL with n_ocr = 0.
 *   valid      uint8 [B, n], n = n_obj + n_ocr: valid[b, i] = 1 iff element i of the concatenated mask rows is non-zero, else 0
 *   codes      uint8 [B, n, n]: where valid[b, i] & valid[b, j], sum_r (r + 1) * rel[b, i, j, r] (the relation code 1..12 of a one-hot row, 0 of an
 *              all-zero row; entries outside {0, 1} are unspecified); elsewhere 0 -- the 12 bytes of such a pair may hold anything and are not
 *              relied upon.  The loss kernels never read a pair with a row that is not valid.
 * B == 0 or n == 0: success, nothing is launched.  n <= 32767.  One launch, no atomics, no workspace, nothing read back. */
#ifndef SAM_HIP_AUX_TARGETS_H
#define SAM_HIP_AUX_TARGETS_H
#include "sam_hip.h"
#ifdef __cplusplus
extern "C" {
#endif

int sam_aux_targets(const int8_t* rel, const void* obj_mask, int64_t ld_obj, int n_obj, const void* ocr_mask, int64_t ld_ocr, int n_ocr,
                    int mask_elem_bytes, int B, int n, uint8_t* codes, uint8_t* valid, void* stream);

#ifdef __cplusplus
}
#endif
#endif

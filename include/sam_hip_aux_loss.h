/* sam_hip_aux_loss.h -- the loss that trains the spatial auxiliary heads, part of the model's ABI: sam_hip.h includes this file beside
 * sam_aux_pair_fwd / sam_aux_pair_bwd, and a C caller needs nothing but sam_hip.h.  Same conventions as there.
 *
 * The loss is this project's own (the reference computes spatial_head_out and stops, sam/sa_m4c.py:194, 316-347).  With
 *   S[b,i,j,r] = spatial_classifier(f(O[b,i], D[b,j]))[r]           the scores of sam_aux_pair_fwd, never written to memory here
 *   Y[b,i,j,r] = (codes[b,i,j] == r + 1)                            codes u8 [B, n, n]: 0 no relation, 1..12 relation; the 12-channel one-hot that
 *                                                                   torch_broadcast_adj_matrix makes of the base relation code (spatial context 1)
 *   M[b,i,j]   = valid[b,i] & valid[b,j]                            valid u8 [B, n]: 1 for a real object / OCR row (the diagonal counts)
 *   loss  = sum(M * (max(S,0) - S*Y + log1p(exp(-|S|)))) / max(count, 1),   count = sum(M)       (M4CDecodingBCEWithMaskLoss's normalisation)
 * A batch without a valid pair gives loss 0, count 0 and all-zero gradients.  Rows that are not valid are never used: they may hold anything.
 *
 * sam_aux_pair_loss_fwd: O, D fp32 [B, n, 32], W fp32 [12, 32], bias fp32 [12] -> loss fp32 [1], count fp32 [1].  Block partials (loss sum, pair count)
 *   go to `ws` (sam_aux_pair_loss_fwd_ws_bytes(B, n) bytes) and one block sums them in a fixed order.
 * sam_aux_pair_loss_bwd: the gradient of grad_out * loss: G = (sigmoid(S) - Y) * M * grad_out / max(count, 1) is rebuilt per pair in registers and fed
 *   to sam_aux_pair_bwd's block; writes dO, dD fp32 [B, n, 32] (rows that are not valid: exact zeros); dW [12, 32] and dbias [12] are added to
 *   (accumulate) or overwritten.  grad_out (NULL = 1) and count (the forward's) are DEVICE scalars read by the kernel: nothing is read back on the host.
 *   `ws`: sam_aux_pair_loss_bwd_ws_bytes(B, n) bytes.
 * Both: no atomics, grids sized from the shape alone: bit-identical from run to run and under sam_set_cu_reserve.  Nothing of size [B, n, n, 12] is
 * written or read.  O, D and ws 16-byte aligned; fusion SAM_AUX_MUL | SAM_AUX_ADD; any B in [1, 65535], n >= 1.  The pairs are counted in integers and
 * `count` holds the total as fp32: exact up to 2^24 valid pairs (B n^2), rounded to fp32 above that, and the divisor with it.
 *
 * sam_relation_codes_from_boxes: codes u8 [B, n, n], n = n_obj + n_ocr, from the batch's boxes (arguments as sam_mask_bits_from_boxes takes them:
 *   element strides ld >= 4, xyxy in columns 0..3, boxes_f64 0 = fp32 rows, 1 = float64 rows; ocr_boxes may be NULL with n_ocr = 0): the relation
 *   code whose channel sam_spatial_relation_tensor(context = 1) sets, 0 where it sets none.  One launch, one thread per pair. */
#ifndef SAM_HIP_AUX_LOSS_H
#define SAM_HIP_AUX_LOSS_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

int64_t sam_aux_pair_loss_fwd_ws_bytes(int B, int n);
int sam_aux_pair_loss_fwd(const float* O, const float* D, const float* W, const float* bias, const uint8_t* codes, const uint8_t* valid, int B, int n,
                          int fusion, float* loss, float* count, float* ws, int64_t ws_bytes, void* stream);
int64_t sam_aux_pair_loss_bwd_ws_bytes(int B, int n);
int sam_aux_pair_loss_bwd(const float* grad_out, const float* count, const float* O, const float* D, const float* W, const float* bias,
                          const uint8_t* codes, const uint8_t* valid, int B, int n, int fusion, float* dO, float* dD, float* dW, float* dbias,
                          int accumulate, float* ws, int64_t ws_bytes, void* stream);
int sam_relation_codes_from_boxes(const void* obj_boxes, int64_t ld_obj, int n_obj, const void* ocr_boxes, int64_t ld_ocr, int n_ocr, int boxes_f64,
                                  int B, double distance_threshold, uint8_t* codes, void* stream);

#ifdef __cplusplus
}
#endif
#endif

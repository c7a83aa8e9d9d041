/* sam_hip_aux_stats.h -- how well the spatial aux heads classify, counted next to the loss that trains them (sam_hip_aux_loss.h), with no [B, n, n, 12]
 * tensor in memory.  An extension of the model's ABI: additive (sam_abi_version() stays what it was), declared here and in no other header; a C caller
 * includes this file, which includes sam_hip.h.  Same conventions as there.
 *
 * S, M, codes and valid as in sam_hip_aux_loss.h.  For every pair (b, i, j) with valid[b,i] & valid[b,j] (the diagonal counts):
 *   true class       c = codes[b,i,j] if it is in 1..12, else 0 (the loss gives a code above 12 an all-zero target: class 0, "no relation")
 *   predicted class  p: best = 0.0f, p = 0; for r = 0..11 in order: if (S[r] > best) { best = S[r]; p = r + 1; }
 *                    -- 0 when no channel's sigmoid exceeds 0.5; the first maximum wins a tie; a NaN score never fires and never wins
 *   fired channels   f[r] = S[r] > 0.0f
 *   confusion[c, p] += 1          int64 [13, 13]
 *   fired[c, r]     += f[r]       int64 [13, 12]
 * The scores are the ones sam_aux_pair_fwd stores (one copy of the per-pair code).  A batch without a valid pair gives all zeros.  Rows that are not
 * valid are never read: they may hold anything.
 *
 * sam_aux_pair_stats: O, D fp32 [B, n, 32], W fp32 [12, 32], bias fp32 [12], codes u8 [B, n, n], valid u8 [B, n].  Block partials (u32, a block counts at
 *   most 1024 pairs) go to `ws` (sam_aux_pair_stats_ws_bytes(B, n, &bytes)); a finishing launch sums them per cell in int64 and stores the result, or
 *   adds it to what confusion / fired hold when accumulate != 0.  No global atomics, grids sized from the shape alone, integer sums: bit-identical from
 *   run to run.  O, D and ws 16-byte aligned, confusion and fired 8-byte aligned; fusion SAM_AUX_MUL | SAM_AUX_ADD; any B in [1, 65535], n >= 1.
 *   Nothing is read back on the host. */
#ifndef SAM_HIP_AUX_STATS_H
#define SAM_HIP_AUX_STATS_H
#include "sam_hip.h"
#ifdef __cplusplus
extern "C" {
#endif

int sam_aux_pair_stats_ws_bytes(int B, int n, int64_t* bytes);
int sam_aux_pair_stats(const float* O, const float* D, const float* W, const float* bias, const uint8_t* codes, const uint8_t* valid, int B, int n,
                       int fusion, int64_t* confusion, int64_t* fired, int accumulate, void* ws, int64_t ws_bytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif

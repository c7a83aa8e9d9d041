/* sam_hip_evalboard.h -- evaluation results collected by question index: a resident results board.  An extension of the
 * model's ABI: additive (sam_abi_version() stays what it was), declared here and in no other header; a C caller includes this file, which includes
 * sam_hip.h.  Same conventions as sam_hip_eval.h / sam_hip_sampler.h: plain C, every function returns 0 or a SAM_ERR_* code with a message in
 * sam_last_error(), arguments are checked on the host before any device call, launches go to the caller's stream, no workspace, no atomics, nothing
 * synchronises.
 *
 * A board for n questions and answer width P is eight tensors in DEVICE memory, row q = question q:
 *   scores fp32 [n, 3], oracle fp32 [n, 3], flags int32 [n], best int32 [n], answer int32 [n, P], answer_len int32 [n]
 *       what sam_eval_beams wrote for that question: best_scores, oracle, best_flags, best, answer, answer_len
 *   seen int32 [n]      how many valid batch slots held the question so far; 0: the row is empty
 *   status int32 [1]    only ever OR-ed into; bit 0 (value 1): a valid slot held an index outside [0, n)
 * An empty board is all zero.  All board addressing is 64-bit (n * P ints pass 2^32 bytes at 260 k questions of P = 4160).
 *
 * sam_evalboard_collect: one batch of B slots into the board.  sample_idx int32 [B]; valid int32 [B] or NULL (every slot valid); best_scores .. answer_len
 * are sam_eval_beams' outputs of those names for the same B samples (answer [B, P]).
 *   slot b is LIVE when (valid is NULL or valid[b] != 0) and 0 <= sample_idx[b] < n.  A slot that is valid but out of range sets status bit 0 and writes
 *   nothing; an out-of-range slot with valid[b] == 0 is ignored.
 *   a live slot OWNS q = sample_idx[b] when no live slot b' < b holds the same q;  m = the number of live slots of this batch that hold q.
 *   the owner: if seen[q] == 0 it copies its row into the board (all P answer columns; answer_len clamped to [0, P]) and sets seen[q] = m; otherwise
 *   the board's row stays (first write wins) and seen[q] += m (two's complement).  No other board element is touched.
 * One wave per slot, four waves per block; ownership and m come from a lane-strided scan of sample_idx / valid.  Distinct owners write distinct rows.
 * Nothing read from device memory is trusted: the indices are range-checked and the length is clamped.
 *
 * sam_evalboard_reduce: out float64 [8], overwritten: out[0..2] the three score sums over the rows with seen > 0, out[3] the number of such rows,
 * out[4..6] the oracle sums over the same rows, out[7] the sum of their seen.  Rows with seen <= 0 contribute nothing, whatever they hold.  The order
 * is sam_score_answers' (score_totals_kernel) and part of the contract: one workgroup of 256 threads, thread t adds rows t, t + 256, ... of the board
 * in ascending order, each fp32 widened to float64, then a halving tree over the threads.  The sums therefore depend on the board alone.
 *
 * sam_evalboard_merge: for every q with src.seen[q] > 0: if dst.seen[q] == 0 the src row is copied (scores, oracle, flags, best, all P answer columns,
 * answer_len as it stands); in either case dst.seen[q] += src.seen[q].  dst.status |= src.status.  One wave per row.  The two boards must not overlap.
 *
 * SAM_ERR_ARG with a message: a null pointer (valid excepted), a misaligned pointer, B < 1, P < 1, n outside [1, 2^31), overlapping boards. */
#ifndef SAM_HIP_EVALBOARD_H
#define SAM_HIP_EVALBOARD_H
#include "sam_hip.h"
#ifdef __cplusplus
extern "C" {
#endif

int sam_evalboard_collect(const int32_t* sample_idx, const int32_t* valid, int B, const float* best_scores, const float* oracle, const int32_t* best_flags,
                          const int32_t* best, const int32_t* answer, const int32_t* answer_len, int64_t n, int P, float* board_scores, float* board_oracle,
                          int32_t* board_flags, int32_t* board_best, int32_t* board_answer, int32_t* board_answer_len, int32_t* board_seen,
                          int32_t* board_status, void* stream);

int sam_evalboard_reduce(const float* board_scores, const float* board_oracle, const int32_t* board_seen, int64_t n, double* out, void* stream);

int sam_evalboard_merge(float* dst_scores, float* dst_oracle, int32_t* dst_flags, int32_t* dst_best, int32_t* dst_answer, int32_t* dst_answer_len,
                        int32_t* dst_seen, int32_t* dst_status, const float* src_scores, const float* src_oracle, const int32_t* src_flags,
                        const int32_t* src_best, const int32_t* src_answer, const int32_t* src_answer_len, const int32_t* src_seen,
                        const int32_t* src_status, int64_t n, int P, void* stream);

#ifdef __cplusplus
}
#endif
#endif

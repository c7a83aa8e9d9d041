/* sam_hip_beam_merge.h -- the entry point of libsam_hip.so that evaluates beam-search output with the answer STRING as the unit of choice: every beam
 * scored and spelled out, the beams of a question that spell the same string merged, their probabilities added, the string with the largest mass kept
 * (DESIGN.md section 3.29).  This is the project's own definition; the reference has nothing like it (its Evaluator.evaluate keeps the single beam with
 * the largest cumulative score, which is sam_eval_beams of sam_hip_eval.h).
 *
 * The conventions of sam_hip_eval.h hold: plain C, every function returns 0 or a SAM_ERR_* code of sam_hip.h with a message in sam_last_error(),
 * arguments are checked before any device call, launches go to the caller's stream and nothing synchronises, no workspace, no global atomics and no float
 * atomics; the model's ABI (sam_hip.h, sam_abi_version()) is untouched.
 */
#ifndef SAM_HIP_BEAM_MERGE_H
#define SAM_HIP_BEAM_MERGE_H
#include "sam_hip.h"
#ifdef __cplusplus
extern "C" {
#endif

/* ---- beam-search output to per-question results, chosen by string: two launches (B * K workgroups, then B), and a third of one workgroup when totals
 * is given ----
 * The inputs (seqs .. eos) are sam_eval_beams' inputs, unchanged and in its order; so are its nine outputs (beam_scores .. answer_len), of which
 * beam_scores, beam_flags and oracle keep its contract bit for bit (the scoring code is the one copy in csrc/score_walk.h).  With P = L * (Lw + 1),
 * per question b and its beams k = 0 .. K - 1 (rows b * K + k):
 *
 *   beam_answer int32 [B * K, P], beam_answer_len int32 [B * K]
 *       every beam's answer string exactly as sam_eval_beams writes `answer` for the beam it chooses: the words joined with blanks, " 's" glued to "'s",
 *       the NO_GLUE bit cleared, Python's strip() applied, ended by EOS or by an out-of-range id, zeros from beam_answer_len on.  The n-best list.
 *   group int32 [B * K]     the lowest beam index (0 .. K - 1) whose string equals beam k's, the group's LEADER: two beams share a group if and only if
 *                           their strings have equal length and equal code points (decided on the code points; a hash only pre-filters).  A beam whose
 *                           beam_flags has bit 0 set (an out-of-range id) never merges: group = k.
 *   n_groups int32 [B]      the number of leaders
 *   mass fp32 [B * K]       the mass of beam k's group, written at every member.  One member: exactly cum[k], no arithmetic (NaN and +-inf pass through).
 *                           Several members, in fp32: m = fmaxf chained over the members' cum in beam order; a NaN member makes the mass NaN; m = -inf
 *                           (every member -inf) makes it -inf; else m + logf(sum of expf(cum[j] - m)), the sum taken in ascending j (a -inf member
 *                           adds 0; a +inf member makes inf - inf, so the mass is NaN).  The operation order is fixed: two runs agree bit for bit.
 *   best int32 [B]          the REPRESENTATIVE.  The winning leader is numpy.argmax's over the leaders' masses in ascending leader index (the first NaN
 *                           wins, else the first leader with no greater mass); the representative is numpy.argmax's over the winning group's members'
 *                           cum in beam order.  best_ids, best_scores, best_flags, answer and answer_len are the representative's rows.
 *   best_mass fp32 [B]      the winning group's mass
 *   plain_best int32 [B]    what sam_eval_beams writes as `best`: numpy.argmax of cum[b * K .. b * K + K)
 *   totals float64 [4], optional: the new best_scores' column sums and B are added to it, in sam_score_answers' fixed order.
 * Every element of every output is written, and nothing else.
 *
 * The limits and their codes are sam_eval_beams' own: 1 <= K <= 64, 0 <= skip < S, 1 <= L <= 64, 1 <= Lg <= 255, and sam_score_answers' LDS bound
 * (3 * (2 * P + 8) ints within 60 KiB).  K > 64, L > 64, Lg > 255 or text past the LDS bound: SAM_ERR_UNSUPPORTED; every other violation: SAM_ERR_ARG. */
int sam_eval_beams_merged(const int64_t* seqs, const float* cum, const int32_t* meta, const int32_t* gt_norm, const int32_t* gt_norm_len,
                          const float* gt_score, const int32_t* gt_raw, const int32_t* gt_raw_len, const int32_t* ocr, const int32_t* ocr_len,
                          const int32_t* vocab_cp, const int32_t* vocab_len, int B, int K, int S, int skip, int A, int Lg, int No, int Lw, int V, int eos,
                          float* beam_scores, int32_t* beam_flags, int32_t* best, int64_t* best_ids, float* best_scores, int32_t* best_flags, float* oracle,
                          int32_t* answer, int32_t* answer_len, int32_t* beam_answer, int32_t* beam_answer_len, int32_t* group, float* mass,
                          int32_t* n_groups, int32_t* plain_best, float* best_mass, double* totals, void* stream);

#ifdef __cplusplus
}
#endif
#endif

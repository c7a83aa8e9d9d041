/* sam_hip_eval.h -- the entry point of libsam_hip.so that evaluates beam-search output: every beam scored, the best beam per question chosen, its
 * scores and its answer string gathered (the second half of the reference's Evaluator.evaluate, evaluator.py:67-135 with evaluate_predictions :304-356).
 *
 * The conventions of sam_hip_pipeline.h hold: plain C, every function returns 0 or a SAM_ERR_* code of sam_hip.h with a message in sam_last_error(),
 * arguments are checked before any device call, launches go to the caller's stream and nothing synchronises, no workspace, no global atomics and no float
 * atomics; the model's ABI (sam_hip.h, sam_abi_version()) is untouched.  The declaration lives in a file of its own because the ctypes binding keeps one
 * table per header and the tables of the other eight headers are pinned by the tests of the entry points they were written for.
 */
#ifndef SAM_HIP_EVAL_H
#define SAM_HIP_EVAL_H
#include "sam_hip.h"
#ifdef __cplusplus
extern "C" {
#endif

/* ---- beam-search output to per-question results: two launches (B * K workgroups, then B), and a third of one workgroup when totals is given ----
 * seqs int64 [B * K, S]: the search's complete_seqs; rows b * K .. b * K + K - 1 are sample b's beams (BeamSearch.init_batch's interleaving).  The first
 * `skip` columns are not scored (the reference drops column 0, the BOS: evaluator.py:333), L = S - skip.  cum fp32 [B * K]: topkscores.  The eight
 * score-table tensors (meta .. ocr_len) and vocab_cp / vocab_len / eos are sam_score_answers' arguments, for B samples: the table is NOT repeated K times.
 *
 *   beam_scores fp32 [B * K, 3], beam_flags int32 [B * K]
 *       CONTRACT: bit for bit what sam_score_answers returns for pred = seqs[:, skip:] on the table with every row repeated K times (beam r reads table
 *       row r / K); both kernels are compiled from one copy of the scoring code (csrc/score_walk.h).
 *   best int32 [B]          the beam numpy.argmax picks from cum[b * K .. b * K + K): the first k such that no beam's score is greater, a NaN counting as
 *                           greater than every number (the first NaN wins); +inf, -inf and -0.0 == 0.0 follow IEEE comparison.
 *   best_ids int64 [B, L], best_scores fp32 [B, 3], best_flags int32 [B]      the chosen beam's row of seqs[:, skip:], beam_scores and beam_flags
 *   oracle fp32 [B, 3]      per metric the maximum over the sample's K beams: fmaxf chained in beam order from beam 0
 *   answer int32 [B, P], P = L * (Lw + 1); answer_len int32 [B]
 *       the chosen beam's string as the reference writes it to the EvalAI file: the words joined with blanks, " 's" glued to "'s", the NO_GLUE bit cleared,
 *       Python's strip() applied; columns from answer_len[b] on are 0.  Where an out-of-range id ended the walk (flag bit 0) the string holds what was
 *       assembled before it.  The text is the score table's and the vocabulary's, lowered per word.
 *   totals float64 [4], optional: best_scores' column sums and B are added to it, in sam_score_answers' fixed order.
 * Every element of every output is written, and nothing else.
 *
 * 1 <= K <= 64, 0 <= skip < S, 1 <= L <= 64, 1 <= Lg <= 255, and sam_score_answers' LDS bound (3 * (2 * P + 8) ints within 60 KiB).  K > 64, L > 64,
 * Lg > 255 or text past the LDS bound: SAM_ERR_UNSUPPORTED; every other violation: SAM_ERR_ARG. */
int sam_eval_beams(const int64_t* seqs, const float* cum, const int32_t* meta, const int32_t* gt_norm, const int32_t* gt_norm_len, const float* gt_score,
                   const int32_t* gt_raw, const int32_t* gt_raw_len, const int32_t* ocr, const int32_t* ocr_len, const int32_t* vocab_cp,
                   const int32_t* vocab_len, int B, int K, int S, int skip, int A, int Lg, int No, int Lw, int V, int eos, float* beam_scores,
                   int32_t* beam_flags, int32_t* best, int64_t* best_ids, float* best_scores, int32_t* best_flags, float* oracle, int32_t* answer,
                   int32_t* answer_len, double* totals, void* stream);

#ifdef __cplusplus
}
#endif
#endif

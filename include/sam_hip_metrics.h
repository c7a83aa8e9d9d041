/* sam_hip_metrics.h -- the entry point of libsam_hip.so that builds the metrics' score tables from the TEXT of the answers and the OCR tokens.
 *
 * The conventions of sam_hip_pipeline.h hold: plain C, every function returns 0 or a SAM_ERR_* code of sam_hip.h with a message in sam_last_error(),
 * arguments are checked before any device call, launches go to the caller's stream and nothing synchronises, no workspace, no global atomics; the
 * model's ABI (sam_hip.h, sam_abi_version()) is untouched.  The declaration lives in a file of its own because the ctypes binding keeps one table per
 * header and the tables of the other seven headers are pinned by the tests of the entry points they were written for.
 */
#ifndef SAM_HIP_METRICS_H
#define SAM_HIP_METRICS_H
#include "sam_hip.h"
#ifdef __cplusplus
extern "C" {
#endif

/* ---- the score tables of a batch (the input of sam_score_answers) from text, one launch, one workgroup of four waves per sample ----
 * The ground-truth half of TextVQAAccuracy / STVQAAccuracy / STVQAANLS (sam/datasets/metrics.py:265-382): what metrics.build_score_table computes per
 * sample and metrics.collate_score_tables pads to the capacities (A, Lw, Lg).
 *
 * CONTRACT: for every sample the eight output tensors equal, bit for bit, the rows of collate_score_tables([build_score_table(answers, tokens)],
 * (A, Lw, Lg)) with tokens = the first ocr_count[b] OCR slots, every padding element included (the kernel writes every element of its outputs, and
 * nothing else) -- for text t with ascii_lower(t) == t.lower() (metrics.device_lowerable): THE ONE DEVIATION is that the kernel lowers ASCII "A"-"Z"
 * only, where the host uses str.lower(); code points >= 0x80 pass through unchanged.
 *   gt_norm / gt_norm_len / gt_score / meta[0]   every lowered answer through the normaliser (metrics.normalize_answer: the passes sam_score_answers runs
 *       on the prediction), the results deduplicated in first-seen order, each with the leave-one-out soft score of answers.soft_scores over the
 *       normalised list (summed in float64 in answer order, divided by A, rounded to fp32)
 *   gt_raw / gt_raw_len / meta[1]                the distinct strip(lower(a)) strings in first-seen order; strip removes Python's whitespace
 *   ocr / ocr_len                                slots below ocr_count[b] hold the lowered token, an "s" that was "S" right after an apostrophe carrying
 *       bit 30 (metrics.NO_GLUE); slots from ocr_count[b] to No hold "<pad>" with length 5.  A token may be the empty string: length 0 is not padding,
 *       which is why the count is an argument.  With No = 0 the two tensors keep one all-zero slot, as collate_score_tables shapes them.
 *   meta[2] = meta[3] = 0
 * Where collate_score_tables raises for a sample, status[b] holds ONE bit and all the sample's rows are zero: 1 = a normalised or a raw answer exceeds Lg
 * code points ("'s" -> " 's" and the contractions lengthen text); else 2 = "<pad>" does not fit a slot (Lw < 5 and ocr_count[b] < No).  A clean sample
 * has status 0.
 *
 * answer_text int32 [B * A, ld_answer]: the exact code points of answer (b, a) in its first answer_len[b * A + a] columns; ocr_text int32
 * [B * No, ld_ocr] / ocr_len int32 [B * No]: the OCR tokens' exact code points, slot by slot; ocr_count int32 [B].  The kernel clamps the lengths to
 * [0, La] / [0, Lw] and the counts to [0, No].  With No = 0 the three OCR pointers are not read and may be NULL.
 * 1 <= La <= 128, 1 <= Lw <= 64, 1 <= Lg <= 255, No >= 0, ld_* >= the width.  A > 64, or shapes whose staging (A * (La + Lg) + 16 * La code points)
 * exceeds 64 KiB of LDS: SAM_ERR_UNSUPPORTED.
 * Outputs: meta int32 [B, 4], gt_norm / gt_raw int32 [B, A, Lg], gt_norm_len / gt_raw_len int32 [B, A], gt_score fp32 [B, A], ocr int32
 * [B, max(No, 1), Lw], ocr_out_len int32 [B, max(No, 1)], status int32 [B]. */
int sam_score_table_from_text(const int32_t* answer_text, int64_t ld_answer, const int32_t* answer_len, const int32_t* ocr_text, int64_t ld_ocr,
                              const int32_t* ocr_len, const int32_t* ocr_count, int B, int A, int La, int No, int Lw, int Lg, int32_t* meta,
                              int32_t* gt_norm, int32_t* gt_norm_len, float* gt_score, int32_t* gt_raw, int32_t* gt_raw_len, int32_t* ocr,
                              int32_t* ocr_out_len, int32_t* status, void* stream);

#ifdef __cplusplus
}
#endif
#endif

/* sam_hip_answers.h -- dataset-side entry points of libsam_hip.so that start from the TEXT of the answers (code points).
 *
 * The conventions of sam_hip_pipeline.h hold: plain C, every function returns 0 or a SAM_ERR_* code of sam_hip.h with a message in sam_last_error(),
 * arguments are checked before any device call, launches go to the caller's stream and nothing synchronises, no workspace, no global atomics; the
 * model's ABI (sam_hip.h, sam_abi_version()) is untouched.  The declarations live in a file of their own because the ctypes binding keeps one table per
 * header and the tables of the other three headers are pinned by the tests of the entry points they were written for.
 */
#ifndef SAM_HIP_ANSWERS_H
#define SAM_HIP_ANSWERS_H
#include "sam_hip.h"
#ifdef __cplusplus
extern "C" {
#endif

/* ---- the M4C answer tables of a batch from the answers' and the OCR tokens' text, one launch, one workgroup per sample ----
 * The string half of M4CAnswerProcessor.__call__ (sam/datasets/processors.py:586-692 with match_answer_to_vocab_ocr_seq :542-578 and get_all_indices
 * :694-707): soft scores of the A answers, every answer word matched against the answer vocabulary and the OCR tokens, the per-word matches expanded
 * into at most max_match_num decoding sequences per answer, the index lists of every scored step -- what answers.build_answer_table computes per sample
 * and answers.collate_answer_tables pads to the capacities S, L, G, E.
 *
 * CONTRACT: for every sample the eight output tensors equal, bit for bit, the rows of collate_answer_tables([build_answer_table(...)], (S, L, G, E)),
 * every padding element included (the kernel writes every element of its outputs).  Where the host raises for a sample, status[b] holds ONE bit and the
 * sample's rows are all zero (meta = 0: "no candidate" for sam_answer_sample): 4 = a scored index is an OCR slot whose text is "<pad>", 8 = <unk> among
 * the target indices of a scored index (of these two the one the host meets first), else 1 = more than G groups, else 2 = more than E target indices.
 * A clean sample has status 0.
 *
 * answer_text int32 [B * A, ld_answer]: the exact code points of answer (b, a) in its first answer_len[b * A + a] columns (nothing lowered, no flag
 * bits); ocr_text int32 [B * No, ld_ocr] / ocr_len int32 [B * No]: the OCR tokens' exact code points, slot by slot (a slot of length 0 matches no
 * word).  Lengths are clamped to [0, La] / [0, Lw] by the kernel.  Words are split at the code points Python's str.isspace() accepts.
 * The vocabulary index (answers.vocab_index): vocab_cp int32 [V, ld_vocab] / vocab_len int32 [V] the exact code points of the word list; slots
 * int32 [T] an open-addressed table of word indices, T a power of two >= 2 V, -1 = empty, home slot hash & (T - 1) with the 32-bit hash of
 * csrc/answer_text.hip (FNV-1a over the code points, then lowbias32), linear probing; a probe ends in a full comparison of length and code points.
 * unk / eos: the indices of "<unk>" and "</s>" in the vocabulary.
 * 1 <= La <= 128, 1 <= Lw <= 64, 1 <= Lv <= 64, ld_* >= the width, L >= 1, S >= A * max_match_num, 1 <= G <= 32767, E >= 1, max_match_num >= 1.
 * A > 255, No > 64 (one OCR slot per lane) or shapes whose staging exceeds 64 KiB of LDS: SAM_ERR_UNSUPPORTED.
 * Outputs: meta int32 [B, 4], seq_len int32 [B, S], seq_grp int16 [B, S, L], step0_idx int32 / step0_val fp32 [B, S], grp_idx int32 [B, G],
 * grp_off int32 [B, G + 1], grp_extra int32 [B, E], status int32 [B]. */
int sam_answer_table_from_text(const int32_t* answer_text, int64_t ld_answer, const int32_t* answer_len, const int32_t* ocr_text, int64_t ld_ocr,
                               const int32_t* ocr_len, const int32_t* vocab_cp, int64_t ld_vocab, const int32_t* vocab_len, const int32_t* slots, int B, int A,
                               int La, int No, int Lw, int V, int Lv, int T, int unk, int eos, int S, int L, int G, int E, int max_match_num, int32_t* meta,
                               int32_t* seq_len, int16_t* seq_grp, int32_t* step0_idx, float* step0_val, int32_t* grp_idx, int32_t* grp_off,
                               int32_t* grp_extra, int32_t* status, void* stream);

#ifdef __cplusplus
}
#endif
#endif

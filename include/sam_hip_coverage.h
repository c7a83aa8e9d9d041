/* sam_hip_coverage.h -- answer-space upper bounds: the witness sequences of a batch's ground-truth answers.  An extension of the
 * model's ABI: additive (sam_abi_version() stays what it was), declared here and in no other header; a C caller includes this file, which includes
 * sam_hip.h.  Same conventions as sam_hip_answers.h / sam_hip_evalboard.h: plain C, the function returns 0 or a SAM_ERR_* code with a message in
 * sam_last_error(), arguments are checked on the host before any device call, the launch goes to the caller's stream, no workspace, no atomics,
 * nothing synchronises, every element of every output is written.
 *
 * sam_answer_witness: one launch, one workgroup per sample, its four waves striding over the sample's A answers.  For every answer (b, a) and every
 * SOURCE s (0 = the answer vocabulary alone, 1 = the sample's OCR tokens alone, 2 = both) it writes the id sequence a perfect decoder would emit when
 * it may draw from that source only -- a WITNESS -- or says that there is none.
 *
 * Inputs, as sam_answer_table_from_text takes them (sam_hip_answers.h): answer_text int32 [B * A, ld_answer] / answer_len int32 [B * A] the answers'
 * exact code points; ocr_text int32 [B * No, ld_ocr] / ocr_len int32 [B * No] the OCR tokens', slot by slot; lengths are clamped to [0, La] / [0, Lw]
 * by the kernel.  The vocabulary index (answers.vocab_index): vocab_cp int32 [V, ld_vocab] / vocab_len int32 [V], slots int32 [T], T a power of two
 * >= 2 V, -1 = empty, linear probing from text_hash & (T - 1) (csrc/text.h).  eos: the index of "</s>"; L: the decoding length.
 *
 * Words are split at the code points Python's str.isspace() accepts (128 code points hold at most 64 words).  A word MATCHES the vocabulary when the
 * index holds exactly its code points, and MATCHES OCR when some slot < No of the sample has non-zero length and holds exactly its code points; its
 * id is then the vocabulary index, or V + the LOWEST such slot.  Under source 2 the vocabulary id wins when both match.  An answer is REACHABLE from a
 * source when it has at least one word and every word matches; its witness is the ids of its words in order, which under source 2 is
 * match_answer_to_vocab_ocr_seq(answer, vocab2idx, ocr2inds)[0] of the reference's answer processor.
 *
 * Outputs:
 *   words  int32 [B, A]       the answer's word count
 *   reach  int32 [3, B, A]    1 when the answer is reachable from the source, else 0
 *   any    int32 [3, B]       the OR of reach over the sample's answers
 *   seqs   int64 [3, B * A, L]  source-major: seqs[s] is a sam_eval_beams input of K = A beams per sample, skip = 0.  The row of a reachable answer
 *                             holds its first min(words, L) ids, then eos (an answer of more than L words is reachable; its witness is cut to L ids).
 *                             The row of an unreachable answer is a copy of the row of the sample's lowest-numbered answer reachable from that source,
 *                             so it adds nothing to a maximum over the sample's rows; a sample with any == 0 has all-eos rows.
 *   counts int32 [B, 4]       over all words of the sample's A answers: how many there are, how many match the vocabulary, how many match OCR, how
 *                             many match neither
 *
 * Every loop whose trip count comes from device memory is bounded by a capacity the host passed: the probe by T steps, the word scan by 64 words of
 * La code points, the slot scan by No slots of Lw code points; an index value outside [0, V) ends a probe.  A corrupt index or length gives a wrong
 * answer, never a read outside the tensors and never a hang.
 *
 * SAM_ERR_ARG with a message: a null or misaligned pointer (seqs holds 8-byte elements), B, A, No, La, Lw, Lv, L or V below 1, ld_* below the width,
 * T not a power of two >= 2 V, eos outside [0, V).  SAM_ERR_UNSUPPORTED: La > 128, Lw > 64, Lv > 64, No > 64 (one OCR slot per lane), L > 64 or
 * A > 64 (sam_eval_beams' limits on steps and beams). */
#ifndef SAM_HIP_COVERAGE_H
#define SAM_HIP_COVERAGE_H
#include "sam_hip.h"
#ifdef __cplusplus
extern "C" {
#endif

int sam_answer_witness(const int32_t* answer_text, int64_t ld_answer, const int32_t* answer_len, const int32_t* ocr_text, int64_t ld_ocr,
                       const int32_t* ocr_len, const int32_t* vocab_cp, int64_t ld_vocab, const int32_t* vocab_len, const int32_t* slots, int B, int A,
                       int La, int No, int Lw, int V, int Lv, int T, int eos, int L, int32_t* words, int32_t* reach, int32_t* any, int64_t* seqs,
                       int32_t* counts, void* stream);

#ifdef __cplusplus
}
#endif
#endif

/* sam_hip_question.h -- dataset-side entry points of libsam_hip.so that start from the TEXT of the question (code points).
 *
 * The conventions of sam_hip_pipeline.h hold: plain C, every function returns 0 or a SAM_ERR_* code of sam_hip.h with a message in sam_last_error(),
 * arguments are checked before any device call, launches go to the caller's stream and nothing synchronises, no workspace, no global atomics; the
 * model's ABI (sam_hip.h, sam_abi_version()) is untouched.  The declarations live in a file of their own because the ctypes binding keeps one table per
 * header and the tables of the other five headers are pinned by the tests of the entry points they were written for.
 */
#ifndef SAM_HIP_QUESTION_H
#define SAM_HIP_QUESTION_H
#include "sam_hip.h"
#ifdef __cplusplus
extern "C" {
#endif

/* ---- BERT WordPiece ids of the questions from their text, one launch, one wave per sample ----
 * The reference's BertTokenizerProcessor (sam/datasets/processors.py:467-498) calls BertTokenizer.encode(question, add_special_tokens=True) of an uncased
 * model on the host, cuts the ids to max_length and pads with [PAD] = 0.  This entry point computes the same three tensors from the question's code
 * points as wordpiece.pack_question_text packs them: an ASCII question raw, a non-ASCII one after the steps that need Unicode tables (control characters
 * dropped, Unicode spaces mapped to U+0020, str.lower() then NFD without combining marks per word), with bit 30 set on every non-ASCII punctuation
 * character.  wordpiece.encode_host is the host twin.
 *
 * CONTRACT on the first clamp(text_len[b], 0, Lq) code points of row b, bits 30 and 31 masked off before any comparison or hash (bit 30 is kept as the
 * "punctuation" flag):
 *   c < 128:   0x20 0x09 0x0A 0x0D separate words; every other c < 0x20 and 0x7F is dropped (dropping does not separate: a \x01 b is the word "ab");
 *              A-Z become lower case; 33-47, 58-64, 91-96, 123-126 each form a word of one character; everything else is a word character.
 *   c >= 128:  a flagged code point and a CJK code point (the eight ranges of BERT's _is_chinese_char) form a word of one character; everything else is a
 *              word character.
 *   A word of more than 100 code points gives unk.  Otherwise WordPiece, greedy longest-match-first from the left: the candidate at position s > 0 of
 *   the word is '#' '#' followed by the substring, a candidate of more than Lv code points cannot match; if any position has no match the WHOLE word is a
 *   single unk and none of its earlier pieces is emitted.
 *   The row is cls, the ids, sep, cut to its first T entries (a long question loses its sep and may end inside a word, as indices[:max_length] does).
 * indices int64 [B, ld_indices >= T]: the row, 0 ([PAD]) behind the count; mask int64 [B, ld_mask >= T]: 1 on the first count entries, else 0;
 * count int32 [B]: min(T, 2 + number of ids); an empty question gives cls sep, count 2.  Every element of the T columns of both rows and of count is
 * written, nothing outside them.
 *
 * text int32 [B, ld_text], ld_text >= Lq, 1 <= Lq <= 1024; text_len int32 [B], clamped, never trusted.  The vocabulary index (wordpiece.vocab_index,
 * the layout of answers.vocab_index): vocab_cp int32 [V, ld_vocab] / vocab_len int32 [V] the exact code points of vocab.txt's lines in id order,
 * continuation pieces WITH their two '#'; slots int32 [n_slots] an open-addressed table of ids, n_slots a power of two, -1 = empty, home slot
 * hash & (n_slots - 1) with the 32-bit hash of csrc/answer_text.hip (FNV-1a over the code points, then lowbias32), linear probing, a probe ends after
 * n_slots steps and in a full comparison of length and code points.  1 <= Lv <= 64, ld_vocab >= Lv, 1 <= T <= 64, unk / cls / sep in [0, V). */
int sam_wordpiece_from_text(const int32_t* text, int64_t ld_text, const int32_t* text_len, const int32_t* vocab_cp, int64_t ld_vocab, const int32_t* vocab_len,
                            const int32_t* slots, int B, int Lq, int V, int Lv, int n_slots, int unk, int cls, int sep, int T, int64_t* indices, int64_t ld_indices,
                            int64_t* mask, int64_t ld_mask, int32_t* count, void* stream);

#ifdef __cplusplus
}
#endif
#endif

/* sam_hip_unicode.h -- the entry points of libsam_hip.so that read a Unicode character table resident on the device: the batch's raw strings lowered
 * with Python's str.lower() while they are cleaned and packed, and the questions' raw strings normalised and packed as wordpiece.pack_question_text
 * packs them (BasicTokenizer's table-driven steps).  With them no string of a sample has to be lowered or normalised on the host.
 *
 * The conventions of sam_hip_pipeline.h hold: plain C, every function returns 0 or a SAM_ERR_* code of sam_hip.h with a message in sam_last_error(),
 * arguments are checked before any device call, launches go to the caller's stream and nothing synchronises, no workspace, no atomics; the model's
 * ABI (sam_hip.h, sam_abi_version()) is untouched.  The declarations live in a file of their own because the ctypes binding keeps one table per
 * header and the tables of the other ten headers are pinned by the tests of the entry points they were written for.
 *
 * The table (unicode_table.py builds it from the interpreter's own str.lower() and unicodedata and states the bit layout) is passed as plain pointers
 * and sizes, all int32 in device memory:
 *   uni_block [uni_n_stage1]        uni_n_stage1 must be 8704 = 0x110000 / 128; uni_block[cp >> 7] is the record block of cp
 *   uni_rec [uni_n_blocks, 128, 2]  two words per code point, 8-byte aligned; a block number outside [0, uni_n_blocks) reads block 0
 *   uni_pool [uni_n_pool]           the results of more than one code point; an offset outside the pool yields nothing
 * so a table that is not one gives wrong text and never a read outside the three arrays.
 */
#ifndef SAM_HIP_UNICODE_H
#define SAM_HIP_UNICODE_H
#include "sam_hip.h"
#ifdef __cplusplus
extern "C" {
#endif

/* ---- UTF-8 bytes to cleaned code points, lowered as str.lower() lowers: one launch, one wave per slot ----
 * The contract of sam_text_from_utf8 (sam_hip_textprep.h: raw, raw_off, the four mode bits and their order, text, text_len, status and its three bits,
 * the limits) with one difference: bit 1 of mode is Python's str.lower() of the whole decoded slot -- every character's lower case from the table,
 * U+0130 becoming two code points, and U+03A3 becoming U+03C2 where str.lower() applies the final-sigma rule (the nearest character before it that is
 * not case-ignorable is cased, and the nearest one behind it is not, or there is none), U+03C3 elsewhere.  The slot is lowered as a whole, blanks
 * included, before bits 2, 4 and 8 apply, as word_cleaner does.  On all-ASCII input the result equals sam_text_from_utf8's for every mode.
 *
 * S >= 1, 1 <= L <= 128, 0 <= mode <= 15, 0 <= nbytes < 2^31, uni_n_stage1 == 8704, uni_n_blocks >= 1, uni_n_pool >= 1: anything else is SAM_ERR_ARG. */
int sam_text_from_utf8_unicode(const uint8_t* raw, int64_t nbytes, const int32_t* raw_off, int S, int L, int mode, const int32_t* uni_block, int uni_n_stage1,
                               const int32_t* uni_rec, int uni_n_blocks, const int32_t* uni_pool, int uni_n_pool, int32_t* text, int32_t* text_len,
                               int32_t* status, void* stream);

/* ---- UTF-8 bytes of the questions to the packed text sam_wordpiece_from_text reads: one launch, one wave per question ----
 * raw / raw_off as above, one slot per question.  question_text int32 [B, Lq] and question_text_len int32 [B] equal what
 * wordpiece.pack_question_text([q], max_chars=Lq) writes for the slot's string, bit for bit, zeros behind the length:
 *   a slot of ASCII bytes only is copied verbatim (sam_wordpiece_from_text normalises ASCII itself);
 *   any other slot is normalised, in this order: characters the table marks as dropped vanish; separators, and the two sides of a CJK ideograph, split
 *   the rest into words; each word is lowered with str.lower() (the final-sigma rule sees the word alone, without the dropped characters) and every
 *   character replaced by NFD of its lower case without the marks of category Mn (0..3 code points from the table, Hangul syllables by arithmetic);
 *   words that become empty vanish; single blanks join the rest; bit 30 (PUNCT_FLAG) is set on every result >= 128 of a category P*.
 *
 *   status int32 [B]   0, or exactly one of (the first that applies in this order: 4, 1, 8, 16, 2)
 *       1  the slot is not strict UTF-8                             4  the slot's offsets are not 0 <= raw_off[b] <= raw_off[b + 1] <= nbytes
 *       8  one of [PAD] [UNK] [CLS] [SEP] [MASK] occurs literally in the slot (pack_question_text's ValueError)
 *      16  the slot holds one of the few code points that are not of category Mn yet have a non-zero combining class: canonical reordering can move
 *          them, which no per-character table expresses; normalise that question on the host
 *       2  more than Lq code points after normalisation
 *     A flagged slot gets an all-zero row and length 0.
 *
 * B >= 1, 1 <= Lq <= 1024, 0 <= nbytes < 2^31 and the table's limits above: anything else is SAM_ERR_ARG. */
int sam_question_from_utf8(const uint8_t* raw, int64_t nbytes, const int32_t* raw_off, int B, int Lq, const int32_t* uni_block, int uni_n_stage1,
                           const int32_t* uni_rec, int uni_n_blocks, const int32_t* uni_pool, int uni_n_pool, int32_t* question_text,
                           int32_t* question_text_len, int32_t* status, void* stream);

#ifdef __cplusplus
}
#endif
#endif

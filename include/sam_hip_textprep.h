/* sam_hip_textprep.h -- the entry point of libsam_hip.so that turns the batch's raw strings, shipped as UTF-8 bytes with offsets, into the cleaned,
 * zero-padded code-point tensors every text kernel reads (ocr_text / answer_text): the reference's Processors.word_cleaner / word_cleaner_lower
 * (sam/datasets/processors.py:746-755) and the per-character packing loops of phoc.pack_ocr_text / answers.pack_answer_text.
 *
 * The conventions of sam_hip_pipeline.h hold: plain C, every function returns 0 or a SAM_ERR_* code of sam_hip.h with a message in sam_last_error(),
 * arguments are checked before any device call, launches go to the caller's stream and nothing synchronises, no workspace, no atomics; the model's
 * ABI (sam_hip.h, sam_abi_version()) is untouched.  The declaration lives in a file of its own because the ctypes binding keeps one table per header
 * and the tables of the other nine headers are pinned by the tests of the entry points they were written for.
 */
#ifndef SAM_HIP_TEXTPREP_H
#define SAM_HIP_TEXTPREP_H
#include "sam_hip.h"
#ifdef __cplusplus
extern "C" {
#endif

/* ---- UTF-8 bytes to cleaned code points: one launch, one wave per slot ----
 * raw uint8 [nbytes]: the UTF-8 of all S slots back to back; raw_off int32 [S + 1]: slot s owns raw[raw_off[s] .. raw_off[s + 1]), an empty range is an
 * empty slot.  A slot's raw length is unbounded: the wave walks it 64 bytes at a time.  No byte outside a slot's own range is read.
 *
 * mode, a bit set applied in this order to the decoded code points:
 *   1  lower ASCII 'A'..'Z' (anything else is lowered by the caller before encoding: textprep.pack_utf8)
 *   2  delete ',' and '?'
 *   4  replace each "'s" of the stream left by bit 2 with " 's"  (Python's chained str.replace: "'?s" becomes " 's")
 *   8  strip leading and trailing code points for which Python's str.isspace() is true
 * 15 is word_cleaner, 9 word_cleaner_lower, 0 decodes and packs verbatim.
 *
 *   text int32 [S, L]    the slot's code points, zeros behind its length: every word of every row is written
 *   text_len int32 [S]
 *   status int32 [S]     0, or exactly one of
 *       1  the slot is not strict UTF-8 (truncated sequence, stray continuation byte, overlong form, surrogate, value above U+10FFFF, bytes C0 C1
 *          F5..FF): exactly where bytes.decode("utf-8") raises
 *       2  more than L code points after cleaning
 *       4  the slot's offsets are not 0 <= raw_off[s] <= raw_off[s + 1] <= nbytes (nothing of raw is read for it)
 *     A flagged slot gets an all-zero row and length 0: nothing is truncated.
 *
 * S >= 1, 1 <= L <= 128, 0 <= mode <= 15, 0 <= nbytes < 2^31 (raw may be NULL when nbytes is 0): anything else is SAM_ERR_ARG. */
int sam_text_from_utf8(const uint8_t* raw, int64_t nbytes, const int32_t* raw_off, int S, int L, int mode, int32_t* text, int32_t* text_len, int32_t* status,
                       void* stream);

#ifdef __cplusplus
}
#endif
#endif

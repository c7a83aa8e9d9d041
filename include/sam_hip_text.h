/* sam_hip_text.h -- dataset-side entry points of libsam_hip.so that start from the TEXT of the OCR tokens (code points), included by sam_hip_pipeline.h.
 *
 * The conventions of sam_hip_pipeline.h hold: plain C, every function returns 0 or a SAM_ERR_* code of sam_hip.h with a message in sam_last_error(),
 * arguments are checked before any device call, launches go to the caller's stream and nothing synchronises, no workspace, no global atomics; the
 * model's ABI (sam_hip.h, sam_abi_version()) is untouched.  The declarations live in a file of their own because the ctypes binding keeps one table per
 * header and the table of sam_hip_pipeline.h is pinned by the tests of the entry point it was written for.
 */
#ifndef SAM_HIP_TEXT_H
#define SAM_HIP_TEXT_H
#include "sam_hip.h"
#ifdef __cplusplus
extern "C" {
#endif

/* ---- PHOC features of the OCR tokens from their text, one launch ----
 * The reference builds the 604-column pyramidal histogram of characters per token on the host (sam/phoc/build_phoc.py: lower, keep a-z 0-9;
 * sam/phoc/cphoc.c: unigram levels 2..5 = 14 regions x 36 characters, then the 50 listed bigrams x 2 regions of level 2), PhocProcessor
 * (sam/datasets/processors.py:407-440) pads it to fp32 [50, 604] and every batch ships it.  This entry point computes the same rows from the tokens' code
 * points -- the tensors a batch that scores on the GPU already holds as score_table["ocr"] / ["ocr_len"].
 *
 * CONTRACT: for every slot the 604 columns equal, bit for bit, build_phoc of the slot's token (the region test is the reference's fp32 sequence, not the
 * exact rational one: csrc/phoc.hip), written as a part of sam_ragged_expand would write the same 0/1 source row: normalize = 0 the 0/1 row, normalize = 1
 * the row times 1 / max(sqrt(number of ones), eps), rounded once to the destination type; columns outside [col0, col0 + 604) are not touched.
 *
 * text int32 [B * n_max, ld_text]: code points of slot (b, i) in its first text_len[b * n_max + i] columns; text_len int32 [B * n_max], clamped to
 * [0, Lw] by the kernel (bits 30 and 31 of a code point are ignored: the score table flags an "s" there); counts int32 [B] or NULL: valid slots per sample, clamped to [0, n_max] as sam_ragged_expand clamps -- slots i >= count give an
 * all-zero row whatever their text holds; NULL: every slot is taken at its text_len.  1 <= Lw <= 64 (one code point per lane; wider:
 * SAM_ERR_UNSUPPORTED), ld_text >= Lw.  Folding: A-Z to lower case, U+0130 -> i, U+212A -> k (the code points whose str.lower() holds a kept character),
 * then only a-z 0-9 are kept; a token with no kept character gives an all-zero row.
 * dst [B * n_max, ld_dst] fp32 (dst_f32 = 1) or bf16 (0), 0 <= col0, col0 + 604 <= ld_dst; eps > 0. */
int sam_phoc_from_text(const int32_t* text, int64_t ld_text, const int32_t* text_len, const int32_t* counts, int B, int n_max, int Lw, void* dst,
                       int64_t ld_dst, int col0, int dst_f32, int normalize, float eps, void* stream);

#ifdef __cplusplus
}
#endif
#endif

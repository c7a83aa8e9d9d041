/* sam_hip_fasttext.h -- dataset-side entry point of libsam_hip.so that computes the OCR tokens' FastText vectors from their TEXT (code points).
 *
 * The conventions of sam_hip_text.h hold: plain C, every function returns 0 or a SAM_ERR_* code of sam_hip.h with a message in sam_last_error(),
 * arguments are checked before any device call, launches go to the caller's stream and nothing synchronises, no workspace, no global atomics; the
 * model's ABI (sam_hip.h, sam_abi_version()) is untouched.  The declaration lives in a file of its own because the ctypes binding keeps one table per
 * header and the tables of the other six headers are pinned by the tests of the entry points they were written for.
 */
#ifndef SAM_HIP_FASTTEXT_H
#define SAM_HIP_FASTTEXT_H
#include "sam_hip.h"
#ifdef __cplusplus
extern "C" {
#endif

/* ---- FastText vectors of the OCR tokens from their text and a resident table, one launch, one wave per slot ----
 * The reference's FastTextProcessor (sam/datasets/processors.py:181-226, 96-102) loads a fastText model into every DataLoader worker and ships
 * np.mean([get_word_vector(w) for w in token.split(" ")], axis=0) as fp32 [50, 300] with every sample.  This entry point computes the same rows from the
 * tokens' code points (the layout of sam_phoc_from_text) and the model's input matrix kept on the device.  fasttext.vectors_host_text is the host twin;
 * the rules below are the contract (written from the library's published behaviour; equality with the library's own output is NOT tested).
 *
 * CONTRACT for slot (b, i), on the first clamp(text_len, 0, Lw) code points of its row, each masked with 0x1FFFFF (bits 30 and 31 are flags of the score
 * table, never part of a code point):
 *   pieces    the token is cut at every U+0020 (str.split(" ")): k spaces give k + 1 pieces, empty ones included.
 *   ids       of a piece w: the word id from the exact-match index (below) when w is a dictionary word, followed -- unless that id is eos_id -- by
 *             the subword ids of "<" w ">"; a piece that is no dictionary word (or longer than Lv code points) has the subword ids only.
 *   subwords  of s = "<" w ">" in UTF-8 (1-4 bytes per code point, encoded arithmetically): for every character position j in increasing order, for
 *             n = 1 .. maxn characters while characters remain: the id nwords + hash % bucket when n >= minn and not (n == 1 and the n-gram touches
 *             either end of s); start-major, length-minor.  hash is FNV-1a over the BYTES taken as signed chars (h ^= (uint32_t)(int8_t)c, h *= 16777619,
 *             from 2166136261): a byte >= 0x80 flips the upper 24 bits too.
 *   vector    v = 0, then v += matrix[id] for every id in order, plain fp32 adds, never reassociated or contracted; with at least one id
 *             v *= (float)(1.0 / count); no id gives the zero vector.
 *   token     the piece vectors added in order in fp32 (the first one copied), then ONE fp32 division by the number of pieces: numpy's mean over axis 0.
 * Slots i >= clamp(counts[b], 0, n_max) give an all-zero row whatever their text holds (counts NULL: every slot at its text_len).
 * dst [B * n_max, ld_dst] fp32 (dst_f32 = 1) or bf16 (0): columns [col0, col0 + dim) receive the vector (normalize = 0: as it is or rounded once to
 * bf16; normalize = 1: what sam_l2norm_pack_bf16 writes from that fp32 row -- the row body of csrc/rowwise.h's l2norm_row); other columns are not touched.
 *
 * text int32 [B * n_max, ld_text], ld_text >= Lw; text_len int32 [B * n_max]; matrix fp32 [nwords + bucket, ld_matrix], ld_matrix >= dim, 16-byte
 * aligned rows.  The index (fasttext.model_index; the layout of answers.vocab_index): index_cp int32 [nwords, ld_index] / index_len int32 [nwords] the
 * code points of dictionary word i (index_len < 0: the word has no entry), slots int32 [n_slots] an open-addressed table of word ids, n_slots a power of
 * two, -1 = empty, home slot hash & (n_slots - 1) with the 32-bit hash of csrc/answer_text.hip (FNV-1a over the code points, then lowbias32), linear
 * probing, a probe ends at an empty slot or after n_slots steps, every candidate compared in full.  eos_id: the id of "</s>" or -1.
 * LIMITS (anything else of these: SAM_ERR_UNSUPPORTED, nothing launched): 1 <= Lw <= 64, dim % 4 == 0, 4 <= dim <= 512, 0 <= minn <= maxn <= 8, and a
 * destination the 4-wide stores can address (col0 % 4 == 0, ld_dst % 4 == 0, dst aligned to 4 elements).  bucket >= 1 unless maxn == 0. */
int sam_fasttext_from_text(const int32_t* text, int64_t ld_text, const int32_t* text_len, const int32_t* counts, int B, int n_max, int Lw, const float* matrix,
                           int64_t ld_matrix, const int32_t* index_cp, int64_t ld_index, const int32_t* index_len, const int32_t* slots, int Lv, int n_slots,
                           int minn, int maxn, int bucket, int nwords, int eos_id, int dim, void* dst, int64_t ld_dst, int col0, int dst_f32, int normalize,
                           float eps, void* stream);

#ifdef __cplusplus
}
#endif
#endif

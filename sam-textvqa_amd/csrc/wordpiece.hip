// BERT WordPiece ids of the questions straight from their text (gfx950): one launch per batch, one wave per sample.
//   wordpiece_from_text  <- BertTokenizerProcessor.__call__ (sam/datasets/processors.py:467-498): BertTokenizer.encode(question, add_special_tokens=True) of an
//                           uncased model (BasicTokenizer: clean, lower, strip accents, split at punctuation; WordpieceTokenizer: greedy longest match against
//                           vocab.txt, a word of more than 100 characters or with an unmatched position is [UNK]), cut to max_length, padded with [PAD] = 0.
// The batch carries the question as code points (wordpiece.pack_question_text: an ASCII question raw; a non-ASCII one after the steps that need Unicode
// tables, with bit 30 on every non-ASCII punctuation character), the run keeps vocab.txt on the device as the exact-match word index of
// csrc/text.h (wordpiece.vocab_index; continuation pieces stored WITH their "##").  include/sam_hip_question.h states the rules; wordpiece.encode_host
// is the host twin and the outputs equal it element for element.
//
// The work is latency-bound (a question is ~10 words of ~5 characters): one 64-lane block per sample.
//   pass 1   64 code points per trip: every lane classifies one (word character / one-character word / separator / dropped) and lowers A-Z; the kept
//            ones are compacted into LDS with a ballot and a prefix count, their class in bits 30-31; a second trip over the compacted text leaves
//            one 64-bit "not a word character" mask per 64 positions, from which a word's end is a find-first-set.
//   pass 2   the wave walks the words.  At a piece start s lane j takes the candidate that ends at min(n, s + Lv') - j (Lv' = Lv, or Lv - 2 behind the
//            "##" of a continuation), hashes it out of LDS, probes the index and compares in full; the lowest lane that matched holds the longest match.
//            A word's pieces wait in LDS until its last position has matched, then go to the row; the walk stops once T entries are written.
// Every loop is bounded (positions only advance, a probe ends after n_slots steps).  No global atomics, no workspace, every output element written once.
#include "common.h"
#include "text.h"
#include "sam_hip_question.h"

namespace {

constexpr int kMaxText = 1024, kMaxWordChars = 100, kMaxPiece = 64, kMaxT = 64;
constexpr unsigned kCpMask = 0x3fffffffu;            // bits 30 / 31 are flags, never part of a code point
enum { C_WORD = 0, C_SINGLE = 1, C_SEP = 2, C_DROP = 3 };

// BERT's _is_chinese_char: a CJK ideograph stands alone as a word
__device__ __forceinline__ bool is_cjk(int c) {
  return (c >= 0x4E00 && c <= 0x9FFF) || (c >= 0x3400 && c <= 0x4DBF) || (c >= 0x20000 && c <= 0x2A6DF) || (c >= 0x2A700 && c <= 0x2B73F) ||
         (c >= 0x2B740 && c <= 0x2B81F) || (c >= 0x2B820 && c <= 0x2CEAF) || (c >= 0xF900 && c <= 0xFAFF) || (c >= 0x2F800 && c <= 0x2FA1F);
}

// class of a masked code point; c is lowered in place
__device__ __forceinline__ int classify(int& c, bool flagged) {
  if (c >= 128) return (flagged || is_cjk(c)) ? C_SINGLE : C_WORD;
  if (c == 0x20 || c == 0x09 || c == 0x0A || c == 0x0D) return C_SEP;
  if (c < 0x20 || c == 0x7F) return C_DROP;
  if (c >= 'A' && c <= 'Z') { c += 'a' - 'A'; return C_WORD; }
  if ((c >= 33 && c <= 47) || (c >= 58 && c <= 64) || (c >= 91 && c <= 96) || (c >= 123 && c <= 126)) return C_SINGLE;
  return C_WORD;
}

// the id of the piece made of `pre` '#' followed by w[0..n) (LDS, class bits still on), or -1: index_lookup of text.h (its hash, by its constants, and its
// walk) with the "##" prefix and the class mask written out.  Kept in this form because the kernel is 3 us slower through the shared accessor probe, and
// pass 1 below 1.3 us slower through wave_emit (profiles/text_refactor_bench.txt).
__device__ int piece_lookup(const int* w, int n, int pre, const int32_t* __restrict__ vocab_cp, int64_t ld_vocab, const int32_t* __restrict__ vocab_len,
                            const int32_t* __restrict__ slots, int V, int n_slots) {
  const int total = pre + n;
  unsigned h = kTextHashBasis;
  for (int i = 0; i < pre; ++i) h = (h ^ (unsigned)'#') * kTextHashPrime;
  for (int i = 0; i < n; ++i) h = (h ^ ((unsigned)w[i] & kCpMask)) * kTextHashPrime;
  unsigned s = mix32(h) & (unsigned)(n_slots - 1);
  for (int it = 0; it < n_slots; ++it) {
    const int wi = slots[s];
    if (wi < 0 || wi >= V) return -1;
    if (vocab_len[wi] == total) {
      const int32_t* c = vocab_cp + (int64_t)wi * ld_vocab;
      int i = 0;
      while (i < pre && c[i] == '#') ++i;
      if (i == pre) {
        while (i < total && (unsigned)c[i] == ((unsigned)w[i - pre] & kCpMask)) ++i;
        if (i == total) return wi;
      }
    }
    s = (s + 1) & (unsigned)(n_slots - 1);
  }
  return -1;
}

// grid B, block 64: wave = sample.  Everything that steers the walk (positions, counts) comes out of ballots and uniform LDS reads: the wave never diverges
// around a ballot, a shuffle or a barrier.
__global__ __launch_bounds__(64) void wordpiece_from_text_kernel(const int32_t* __restrict__ text, int64_t ld_text, const int32_t* __restrict__ text_len,
                                                                 const int32_t* __restrict__ vocab_cp, int64_t ld_vocab, const int32_t* __restrict__ vocab_len,
                                                                 const int32_t* __restrict__ slots, int Lq, int V, int Lv, int n_slots, int unk, int cls, int sep,
                                                                 int T, int64_t* __restrict__ indices, int64_t ld_indices, int64_t* __restrict__ mask,
                                                                 int64_t ld_mask, int32_t* __restrict__ count) {
  __shared__ int s_cp[kMaxText];
  __shared__ unsigned long long s_brk[kMaxText / 64];
  __shared__ int s_piece[kMaxWordChars];
  __shared__ int s_out[kMaxT];
  const int b = blockIdx.x, lane = threadIdx.x;
  int len = text_len[b];
  len = len < 0 ? 0 : (len > Lq ? Lq : len);                           // clamped, never trusted
  const int32_t* row = text + (int64_t)b * ld_text;

  // ---- pass 1: classify, lower, compact
  int n = 0;
  for (int base = 0; base < len; base += 64) {
    const int i = base + lane;
    int c = 0, kind = C_DROP;
    if (i < len) {
      const unsigned v = (unsigned)row[i];
      c = (int)(v & kCpMask);
      kind = classify(c, (v >> 30) & 1u);
    }
    const unsigned long long keep = __ballot(kind != C_DROP);
    if (kind != C_DROP) s_cp[n + __popcll(keep & ((1ull << lane) - 1ull))] = (int)((unsigned)c | ((unsigned)kind << 30));
    n += __popcll(keep);
  }
  __syncthreads();
  const int n_chunk = (n + 63) >> 6;
  for (int k = 0; k < n_chunk; ++k) {
    const int i = k * 64 + lane;
    const unsigned long long m = __ballot(i < n && ((unsigned)s_cp[i < n ? i : 0] >> 30) != C_WORD);
    if (lane == 0) s_brk[k] = m;
  }
  if (lane == 0) s_out[0] = cls;
  __syncthreads();

  // ---- pass 2: the words, left to right
  int cnt = 1, p = 0;
  while (p < n && cnt < T) {
    const int kind = (int)((unsigned)s_cp[p] >> 30);
    if (kind == C_SEP) { ++p; continue; }
    int e = p + 1;
    if (kind == C_WORD) {                                              // the next position that is not a word character
      int k = p >> 6;
      unsigned long long m = s_brk[k] & (~0ull << (p & 63));
      while (!m && ++k < n_chunk) m = s_brk[k];
      e = m ? k * 64 + __ffsll((long long)m) - 1 : n;
    }
    const int L = e - p;
    bool bad = L > kMaxWordChars;
    int n_piece = 0;
    for (int s = 0; !bad && s < L;) {
      const int pre = s > 0 ? 2 : 0;
      const int top = min(L, s + Lv - pre), end = top - lane;          // lane j: the candidate [s, top - j)
      int id = -1;
      if (end > s) id = piece_lookup(s_cp + p + s, end - s, pre, vocab_cp, ld_vocab, vocab_len, slots, V, n_slots);
      const unsigned long long hit = __ballot(id >= 0);
      if (!hit) { bad = true; break; }                                 // one position without a match: the whole word is unk
      const int src = __ffsll((long long)hit) - 1;                     // the lowest lane = the longest match
      id = __shfl(id, src);
      if (lane == 0) s_piece[n_piece] = id;
      ++n_piece;                                                       // (every piece takes at least one character: n_piece <= L <= 100)
      s = top - src;
    }
    __syncthreads();
    if (bad) {
      if (lane == 0) s_out[cnt] = unk;
      cnt += 1;
    } else {
      for (int j = lane; j < n_piece; j += 64)
        if (cnt + j < T) s_out[cnt + j] = s_piece[j];
      cnt += n_piece;
    }
    __syncthreads();
    p = e;
  }
  if (cnt < T) {
    if (lane == 0) s_out[cnt] = sep;
    ++cnt;
  }
  cnt = min(cnt, T);
  __syncthreads();

  // ---- outputs: every element of the T columns, zeros behind the count
  if (lane < T) {
    indices[(int64_t)b * ld_indices + lane] = lane < cnt ? (int64_t)s_out[lane] : 0;
    mask[(int64_t)b * ld_mask + lane] = lane < cnt ? 1 : 0;
  }
  if (lane == 0) count[b] = cnt;
}

}  // namespace

extern "C" int sam_wordpiece_from_text(const int32_t* text, int64_t ld_text, const int32_t* text_len, const int32_t* vocab_cp, int64_t ld_vocab,
                                       const int32_t* vocab_len, const int32_t* slots, int B, int Lq, int V, int Lv, int n_slots, int unk, int cls, int sep, int T,
                                       int64_t* indices, int64_t ld_indices, int64_t* mask, int64_t ld_mask, int32_t* count, void* stream) {
  SAM_REQUIRE(text && text_len, "sam_wordpiece_from_text: null text / text_len pointer");
  if (const int rc = word_index_check("sam_wordpiece_from_text", "ld_vocab", vocab_cp, ld_vocab, vocab_len, slots, Lv, kMaxPiece, n_slots)) return rc;
  SAM_REQUIRE(indices && mask && count, "sam_wordpiece_from_text: null output pointer");
  SAM_REQUIRE(B >= 1, "sam_wordpiece_from_text: bad batch size B=%d", B);
  SAM_REQUIRE(T >= 1 && T <= kMaxT, "sam_wordpiece_from_text: T=%d outside 1..%d", T, kMaxT);
  SAM_REQUIRE(Lq >= 1 && Lq <= kMaxText, "sam_wordpiece_from_text: Lq=%d outside 1..%d", Lq, kMaxText);
  SAM_REQUIRE(ld_text >= Lq, "sam_wordpiece_from_text: need ld_text >= Lq (ld_text=%ld Lq=%d)", (long)ld_text, Lq);
  SAM_REQUIRE(V >= 1 && unk >= 0 && unk < V && cls >= 0 && cls < V && sep >= 0 && sep < V, "sam_wordpiece_from_text: unk=%d / cls=%d / sep=%d outside [0, %d)", unk, cls, sep, V);
  SAM_REQUIRE(ld_indices >= T && ld_mask >= T, "sam_wordpiece_from_text: need ld_indices >= T and ld_mask >= T (%ld %ld T=%d)", (long)ld_indices, (long)ld_mask, T);
  SAM_REQUIRE(((uintptr_t)text | (uintptr_t)text_len | (uintptr_t)count) % 4 == 0 &&
              ((uintptr_t)indices | (uintptr_t)mask) % 8 == 0, "sam_wordpiece_from_text: misaligned operand");
  wordpiece_from_text_kernel<<<dim3((unsigned)B), dim3(64), 0, (hipStream_t)stream>>>(text, ld_text, text_len, vocab_cp, ld_vocab, vocab_len, slots, Lq, V, Lv, n_slots,
                                                                                      unk, cls, sep, T, indices, ld_indices, mask, ld_mask, count);
  SAM_LAUNCH_CHECK();
  return SAM_OK;
}

// Answer-space upper bounds (gfx950): the witness sequences of a batch's ground-truth answers, one launch, one workgroup per sample.
//   answer_witness  <- match_answer_to_vocab_ocr_seq (sam/datasets/processors.py:542-578) asked three times per answer -- with the vocabulary alone, the
//                      OCR tokens alone, and both -- and only for its FIRST sequence: the id a perfect decoder would emit for every word, the vocabulary id
//                      before the lowest OCR slot.  coverage.witness_host is the host twin; the outputs equal it bit for bit, padding included.
// The sample's OCR slots are staged in LDS once and read by all four waves; a wave takes the answers a = wave, wave + 4, ...: it stages the answer's code
// points in its own LDS row, finds the words from two ballots over the 128 positions (a word starts where a non-space follows a space), and matches a word
// against the OCR slots one slot per lane (a ballot; the lowest set bit is the slot) and against the vocabulary with index_lookup_wave of text.h.  The ids of
// the first L words wait in LDS (vocabulary id and lowest slot: source 2 is read off the two) until every wave is done, because the row of an unreachable
// answer is a copy of the row of the sample's first reachable one.  No atomics, no workspace, every output element is written once by one thread.
// Trip counts: the word loop by kWordsPerAnswer, the slot compare by the clamped lengths (<= Lw), the probe by T (index_lookup_wave): include/sam_hip_coverage.h.
#include "common.h"
#include "text.h"
#include "sam_hip_coverage.h"

namespace {

constexpr int kThreads = 256, kWaves = kThreads / 64;
constexpr int kMaxAnswerChars = 128, kMaxWordChars = 64, kWordsPerAnswer = kMaxAnswerChars / 2;   // a word and its separator take two code points
constexpr int kMaxAnswers = 64, kMaxSteps = 64, kMaxSlots = 64;                                   // sam_eval_beams' K and L; one OCR slot per lane
constexpr int kSources = 3;

// the LDS carve, shared by the host (size) and the kernel; every offset a multiple of 16 bytes
struct Carve {
  int ocr, olen, ans, wv, wo, nw, reach, first, cnt, total;
};
__host__ __device__ inline int up16(int x) { return (x + 15) & ~15; }
__host__ __device__ inline Carve carve(int A, int La, int No, int Lw, int L) {
  Carve c;
  int o = 0;
#define SAM_TAKE(field, bytes) c.field = o; o += up16(bytes);
  SAM_TAKE(ocr, 4 * No * Lw) SAM_TAKE(olen, 4 * No) SAM_TAKE(ans, 4 * kWaves * La) SAM_TAKE(wv, 4 * A * L) SAM_TAKE(wo, 4 * A * L) SAM_TAKE(nw, 4 * A)
  SAM_TAKE(reach, 4 * kSources * A) SAM_TAKE(first, 4 * 4) SAM_TAKE(cnt, 4 * 4 * kWaves)
#undef SAM_TAKE
  c.total = o;                                   // at the limits: 16384 + 256 + 2048 + 2 * 16384 + 256 + 768 + 16 + 64 = 52560 bytes
  return c;
}

// the first position >= p that holds no word character; ns1:ns0 = the 128 positions' "is a word character" bits, p a set bit
__device__ __forceinline__ int word_end(unsigned long long ns0, unsigned long long ns1, int p) {
  if (p < 64) {
    const unsigned long long z = ~ns0 & (~0ull << p);
    if (z) return __ffsll((long long)z) - 1;
    return ~ns1 ? 64 + __ffsll((long long)~ns1) - 1 : kMaxAnswerChars;
  }
  const unsigned long long z = ~ns1 & (~0ull << (p - 64));
  return z ? 64 + __ffsll((long long)z) - 1 : kMaxAnswerChars;
}

__global__ __launch_bounds__(kThreads) void answer_witness_kernel(
    const int32_t* __restrict__ answer_text, int64_t ld_answer, const int32_t* __restrict__ answer_len, const int32_t* __restrict__ ocr_text, int64_t ld_ocr,
    const int32_t* __restrict__ ocr_len, WordIndex index, int B, int A, int La, int No, int Lw, int Lv, int eos, int L, int32_t* __restrict__ words,
    int32_t* __restrict__ reach, int32_t* __restrict__ any, int64_t* __restrict__ seqs, int32_t* __restrict__ counts) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const Carve c = carve(A, La, No, Lw, L);
  int* s_ocr = (int*)(smem + c.ocr); int* s_olen = (int*)(smem + c.olen); int* s_ans = (int*)(smem + c.ans); int* s_wv = (int*)(smem + c.wv);
  int* s_wo = (int*)(smem + c.wo); int* s_nw = (int*)(smem + c.nw); int* s_reach = (int*)(smem + c.reach); int* s_first = (int*)(smem + c.first);
  int* s_cnt = (int*)(smem + c.cnt);
  const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, V = index.n_words;

  // ---- stage the sample's OCR slots
  for (int i = tid; i < No * Lw; i += kThreads) s_ocr[i] = ocr_text[((int64_t)b * No + i / Lw) * ld_ocr + i % Lw];
  for (int i = tid; i < No; i += kThreads) s_olen[i] = max(0, min(ocr_len[(int64_t)b * No + i], Lw));
  __syncthreads();

  // ---- a wave per answer: words from two ballots, every word against the slots (a lane each) and the index (the whole wave)
  int n_words = 0, n_vocab = 0, n_ocr = 0, n_none = 0;                       // (wave-uniform, like everything below that is not named `hit`)
  int* w = s_ans + wave * La;
  for (int a = wave; a < A; a += kWaves) {
    const int64_t row = (int64_t)b * A + a;
    const int n = max(0, min(answer_len[row], La));
    const int32_t* src = answer_text + row * ld_answer;
    const int c0 = lane < n ? src[lane] : ' ', c1 = lane + 64 < n ? src[lane + 64] : ' ';
    if (lane < n) w[lane] = c0;
    if (lane + 64 < n) w[lane + 64] = c1;
    const unsigned long long ns0 = __ballot(lane < n && !is_space(c0)), ns1 = __ballot(lane + 64 < n && !is_space(c1));
    __builtin_amdgcn_wave_barrier();                                         // (the row is read by other lanes than wrote it)
    unsigned long long st0 = ns0 & ~(ns0 << 1), st1 = ns1 & ~((ns1 << 1) | (ns0 >> 63));      // a word starts where no word character precedes one
    const int nw = __popcll(st0) + __popcll(st1);                            // <= 64: a start needs a separator in front of it, or position 0
    bool all_v = nw > 0, all_o = nw > 0, all_vo = nw > 0;
    for (int k = 0; k < kWordsPerAnswer && (st0 | st1); ++k) {
      int p;
      if (st0) { p = __ffsll((long long)st0) - 1; st0 &= st0 - 1; }
      else { p = 64 + __ffsll((long long)st1) - 1; st1 &= st1 - 1; }
      const int m = word_end(ns0, ns1, p) - p;                               // 1 <= m <= n - p
      const int* wp = w + p;
      bool hit = lane < No && s_olen[lane < No ? lane : 0] == m;             // (a clamped length: m <= Lw; an empty slot never, m >= 1)
      if (hit) {
        const int* t = s_ocr + lane * Lw;
        for (int i = 0; hit && i < m; ++i) hit = t[i] == wp[i];
      }
      const unsigned long long mask = __ballot(hit);
      const int o = mask ? __ffsll((long long)mask) - 1 : -1;
      const int v = m > Lv ? -1 : index_lookup_wave(index, m, lane, [wp](int i) { return wp[i]; });
      n_words += 1; n_vocab += v >= 0; n_ocr += o >= 0; n_none += v < 0 && o < 0;
      all_v = all_v && v >= 0; all_o = all_o && o >= 0; all_vo = all_vo && (v >= 0 || o >= 0);
      if (k < L && lane == 0) { s_wv[a * L + k] = v; s_wo[a * L + k] = o; }
    }
    if (lane == 0) { s_nw[a] = nw; s_reach[a] = all_v; s_reach[A + a] = all_o; s_reach[2 * A + a] = all_vo; }
    __builtin_amdgcn_wave_barrier();                                         // (the next answer overwrites the row)
  }
  if (lane == 0) { s_cnt[4 * wave] = n_words; s_cnt[4 * wave + 1] = n_vocab; s_cnt[4 * wave + 2] = n_ocr; s_cnt[4 * wave + 3] = n_none; }
  __syncthreads();

  // ---- per source the sample's first reachable answer (A <= 64: a ballot of wave 0)
  if (wave == 0) {
    for (int s = 0; s < kSources; ++s) {
      const unsigned long long m = __ballot(lane < A && s_reach[s * A + (lane < A ? lane : 0)] != 0);
      if (lane == 0) { s_first[s] = m ? __ffsll((long long)m) - 1 : -1; any[(int64_t)s * B + b] = m ? 1 : 0; }
    }
  }
  __syncthreads();

  // ---- outputs: every element once
  for (int a = tid; a < A; a += kThreads) {
    words[(int64_t)b * A + a] = s_nw[a];
    for (int s = 0; s < kSources; ++s) reach[((int64_t)s * B + b) * A + a] = s_reach[s * A + a];
  }
  if (tid < 4) {
    int sum = 0;
    for (int k = 0; k < kWaves; ++k) sum += s_cnt[4 * k + tid];
    counts[4 * (int64_t)b + tid] = sum;
  }
  const int per = A * L;
  for (int i = tid; i < kSources * per; i += kThreads) {
    const int s = i / per, r = i - s * per, a = r / L, t = r - a * L;
    const int from = s_reach[s * A + a] ? a : s_first[s];                    // -1: no answer of the sample is reachable from s
    int id = eos;
    if (from >= 0 && t < min(s_nw[from], L)) {
      const int v = s_wv[from * L + t], o = s_wo[from * L + t];              // (reachable: whichever of the two s reads is >= 0)
      id = s == 0 ? v : (s == 1 ? V + o : (v >= 0 ? v : V + o));
    }
    seqs[((int64_t)s * B + b) * per + r] = id;
  }
}

}  // namespace

extern "C" int sam_answer_witness(const int32_t* answer_text, int64_t ld_answer, const int32_t* answer_len, const int32_t* ocr_text, int64_t ld_ocr,
                                  const int32_t* ocr_len, const int32_t* vocab_cp, int64_t ld_vocab, const int32_t* vocab_len, const int32_t* slots, int B, int A,
                                  int La, int No, int Lw, int V, int Lv, int T, int eos, int L, int32_t* words, int32_t* reach, int32_t* any, int64_t* seqs,
                                  int32_t* counts, void* stream) {
  const char* who = "sam_answer_witness";
  SAM_REQUIRE(answer_text && answer_len && ocr_text && ocr_len, "%s: null answer / OCR text pointer", who);
  SAM_REQUIRE(words && reach && any && seqs && counts, "%s: null output pointer (words, reach, any, seqs, counts)", who);
  SAM_REQUIRE(B >= 1 && A >= 1 && No >= 1, "%s: bad shape B=%d A=%d No=%d", who, B, A, No);
  SAM_REQUIRE(La >= 1 && Lw >= 1 && Lv >= 1 && L >= 1, "%s: bad shape La=%d Lw=%d Lv=%d L=%d (each at least 1)", who, La, Lw, Lv, L);
  if (La > kMaxAnswerChars || Lw > kMaxWordChars || Lv > kMaxWordChars || No > kMaxSlots || L > kMaxSteps || A > kMaxAnswers) {
    sam_set_error("%s: La=%d Lw=%d Lv=%d No=%d L=%d A=%d: at most %d code points per answer, %d per word, %d OCR slots (one per lane), %d steps and %d answers "
                  "(sam_eval_beams' limits)", who, La, Lw, Lv, No, L, A, kMaxAnswerChars, kMaxWordChars, kMaxSlots, kMaxSteps, kMaxAnswers);
    return SAM_ERR_UNSUPPORTED;
  }
  if (const int rc = word_index_check(who, "ld_vocab", vocab_cp, ld_vocab, vocab_len, slots, Lv, kMaxWordChars, T)) return rc;
  SAM_REQUIRE(V >= 1 && (int64_t)T >= 2 * (int64_t)V, "%s: T=%d must be a power of two >= 2 V (V=%d)", who, T, V);
  SAM_REQUIRE(eos >= 0 && eos < V, "%s: eos=%d outside [0, %d)", who, eos, V);
  SAM_REQUIRE(ld_answer >= La && ld_ocr >= Lw, "%s: need ld_answer >= La, ld_ocr >= Lw (%ld %ld)", who, (long)ld_answer, (long)ld_ocr);
  SAM_REQUIRE(((uintptr_t)answer_text | (uintptr_t)answer_len | (uintptr_t)ocr_text | (uintptr_t)ocr_len | (uintptr_t)words | (uintptr_t)reach | (uintptr_t)any |
               (uintptr_t)counts) % 4 == 0 && (uintptr_t)seqs % 8 == 0, "%s: misaligned operand (seqs holds 8-byte elements, every other tensor 4-byte ones)", who);
  const Carve c = carve(A, La, No, Lw, L);       // <= 52560 bytes at the limits above
  const WordIndex index{vocab_cp, ld_vocab, vocab_len, slots, V, T};
  answer_witness_kernel<<<dim3((unsigned)B), dim3(kThreads), (size_t)c.total, (hipStream_t)stream>>>(
      answer_text, ld_answer, answer_len, ocr_text, ld_ocr, ocr_len, index, B, A, La, No, Lw, Lv, eos, L, words, reach, any, seqs, counts);
  SAM_LAUNCH_CHECK();
  return SAM_OK;
}

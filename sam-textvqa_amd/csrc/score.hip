// TextVQA / ST-VQA metrics of a batch of predictions, straight from per-sample score tables: what TextVQAAccuracy.calculate
// (sam/datasets/metrics.py:21-68) and its three evaluators compute on the host -- the index -> word walk (:39-51), EvalAIAnswerProcessor (:265-302) on the
// prediction, the soft-score lookup (:335-337), the ST-VQA membership test (:351-353) and ANLS (:366-379) -- with the ground-truth half precomputed by
// metrics.build_score_table.  Text is int32 Unicode code points; lowercasing happened on the host (metrics.py's docstring lists the two deviations).
//
// One block of four waves per sample (the device code is csrc/score_walk.h, which eval_beams.hip shares):
//   1. thread 0 walks the row's ids into (source, length, offset) triples; all threads copy the words into LDS, joined with blanks; wave 0 glues " 's" to
//      "'s" (every blank that "'s" follows goes: the pattern cannot overlap itself, so this is str.replace's left-to-right result).
//   2. waves 1-3 take the ground truths of ANLS in turn.  Levenshtein runs by rows: the ground truth's m + 1 columns lie across the lanes (up to four cells
//      per lane, in registers); for row i, t[j] = min(up + 1, diag + cost) needs only the previous row, and D[i][j] = j + min_{k <= j} (t[k] - k) is an
//      inclusive prefix-min over the lanes with a carry between the 64-column chunks.  The >= 0.5 threshold is decided in integers (2 d <= max len).
//   3. wave 0 meanwhile normalises the string by the rules of metrics.normalize_answer: every per-character pass is a wave-wide filter (ballot + popcount
//      give each lane its output position), the word pass walks the words in order with the 135 table entries spread over the lanes; then the result is
//      compared with the sample's normalised ground truths.
// Nothing is written outside the sample's three scores and its flag word; every table length is clamped to its capacity before it is used.
// A second launch of one block adds the batch sums and the count to the float64 accumulator in a fixed order (no float atomics): repeated runs agree bit
// for bit.
#include "common.h"
#include "sam_hip.h"

// ---- the normaliser's tables.  The passes that read them are in score_norm.h, shared with score_text.hip; the tables stay in this file because
// tests/test_metrics_cpu.py compares their text here with the Python lists.  score_text.hip includes this file up to the #ifndef below.
namespace {

constexpr int kNoGlue = 1 << 30;       // metrics.NO_GLUE
constexpr int kMaxPeriods = 32;        // metrics.MAX_PERIODS

struct MapEntry { char key[16]; char val[16]; };
// metrics.WORD_MAP: number words, articles (empty value: the word is dropped), contractions (tests/test_metrics_cpu.py compares the two lists)
__constant__ MapEntry kWordMap[] = {
    {"none", "0"}, {"zero", "0"}, {"one", "1"}, {"two", "2"}, {"three", "3"}, {"four", "4"}, {"five", "5"}, {"six", "6"}, {"seven", "7"}, {"eight", "8"},
    {"nine", "9"}, {"ten", "10"}, {"a", ""}, {"an", ""}, {"the", ""}, {"aint", "ain't"}, {"arent", "aren't"}, {"cant", "can't"}, {"couldve", "could've"},
    {"couldnt", "couldn't"}, {"couldn'tve", "couldn't've"}, {"couldnt've", "couldn't've"}, {"didnt", "didn't"}, {"doesnt", "doesn't"}, {"dont", "don't"},
    {"hadnt", "hadn't"}, {"hadnt've", "hadn't've"}, {"hadn'tve", "hadn't've"}, {"hasnt", "hasn't"}, {"havent", "haven't"}, {"hed", "he'd"},
    {"hed've", "he'd've"}, {"he'dve", "he'd've"}, {"hes", "he's"}, {"howd", "how'd"}, {"howll", "how'll"}, {"hows", "how's"}, {"Id've", "I'd've"},
    {"I'dve", "I'd've"}, {"Im", "I'm"}, {"Ive", "I've"}, {"isnt", "isn't"}, {"itd", "it'd"}, {"itd've", "it'd've"}, {"it'dve", "it'd've"}, {"itll", "it'll"},
    {"let's", "let's"}, {"maam", "ma'am"}, {"mightnt", "mightn't"}, {"mightnt've", "mightn't've"}, {"mightn'tve", "mightn't've"}, {"mightve", "might've"},
    {"mustnt", "mustn't"}, {"mustve", "must've"}, {"neednt", "needn't"}, {"notve", "not've"}, {"oclock", "o'clock"}, {"oughtnt", "oughtn't"},
    {"ow's'at", "'ow's'at"}, {"'ows'at", "'ow's'at"}, {"'ow'sat", "'ow's'at"}, {"shant", "shan't"}, {"shed've", "she'd've"}, {"she'dve", "she'd've"},
    {"she's", "she's"}, {"shouldve", "should've"}, {"shouldnt", "shouldn't"}, {"shouldnt've", "shouldn't've"}, {"shouldn'tve", "shouldn't've"},
    {"somebody'd", "somebodyd"}, {"somebodyd've", "somebody'd've"}, {"somebody'dve", "somebody'd've"}, {"somebodyll", "somebody'll"},
    {"somebodys", "somebody's"}, {"someoned", "someone'd"}, {"someoned've", "someone'd've"}, {"someone'dve", "someone'd've"}, {"someonell", "someone'll"},
    {"someones", "someone's"}, {"somethingd", "something'd"}, {"somethingd've", "something'd've"}, {"something'dve", "something'd've"},
    {"somethingll", "something'll"}, {"thats", "that's"}, {"thered", "there'd"}, {"thered've", "there'd've"}, {"there'dve", "there'd've"},
    {"therere", "there're"}, {"theres", "there's"}, {"theyd", "they'd"}, {"theyd've", "they'd've"}, {"they'dve", "they'd've"}, {"theyll", "they'll"},
    {"theyre", "they're"}, {"theyve", "they've"}, {"twas", "'twas"}, {"wasnt", "wasn't"}, {"wed've", "we'd've"}, {"we'dve", "we'd've"}, {"weve", "we've"},
    {"werent", "weren't"}, {"whatll", "what'll"}, {"whatre", "what're"}, {"whats", "what's"}, {"whatve", "what've"}, {"whens", "when's"}, {"whered", "where'd"},
    {"wheres", "where's"}, {"whereve", "where've"}, {"whod", "who'd"}, {"whod've", "who'd've"}, {"who'dve", "who'd've"}, {"wholl", "who'll"}, {"whos", "who's"},
    {"whove", "who've"}, {"whyll", "why'll"}, {"whyre", "why're"}, {"whys", "why's"}, {"wont", "won't"}, {"wouldve", "would've"}, {"wouldnt", "wouldn't"},
    {"wouldnt've", "wouldn't've"}, {"wouldn'tve", "wouldn't've"}, {"yall", "y'all"}, {"yall'll", "y'all'll"}, {"y'allll", "y'all'll"},
    {"yall'd've", "y'all'd've"}, {"y'alld've", "y'all'd've"}, {"y'all'dve", "y'all'd've"}, {"youd", "you'd"}, {"youd've", "you'd've"}, {"you'dve", "you'd've"},
    {"youll", "you'll"}, {"youre", "you're"}, {"youve", "you've"},
};
constexpr int kMapSize = sizeof(kWordMap) / sizeof(MapEntry);

__device__ __forceinline__ int punct_index(int c) {      // metrics.PUNCTUATION
  switch (c) {
    case ';': return 0;  case '/': return 1;  case '[': return 2;  case ']': return 3;  case '"': return 4;  case '{': return 5;  case '}': return 6;
    case '(': return 7;  case ')': return 8;  case '=': return 9;  case '+': return 10; case '\\': return 11; case '_': return 12; case '-': return 13;
    case '>': return 14; case '<': return 15; case '@': return 16; case '`': return 17; case ',': return 18; case '?': return 19; case '!': return 20;
    default: return -1;
  }
}

}  // namespace

#ifndef SAM_SCORE_TABLES_ONLY
#include "score_walk.h"         // the id walk with the glue, the edit distance, the scoring of one prediction and the totals: shared with eval_beams.hip

namespace {

__global__ __launch_bounds__(kScoreThreads) void score_kernel(const int64_t* __restrict__ pred, ScoreTable T, int L, int X, float* __restrict__ scores,
                                                              int32_t* __restrict__ flags) {
  extern __shared__ int sbuf[];                    // three text buffers of X code points
  __shared__ ScoreShared sh;
  const int64_t b = blockIdx.x;
  block_score(pred + b * L, L, b, T, sh, sbuf, X, scores + 3 * b, flags + b);
}

}  // namespace

extern "C" int sam_score_answers(const int64_t* pred, const int32_t* meta, const int32_t* gt_norm, const int32_t* gt_norm_len, const float* gt_score,
                                 const int32_t* gt_raw, const int32_t* gt_raw_len, const int32_t* ocr, const int32_t* ocr_len, const int32_t* vocab_cp,
                                 const int32_t* vocab_len, int B, int L, int A, int Lg, int No, int Lw, int V, int eos, float* scores, int32_t* flags,
                                 double* totals, void* stream) {
  SAM_REQUIRE(pred && meta && gt_norm && gt_norm_len && gt_score && gt_raw && gt_raw_len && ocr && ocr_len && vocab_cp && vocab_len && scores && flags,
              "sam_score_answers: null pointer");
  SAM_REQUIRE(B > 0 && L > 0 && A > 0 && Lg > 0 && No >= 0 && Lw > 0 && V > 0, "sam_score_answers: bad shape");
  SAM_REQUIRE(L <= kMaxSteps, "sam_score_answers: L = %d decoding steps exceed %d", L, kMaxSteps);
  SAM_REQUIRE(Lg <= 64 * kMaxQ - 1, "sam_score_answers: Lg = %d code points per ground truth exceed %d", Lg, 64 * kMaxQ - 1);
  SAM_REQUIRE(((uintptr_t)pred % 8) == 0 && (!totals || ((uintptr_t)totals % 8) == 0), "sam_score_answers: misaligned operand");
  // the joined words hold at most P = L * (Lw + 1) code points; "'s" -> " 's" adds at most one per two, a contraction at most one per four
  const int64_t P = (int64_t)L * (Lw + 1), X = 2 * P + 8;
  const size_t lds = (size_t)(3 * X) * sizeof(int);
  SAM_REQUIRE(lds <= 60 * 1024, "sam_score_answers: L * (Lw + 1) = %lld code points do not fit the LDS text buffers", (long long)P);
  hipStream_t st = (hipStream_t)stream;
  const ScoreTable T = {meta, gt_norm, gt_norm_len, gt_score, gt_raw, gt_raw_len, ocr, ocr_len, vocab_cp, vocab_len, A, Lg, No, Lw, V, eos};
  score_kernel<<<dim3(B), dim3(kScoreThreads), lds, st>>>(pred, T, L, (int)X, scores, flags);
  SAM_LAUNCH_CHECK();
  if (totals) {
    score_totals_kernel<<<dim3(1), dim3(kScoreThreads), 0, st>>>(scores, B, totals);
    SAM_LAUNCH_CHECK();
  }
  return SAM_OK;
}
#endif  // SAM_SCORE_TABLES_ONLY

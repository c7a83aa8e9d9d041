// The metric score tables of a batch straight from the answers' and the OCR tokens' text (gfx950): one launch per batch, one workgroup
// of four waves per sample.
//   score_table_from_text  <- metrics.build_score_table + metrics.collate_score_tables of every sample: the ground-truth half of TextVQAAccuracy /
//                             STVQAAccuracy / STVQAANLS (sam/datasets/metrics.py:265-382), which score.hip reads once per step.
// The outputs equal the host's bit for bit, padding included; metrics.score_tables_from_text_host is the host twin.  The host rules, and how each is kept:
//   lowering     ASCII "A"-"Z" only (the one deviation: include/sam_hip_metrics.h); in the OCR text an "s" that was "S" right after an apostrophe carries
//                NO_GLUE, as metrics._lower_word flags it
//   normaliser   metrics._normalize_lowered: the passes of score_norm.h, the same code score_kernel runs on the prediction.  Wave w takes answers
//                w, w + 4, ... in two scratch buffers of its own; its input is the staged, lowered answer
//   soft scores  answers.soft_scores over the normalised list: leave-one-out min(1, k / 3), summed in f64 in answer order, divided by A, rounded to fp32
//                (answer_text.hip's header shows why the fp32 value does not depend on how the host's sum() associates; A <= 64 here)
//   order        unique strings in first-seen order: answer a is "first" when no earlier answer equals it, its slot is the number of firsts before it
//   raw          strip(lower(a)) is a sub-range of the staged answer: only its bounds are kept
// Where collate_score_tables raises the sample's rows are all zero and status[b] holds one bit (the header lists them).  No global atomics, no workspace;
// every output element is written exactly once, by one thread.
#include "common.h"
#include "sam_hip_metrics.h"
#define SAM_SCORE_TABLES_ONLY          // kWordMap, kMapSize, punct_index, kMaxPeriods, kNoGlue: score.hip holds the one copy
#include "score.hip"
#undef SAM_SCORE_TABLES_ONLY
#include "score_norm.h"

namespace {

constexpr int kTextThreads = 256, kTextWaves = kTextThreads / 64;
constexpr int kMaxAnswers = 64, kMaxAnswerChars = 128, kMaxWordChars = 64, kMaxGt = 255;
enum { ST_LG = 1, ST_PAD = 2 };

// the LDS carve in ints, shared by the host (size check) and the kernel
struct TextCarve { int X, scratch, low, norm, alen, nlen, rlo, rhi, nfirst, rfirst, nsrc, rsrc, score, misc, total; };
__host__ __device__ inline TextCarve text_carve(int A, int La, int Lg) {
  TextCarve c;
  c.X = 2 * La + 8;
  int o = 0;
#define SAM_TAKE(field, ints) c.field = o; o += (ints);
  SAM_TAKE(scratch, kTextWaves * 2 * c.X) SAM_TAKE(low, A * La) SAM_TAKE(norm, A * Lg) SAM_TAKE(alen, A) SAM_TAKE(nlen, A) SAM_TAKE(rlo, A) SAM_TAKE(rhi, A)
  SAM_TAKE(nfirst, A) SAM_TAKE(rfirst, A) SAM_TAKE(nsrc, A) SAM_TAKE(rsrc, A) SAM_TAKE(score, A) SAM_TAKE(misc, 4)
#undef SAM_TAKE
  c.total = o;
  return c;
}
enum { M_STATUS, M_NNORM, M_NRAW, M_PAD };

__device__ __forceinline__ int ascii_lower(int c) { return (c >= 'A' && c <= 'Z') ? c + 32 : c; }

__global__ __launch_bounds__(kTextThreads) void score_table_from_text_kernel(
    const int32_t* __restrict__ answer_text, int64_t ld_answer, const int32_t* __restrict__ answer_len, const int32_t* __restrict__ ocr_text, int64_t ld_ocr,
    const int32_t* __restrict__ ocr_len, const int32_t* __restrict__ ocr_count, int A, int La, int No, int Lw, int Lg, int32_t* __restrict__ meta,
    int32_t* __restrict__ gt_norm, int32_t* __restrict__ gt_norm_len, float* __restrict__ gt_score, int32_t* __restrict__ gt_raw,
    int32_t* __restrict__ gt_raw_len, int32_t* __restrict__ ocr, int32_t* __restrict__ ocr_out_len, int32_t* __restrict__ status) {
  extern __shared__ int smem[];
  const TextCarve c = text_carve(A, La, Lg);
  int* s_low = smem + c.low; int* s_norm = smem + c.norm; int* s_alen = smem + c.alen; int* s_nlen = smem + c.nlen; int* s_rlo = smem + c.rlo;
  int* s_rhi = smem + c.rhi; int* s_nfirst = smem + c.nfirst; int* s_rfirst = smem + c.rfirst; int* s_nsrc = smem + c.nsrc; int* s_rsrc = smem + c.rsrc;
  float* s_score = (float*)(smem + c.score); int* misc = smem + c.misc;
  const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int NoOut = max(No, 1);                    // collate_score_tables keeps one (all-zero) slot when there is none
  meta += 4 * (int64_t)b; gt_norm += (int64_t)b * A * Lg; gt_norm_len += (int64_t)b * A; gt_score += (int64_t)b * A; gt_raw += (int64_t)b * A * Lg;
  gt_raw_len += (int64_t)b * A; ocr += (int64_t)b * NoOut * Lw; ocr_out_len += (int64_t)b * NoOut;
  const int count = No > 0 ? max(0, min(ocr_count[b], No)) : 0;

  // ---- stage the lowered answers (zeros behind their lengths)
  for (int a = tid; a < A; a += kTextThreads) s_alen[a] = max(0, min(answer_len[(int64_t)b * A + a], La));
  if (tid < 4) misc[tid] = 0;
  for (int i = tid; i < A * La; i += kTextThreads) {
    const int a = i / La, j = i - a * La;
    const int n = max(0, min(answer_len[(int64_t)b * A + a], La));
    s_low[i] = j < n ? ascii_lower(answer_text[((int64_t)b * A + a) * ld_answer + j]) : 0;
  }
  __syncthreads();

  // ---- wave w normalises answers w, w + 4, ...; the bounds of strip(lower(a))
  {
    int* bufA = smem + c.scratch + wv * 2 * c.X;
    int* bufC = bufA + c.X;
    for (int a = wv; a < A; a += kTextWaves) {
      const int* src = s_low + a * La;
      const int n = s_alen[a];
      const int out = wave_normalize(src, n, bufA, bufC, lane);
      if (out <= Lg) {
        for (int j = lane; j < out; j += 64) s_norm[a * Lg + j] = bufA[j];
      }
      int lo, hi;
      wave_strip(src, n, lane, lo, hi);
      if (lane == 0) { s_nlen[a] = out; s_rlo[a] = lo; s_rhi[a] = hi; if (out > Lg || hi - lo > Lg) misc[M_STATUS] = ST_LG; }
      __builtin_amdgcn_wave_barrier();             // (the next answer's passes overwrite bufA)
    }
  }
  if (tid == 0 && Lw < 5 && count < No) misc[M_PAD] = ST_PAD;          // "<pad>" does not fit an OCR slot; the host meets the answers first
  __syncthreads();
  const int st = misc[M_STATUS] ? misc[M_STATUS] : misc[M_PAD];

  // ---- a thread per answer: the first answer it equals (normalised, raw), the soft score of its normalised string
  if (!st) {
    for (int a = tid; a < A; a += kTextThreads) {
      const int n = s_nlen[a], rl = s_rhi[a] - s_rlo[a];
      const int* w = s_norm + a * Lg;
      const int* r = s_low + a * La + s_rlo[a];
      auto same = [&](int o) {
        bool eq = s_nlen[o] == n;
        const int* v = s_norm + o * Lg;
        for (int i = 0; eq && i < n; ++i) eq = v[i] == w[i];
        return eq;
      };
      int nfirst = a, rfirst = a, cnt = 0;
      for (int o = A - 1; o >= 0; --o) {
        if (same(o)) { ++cnt; if (o < a) nfirst = o; }
        if (o < a && s_rhi[o] - s_rlo[o] == rl) {
          const int* v = s_low + o * La + s_rlo[o];
          bool eq = true;
          for (int i = 0; eq && i < rl; ++i) eq = v[i] == r[i];
          if (eq) rfirst = o;
        }
      }
      // answers.soft_scores: per answer min(1, (count - (it equals this one)) / 3), summed in order, / A
      double sum = 0.0;
      for (int o = 0; o < A; ++o) {
        const double x = (double)(cnt - (same(o) ? 1 : 0)) / 3.0;
        sum += x < 1.0 ? x : 1.0;
      }
      s_score[a] = (float)(sum / (double)A);
      s_nfirst[a] = nfirst;
      s_rfirst[a] = rfirst;
    }
  }
  __syncthreads();
  // ---- first-seen compaction: the slot of a first answer is the number of firsts in front of it
  if (!st) {
    for (int a = tid; a < A; a += kTextThreads) {
      int kn = 0, kr = 0;
      for (int o = 0; o < a; ++o) { kn += s_nfirst[o] == o; kr += s_rfirst[o] == o; }
      if (s_nfirst[a] == a) s_nsrc[kn] = a;
      if (s_rfirst[a] == a) s_rsrc[kr] = a;
      if (a == A - 1) { misc[M_NNORM] = kn + (s_nfirst[a] == a); misc[M_NRAW] = kr + (s_rfirst[a] == a); }
    }
  }
  __syncthreads();

  // ---- outputs: every element once, zeros behind the counts, all zeros for a flagged sample
  const int n_norm = st ? 0 : misc[M_NNORM], n_raw = st ? 0 : misc[M_NRAW];
  if (tid == 0) { meta[0] = n_norm; meta[1] = n_raw; meta[2] = 0; meta[3] = 0; status[b] = st; }
  for (int k = tid; k < A; k += kTextThreads) {
    const int sn = k < n_norm ? s_nsrc[k] : 0, sr = k < n_raw ? s_rsrc[k] : 0;
    gt_norm_len[k] = k < n_norm ? s_nlen[sn] : 0;
    gt_score[k] = k < n_norm ? s_score[sn] : 0.f;
    gt_raw_len[k] = k < n_raw ? s_rhi[sr] - s_rlo[sr] : 0;
  }
  for (int i = tid; i < A * Lg; i += kTextThreads) {
    const int k = i / Lg, j = i - k * Lg;
    int vn = 0, vr = 0;
    if (k < n_norm) { const int a = s_nsrc[k]; if (j < s_nlen[a]) vn = s_norm[a * Lg + j]; }
    if (k < n_raw) { const int a = s_rsrc[k]; if (j < s_rhi[a] - s_rlo[a]) vr = s_low[a * La + s_rlo[a] + j]; }
    gt_norm[i] = vn;
    gt_raw[i] = vr;
  }
  for (int o = tid; o < NoOut; o += kTextThreads) {
    int n = 0;
    if (!st && o < No) n = o < count ? max(0, min(ocr_len[(int64_t)b * No + o], Lw)) : 5;
    ocr_out_len[o] = n;
  }
  for (int i = tid; i < NoOut * Lw; i += kTextThreads) {
    const int o = i / Lw, j = i - o * Lw;
    int v = 0;
    if (!st && o < No) {
      if (o < count) {
        const int n = max(0, min(ocr_len[(int64_t)b * No + o], Lw));
        if (j < n) {
          const int32_t* t = ocr_text + ((int64_t)b * No + o) * ld_ocr;
          const int ch = t[j];
          v = ascii_lower(ch);
          if (ch == 'S' && j > 0 && t[j - 1] == '\'') v |= kNoGlue;
        }
      } else if (j < 5) {
        v = j == 0 ? '<' : j == 1 ? 'p' : j == 2 ? 'a' : j == 3 ? 'd' : '>';
      }
    }
    ocr[i] = v;
  }
}

}  // namespace

extern "C" int sam_score_table_from_text(const int32_t* answer_text, int64_t ld_answer, const int32_t* answer_len, const int32_t* ocr_text, int64_t ld_ocr,
                                         const int32_t* ocr_len, const int32_t* ocr_count, int B, int A, int La, int No, int Lw, int Lg, int32_t* meta,
                                         int32_t* gt_norm, int32_t* gt_norm_len, float* gt_score, int32_t* gt_raw, int32_t* gt_raw_len, int32_t* ocr,
                                         int32_t* ocr_out_len, int32_t* status, void* stream) {
  SAM_REQUIRE(answer_text && answer_len, "sam_score_table_from_text: null answer text pointer");
  SAM_REQUIRE(No == 0 || (ocr_text && ocr_len && ocr_count), "sam_score_table_from_text: null OCR text pointer");
  SAM_REQUIRE(meta && gt_norm && gt_norm_len && gt_score && gt_raw && gt_raw_len && ocr && ocr_out_len && status, "sam_score_table_from_text: null output pointer");
  SAM_REQUIRE(B >= 1 && A >= 1 && No >= 0, "sam_score_table_from_text: bad shape B=%d A=%d No=%d", B, A, No);
  SAM_REQUIRE(La >= 1 && La <= kMaxAnswerChars, "sam_score_table_from_text: La=%d outside 1..%d", La, kMaxAnswerChars);
  SAM_REQUIRE(Lw >= 1 && Lw <= kMaxWordChars, "sam_score_table_from_text: Lw=%d outside 1..%d", Lw, kMaxWordChars);
  SAM_REQUIRE(Lg >= 1 && Lg <= kMaxGt, "sam_score_table_from_text: Lg=%d outside 1..%d", Lg, kMaxGt);
  SAM_REQUIRE(ld_answer >= La && (No == 0 || ld_ocr >= Lw), "sam_score_table_from_text: need ld_answer >= La and ld_ocr >= Lw (%ld %ld)", (long)ld_answer, (long)ld_ocr);
  SAM_REQUIRE(((uintptr_t)answer_text | (uintptr_t)answer_len | (uintptr_t)ocr_text | (uintptr_t)ocr_len | (uintptr_t)ocr_count | (uintptr_t)meta |
               (uintptr_t)gt_norm | (uintptr_t)gt_norm_len | (uintptr_t)gt_score | (uintptr_t)gt_raw | (uintptr_t)gt_raw_len | (uintptr_t)ocr |
               (uintptr_t)ocr_out_len | (uintptr_t)status) % 4 == 0, "sam_score_table_from_text: misaligned operand");
  if (A > kMaxAnswers) {
    sam_set_error("sam_score_table_from_text: A=%d: at most %d answers per sample", A, kMaxAnswers);
    return SAM_ERR_UNSUPPORTED;
  }
  const TextCarve c = text_carve(A, La, Lg);       // (A <= 64, La <= 128, Lg <= 255: far inside int)
  if ((size_t)c.total * sizeof(int) > 65536) {
    sam_set_error("sam_score_table_from_text: A=%d La=%d Lg=%d need more than 64 KiB of LDS", A, La, Lg);
    return SAM_ERR_UNSUPPORTED;
  }
  score_table_from_text_kernel<<<dim3((unsigned)B), dim3(kTextThreads), (size_t)c.total * sizeof(int), (hipStream_t)stream>>>(
      answer_text, ld_answer, answer_len, ocr_text, ld_ocr, ocr_len, ocr_count, A, La, No, Lw, Lg, meta, gt_norm, gt_norm_len, gt_score, gt_raw, gt_raw_len, ocr,
      ocr_out_len, status);
  SAM_LAUNCH_CHECK();
  return SAM_OK;
}

// Beam-search output to per-question results on the device (gfx950): what evaluate_predictions (evaluator.py:304-356) and the answer-file
// loop of Evaluator.evaluate (:122-130) do on the host with pandas, from complete_seqs and topkscores as the decoding steps leave them.
//   eval_score_kernel   one workgroup of four waves per BEAM: block_score of score_walk.h, the code score_kernel runs, against table row r / K -- the
//                       table of B samples is read in place, never repeated K times
//   eval_select_kernel  one workgroup per SAMPLE: wave 0 holds one beam's cumulative score per lane and picks numpy.argmax's beam (a ballot finds the first
//                       NaN; else a butterfly maximum and a ballot of the lanes that equal it, lowest lane first); the block gathers the chosen beam's ids,
//                       scores and flags, chains the per-metric maximum over the beams, and walks the chosen ids once more into LDS (block_assemble) to
//                       write the stripped answer string and its zero padding
//   score_totals_kernel (score_walk.h) over best_scores when the caller keeps a float64 accumulator
// No global atomics, no workspace; every output element is written exactly once, by one thread.
#include "common.h"
#include "sam_hip_eval.h"
#define SAM_SCORE_TABLES_ONLY          // kWordMap, kMapSize, punct_index, kMaxPeriods, kNoGlue: score.hip holds the one copy
#include "score.hip"
#undef SAM_SCORE_TABLES_ONLY
#include "score_walk.h"

namespace {

constexpr int kMaxBeams = 64;          // one beam per lane of the selecting wave

__global__ __launch_bounds__(kScoreThreads) void eval_score_kernel(const int64_t* __restrict__ seqs, ScoreTable T, int K, int S, int skip, int X,
                                                                   float* __restrict__ beam_scores, int32_t* __restrict__ beam_flags) {
  extern __shared__ int sbuf[];                    // three text buffers of X code points
  __shared__ ScoreShared sh;
  const int64_t r = blockIdx.x;
  block_score(seqs + r * S + skip, S - skip, r / K, T, sh, sbuf, X, beam_scores + 3 * r, beam_flags + r);
}

__global__ __launch_bounds__(kScoreThreads) void eval_select_kernel(const int64_t* __restrict__ seqs, const float* __restrict__ cum, ScoreTable T, int K, int S,
                                                                    int skip, int P, const float* __restrict__ beam_scores,
                                                                    const int32_t* __restrict__ beam_flags, int32_t* __restrict__ best,
                                                                    int64_t* __restrict__ best_ids, float* __restrict__ best_scores,
                                                                    int32_t* __restrict__ best_flags, float* __restrict__ oracle, int32_t* __restrict__ answer,
                                                                    int32_t* __restrict__ answer_len) {
  extern __shared__ int sbuf[];                    // two text buffers of P code points
  __shared__ ScoreShared sh;
  __shared__ int s_best;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, L = S - skip;
  const int64_t b = blockIdx.x, r0 = b * K;
  if (wave == 0) {
    const bool live = lane < K;
    const float v = live ? cum[r0 + lane] : -INFINITY;
    const unsigned long long nan = __ballot(live && v != v);
    int k;
    if (nan) {
      k = __ffsll((long long)nan) - 1;             // numpy.argmax: a NaN is greater than every number, the first one wins
    } else {
      float m = v;
#pragma unroll
      for (int o = 32; o >= 1; o >>= 1) m = fmaxf(m, __shfl_xor(m, o, 64));
      k = __ffsll((long long)__ballot(live && v == m)) - 1;      // (some live lane holds m: K >= 1, and a dead lane's -inf never exceeds a live value)
    }
    if (lane == 0) s_best = k;
  }
  __syncthreads();
  const int k = s_best;
  const int64_t r = r0 + k;
  for (int t = tid; t < L; t += kScoreThreads) best_ids[b * L + t] = seqs[r * S + skip + t];
  if (tid < 3) {
    best_scores[3 * b + tid] = beam_scores[3 * r + tid];
    float m = beam_scores[3 * r0 + tid];
    for (int j = 1; j < K; ++j) m = fmaxf(m, beam_scores[3 * (r0 + j) + tid]);
    oracle[3 * b + tid] = m;
  }
  if (tid == 3) { best[b] = k; best_flags[b] = beam_flags[r]; }
  // the chosen beam's string: the walk and the glue of the scoring kernel, then Python's strip()
  int* bufA = sbuf;
  int* bufB = sbuf + P;
  const int n1 = block_assemble(seqs + r * S + skip, L, b, T, sh, bufA, bufB, tid);      // n1 <= L * Lw + L - 1 < P
  int lo, hi;
  wave_strip(bufB, n1, lane, lo, hi);              // (every wave computes the same bounds)
  const int n = hi - lo;
  for (int i = tid; i < P; i += kScoreThreads) answer[b * P + i] = i < n ? bufB[lo + i] : 0;
  if (tid == 0) answer_len[b] = n;
}

}  // namespace

extern "C" int sam_eval_beams(const int64_t* seqs, const float* cum, const int32_t* meta, const int32_t* gt_norm, const int32_t* gt_norm_len,
                              const float* gt_score, const int32_t* gt_raw, const int32_t* gt_raw_len, const int32_t* ocr, const int32_t* ocr_len,
                              const int32_t* vocab_cp, const int32_t* vocab_len, int B, int K, int S, int skip, int A, int Lg, int No, int Lw, int V, int eos,
                              float* beam_scores, int32_t* beam_flags, int32_t* best, int64_t* best_ids, float* best_scores, int32_t* best_flags, float* oracle,
                              int32_t* answer, int32_t* answer_len, double* totals, void* stream) {
  SAM_REQUIRE(seqs && cum && meta && gt_norm && gt_norm_len && gt_score && gt_raw && gt_raw_len && ocr && ocr_len && vocab_cp && vocab_len,
              "sam_eval_beams: null pointer among the inputs");
  SAM_REQUIRE(beam_scores && beam_flags && best && best_ids && best_scores && best_flags && oracle && answer && answer_len,
              "sam_eval_beams: null pointer among the outputs");
  SAM_REQUIRE(B > 0 && K > 0 && S > 0 && A > 0 && Lg > 0 && No >= 0 && Lw > 0 && V > 0, "sam_eval_beams: bad shape (B=%d K=%d S=%d A=%d Lg=%d No=%d Lw=%d V=%d)",
              B, K, S, A, Lg, No, Lw, V);
  SAM_REQUIRE(skip >= 0 && skip < S, "sam_eval_beams: skip=%d leaves no column of S=%d to score", skip, S);
  SAM_REQUIRE((int64_t)B * K <= 0x7fffffff, "sam_eval_beams: B * K = %lld beams exceed the grid", (long long)B * K);
  SAM_REQUIRE(((uintptr_t)seqs % 8) == 0 && ((uintptr_t)best_ids % 8) == 0 && (!totals || ((uintptr_t)totals % 8) == 0), "sam_eval_beams: misaligned operand");
  const int L = S - skip;
  if (K > kMaxBeams) {
    sam_set_error("sam_eval_beams: K=%d: at most %d beams per sample", K, kMaxBeams);
    return SAM_ERR_UNSUPPORTED;
  }
  if (L > kMaxSteps) {
    sam_set_error("sam_eval_beams: L=%d scored steps exceed %d", L, kMaxSteps);
    return SAM_ERR_UNSUPPORTED;
  }
  if (Lg > 64 * kMaxQ - 1) {
    sam_set_error("sam_eval_beams: Lg=%d code points per ground truth exceed %d", Lg, 64 * kMaxQ - 1);
    return SAM_ERR_UNSUPPORTED;
  }
  // sam_score_answers' buffers: the joined words hold at most P = L * (Lw + 1) code points, the normaliser lengthens them to at most 2 * P + 8
  const int64_t P = (int64_t)L * (Lw + 1), X = 2 * P + 8;
  const size_t lds = (size_t)(3 * X) * sizeof(int);
  if (lds > 60 * 1024) {
    sam_set_error("sam_eval_beams: L * (Lw + 1) = %lld code points do not fit the LDS text buffers", (long long)P);
    return SAM_ERR_UNSUPPORTED;
  }
  hipStream_t st = (hipStream_t)stream;
  const ScoreTable T = {meta, gt_norm, gt_norm_len, gt_score, gt_raw, gt_raw_len, ocr, ocr_len, vocab_cp, vocab_len, A, Lg, No, Lw, V, eos};
  eval_score_kernel<<<dim3((unsigned)(B * K)), dim3(kScoreThreads), lds, st>>>(seqs, T, K, S, skip, (int)X, beam_scores, beam_flags);
  SAM_LAUNCH_CHECK();
  eval_select_kernel<<<dim3((unsigned)B), dim3(kScoreThreads), (size_t)(2 * P) * sizeof(int), st>>>(seqs, cum, T, K, S, skip, (int)P, beam_scores, beam_flags, best,
                                                                                                best_ids, best_scores, best_flags, oracle, answer, answer_len);
  SAM_LAUNCH_CHECK();
  if (totals) {
    score_totals_kernel<<<dim3(1), dim3(kScoreThreads), 0, st>>>(best_scores, B, totals);
    SAM_LAUNCH_CHECK();
  }
  return SAM_OK;
}

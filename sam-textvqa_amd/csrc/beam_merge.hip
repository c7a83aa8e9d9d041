// Beam-search output to per-question results with the answer STRING as the unit of choice (gfx950): the beams of a question that spell
// the same string are one group, a group's mass is the log of its members' summed probabilities, the group with the largest mass wins and its member with
// the largest cumulative score stands for it.  The project's own definition: the reference keeps the single best beam (eval_beams.hip).
//   merge_score_kernel  one workgroup of four waves per BEAM: block_score of score_walk.h, the code eval_score_kernel and score_kernel run, against table
//                       row r / K; the glued string it leaves in LDS is then stripped and written out with its zero padding -- the n-best list
//   merge_select_kernel one workgroup per SAMPLE.  The four waves take the beams in turn: a hash of each string (a pre-filter only), then per beam the
//                       lower beams of equal length and hash in ascending order, compared code point by code point until one is equal: the leader.  Wave 0
//                       then holds one beam per lane -- cumulative score and leader in registers, the other lanes' values by cross-lane reads: the K x K
//                       mass loop, numpy.argmax's rule over the leaders' masses (a ballot finds the first NaN; else a butterfly maximum and a ballot of
//                       the lanes that equal it, lowest first), the same rule over the winning group's members, and over all beams for plain_best.  The
//                       block gathers the representative's ids, scores, flags and string and chains the per-metric maximum over the beams.
//   score_totals_kernel (score_walk.h) over best_scores when the caller keeps a float64 accumulator
// No global atomics, no workspace; every output element is written exactly once, by one thread.
#include "common.h"
#include "sam_hip_beam_merge.h"
#define SAM_SCORE_TABLES_ONLY          // kWordMap, kMapSize, punct_index, kMaxPeriods, kNoGlue: score.hip holds the one copy
#include "score.hip"
#undef SAM_SCORE_TABLES_ONLY
#include "score_walk.h"

namespace {

constexpr int kMaxBeams = 64;          // one beam per lane of the selecting wave
constexpr int kWaves = kScoreThreads / 64;

__global__ __launch_bounds__(kScoreThreads) void merge_score_kernel(const int64_t* __restrict__ seqs, ScoreTable T, int K, int S, int skip, int X, int P,
                                                                    float* __restrict__ beam_scores, int32_t* __restrict__ beam_flags,
                                                                    int32_t* __restrict__ beam_answer, int32_t* __restrict__ beam_answer_len) {
  extern __shared__ int sbuf[];                    // three text buffers of X code points
  __shared__ ScoreShared sh;
  const int tid = threadIdx.x, lane = tid & 63;
  const int64_t r = blockIdx.x;
  block_score(seqs + r * S + skip, S - skip, r / K, T, sh, sbuf, X, beam_scores + 3 * r, beam_flags + r);
  // block_score's second buffer still holds the glued string (its normaliser only reads it), sh.n its length: Python's strip(), as eval_select_kernel
  const int* str = sbuf + X;
  int lo, hi;
  wave_strip(str, sh.n, lane, lo, hi);             // (every wave computes the same bounds)
  const int n = hi - lo;                           // n <= sh.n < P
  for (int i = tid; i < P; i += kScoreThreads) beam_answer[r * P + i] = i < n ? str[lo + i] : 0;
  if (tid == 0) beam_answer_len[r] = n;
}

// numpy.argmax over the lanes of the wave-uniform, non-empty set `in`: the first lane that holds a NaN, else the first that holds the maximum
__device__ __forceinline__ int wave_argmax_first(float v, bool in) {
  const unsigned long long nan = __ballot(in && v != v);
  if (nan) return __ffsll((long long)nan) - 1;
  float m = in ? v : -INFINITY;
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) m = fmaxf(m, __shfl_xor(m, o, 64));
  return __ffsll((long long)__ballot(in && v == m)) - 1;       // (some lane of the set holds m: a lane outside it counts as -inf, which exceeds nothing)
}

__global__ __launch_bounds__(kScoreThreads) void merge_select_kernel(const int64_t* __restrict__ seqs, const float* __restrict__ cum, int K, int S, int skip,
                                                                     int P, const float* __restrict__ beam_scores, const int32_t* __restrict__ beam_flags,
                                                                     const int32_t* __restrict__ beam_answer, const int32_t* __restrict__ beam_answer_len,
                                                                     int32_t* __restrict__ best, int64_t* __restrict__ best_ids,
                                                                     float* __restrict__ best_scores, int32_t* __restrict__ best_flags,
                                                                     float* __restrict__ oracle, int32_t* __restrict__ answer, int32_t* __restrict__ answer_len,
                                                                     int32_t* __restrict__ group, float* __restrict__ mass, int32_t* __restrict__ n_groups,
                                                                     int32_t* __restrict__ plain_best, float* __restrict__ best_mass) {
  __shared__ int s_len[kMaxBeams], s_bad[kMaxBeams], s_group[kMaxBeams];
  __shared__ unsigned s_hash[kMaxBeams];
  __shared__ int s_best;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, L = S - skip;
  const int64_t b = blockIdx.x, r0 = b * K;
  // per beam: length, hash of the code points (position-weighted sum: any order of addition gives the same word), the out-of-range flag
  for (int k = wave; k < K; k += kWaves) {
    const int n = max(0, min(beam_answer_len[r0 + k], P));
    const int32_t* row = beam_answer + (r0 + k) * P;
    unsigned h = 0;
    for (int i = lane; i < n; i += 64) h += (unsigned)row[i] * (((unsigned)i + 1u) * 2654435761u | 1u);
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) h += __shfl_xor(h, o, 64);
    if (lane == 0) { s_len[k] = n; s_hash[k] = h; s_bad[k] = beam_flags[r0 + k] & 1; }
  }
  __syncthreads();
  // per beam k its leader: the lowest beam j <= k with the same string.  Lane j holds beam j's length, hash and flag; the candidates j < k go in
  // ascending order through the comparison of code points, which alone decides.  A flagged beam is no candidate and has none.
  {
    const bool have = lane < K;
    const int ln = have ? s_len[lane] : -1;
    const unsigned hs = have ? s_hash[lane] : 0u;
    const bool ok = have && !s_bad[lane];
    for (int k = wave; k < K; k += kWaves) {
      const int nk = s_len[k];
      unsigned long long cand = __ballot(ok && lane < k && ln == nk && hs == s_hash[k]);
      if (s_bad[k]) cand = 0ull;
      const int32_t* rk = beam_answer + (r0 + k) * P;
      int lead = k;
      while (cand) {                               // (wave-uniform)
        const int j = __ffsll((long long)cand) - 1;
        cand &= cand - 1ull;
        const int32_t* rj = beam_answer + (r0 + j) * P;
        bool diff = false;
        for (int i = lane; i < nk; i += 64) diff |= rj[i] != rk[i];
        if (__ballot(diff) == 0ull) { lead = j; break; }
      }
      if (lane == 0) s_group[k] = lead;
    }
  }
  __syncthreads();
  if (wave == 0) {
    const bool live = lane < K;
    const float c = live ? cum[r0 + lane] : 0.f;
    const int g = live ? s_group[lane] : -1;       // (a dead lane's -1 is no beam's leader)
    // the group's members in beam order: their number, whether one is a NaN, fmaxf chained from the first (every lane runs both loops: the cross-lane
    // reads stay in uniform control flow)
    int cnt = 0;
    bool any_nan = false;
    float m = 0.f;
    for (int j = 0; j < K; ++j) {
      const float cj = __shfl(c, j, 64);
      const int gj = __shfl(g, j, 64);
      if (gj == g) {
        any_nan |= cj != cj;
        m = cnt ? fmaxf(m, cj) : cj;
        ++cnt;
      }
    }
    float s = 0.f;
    for (int j = 0; j < K; ++j) {
      const float cj = __shfl(c, j, 64);
      const int gj = __shfl(g, j, 64);
      if (gj == g) s += expf(cj - m);
    }
    float ms = c;                                  // one member: its cumulative score as it stands
    if (cnt > 1) ms = any_nan ? __builtin_nanf("") : (m == -INFINITY ? -INFINITY : m + logf(s));
    const bool leader = live && g == lane;
    const int n_lead = __popcll(__ballot(leader));
    const int win = wave_argmax_first(ms, leader);
    const int rep = wave_argmax_first(c, live && g == win);
    const int plain = wave_argmax_first(c, live);
    const float win_mass = __shfl(ms, win, 64);
    if (live) { group[r0 + lane] = g; mass[r0 + lane] = ms; }
    if (lane == 0) { n_groups[b] = n_lead; plain_best[b] = plain; best_mass[b] = win_mass; s_best = rep; }
  }
  __syncthreads();
  const int k = s_best;
  const int64_t r = r0 + k;
  for (int t = tid; t < L; t += kScoreThreads) best_ids[b * L + t] = seqs[r * S + skip + t];
  if (tid < 3) {
    best_scores[3 * b + tid] = beam_scores[3 * r + tid];
    float mx = beam_scores[3 * r0 + tid];
    for (int j = 1; j < K; ++j) mx = fmaxf(mx, beam_scores[3 * (r0 + j) + tid]);
    oracle[3 * b + tid] = mx;
  }
  if (tid == 3) { best[b] = k; best_flags[b] = beam_flags[r]; answer_len[b] = beam_answer_len[r]; }
  for (int i = tid; i < P; i += kScoreThreads) answer[b * P + i] = beam_answer[r * P + i];      // (the row carries its zero padding)
}

}  // namespace

extern "C" int sam_eval_beams_merged(const int64_t* seqs, const float* cum, const int32_t* meta, const int32_t* gt_norm, const int32_t* gt_norm_len,
                                     const float* gt_score, const int32_t* gt_raw, const int32_t* gt_raw_len, const int32_t* ocr, const int32_t* ocr_len,
                                     const int32_t* vocab_cp, const int32_t* vocab_len, int B, int K, int S, int skip, int A, int Lg, int No, int Lw, int V,
                                     int eos, float* beam_scores, int32_t* beam_flags, int32_t* best, int64_t* best_ids, float* best_scores,
                                     int32_t* best_flags, float* oracle, int32_t* answer, int32_t* answer_len, int32_t* beam_answer, int32_t* beam_answer_len,
                                     int32_t* group, float* mass, int32_t* n_groups, int32_t* plain_best, float* best_mass, double* totals, void* stream) {
  SAM_REQUIRE(seqs && cum && meta && gt_norm && gt_norm_len && gt_score && gt_raw && gt_raw_len && ocr && ocr_len && vocab_cp && vocab_len,
              "sam_eval_beams_merged: null pointer among the inputs");
  SAM_REQUIRE(beam_scores && beam_flags && best && best_ids && best_scores && best_flags && oracle && answer && answer_len && beam_answer && beam_answer_len &&
                  group && mass && n_groups && plain_best && best_mass,
              "sam_eval_beams_merged: null pointer among the outputs");
  SAM_REQUIRE(B > 0 && K > 0 && S > 0 && A > 0 && Lg > 0 && No >= 0 && Lw > 0 && V > 0,
              "sam_eval_beams_merged: bad shape (B=%d K=%d S=%d A=%d Lg=%d No=%d Lw=%d V=%d)", B, K, S, A, Lg, No, Lw, V);
  SAM_REQUIRE(skip >= 0 && skip < S, "sam_eval_beams_merged: skip=%d leaves no column of S=%d to score", skip, S);
  SAM_REQUIRE((int64_t)B * K <= 0x7fffffff, "sam_eval_beams_merged: B * K = %lld beams exceed the grid", (long long)B * K);
  SAM_REQUIRE(((uintptr_t)seqs % 8) == 0 && ((uintptr_t)best_ids % 8) == 0 && (!totals || ((uintptr_t)totals % 8) == 0),
              "sam_eval_beams_merged: misaligned operand");
  const int L = S - skip;
  if (K > kMaxBeams) {
    sam_set_error("sam_eval_beams_merged: K=%d: at most %d beams per sample", K, kMaxBeams);
    return SAM_ERR_UNSUPPORTED;
  }
  if (L > kMaxSteps) {
    sam_set_error("sam_eval_beams_merged: L=%d scored steps exceed %d", L, kMaxSteps);
    return SAM_ERR_UNSUPPORTED;
  }
  if (Lg > 64 * kMaxQ - 1) {
    sam_set_error("sam_eval_beams_merged: Lg=%d code points per ground truth exceed %d", Lg, 64 * kMaxQ - 1);
    return SAM_ERR_UNSUPPORTED;
  }
  // sam_score_answers' buffers: the joined words hold at most P = L * (Lw + 1) code points, the normaliser lengthens them to at most 2 * P + 8
  const int64_t P = (int64_t)L * (Lw + 1), X = 2 * P + 8;
  const size_t lds = (size_t)(3 * X) * sizeof(int);
  if (lds > 60 * 1024) {
    sam_set_error("sam_eval_beams_merged: L * (Lw + 1) = %lld code points do not fit the LDS text buffers", (long long)P);
    return SAM_ERR_UNSUPPORTED;
  }
  hipStream_t st = (hipStream_t)stream;
  const ScoreTable T = {meta, gt_norm, gt_norm_len, gt_score, gt_raw, gt_raw_len, ocr, ocr_len, vocab_cp, vocab_len, A, Lg, No, Lw, V, eos};
  merge_score_kernel<<<dim3((unsigned)(B * K)), dim3(kScoreThreads), lds, st>>>(seqs, T, K, S, skip, (int)X, (int)P, beam_scores, beam_flags, beam_answer,
                                                                                beam_answer_len);
  SAM_LAUNCH_CHECK();
  merge_select_kernel<<<dim3((unsigned)B), dim3(kScoreThreads), 0, st>>>(seqs, cum, K, S, skip, (int)P, beam_scores, beam_flags, beam_answer, beam_answer_len, best,
                                                                         best_ids, best_scores, best_flags, oracle, answer, answer_len, group, mass, n_groups,
                                                                         plain_best, best_mass);
  SAM_LAUNCH_CHECK();
  if (totals) {
    score_totals_kernel<<<dim3(1), dim3(kScoreThreads), 0, st>>>(best_scores, B, totals);
    SAM_LAUNCH_CHECK();
  }
  return SAM_OK;
}

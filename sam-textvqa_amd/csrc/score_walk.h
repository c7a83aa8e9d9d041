// The per-prediction half of the metrics as block-wide device code, shared by score.hip (one prediction per table row) and
// eval_beams.hip (K beams per table row, and the chosen beam's answer string).  One copy each of
//   wave_levenshtein    the edit distance by rows, the ground truth's columns across the lanes
//   block_assemble      the id walk of sam/datasets/metrics.py:39-51 into LDS, the words joined with blanks, " 's" glued to "'s"
//   block_score         block_assemble, then ANLS on waves 1-3 and the normaliser with the soft-score lookup on wave 0: the three scores and the flag word
//   score_totals_kernel the batch sums into the float64 accumulator, in a fixed order
// Every function is called by all kScoreThreads threads of a block (four waves).  The normaliser's tables (kWordMap, punct_index, kNoGlue) are defined in
// score.hip in front of this header; a file that includes this one includes that section of score.hip first, as score_text.hip does for score_norm.h.
#pragma once
#include "score_norm.h"

constexpr int kScoreThreads = 256;
constexpr int kMaxSteps = 64;          // decoding steps per row (shared word-list capacity)
constexpr int kMaxQ = 4;               // 64-column chunks of a distance row: ground truths of up to 255 code points

// what a block keeps in static LDS while it scores one prediction
struct ScoreShared {
  const int32_t* src[kMaxSteps];
  int len[kMaxSteps], off[kMaxSteps];
  int nw, n, flag;
  float anls[4], vqa, acc;
  int empty[4];
};

// the score table of a batch and the vocabulary's text, as the entry points receive them
struct ScoreTable {
  const int32_t *meta, *gt_norm, *gt_norm_len;
  const float* gt_score;
  const int32_t *gt_raw, *gt_raw_len, *ocr, *ocr_len, *vocab, *vocab_len;
  int A, Lg, No, Lw, V, eos;
};

// Levenshtein distance between a[0, n) (LDS) and g[0, m) (global), m <= 64 * kMaxQ - 1; every argument wave-uniform, so is the result
static __device__ int wave_levenshtein(const int* a, int n, const int32_t* __restrict__ g, int m, int lane) {
  const int Q = (m >> 6) + 1;
  int prev[kMaxQ], gq[kMaxQ];
#pragma unroll
  for (int q = 0; q < kMaxQ; ++q) {
    const int j = q * 64 + lane;
    prev[q] = j;
    gq[q] = (j >= 1 && j <= m) ? g[j - 1] : -1;
  }
  for (int i = 1; i <= n; ++i) {
    const int ca = a[i - 1];
    int cur[kMaxQ];
    int carry = 1 << 29, left = 0;                 // left: the previous row's cell just left of this chunk
#pragma unroll
    for (int q = 0; q < kMaxQ; ++q) {
      cur[q] = prev[q];
      if (q < Q) {
        const int j = q * 64 + lane;
        int diag = __shfl_up(prev[q], 1, 64);
        if (lane == 0) diag = left;
        left = __shfl(prev[q], 63, 64);
        int t = min(prev[q] + 1, diag + (ca != gq[q] ? 1 : 0));
        if (j == 0) t = i;
        int v = t - j;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
          const int u = __shfl_up(v, o, 64);
          if (lane >= o) v = min(v, u);
        }
        v = min(v, carry);
        carry = __shfl(v, 63, 64);
        cur[q] = v + j;
      }
    }
#pragma unroll
    for (int q = 0; q < kMaxQ; ++q) prev[q] = cur[q];
  }
  int d = 0;
#pragma unroll
  for (int q = 0; q < kMaxQ; ++q) {
    const int v = __shfl(prev[q], m & 63, 64);
    if (q == (m >> 6)) d = v;
  }
  return d;
}

// The id walk (metrics.py:39-51) of row[0, L) over table row tb: thread 0 walks the ids into (source, length, offset) triples; all threads copy the
// words into bufA, joined with blanks; wave 0 glues " 's" to "'s" into bufB (every blank that "'s" follows goes: the pattern cannot overlap itself, so this
// is str.replace's left-to-right result) and clears the NO_GLUE bits, which have done their work after it.  -> the length of bufB's string, block-uniform;
// sh.flag is 1 when an id outside [0, V + No) ended the walk.  bufA and bufB hold at least L * (Lw + 1) ints each.  Ends with a block barrier.
__device__ __forceinline__ int block_assemble(const int64_t* __restrict__ row, int L, int64_t tb, const ScoreTable& T, ScoreShared& sh, int* bufA, int* bufB,
                                              int tid) {
  if (tid == 0) {
    int nw = 0, off = 0, flag = 0;
    for (int t = 0; t < L; ++t) {
      const int64_t id = row[t];
      if (id < 0 || id >= (int64_t)T.V + T.No) { flag = 1; break; }
      const int32_t* src;
      int len;
      if (id < T.V) {
        if (id == T.eos) break;
        src = T.vocab + id * T.Lw;
        len = T.vocab_len[id];
      } else {
        const int64_t slot = tb * T.No + (id - T.V);
        src = T.ocr + slot * T.Lw;
        len = T.ocr_len[slot];
      }
      len = max(0, min(len, T.Lw));
      if (nw > 0) off += 1;                        // the blank of " ".join
      sh.src[nw] = src; sh.len[nw] = len; sh.off[nw] = off;
      off += len;
      ++nw;
    }
    sh.nw = nw; sh.n = off; sh.flag = flag;        // off <= L * Lw + L - 1
    sh.vqa = 0.f; sh.acc = 0.f;
  }
  if (tid < 4) { sh.anls[tid] = 0.f; sh.empty[tid] = 0; }
  __syncthreads();
  const int nw = sh.nw, n0 = sh.n;
  for (int w = 0; w < nw; ++w) {
    const int32_t* src = sh.src[w];
    const int len = sh.len[w], off = sh.off[w];
    if (w > 0 && tid == 0) bufA[off - 1] = ' ';
    for (int i = tid; i < len; i += kScoreThreads) bufA[off + i] = src[i];
  }
  __syncthreads();
  if ((tid >> 6) == 0) {
    const int n1 = wave_emit(n0, bufB, tid & 63, [&](int i, int& v0, int& v1) {
      const int c = bufA[i];
      if (c == ' ' && i + 2 < n0 && bufA[i + 1] == '\'' && bufA[i + 2] == 's') return 0;
      v0 = c & ~kNoGlue;
      return 1;
    });
    if (tid == 0) sh.n = n1;
  }
  __syncthreads();
  return sh.n;
}

// The three scores and the flag word of the prediction row[0, L) against table row tb.  sbuf: three text buffers of X >= 2 * L * (Lw + 1) + 8 ints.
//   ANLS (metrics.py:366-379): waves 1-3 take the raw ground truths in turn.  Levenshtein runs by rows: the ground truth's m + 1 columns lie across the
//     lanes (up to four cells per lane, in registers); the >= 0.5 threshold is decided in integers (2 d <= max len).
//   wave 0 meanwhile normalises the string by the rules of metrics.normalize_answer and compares the result with the sample's normalised ground truths.
// Thread 0 writes scores[0..2] and *flag; nothing else is written.  On return sbuf[X, X + sh.n) still holds block_assemble's glued string, visible to
// every thread (the normaliser only reads it): beam_merge.hip strips it and writes it out.
__device__ __forceinline__ void block_score(const int64_t* __restrict__ row, int L, int64_t tb, const ScoreTable& T, ScoreShared& sh, int* sbuf, int X,
                                            float* __restrict__ scores, int32_t* __restrict__ flag) {
  int* bufA = sbuf;
  int* bufB = sbuf + X;
  int* bufC = sbuf + 2 * X;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int A = T.A, Lg = T.Lg;
  const int n1 = block_assemble(row, L, tb, T, sh, bufA, bufB, tid);
  const int32_t* mt = T.meta + 4 * tb;

  if (wave > 0) {
    const int n_raw = max(0, min(mt[1], A));
    int lo, hi;
    wave_strip(bufB, n1, lane, lo, hi);
    const int n = hi - lo;
    float best = 0.f;
    int empty = 0;
    for (int a = wave - 1; a < n_raw; a += 3) {
      const int m = max(0, min(T.gt_raw_len[tb * A + a], Lg));
      const int mx = max(n, m);
      if (mx == 0) { empty = 1; continue; }        // the reference divides by zero here: 0 and flag bit 1
      const int d = wave_levenshtein(bufB + lo, n, T.gt_raw + (tb * A + a) * Lg, m, lane);
      if (2 * d <= mx) best = fmaxf(best, 1.0f - (float)d / (float)mx);
    }
    if (lane == 0) { sh.anls[wave] = best; sh.empty[wave] = empty; }
  } else {
    const int out = wave_normalize(bufB, n1, bufA, bufC, lane);
    const int n_norm = max(0, min(mt[0], A));
    for (int a = 0; a < n_norm; ++a) {
      const int m = max(0, min(T.gt_norm_len[tb * A + a], Lg));
      if (m != out) continue;
      const int32_t* g = T.gt_norm + (tb * A + a) * Lg;
      bool diff = false;
      for (int j = lane; j < m; j += 64) diff |= bufA[j] != g[j];
      if (__ballot(diff) == 0ull) {
        if (lane == 0) { sh.vqa = T.gt_score[tb * A + a]; sh.acc = 1.0f; }
        break;
      }
    }
  }
  __syncthreads();
  if (tid == 0) {
    scores[0] = sh.vqa;
    scores[1] = sh.acc;
    scores[2] = fmaxf(fmaxf(sh.anls[1], sh.anls[2]), sh.anls[3]);
    *flag = sh.flag | ((sh.empty[1] | sh.empty[2] | sh.empty[3]) ? 2 : 0);
  }
}

// totals[0..2] += the column sums of scores [B, 3] in float64, totals[3] += B: per thread in ascending sample order, then a fixed tree over the block
static __global__ __launch_bounds__(kScoreThreads) void score_totals_kernel(const float* __restrict__ scores, int B, double* __restrict__ totals) {
  __shared__ double red[3][kScoreThreads];
  const int tid = threadIdx.x;
  double acc[3] = {0.0, 0.0, 0.0};
  for (int b = tid; b < B; b += kScoreThreads) {
#pragma unroll
    for (int c = 0; c < 3; ++c) acc[c] += (double)scores[3 * (int64_t)b + c];
  }
#pragma unroll
  for (int c = 0; c < 3; ++c) red[c][tid] = acc[c];
  __syncthreads();
  for (int o = kScoreThreads / 2; o >= 1; o >>= 1) {
    if (tid < o) {
#pragma unroll
      for (int c = 0; c < 3; ++c) red[c][tid] += red[c][tid + o];
    }
    __syncthreads();
  }
  if (tid < 3) totals[tid] += red[tid][0];
  if (tid == 3) totals[3] += (double)B;
}

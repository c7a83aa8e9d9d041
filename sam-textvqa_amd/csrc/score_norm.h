// The device normaliser of the metrics: metrics.normalize_answer's rules on lowered text, one wave per string, shared by
// score.hip (the predicted string, once per step) and score_text.hip (the ground truths, when the score table is built from text).  is_space and wave_emit
// come from text.h; one copy each of
//   wave_strip     the string without the whitespace at either end
//   wave_normalize the pass sequence of metrics._normalize_lowered
// The two tables the passes read -- kWordMap / kMapSize (metrics.WORD_MAP) and punct_index (metrics.PUNCTUATION), with kMaxPeriods -- stay in score.hip,
// where tests/test_metrics_cpu.py compares their text with the Python lists; score.hip defines them in front of this header, and score_text.hip includes
// that section of score.hip (SAM_SCORE_TABLES_ONLY) before it includes this file.
#pragma once
#include "common.h"
#include "text.h"

// [lo, hi) of s[0, n) without the whitespace at either end (lo = hi = 0 when nothing else is there); wave-uniform result
__device__ __forceinline__ void wave_strip(const int* s, int n, int lane, int& lo, int& hi) {
  int first = 0x7fffffff, last = -1;
  for (int i = lane; i < n; i += 64) {
    if (!is_space(s[i])) { first = min(first, i); last = max(last, i); }
  }
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) {
    first = min(first, __shfl_xor(first, o, 64));
    last = max(last, __shfl_xor(last, o, 64));
  }
  lo = last < 0 ? 0 : first;
  hi = last < 0 ? 0 : last + 1;
}

// metrics._normalize_lowered on src[0, n0) (LDS, lowered text; only read), by one wave: the result lies in bufA[0, return value).  bufA and bufC are the
// wave's own scratch of at least 2 * n0 + 8 ints each: "'s" -> " 's" adds at most one code point per two of the input, a contraction at most one per
// four, and the two never meet in one word.  n0 is wave-uniform, and so is the result.
__device__ __forceinline__ int wave_normalize(const int* src, int n0, int* bufA, int* bufC, int lane) {
  int n = wave_emit(n0, bufA, lane, [&](int i, int& v0, int& v1) {           // every "," and "?" goes
    v0 = src[i];
    return (v0 == ',' || v0 == '?') ? 0 : 1;
  });
  n = wave_emit(n, bufC, lane, [&](int i, int& v0, int& v1) {                // "'s" -> " 's"
    v0 = bufA[i];
    if (v0 == '\'' && i + 1 < n && bufA[i + 1] == 's') { v0 = ' '; v1 = '\''; return 2; }
    return 1;
  });
  int lo, hi;
  wave_strip(bufC, n, lane, lo, hi);
  int* s = bufC + lo;
  n = hi - lo;
  unsigned touch = 0;                            // per punctuation character: does some occurrence touch a blank (newline and tab count as blanks by now)
  for (int i = lane; i < n; i += 64) {
    const int c = s[i];
    if (c == '\n' || c == '\t') s[i] = ' ';
  }
  __builtin_amdgcn_wave_barrier();
  for (int i = lane; i < n; i += 64) {
    const int k = punct_index(s[i]);
    if (k >= 0 && ((i + 1 < n && s[i + 1] == ' ') || (i > 0 && s[i - 1] == ' '))) touch |= 1u << k;
  }
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) touch |= __shfl_xor(touch, o, 64);
  n = wave_emit(n, bufA, lane, [&](int i, int& v0, int& v1) {
    v0 = s[i];
    const int k = punct_index(v0);
    if (k < 0) return 1;
    if ((touch >> k) & 1u) return 0;
    v0 = ' ';
    return 1;
  });
  {                                              // the first 32 periods that no digit follows go
    int out = 0, seen = 0;
    const unsigned long long lt = (1ull << lane) - 1ull;
    for (int base = 0; base < n; base += 64) {
      const int i = base + lane;
      int c = 0;
      bool cand = false;
      if (i < n) {
        c = bufA[i];
        const int nx = i + 1 < n ? bufA[i + 1] : 0;
        cand = c == '.' && !(nx >= '0' && nx <= '9');
      }
      const unsigned long long mc = __ballot(cand);
      const bool keep = i < n && !(cand && seen + __popcll(mc & lt) < kMaxPeriods);
      const unsigned long long mk = __ballot(keep);
      if (keep) bufC[out + __popcll(mk & lt)] = c;
      out += __popcll(mk);
      seen += __popcll(mc);
    }
    __builtin_amdgcn_wave_barrier();
    n = out;
  }
  // words: number words, articles, contractions (one lookup), joined with blanks
  int out = 0, i = 0;
  while (i < n) {
    while (i < n && is_space(bufC[i])) ++i;
    if (i >= n) break;
    const int ws = i;
    while (i < n && !is_space(bufC[i])) ++i;
    const int len = i - ws;
    int hit = -1;
    if (len <= 15) {
      bool match = false;
      int mine = -1;
      for (int k = lane; k < kMapSize; k += 64) {
        bool eq = kWordMap[k].key[len] == 0;
        for (int j = 0; j < len && eq; ++j) eq = (int)(unsigned char)kWordMap[k].key[j] == bufC[ws + j];
        if (eq) { match = true; mine = k; }
      }
      const unsigned long long mm = __ballot(match);
      if (mm) hit = __shfl(mine, __ffsll((long long)mm) - 1, 64);
    }
    if (hit >= 0) {
      int vl = 0;
      while (vl < 16 && kWordMap[hit].val[vl]) ++vl;
      if (vl == 0) continue;                     // an article: dropped
      if (out > 0) { if (lane == 0) bufA[out] = ' '; ++out; }
      if (lane < vl) bufA[out + lane] = (int)(unsigned char)kWordMap[hit].val[lane];
      out += vl;
    } else {
      if (out > 0) { if (lane == 0) bufA[out] = ' '; ++out; }
      for (int j = lane; j < len; j += 64) bufA[out + j] = bufC[ws + j];
      out += len;
    }
  }
  __builtin_amdgcn_wave_barrier();
  return out;
}

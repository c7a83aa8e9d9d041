// The M4C answer tables of a batch straight from the answers' and the OCR tokens' text (gfx950): one launch per batch, one workgroup per sample.
//   answer_table_from_text  <- the string half of M4CAnswerProcessor.__call__ (sam/datasets/processors.py:586-692, match_answer_to_vocab_ocr_seq :542-578,
//                              get_all_indices :694-707), i.e. answers.build_answer_table + answers.collate_answer_tables of every sample.
// The outputs equal the host's bit for bit, orders and padding included; answers.tables_from_text_host is the host twin.  The host rules, and how each is
// kept here:
//   splitting      str.split(): a word ends at every code point Python's str.isspace() accepts (is_space of text.h; the CPU test enumerates all code points)
//   soft scores    leave-one-out min(1, k / 3), summed over the A answers in answer order and divided by A, in f64.  Only the fp32 rounding of a score
//                  leaves the kernel (step0_val), and the scores are compared only with each other.  The exact value is q / (3 A) with an integer q.
//                  If it is dyadic its denominator is a power of two below 3 A <= 765, so it is an fp32 number; otherwise its distance to any fp32
//                  rounding boundary k / 2^p is |q 2^p - 3 A k| / (3 A 2^p) >= 1 / (3 A 2^p), i.e. at least 2^-25 / (3 A) >= 2^-35 of its own size,
//                  while A + 2 f64 roundings of non-negative terms err by at most (A + 2) 2^-53 <= 2^-44 of it (A <= 255, enforced by the entry
//                  point) -- whichever way the host's sum() associates or compensates, the fp32 value is the same.  fp32 rounding is monotone, so the maximum of
//                  the rounded scores is the rounded maximum: the step-0 maximum is taken on the fp32 bit patterns (non-negative: unsigned order).
//   matching       the word's vocabulary index first (exact lookup in the hash index), then V + o for every OCR slot o holding the word, ascending:
//                  one wave per word, one OCR slot per lane, the slots as a ballot mask.  vocab_lookup is index_lookup of text.h behind the lengths no word has.
//   expansion      the reference's product, cut to max_match_num after every word, is the first min(max_match_num, product) tuples of the full product
//                  in lexicographic order (every cut keeps a prefix, the last word runs fastest): sequence j is read off the mixed-radix digits of j
//   groups         numbered by first occurrence in the scan over (sequence, step): every scanned value is entered into an LDS hash table with the
//                  minimum of its scan positions (atomicMin: the result does not depend on the order the threads arrive in), the group id of a value
//                  is the rank of its minimum.  Step-0 indices likewise by the first sequence that starts with them.
//   target lists   per scored group the index itself, then for an OCR slot its token's vocabulary word unless <unk>, for a vocabulary word V + o of every
//                  OCR slot holding it (a ballot again)
// Where the host raises the kernel sets one status bit and writes an all-zero table (the header describes which).  No global atomics, no workspace, every
// output element written exactly once by one thread.
#include "common.h"
#include "text.h"
#include "sam_hip_answers.h"

namespace {

constexpr int kThreads = 256, kWaves = kThreads / 64;
constexpr int kMaxAnswerChars = 128, kMaxWordChars = 64, kWordsPerAnswer = kMaxAnswerChars / 2;   // a word and its separator take two code points
constexpr int kNone = 0x7fffffff;
enum { ST_GROUPS = 1, ST_EXTRA = 2, ST_PAD_SLOT = 4, ST_UNK_TARGET = 8 };

__device__ __forceinline__ int nth_set_bit(unsigned long long m, int n) {
  for (int i = 0; i < n; ++i) m &= m - 1;
  return m ? __ffsll((long long)m) - 1 : 0;
}

// the LDS carve, shared by the host (size check) and the kernel; every offset a multiple of 8 bytes
struct Carve {
  int ans, alen, ocr, olen, tokv, omin, nw, dead, nseq, seqoff, score, wv, wmask, wstart, wlen, wcnt, seq, seqans, hkey, hmin, hmin0, hs0, hscored, hgid, gkey,
      gscored, gcnt, gv, gmask, goff, s0idx, s0val, misc, total, H;
};
__host__ __device__ inline int up8(int x) { return (x + 7) & ~7; }
__host__ __device__ inline Carve carve(int A, int La, int No, int Lw, int S, int L, int G) {
  Carve c;
  int H = 64;
  while (H < 2 * (G + 1)) H *= 2;
  c.H = H;
  int o = 0;
#define SAM_TAKE(field, bytes) c.field = o; o += up8(bytes);
  SAM_TAKE(wmask, 8 * A * L) SAM_TAKE(gmask, 8 * G)
  SAM_TAKE(ans, 4 * A * La) SAM_TAKE(alen, 4 * A) SAM_TAKE(ocr, 4 * No * Lw) SAM_TAKE(olen, 4 * No) SAM_TAKE(tokv, 4 * No) SAM_TAKE(omin, 4 * No)
  SAM_TAKE(nw, 4 * A) SAM_TAKE(dead, 4 * A) SAM_TAKE(nseq, 4 * A) SAM_TAKE(seqoff, 4 * (A + 1)) SAM_TAKE(score, 4 * A) SAM_TAKE(wv, 4 * A * L)
  SAM_TAKE(wstart, A * kWordsPerAnswer) SAM_TAKE(wlen, A * kWordsPerAnswer) SAM_TAKE(wcnt, A * kWordsPerAnswer)
  SAM_TAKE(seq, 4 * S * L) SAM_TAKE(seqans, S)
  SAM_TAKE(hkey, 4 * H) SAM_TAKE(hmin, 4 * H) SAM_TAKE(hmin0, 4 * H) SAM_TAKE(hs0, 4 * H) SAM_TAKE(hscored, 4 * H) SAM_TAKE(hgid, 4 * H)
  SAM_TAKE(gkey, 4 * G) SAM_TAKE(gscored, 4 * G) SAM_TAKE(gcnt, 4 * G) SAM_TAKE(gv, 4 * G) SAM_TAKE(goff, 4 * (G + 1)) SAM_TAKE(s0idx, 4 * G) SAM_TAKE(s0val, 4 * G)
  SAM_TAKE(misc, 4 * 16)
#undef SAM_TAKE
  c.total = o;
  return c;
}
enum { M_NSEQ, M_OVERFLOW, M_NGRP, M_N0, M_UNKPOS, M_UNKSCORED, M_OCRSCORED_LO, M_OCRSCORED_HI, M_STATUS, M_NEXTRA };

// slot of `val` in the group table, inserting it when absent; -1: the table is full (more than H > G distinct values)
__device__ __forceinline__ int group_slot(int* hkey, int H, int val, bool insert) {
  unsigned s = mix32((unsigned)val) & (unsigned)(H - 1);
  for (int it = 0; it < H; ++it) {
    int k = hkey[s];
    if (k == -1 && insert) {
      const int old = atomicCAS(&hkey[s], -1, val);          // (a key, once written, never changes)
      k = old == -1 ? val : old;
    }
    if (k == val) return (int)s;
    if (k == -1) return -1;
    s = (s + 1) & (unsigned)(H - 1);
  }
  return -1;
}

__global__ __launch_bounds__(kThreads) void answer_table_from_text_kernel(
    const int32_t* __restrict__ answer_text, int64_t ld_answer, const int32_t* __restrict__ answer_len, const int32_t* __restrict__ ocr_text, int64_t ld_ocr,
    const int32_t* __restrict__ ocr_len, const int32_t* __restrict__ vocab_cp, int64_t ld_vocab, const int32_t* __restrict__ vocab_len,
    const int32_t* __restrict__ slots, int A, int La, int No, int Lw, int V, int Lv, int T, int unk, int eos, int S, int L, int G, int E, int max_match,
    int32_t* __restrict__ meta, int32_t* __restrict__ seq_len, int16_t* __restrict__ seq_grp, int32_t* __restrict__ step0_idx, float* __restrict__ step0_val,
    int32_t* __restrict__ grp_idx, int32_t* __restrict__ grp_off, int32_t* __restrict__ grp_extra, int32_t* __restrict__ status) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const Carve c = carve(A, La, No, Lw, S, L, G);
  const int H = c.H;
  int* s_ans = (int*)(smem + c.ans); int* s_alen = (int*)(smem + c.alen); int* s_ocr = (int*)(smem + c.ocr); int* s_olen = (int*)(smem + c.olen);
  int* s_tokv = (int*)(smem + c.tokv); int* s_omin = (int*)(smem + c.omin); int* s_nw = (int*)(smem + c.nw); int* s_dead = (int*)(smem + c.dead);
  int* s_nseq = (int*)(smem + c.nseq); int* s_seqoff = (int*)(smem + c.seqoff); float* s_score = (float*)(smem + c.score); int* s_wv = (int*)(smem + c.wv);
  unsigned long long* s_wmask = (unsigned long long*)(smem + c.wmask);
  unsigned char* s_wstart = smem + c.wstart; unsigned char* s_wlen = smem + c.wlen; unsigned char* s_wcnt = smem + c.wcnt;
  int* s_seq = (int*)(smem + c.seq); unsigned char* s_seqans = smem + c.seqans;
  int* h_key = (int*)(smem + c.hkey); int* h_min = (int*)(smem + c.hmin); int* h_min0 = (int*)(smem + c.hmin0); unsigned* h_s0 = (unsigned*)(smem + c.hs0);
  int* h_scored = (int*)(smem + c.hscored); int* h_gid = (int*)(smem + c.hgid);
  int* g_key = (int*)(smem + c.gkey); int* g_scored = (int*)(smem + c.gscored); int* g_cnt = (int*)(smem + c.gcnt); int* g_v = (int*)(smem + c.gv);
  unsigned long long* g_mask = (unsigned long long*)(smem + c.gmask); int* g_off = (int*)(smem + c.goff);
  int* s0_idx = (int*)(smem + c.s0idx); unsigned* s0_val = (unsigned*)(smem + c.s0val); int* misc = (int*)(smem + c.misc);

  const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const WordIndex index{vocab_cp, ld_vocab, vocab_len, slots, V, T};
  auto vocab_lookup = [&](const int* w, int n) { return (n <= 0 || n > Lv) ? -1 : index_lookup(index, n, [w](int i) { return w[i]; }); };
  meta += 4 * (int64_t)b; seq_len += (int64_t)b * S; seq_grp += (int64_t)b * S * L; step0_idx += (int64_t)b * S; step0_val += (int64_t)b * S;
  grp_idx += (int64_t)b * G; grp_off += (int64_t)b * (G + 1); grp_extra += (int64_t)b * E;

  // ---- stage the sample's texts, clear the tables
  for (int i = tid; i < A * La; i += kThreads) s_ans[i] = answer_text[((int64_t)b * A + i / La) * ld_answer + i % La];
  for (int i = tid; i < No * Lw; i += kThreads) s_ocr[i] = ocr_text[((int64_t)b * No + i / Lw) * ld_ocr + i % Lw];
  for (int i = tid; i < A; i += kThreads) { s_alen[i] = max(0, min(answer_len[(int64_t)b * A + i], La)); s_dead[i] = 0; }
  for (int i = tid; i < No; i += kThreads) { s_olen[i] = max(0, min(ocr_len[(int64_t)b * No + i], Lw)); s_omin[i] = kNone; }
  for (int i = tid; i < H; i += kThreads) { h_key[i] = -1; h_min[i] = kNone; h_min0[i] = kNone; h_s0[i] = 0u; h_scored[i] = 0; h_gid[i] = 0; }
  if (tid < 16) misc[tid] = tid == M_UNKPOS ? kNone : 0;
  __syncthreads();

  // ---- words and soft score of every answer (a thread per answer), vocabulary word of every OCR token (a thread per slot)
  for (int a = tid; a < A; a += kThreads) {
    const int* w = s_ans + a * La;
    const int n = s_alen[a];
    int nw = 0, start = -1;
    for (int i = 0; i <= n; ++i) {
      const bool sp = i == n || is_space(w[i]);
      if (!sp && start < 0) start = i;
      if (sp && start >= 0) {
        if (nw < kWordsPerAnswer) { s_wstart[a * kWordsPerAnswer + nw] = (unsigned char)start; s_wlen[a * kWordsPerAnswer + nw] = (unsigned char)(i - start); ++nw; }
        start = -1;
      }
    }
    s_nw[a] = nw;
    // answers.soft_scores: count = the answers equal to this one; per answer min(1, (count - (it is this one)) / 3), summed in order, / A
    auto same = [&](int o) {
      bool eq = s_alen[o] == n;
      const int* v = s_ans + o * La;
      for (int i = 0; eq && i < n; ++i) eq = v[i] == w[i];
      return eq;
    };
    int count = 0;
    for (int o = 0; o < A; ++o) count += same(o);
    double sum = 0.0;
    for (int o = 0; o < A; ++o) {
      const double x = (double)(count - (same(o) ? 1 : 0)) / 3.0;
      sum += x < 1.0 ? x : 1.0;
    }
    s_score[a] = (float)(sum / (double)A);
  }
  for (int o = tid; o < No; o += kThreads) s_tokv[o] = vocab_lookup(s_ocr + o * Lw, s_olen[o]);
  __syncthreads();

  // ---- matches of every word: a wave per word, an OCR slot per lane
  for (int a = 0; a < A; ++a) {
    const int nw = s_nw[a];
    for (int k = wv; k < nw; k += kWaves) {
      const int* w = s_ans + a * La + s_wstart[a * kWordsPerAnswer + k];
      const int n = s_wlen[a * kWordsPerAnswer + k];
      bool hit = lane < No && s_olen[lane < No ? lane : 0] == n;
      if (hit) {
        const int* t = s_ocr + lane * Lw;
        for (int i = 0; hit && i < n; ++i) hit = t[i] == w[i];
      }
      const unsigned long long mask = __ballot(hit);
      const int v = vocab_lookup(w, n);      // (the same probe in every lane: uniform)
      if (lane == 0) {
        const int cnt = (v >= 0) + __popcll(mask);
        s_wcnt[a * kWordsPerAnswer + k] = (unsigned char)cnt;
        if (cnt == 0) s_dead[a] = 1;
        if (k < L) { s_wv[a * L + k] = v; s_wmask[a * L + k] = mask; }
      }
    }
  }
  __syncthreads();

  // ---- sequences per answer: min(max_match, product of the match counts), none when a word matched nothing or there is no word
  for (int a = tid; a < A; a += kThreads) {
    const int nw = s_nw[a];
    long long prod = (nw == 0 || s_dead[a]) ? 0 : 1;
    for (int k = 0; k < nw && prod; ++k) prod = min(prod * (long long)s_wcnt[a * kWordsPerAnswer + k], (long long)max_match);
    s_nseq[a] = (int)prod;
  }
  __syncthreads();
  if (tid == 0) {
    int off = 0;
    for (int a = 0; a < A; ++a) { s_seqoff[a] = off; off += min(s_nseq[a], S - off); }      // (S >= A * max_match: the clamp never bites)
    s_seqoff[A] = off;
    misc[M_NSEQ] = off;
  }
  __syncthreads();
  const int n_seq = misc[M_NSEQ];

  // ---- the scanned values of every sequence: seq[t] for t < ln, EOS for ln <= t < dec, -1 behind
  for (int i = tid; i < n_seq; i += kThreads) {
    int a = 0;
    while (a + 1 < A && s_seqoff[a + 1] <= i) ++a;
    s_seqans[i] = (unsigned char)a;
    const int nw = s_nw[a];
    int r = i - s_seqoff[a];
    for (int k = nw - 1; k >= 0; --k) {
      const int cnt = s_wcnt[a * kWordsPerAnswer + k], d = r % cnt;
      r /= cnt;
      if (k < L) {
        const int v = s_wv[a * L + k];
        const unsigned long long m = s_wmask[a * L + k];
        s_seq[i * L + k] = v >= 0 ? (d == 0 ? v : V + nth_set_bit(m, d - 1)) : V + nth_set_bit(m, d);
      }
    }
    const int ln = min(nw, L), dec = min(1 + nw, L);
    for (int t = ln; t < L; ++t) s_seq[i * L + t] = t < dec ? eos : -1;
  }
  __syncthreads();

  // ---- every scanned value into the group table with its first scan position; what the host's two assertions need, independent of the table
  for (int p = tid; p < n_seq * L; p += kThreads) {
    const int val = s_seq[p];
    if (val < 0) continue;
    const int i = p / L, t = p - i * L;
    if (val == unk) { atomicMin(&misc[M_UNKPOS], p); if (t >= 1) misc[M_UNKSCORED] = 1; }
    if (val >= V) {
      const int o = min(val - V, No - 1);
      atomicMin(&s_omin[o], p);
      if (t >= 1) atomicOr((unsigned*)&misc[o < 32 ? M_OCRSCORED_LO : M_OCRSCORED_HI], 1u << (o & 31));
    }
    const int s = group_slot(h_key, H, val, true);
    if (s < 0) { misc[M_OVERFLOW] = 1; continue; }
    atomicMin(&h_min[s], p);
    if (t == 0) { atomicMin(&h_min0[s], i); atomicMax(&h_s0[s], __float_as_uint(s_score[s_seqans[i]])); }
    else h_scored[s] = 1;
  }
  __syncthreads();

  // ---- the host's assertions, the one it meets first (groups are walked in first-occurrence order): <pad> in a scored OCR slot, <unk> scored
  if (tid == 0) {
    int first = kNone, st = 0;
    if (misc[M_UNKSCORED]) { first = misc[M_UNKPOS]; st = ST_UNK_TARGET; }
    for (int o = 0; o < No; ++o) {
      const bool scored = ((unsigned)misc[o < 32 ? M_OCRSCORED_LO : M_OCRSCORED_HI] >> (o & 31)) & 1u;
      const int* t = s_ocr + o * Lw;
      if (scored && s_olen[o] == 5 && t[0] == '<' && t[1] == 'p' && t[2] == 'a' && t[3] == 'd' && t[4] == '>' && s_omin[o] < first) { first = s_omin[o]; st = ST_PAD_SLOT; }
    }
    if (!st && misc[M_OVERFLOW]) st = ST_GROUPS;
    misc[M_STATUS] = st;
  }
  __syncthreads();

  // ---- group ids = rank of the first position; step-0 order = rank of the first sequence
  if (!misc[M_STATUS]) {
    for (int s = tid; s < H; s += kThreads) {
      if (h_key[s] == -1) continue;
      const int mine = h_min[s], mine0 = h_min0[s];
      int gid = 0, r0 = 0;
      for (int o = 0; o < H; ++o) { gid += h_min[o] < mine; r0 += h_min0[o] < mine0; }
      h_gid[s] = gid;
      atomicAdd(&misc[M_NGRP], 1);
      if (gid < G) { g_key[gid] = h_key[s]; g_scored[gid] = h_scored[s]; }
      if (mine0 != kNone) {
        atomicAdd(&misc[M_N0], 1);
        if (r0 < G) { s0_idx[r0] = h_key[s]; s0_val[r0] = h_s0[s]; }
      }
    }
  }
  __syncthreads();
  if (tid == 0 && !misc[M_STATUS] && misc[M_NGRP] > G) misc[M_STATUS] = ST_GROUPS;
  __syncthreads();
  const int n_grp = misc[M_NGRP], n0 = misc[M_N0];

  // ---- target lists: a wave per group
  if (!misc[M_STATUS]) {
    for (int g = wv; g < n_grp; g += kWaves) {
      const int key = g_key[g];
      int cnt = 0, v = -1;
      unsigned long long mask = 0ull;
      if (g_scored[g]) {                                                                  // (uniform per wave)
        cnt = 1;
        if (key >= V) {
          v = s_tokv[min(key - V, No - 1)];
          if (v == unk) v = -1;
          cnt += v >= 0;
        } else {
          const int n = max(0, min(vocab_len[key], Lv));
          const int32_t* w = vocab_cp + (int64_t)key * ld_vocab;
          bool hit = lane < No && n > 0 && s_olen[lane < No ? lane : 0] == n;
          if (hit) {
            const int* t = s_ocr + lane * Lw;
            for (int i = 0; hit && i < n; ++i) hit = t[i] == w[i];
          }
          mask = __ballot(hit);
          cnt += __popcll(mask);
        }
      }
      if (lane == 0) { g_cnt[g] = cnt; g_v[g] = v; g_mask[g] = mask; }
    }
  }
  __syncthreads();
  if (tid == 0 && !misc[M_STATUS]) {
    int off = 0;
    for (int g = 0; g < n_grp; ++g) { g_off[g] = off; off += g_cnt[g]; }
    g_off[n_grp] = off;
    misc[M_NEXTRA] = off;
    if (off > E) misc[M_STATUS] = ST_EXTRA;
  }
  __syncthreads();

  // ---- outputs: every element once, zeros behind the sample's counts, all zeros for a flagged sample
  const int st = misc[M_STATUS];
  const bool ok = st == 0;
  const int ns = ok ? n_seq : 0, ng = ok ? n_grp : 0, nz = ok ? n0 : 0, ne = ok ? misc[M_NEXTRA] : 0;
  if (tid == 0) { meta[0] = ns; meta[1] = nz; meta[2] = ng; meta[3] = ne; status[b] = st; }
  int eos_gid = 0;
  if (ok && n_seq > 0) { const int s = group_slot(h_key, H, eos, false); eos_gid = s >= 0 ? h_gid[s] : 0; }
  for (int i = tid; i < S; i += kThreads) {
    seq_len[i] = i < ns ? min(s_nw[s_seqans[i]], L) : 0;
    step0_idx[i] = i < nz ? s0_idx[i] : 0;
    step0_val[i] = i < nz ? __uint_as_float(s0_val[i]) : 0.f;
  }
  for (int p = tid; p < S * L; p += kThreads) {
    int g = 0;
    if (p < ns * L) {
      const int val = s_seq[p];
      if (val < 0) g = eos_gid;
      else { const int s = group_slot(h_key, H, val, false); g = s >= 0 ? h_gid[s] : 0; }
    }
    seq_grp[p] = (int16_t)g;
  }
  for (int g = tid; g <= G; g += kThreads) {
    if (g < G) grp_idx[g] = g < ng ? g_key[g] : 0;
    grp_off[g] = (ok && g <= ng) ? g_off[g] : 0;
  }
  for (int e = ne + tid; e < E; e += kThreads) grp_extra[e] = 0;
  for (int g = tid; g < ng; g += kThreads) {
    if (!g_cnt[g]) continue;
    int e = g_off[g];
    grp_extra[e++] = g_key[g];
    if (g_v[g] >= 0) grp_extra[e++] = g_v[g];
    for (unsigned long long m = g_mask[g]; m; m &= m - 1) grp_extra[e++] = V + __ffsll((long long)m) - 1;
  }
}

}  // namespace

extern "C" int sam_answer_table_from_text(const int32_t* answer_text, int64_t ld_answer, const int32_t* answer_len, const int32_t* ocr_text, int64_t ld_ocr,
                                          const int32_t* ocr_len, const int32_t* vocab_cp, int64_t ld_vocab, const int32_t* vocab_len, const int32_t* slots, int B,
                                          int A, int La, int No, int Lw, int V, int Lv, int T, int unk, int eos, int S, int L, int G, int E, int max_match_num,
                                          int32_t* meta, int32_t* seq_len, int16_t* seq_grp, int32_t* step0_idx, float* step0_val, int32_t* grp_idx,
                                          int32_t* grp_off, int32_t* grp_extra, int32_t* status, void* stream) {
  SAM_REQUIRE(answer_text && answer_len && ocr_text && ocr_len, "sam_answer_table_from_text: null answer / OCR text pointer");
  if (const int rc = word_index_check("sam_answer_table_from_text", "ld_vocab", vocab_cp, ld_vocab, vocab_len, slots, Lv, kMaxWordChars, T)) return rc;
  SAM_REQUIRE(meta && seq_len && seq_grp && step0_idx && step0_val && grp_idx && grp_off && grp_extra && status, "sam_answer_table_from_text: null output pointer");
  SAM_REQUIRE(B >= 1 && A >= 1 && No >= 1, "sam_answer_table_from_text: bad shape B=%d A=%d No=%d", B, A, No);
  SAM_REQUIRE(La >= 1 && La <= kMaxAnswerChars, "sam_answer_table_from_text: La=%d outside 1..%d", La, kMaxAnswerChars);
  SAM_REQUIRE(Lw >= 1 && Lw <= kMaxWordChars, "sam_answer_table_from_text: Lw=%d outside 1..%d", Lw, kMaxWordChars);
  SAM_REQUIRE(V >= 1 && (int64_t)T >= 2 * (int64_t)V, "sam_answer_table_from_text: T=%d must be a power of two >= 2 V (V=%d)", T, V);
  SAM_REQUIRE(unk >= 0 && unk < V && eos >= 0 && eos < V && unk != eos, "sam_answer_table_from_text: unk=%d / eos=%d outside [0, %d) or equal", unk, eos, V);
  SAM_REQUIRE(L >= 1, "sam_answer_table_from_text: L=%d must be at least 1", L);
  SAM_REQUIRE(max_match_num >= 1, "sam_answer_table_from_text: max_match_num=%d must be at least 1", max_match_num);
  SAM_REQUIRE((int64_t)S >= (int64_t)A * max_match_num, "sam_answer_table_from_text: need S >= A * max_match_num (S=%d A=%d max_match_num=%d)", S, A, max_match_num);
  SAM_REQUIRE(G >= 1 && G <= 32767 && E >= 1, "sam_answer_table_from_text: need 1 <= G <= 32767 (int16 group ids) and E >= 1 (G=%d E=%d)", G, E);
  SAM_REQUIRE(ld_answer >= La && ld_ocr >= Lw, "sam_answer_table_from_text: need ld_answer >= La, ld_ocr >= Lw (%ld %ld)", (long)ld_answer, (long)ld_ocr);
  SAM_REQUIRE(((uintptr_t)answer_text | (uintptr_t)answer_len | (uintptr_t)ocr_text | (uintptr_t)ocr_len | (uintptr_t)meta | (uintptr_t)seq_len | (uintptr_t)step0_idx | (uintptr_t)step0_val | (uintptr_t)grp_idx | (uintptr_t)grp_off |
               (uintptr_t)grp_extra | (uintptr_t)status) % 4 == 0 && (uintptr_t)seq_grp % 2 == 0, "sam_answer_table_from_text: misaligned operand");
  if (A > 255 || No > 64) {
    sam_set_error("sam_answer_table_from_text: A=%d No=%d: at most 255 answers and 64 OCR slots (one slot per lane)", A, No);
    return SAM_ERR_UNSUPPORTED;
  }
  const int64_t rough = 12ll * A * L + 4ll * S * L + S;        // (in 64 bits first: the exact carve below counts in int)
  if (rough > 65536 || carve(A, La, No, Lw, S, L, G).total > 65536) {
    sam_set_error("sam_answer_table_from_text: A=%d La=%d No=%d Lw=%d S=%d L=%d G=%d need more than 64 KiB of LDS", A, La, No, Lw, S, L, G);
    return SAM_ERR_UNSUPPORTED;
  }
  const Carve c = carve(A, La, No, Lw, S, L, G);
  answer_table_from_text_kernel<<<dim3((unsigned)B), dim3(kThreads), (size_t)c.total, (hipStream_t)stream>>>(
      answer_text, ld_answer, answer_len, ocr_text, ld_ocr, ocr_len, vocab_cp, ld_vocab, vocab_len, slots, A, La, No, Lw, V, Lv, T, unk, eos, S, L, G, E, max_match_num,
      meta, seq_len, seq_grp, step0_idx, step0_val, grp_idx, grp_off, grp_extra, status);
  SAM_LAUNCH_CHECK();
  return SAM_OK;
}

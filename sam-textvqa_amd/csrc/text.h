// Shared device code of the text kernels (answer_text.hip, wordpiece.hip, fasttext.hip, textprep.hip, and through score_norm.h score.hip, score_text.hip and
// eval_beams.hip).  One copy each of
//   is_space           Python's str.isspace() set (wordindex.WHITESPACE; tests/test_answer_text_cpu.py reads the list below and enumerates all code points)
//   WordIndex          the exact-match word index a run keeps on the device (wordindex.build_slots): the words' code points and lengths, and an open-addressed
//                      table of word ids -- n_slots a power of two, -1 = empty, home slot text_hash & (n_slots - 1), linear probing
//   text_hash          FNV-1a over the code points as 32-bit units, then mix32 (wordindex.text_hash)
//   index_lookup       the probe, per lane (answer_text.hip)       (wordindex.lookup_host is the host twin of both)
//   index_lookup_wave  the probe, by a whole wave (fasttext.hip)
//                      (wordpiece.hip keeps the per-lane probe written out over its "##" prefix, on the constants below: it measured faster that way)
//   wave_emit          a wave-wide filter: ballot + popcount give each lane its output position
//   word_index_check   the entry points' argument checks of an index
// A unit that switches fp contraction off (fasttext.hip) includes this header above its pragma, like rowwise.h.
#pragma once
#include "common.h"

__device__ __forceinline__ bool is_space(int c) {
  return (c >= 0x09 && c <= 0x0D) || (c >= 0x1C && c <= 0x20) || c == 0x85 || c == 0xA0 || c == 0x1680 || (c >= 0x2000 && c <= 0x200A) || c == 0x2028 ||
         c == 0x2029 || c == 0x202F || c == 0x205F || c == 0x3000;
}

struct WordIndex {
  const int32_t* cp;      // [n_words, ld]: the words' code points
  int64_t ld;
  const int32_t* len;     // [n_words]: code points per word (a word without an entry: -1)
  const int32_t* slots;   // [n_slots]: word ids
  int n_words, n_slots;
};

constexpr unsigned kTextHashBasis = 0x811C9DC5u, kTextHashPrime = 0x01000193u;      // FNV-1a, 32 bit

// at(i) -> code point i of the query, for i in [0, n)
template <class At>
__device__ __forceinline__ unsigned text_hash(int n, At at) {
  unsigned h = kTextHashBasis;
  for (int i = 0; i < n; ++i) h = (h ^ (unsigned)at(i)) * kTextHashPrime;
  return mix32(h);
}

// the id of the word with exactly the n code points at(0) .. at(n - 1), or -1: linear probing from the home slot, every candidate compared in full.  Ends at
// an empty slot, at a slot value outside [0, n_words), and after n_slots steps.  The caller rules out the lengths no word has (n <= 0, n > Lv).
template <class At>
__device__ int index_lookup(const WordIndex& ix, int n, At at) {
  const unsigned mask = (unsigned)(ix.n_slots - 1);
  unsigned s = text_hash(n, at) & mask;
  for (int it = 0; it < ix.n_slots; ++it) {
    const int wi = ix.slots[s];
    if (wi < 0 || wi >= ix.n_words) return -1;
    if (ix.len[wi] == n) {
      const int32_t* c = ix.cp + (int64_t)wi * ix.ld;
      int i = 0;
      while (i < n && (unsigned)c[i] == (unsigned)at(i)) ++i;
      if (i == n) return wi;
    }
    s = (s + 1) & mask;
  }
  return -1;
}

// the same probe by a whole wave, n <= 64 and wave-uniform: every lane hashes, a candidate is compared one code point per lane, a ballot decides.  The walk
// and the result are wave-uniform.
template <class At>
__device__ __forceinline__ int index_lookup_wave(const WordIndex& ix, int n, int lane, At at) {
  const unsigned mask = (unsigned)(ix.n_slots - 1);
  unsigned s = text_hash(n, at) & mask;
  for (int it = 0; it < ix.n_slots; ++it) {
    const int wi = ix.slots[s];
    if (wi < 0 || wi >= ix.n_words) return -1;
    if (ix.len[wi] == n) {
      const bool differs = lane < n && (unsigned)ix.cp[(int64_t)wi * ix.ld + lane] != (unsigned)at(lane);
      if (__ballot(differs) == 0ull) return wi;
    }
    s = (s + 1) & mask;
  }
  return -1;
}

// A wave-wide filter over src[0, n): f(i, v0, v1) -> how many values (0, 1 or 2) position i emits; they land in dst in order.  n is wave-uniform.
template <class F>
__device__ __forceinline__ int wave_emit(int n, int* dst, int lane, F f) {
  int out = 0;
  const unsigned long long lt = (1ull << lane) - 1ull;
  for (int base = 0; base < n; base += 64) {
    const int i = base + lane;
    int v0 = 0, v1 = 0, cnt = 0;
    if (i < n) cnt = f(i, v0, v1);
    const unsigned long long m1 = __ballot(cnt >= 1), m2 = __ballot(cnt == 2);
    const int pos = out + __popcll(m1 & lt) + __popcll(m2 & lt);
    if (cnt >= 1) dst[pos] = v0;
    if (cnt == 2) dst[pos + 1] = v1;
    out += __popcll(m1) + __popcll(m2);
  }
  __builtin_amdgcn_wave_barrier();
  return out;
}

// The argument checks of an index, once for the entry points that take one: `who` heads the message, ld_name is the public header's name of the row stride.
// (Host code; not under a host-only guard, because the device pass parses the entry points that call it.)
inline int word_index_check(const char* who, const char* ld_name, const int32_t* cp, int64_t ld, const int32_t* len, const int32_t* slots, int Lv, int max_Lv,
                            int n_slots) {
  SAM_REQUIRE(cp && len && slots, "%s: null vocabulary index pointer", who);
  SAM_REQUIRE(Lv >= 1 && Lv <= max_Lv, "%s: Lv=%d outside 1..%d", who, Lv, max_Lv);
  SAM_REQUIRE(ld >= Lv, "%s: need %s >= Lv (%s=%ld Lv=%d)", who, ld_name, ld_name, (long)ld, Lv);
  SAM_REQUIRE(n_slots >= 2 && (n_slots & (n_slots - 1)) == 0, "%s: n_slots=%d must be a power of two", who, n_slots);
  SAM_REQUIRE(((uintptr_t)cp | (uintptr_t)len | (uintptr_t)slots) % 4 == 0, "%s: misaligned index operand", who);
  return SAM_OK;
}

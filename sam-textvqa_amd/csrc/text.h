// Shared device code of the text kernels (answer_text.hip, wordpiece.hip, fasttext.hip, textprep.hip, unicode_text.hip, and through score_norm.h score.hip, score_text.hip and
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
//   utf8_decode_lane   one lane's byte of a strict UTF-8 stream (textprep.hip, unicode_text.hip)
//   UniTable           the Unicode character table a run keeps on the device (unicode_table.py), uni_lookup / uni_pool its two reads, uni_table_check
//   sigma_decide       str.lower()'s final-sigma rule inside a chunk; SigmaCarry its state across chunks
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

// One lane's byte of a UTF-8 stream whose slot ends at hi (textprep.hip, unicode_text.hip): a lane holding a lead byte reads its own 1..3 continuation
// bytes, below hi only, and checks Python's strict ranges.  cp: the code point of an ASCII or lead byte, -1 otherwise; tail: the continuation bytes a lead
// asked for; cont: a continuation byte (it yields nothing and is legal iff some lead claims it: the caller compares the two counts at the slot's end);
// bad: exactly where bytes.decode("utf-8") raises at this byte.  p >= hi: nothing.
__device__ __forceinline__ void utf8_decode_lane(const uint8_t* __restrict__ raw, int64_t p, int64_t hi, int& cp, int& tail, bool& bad, bool& cont) {
  cp = -1;
  tail = 0;
  bad = cont = false;
  if (p >= hi) return;
  const unsigned b0 = raw[p];
  if (b0 < 0x80u) {
    cp = (int)b0;
  } else if (b0 < 0xC0u) {
    cont = true;
  } else if (b0 < 0xC2u || b0 > 0xF4u) {
    bad = true;                                    // C0 C1: overlong two-byte forms; F5..FF: above U+10FFFF
  } else {
    tail = b0 < 0xE0u ? 1 : (b0 < 0xF0u ? 2 : 3);
    if (p + tail >= hi) {
      bad = true;                                  // the slot ends inside the sequence
    } else {
      const unsigned b1 = raw[p + 1];
      const unsigned lo1 = b0 == 0xE0u ? 0xA0u : (b0 == 0xF0u ? 0x90u : 0x80u);      // overlong three- and four-byte forms
      const unsigned hi1 = b0 == 0xEDu ? 0x9Fu : (b0 == 0xF4u ? 0x8Fu : 0xBFu);      // surrogates; above U+10FFFF
      bad = b1 < lo1 || b1 > hi1;
      unsigned v = (tail == 1 ? (b0 & 0x1Fu) : (tail == 2 ? (b0 & 0x0Fu) : (b0 & 0x07u))) << 6 | (b1 & 0x3Fu);
      if (tail >= 2) {
        const unsigned b2 = raw[p + 2];
        bad = bad || (b2 & 0xC0u) != 0x80u;
        v = v << 6 | (b2 & 0x3Fu);
      }
      if (tail == 3) {
        const unsigned b3 = raw[p + 3];
        bad = bad || (b3 & 0xC0u) != 0x80u;
        v = v << 6 | (b3 & 0x3Fu);
      }
      cp = (int)v;
    }
  }
}

// The Unicode character table a run keeps on the device (unicode_table.py states the layout): block[cp >> 7] names a block of 128 records, a record is
// two words -- word 0: x (lower = cp ^ x, or a pool offset) and the flags below; word 1: the question composite (n << 21 | x or pool offset, bit 30 =
// PUNCT_FLAG of a single result).
struct UniTable {
  const int32_t* block;   // [kUniStage1]
  const int2* rec;        // [n_blocks * 128]
  const int32_t* pool;    // [n_pool]
  int n_blocks, n_pool;
};

constexpr int kUniStage1 = 0x110000 >> 7, kUniCpMask = (1 << 21) - 1;
enum { kUniDrop = 1 << 21, kUniSep = 1 << 22, kUniCjk = 1 << 23, kUniPunct = 1 << 24, kUniSigmaC = 1 << 25, kUniSigmaI = 1 << 26, kUniHost = 1 << 27,
       kUniLowerPool = 1 << 28, kUniHangul = 1 << 29, kPunctFlag = 1 << 30 };
constexpr int kSigma = 0x3A3, kSmallSigma = 0x3C3, kFinalSigma = 0x3C2;

// the record of cp in [0, 0x110000).  A block number outside the table reads block 0: a broken table gives wrong text, never a read outside it.
__device__ __forceinline__ int2 uni_lookup(const UniTable& t, int cp) {
  int b = t.block[cp >> 7];
  if ((unsigned)b >= (unsigned)t.n_blocks) b = 0;
  return t.rec[(b << 7) | (cp & 127)];
}

// n <= 3 pool entries at offset o, or none when they would lie outside the pool
__device__ __forceinline__ int uni_pool(const UniTable& t, int o, int n, int& v0, int& v1, int& v2) {
  if (o < 0 || o + n > t.n_pool) return 0;
  v0 = t.pool[o];
  v1 = t.pool[o + 1];
  v2 = n == 3 ? t.pool[o + 2] : 0;
  return n;
}

// str.lower()'s final-sigma rule inside one chunk, for the lane that holds U+03A3.  stop: ballot of the lanes whose character ends a run of
// case-ignorable ones (a character outside class I, or a word boundary); cased: those of them that are of class C; prev_cased: what the last such
// character of the earlier chunks was.  -> 0 small sigma, 1 final sigma, 2 undecided: nothing behind it in this chunk ends the run.
__device__ __forceinline__ int sigma_decide(int lane, unsigned long long stop, unsigned long long cased, bool prev_cased) {
  const unsigned long long below = (1ull << lane) - 1ull;
  const unsigned long long before = stop & below, after = stop & ~below & ~(1ull << lane);
  const bool pc = before ? ((cased >> (63 - __clzll((long long)before))) & 1ull) != 0 : prev_cased;
  if (!pc) return 0;
  if (!after) return 2;
  return ((cased >> (__ffsll((long long)after) - 1)) & 1ull) ? 0 : 1;
}

// The state of that rule across chunks, wave-uniform: prev_cased, and at most one undecided sigma with the position of its output (any later sigma is
// itself of class C and decides the earlier one).  begin() settles a carried sigma at the chunk's first stop; carry() keeps the class of the chunk's
// last stop (call it after the lanes' sigma_decide); hold() takes over the chunk's own undecided sigma (undecided: the lane's sigma_decide gave 2;
// out_pos: where its code point went); finish() at the slot's end: nothing followed, so it is final.  dst[0, cap) is the row in LDS.
struct SigmaCarry {
  bool prev_cased = false, pend = false;
  int pos = 0;
  __device__ __forceinline__ void begin(int lane, unsigned long long stop, unsigned long long cased, int* dst, int cap) {
    if (pend && stop) {
      if (!((cased >> (__ffsll((long long)stop) - 1)) & 1ull) && lane == 0 && pos < cap) dst[pos] = kFinalSigma;
      pend = false;
    }
  }
  __device__ __forceinline__ void hold(bool undecided, int64_t out_pos, int cap) {
    const unsigned long long pm = __ballot(undecided);
    if (pm) {
      pend = true;
      pos = __shfl((int)(out_pos < cap ? out_pos : cap), __ffsll((long long)pm) - 1);
    }
  }
  __device__ __forceinline__ void carry(unsigned long long stop, unsigned long long cased) {
    if (stop) prev_cased = ((cased >> (63 - __clzll((long long)stop))) & 1ull) != 0;
  }
  __device__ __forceinline__ void finish(int lane, int* dst, int cap) {
    if (pend && lane == 0 && pos < cap) dst[pos] = kFinalSigma;
    pend = false;
  }
};

// The argument checks of a table, once for the entry points that take one.
inline int uni_table_check(const char* who, const int32_t* block, int n_stage1, const int32_t* rec, int n_blocks, const int32_t* pool, int n_pool) {
  SAM_REQUIRE(block && rec && pool, "%s: null table pointer", who);
  SAM_REQUIRE(n_stage1 == kUniStage1, "%s: uni_n_stage1=%d must be %d (one entry per 128 code points)", who, n_stage1, kUniStage1);
  SAM_REQUIRE(n_blocks >= 1 && n_blocks <= (1 << 14) && n_pool >= 1 && n_pool <= kUniCpMask, "%s: uni_n_blocks=%d / uni_n_pool=%d out of range", who, n_blocks, n_pool);
  SAM_REQUIRE(((uintptr_t)block | (uintptr_t)pool) % 4 == 0 && (uintptr_t)rec % 8 == 0, "%s: misaligned table operand", who);
  return SAM_OK;
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

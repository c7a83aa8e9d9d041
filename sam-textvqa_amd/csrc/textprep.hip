// The batch's raw strings to cleaned, zero-padded code points on the device (gfx950): what Processors.word_cleaner / word_cleaner_lower
// (sam/datasets/processors.py:746-755) and the [ord(c) for c in t] loops of phoc.pack_ocr_text / answers.pack_answer_text do on the host per string.
//   text_from_utf8_kernel   one wave per slot.  The wave walks the slot's bytes 64 at a time, one byte per lane:
//     decode    a lane holding a lead byte reads its own 1..3 continuation bytes (below the slot's end only: a sequence the slot's end cuts is an error,
//               the neighbour's bytes are never read) and checks Python's strict ranges.  A continuation byte yields nothing; it is legal iff some lead
//               claims it.  Valid leads claim disjoint bytes, all of them continuations, so "every continuation byte is claimed" is one comparison of two
//               counts at the end of the slot: the continuation bytes seen against the bytes the leads asked for.
//     clean     lower ASCII, drop ',' and '?' (lane-local); the possessive looks at the NEXT kept code point, found with a ballot of the kept lanes; an
//               apostrophe that is the chunk's last kept code point is held back (pend) and emitted, with or without its blank, in front of the next
//               chunk's first kept code point or at the slot's end; strip drops everything in front of the first non-space element (leading) and
//               remembers where the last non-space element ended (len_ns): trailing blanks are written but never counted.
//     compact   a lane emits 0, 1 or 2 elements (" '" is two); its position is the prefix popcount of two ballots.
//     lower     sam_text_from_utf8_unicode: bit 1 of mode is str.lower() of the whole slot, read from the resident table in front of
//               the clean step -- a lane may now emit two code points for one (U+0130), and U+03A3 follows the final-sigma rule (text.h: sigma_decide
//               inside a chunk, SigmaCarry across chunks: two more flags and one output position).
//   State across chunks, all wave-uniform: pend, leading, pos, len_ns, the two byte counts.  The row is assembled in LDS and written once at the end,
//   zeros behind the length, or all zeros for a flagged slot.  One wave per workgroup: the barrier in front of the read-out is the wave's own.
#include "common.h"
#include "text.h"
#include "sam_hip_textprep.h"
#include "sam_hip_unicode.h"

namespace {

constexpr int kMaxL = 128;
enum { kLower = 1, kDelete = 2, kPossessive = 4, kStrip = 8 };
enum { kBadUtf8 = 1, kTooLong = 2, kBadOffsets = 4 };

// kUni: bit 1 of mode is str.lower() of the whole slot, read from the table ut (sam_text_from_utf8_unicode); otherwise 'A'..'Z' only and ut is unread
template <bool kUni>
__global__ __launch_bounds__(64) void text_from_utf8_kernel(const uint8_t* __restrict__ raw, int64_t nbytes, const int32_t* __restrict__ raw_off, int L, int mode,
                                                            UniTable ut, int32_t* __restrict__ text, int32_t* __restrict__ text_len, int32_t* __restrict__ status) {
  __shared__ int s_out[kMaxL];
  const int lane = threadIdx.x;
  const int64_t s = blockIdx.x;
  const int64_t lo = raw_off[s], hi = raw_off[s + 1];
  const unsigned long long below = (1ull << lane) - 1ull;
  int st = 0;
  int64_t pos = 0, len_ns = 0;                     // elements emitted behind the leading blanks; where the last non-space one ended
  if (lo < 0 || hi < lo || hi > nbytes) {
    st = kBadOffsets;
  } else {
    bool leading = (mode & kStrip) != 0, pend = false;
    int64_t n_cont = 0, n_claimed = 0;
    SigmaCarry sigma;
    // one element from the whole wave (the held-back apostrophe and its blank)
    auto emit_uniform = [&](int ch, bool space) {
      if (space && leading) return;
      if (!space) leading = false;
      if (lane == 0 && pos < L) s_out[pos] = ch;
      ++pos;
      if (!space) len_ns = pos;
    };
    for (int64_t base = lo; base < hi; base += 64) {
      const int64_t p = base + lane;
      int cp, tail;
      bool bad, cont;
      utf8_decode_lane(raw, p, hi, cp, tail, bad, cont);
      if (__ballot(bad)) {
        st = kBadUtf8;
        break;
      }
      n_cont += __popcll(__ballot(cont));
      n_claimed += __popcll(__ballot(tail >= 1)) + __popcll(__ballot(tail >= 2)) + __popcll(__ballot(tail == 3));
      int second = -1;                             // the second code point of a lowering that has two (U+0130)
      bool undecided = false;                      // this lane's sigma waits for a later chunk
      if constexpr (kUni) {
        if (mode & kLower) {
          const int w = cp >= 0 ? uni_lookup(ut, cp).x : 0;
          const unsigned long long stop = __ballot(cp >= 0 && !(w & kUniSigmaI)), cased = __ballot(cp >= 0 && !(w & kUniSigmaI) && (w & kUniSigmaC));
          sigma.begin(lane, stop, cased, s_out, L);
          if (cp == kSigma) {
            const int d = sigma_decide(lane, stop, cased, sigma.prev_cased);
            undecided = d == 2;
            cp = d == 1 ? kFinalSigma : kSmallSigma;
          } else if (w & kUniLowerPool) {
            int v0 = cp, v1 = -1, v2;
            if (uni_pool(ut, w & kUniCpMask, 2, v0, v1, v2)) {
              cp = v0;
              second = v1;
            }
          } else if (cp >= 0) {
            cp ^= w & kUniCpMask;
          }
          sigma.carry(stop, cased);
        }
      } else {
        if ((mode & kLower) && cp >= 'A' && cp <= 'Z') cp += 'a' - 'A';
      }
      const bool keep = cp >= 0 && !((mode & kDelete) && (cp == ',' || cp == '?'));
      const unsigned long long km = __ballot(keep);
      if (km == 0) continue;                       // nothing left of this chunk: a held-back apostrophe waits on
      const unsigned long long sm = __ballot(keep && cp == 's');
      if (pend) {
        const int first = __ffsll((long long)km) - 1;
        if ((sm >> first) & 1ull) emit_uniform(' ', true);
        emit_uniform('\'', false);
        pend = false;
      }
      int c = keep ? (second >= 0 ? 2 : 1) : 0;    // elements of this lane: 2 is the blank and the apostrophe, or a lowering of two code points
      if (mode & kPossessive) {
        const bool apos = keep && cp == '\'';
        const unsigned long long above = (km & ~below) & ~(1ull << lane);
        if (apos && above == 0) c = 0;             // the chunk's last kept code point: held back
        if (apos && above != 0 && ((sm >> (__ffsll((long long)above) - 1)) & 1ull)) c = 2;
        pend = __ballot(apos && above == 0) != 0;
      }
      bool nonspace = c == 2 || (c == 1 && !is_space(cp));
      if (leading) {
        const unsigned long long nm = __ballot(nonspace);
        if (nm == 0) {
          c = 0;
        } else {
          const int f = __ffsll((long long)nm) - 1;
          if (lane < f) c = 0;
          if (lane == f && c == 2 && second < 0) c = 1;      // its blank is a leading one
          leading = false;
        }
      }
      nonspace = nonspace && c > 0;
      // (inline, not wave_emit of text.h: the positions are cut at L, and pos / len_ns / leading carry over from chunk to chunk and to emit_uniform)
      const unsigned long long m1 = __ballot(c >= 1), m2 = __ballot(c == 2);
      const int64_t q = pos + __popcll(m1 & below) + __popcll(m2 & below);
      if (c == 2) {
        if (q < L) s_out[q] = second >= 0 ? cp : ' ';
        if (q + 1 < L) s_out[q + 1] = second >= 0 ? second : cp;
      } else if (c == 1) {
        if (q < L) s_out[q] = cp;
      }
      const unsigned long long nsm = __ballot(nonspace);
      if (nsm) {
        const int j = 63 - __clzll((long long)nsm);
        const unsigned long long upto = j == 63 ? ~0ull : ((1ull << (j + 1)) - 1ull);
        len_ns = pos + __popcll(m1 & upto) + __popcll(m2 & upto);
      }
      if constexpr (kUni) sigma.hold(undecided, q, L);
      pos += __popcll(m1) + __popcll(m2);
    }
    if (st == 0) {
      if constexpr (kUni) sigma.finish(lane, s_out, L);
      if (pend) emit_uniform('\'', false);
      if (n_cont != n_claimed) st = kBadUtf8;      // a continuation byte no lead asked for
    }
  }
  const int64_t len = (mode & kStrip) ? len_ns : pos;
  if (st == 0 && len > L) st = kTooLong;
  __syncthreads();
  for (int i = lane; i < L; i += 64) text[s * L + i] = (st == 0 && i < len) ? s_out[i] : 0;
  if (lane == 0) {
    text_len[s] = st == 0 ? (int32_t)len : 0;
    status[s] = st;
  }
}

// both entry points: the operand checks, then (kUni) the table's, then the launch
template <bool kUni>
int text_from_utf8_launch(const char* who, const uint8_t* raw, int64_t nbytes, const int32_t* raw_off, int S, int L, int mode, const int32_t* uni_block,
                          int uni_n_stage1, const int32_t* uni_rec, int uni_n_blocks, const int32_t* uni_pool, int uni_n_pool, int32_t* text, int32_t* text_len,
                          int32_t* status, void* stream) {
  SAM_REQUIRE(raw_off && text && text_len && status, "%s: null raw_off / text / text_len / status", who);
  SAM_REQUIRE(nbytes >= 0 && nbytes <= 0x7fffffffLL, "%s: nbytes=%lld must be in [0, 2^31)", who, (long long)nbytes);
  SAM_REQUIRE(raw || nbytes == 0, "%s: null raw with nbytes=%lld", who, (long long)nbytes);
  SAM_REQUIRE(S >= 1, "%s: S=%d slots", who, S);
  SAM_REQUIRE(L >= 1 && L <= kMaxL, "%s: L=%d must be in [1, %d]", who, L, kMaxL);
  SAM_REQUIRE(mode >= 0 && mode <= 15, "%s: mode=%d is not a set of the bits 1, 2, 4, 8", who, mode);
  SAM_REQUIRE(((uintptr_t)raw_off % 4) == 0 && ((uintptr_t)text % 4) == 0 && ((uintptr_t)text_len % 4) == 0 && ((uintptr_t)status % 4) == 0,
              "%s: misaligned raw_off / text / text_len / status", who);
  UniTable ut{};
  if constexpr (kUni) {
    if (int rc = uni_table_check(who, uni_block, uni_n_stage1, uni_rec, uni_n_blocks, uni_pool, uni_n_pool)) return rc;
    ut = UniTable{uni_block, (const int2*)uni_rec, uni_pool, uni_n_blocks, uni_n_pool};
  }
  text_from_utf8_kernel<kUni><<<dim3((unsigned)S), dim3(64), 0, (hipStream_t)stream>>>(raw, nbytes, raw_off, L, mode, ut, text, text_len, status);
  SAM_LAUNCH_CHECK();
  return SAM_OK;
}

}  // namespace

extern "C" int sam_text_from_utf8(const uint8_t* raw, int64_t nbytes, const int32_t* raw_off, int S, int L, int mode, int32_t* text, int32_t* text_len,
                                  int32_t* status, void* stream) {
  return text_from_utf8_launch<false>("sam_text_from_utf8", raw, nbytes, raw_off, S, L, mode, nullptr, 0, nullptr, 0, nullptr, 0, text, text_len, status, stream);
}

extern "C" int sam_text_from_utf8_unicode(const uint8_t* raw, int64_t nbytes, const int32_t* raw_off, int S, int L, int mode, const int32_t* uni_block,
                                          int uni_n_stage1, const int32_t* uni_rec, int uni_n_blocks, const int32_t* uni_pool, int uni_n_pool, int32_t* text,
                                          int32_t* text_len, int32_t* status, void* stream) {
  return text_from_utf8_launch<true>("sam_text_from_utf8_unicode", raw, nbytes, raw_off, S, L, mode, uni_block, uni_n_stage1, uni_rec, uni_n_blocks, uni_pool, uni_n_pool,
                                     text, text_len, status, stream);
}

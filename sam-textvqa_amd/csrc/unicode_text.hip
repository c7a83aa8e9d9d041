// The questions' raw strings to the packed text the WordPiece kernel reads (gfx950): what wordpiece.pack_question_text does on the host
// per character -- BasicTokenizer's table-driven steps for a question that is not ASCII -- from a Unicode character table resident on the device
// (text.h: UniTable; unicode_table.py builds it and normalize_host is this kernel's twin).
//   question_from_utf8_kernel   one wave per question, two walks over the slot's bytes, 64 at a time, one byte per lane (text.h: utf8_decode_lane):
//     scan        strict UTF-8 (as textprep.hip: the continuation bytes seen against the bytes the leads asked for), whether any byte is not ASCII, and
//                 whether a special-token string starts at a '[' (the lane reads its own next 4..5 bytes, below the slot's end only).
//     ASCII       the bytes are the code points: copied verbatim.
//     normalise   per character the record of the table: dropped characters vanish; a separator or a CJK ideograph is a word boundary; every other
//                 character emits its composite (0..3 code points: table, pool or Hangul arithmetic), U+03A3 by the final-sigma rule inside its word
//                 (text.h: sigma_decide, SigmaCarry; a boundary ends the context).  A lane that emits puts a blank in front when something was emitted
//                 before and a boundary lies between the previous emitting character and its own: so words that become empty leave no blank behind.
//                 A lane emits 0..4 elements; its position is the prefix popcount of the three ballots of the count's bits.
//   State across chunks, all wave-uniform: pos, brk (a boundary since the last emitted code point), the sigma carry, the two byte counts.  The row is
//   assembled in LDS and written once at the end, zeros behind the length, or all zeros for a flagged slot.  One wave per workgroup.
#include "common.h"
#include "text.h"
#include "sam_hip_unicode.h"

namespace {

constexpr int kMaxLq = 1024;
enum { kBadUtf8 = 1, kTooLong = 2, kBadOffsets = 4, kSpecial = 8, kNeedsHost = 16 };

// whether [PAD] [UNK] [CLS] [SEP] or [MASK] starts at raw[p] == '[' and ends below hi
__device__ __forceinline__ bool special_at(const uint8_t* __restrict__ raw, int64_t p, int64_t hi) {
  if (p + 5 > hi) return false;
  const unsigned a = raw[p + 1], b = raw[p + 2], c = raw[p + 3], d = raw[p + 4];
  if (d == ']') return (a == 'P' && b == 'A' && c == 'D') || (a == 'U' && b == 'N' && c == 'K') || (a == 'C' && b == 'L' && c == 'S') || (a == 'S' && b == 'E' && c == 'P');
  return a == 'M' && b == 'A' && c == 'S' && d == 'K' && p + 6 <= hi && raw[p + 5] == ']';
}

__global__ __launch_bounds__(64) void question_from_utf8_kernel(const uint8_t* __restrict__ raw, int64_t nbytes, const int32_t* __restrict__ raw_off, int Lq, UniTable ut,
                                                                int32_t* __restrict__ text, int32_t* __restrict__ text_len, int32_t* __restrict__ status) {
  __shared__ int s_out[kMaxLq];
  const int lane = threadIdx.x;
  const int64_t b = blockIdx.x;
  const int64_t lo = raw_off[b], hi = raw_off[b + 1];
  const unsigned long long below = (1ull << lane) - 1ull, upto = below | (1ull << lane);
  int st = 0;
  int64_t pos = 0;
  if (lo < 0 || hi < lo || hi > nbytes) {
    st = kBadOffsets;
  } else {
    bool non_ascii = false, special = false;
    int64_t n_cont = 0, n_claimed = 0;
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
      non_ascii = non_ascii || __ballot(cont || tail > 0) != 0;
      special = special || __ballot(cp == '[' && special_at(raw, p, hi)) != 0;
    }
    if (st == 0 && n_cont != n_claimed) st = kBadUtf8;
    if (st == 0 && special) st = kSpecial;
    if (st == 0 && !non_ascii) {
      if (hi - lo > Lq) {
        st = kTooLong;
      } else {
        pos = hi - lo;
        for (int i = lane; i < (int)pos; i += 64) s_out[i] = raw[lo + i];
      }
    } else if (st == 0) {
      bool brk = false;
      SigmaCarry sigma;
      for (int64_t base = lo; base < hi; base += 64) {
        const int64_t p = base + lane;
        int cp, tail;
        bool bad, cont;
        utf8_decode_lane(raw, p, hi, cp, tail, bad, cont);                 // (valid: the scan went through)
        const bool valid = cp >= 0 && cp < 0x110000;
        const int2 r = valid ? uni_lookup(ut, cp) : make_int2(0, 0);
        if (__ballot(valid && (r.x & kUniHost))) {
          st = kNeedsHost;
          break;
        }
        const bool present = valid && !(r.x & kUniDrop);
        const bool bound = present && (r.x & (kUniSep | kUniCjk));
        const unsigned long long stop = __ballot(present && (bound || !(r.x & kUniSigmaI)));
        const unsigned long long cased = __ballot(present && !bound && !(r.x & kUniSigmaI) && (r.x & kUniSigmaC));
        sigma.begin(lane, stop, cased, s_out, Lq);
        int n = 0, v0 = 0, v1 = 0, v2 = 0;
        bool undecided = false;
        if (present && !(r.x & kUniSep)) {
          if (cp == kSigma) {
            const int d = sigma_decide(lane, stop, cased, sigma.prev_cased);
            undecided = d == 2;
            n = 1;
            v0 = d == 1 ? kFinalSigma : kSmallSigma;
          } else if (r.x & kUniHangul) {
            const int s = cp - 0xAC00;
            n = s % 28 ? 3 : 2;
            v0 = 0x1100 + s / 588;
            v1 = 0x1161 + s % 588 / 28;
            v2 = 0x11A7 + s % 28;
          } else {
            n = (r.y >> 21) & 3;
            if (n == 1) v0 = (cp ^ (r.y & kUniCpMask)) | (r.y & kPunctFlag);
            if (n >= 2) n = uni_pool(ut, r.y & kUniCpMask, n, v0, v1, v2);
          }
        }
        sigma.carry(stop, cased);
        const unsigned long long em = __ballot(n > 0), bm = __ballot(bound);
        bool blank = false;
        if (n > 0) {
          const unsigned long long prev = em & below;
          if (prev) {
            const int j = 63 - __clzll((long long)prev);
            blank = (bm & upto & ~((1ull << j) - 1ull)) != 0;                 // a boundary from the previous emitting lane (a CJK one counts) up to this one
          } else {
            blank = pos > 0 && (brk || (bm & upto) != 0);
          }
        }
        const int cnt = n + (blank ? 1 : 0);
        const unsigned long long m1 = __ballot(cnt & 1), m2 = __ballot(cnt & 2), m4 = __ballot(cnt & 4);
        int64_t q = pos + __popcll(m1 & below) + 2 * __popcll(m2 & below) + 4 * __popcll(m4 & below);
        if (blank) {
          if (q < Lq) s_out[q] = ' ';
          ++q;
        }
        if (n >= 1 && q < Lq) s_out[q] = v0;
        if (n >= 2 && q + 1 < Lq) s_out[q + 1] = v1;
        if (n == 3 && q + 2 < Lq) s_out[q + 2] = v2;
        sigma.hold(undecided, q, Lq);
        if (em) {
          brk = (bm >> (63 - __clzll((long long)em))) != 0;                    // the last emitting lane itself (CJK) or anything behind it
        } else {
          brk = brk || bm != 0;
        }
        pos += __popcll(m1) + 2 * __popcll(m2) + 4 * __popcll(m4);
      }
      if (st == 0) sigma.finish(lane, s_out, Lq);
      if (st == 0 && pos > Lq) st = kTooLong;
    }
  }
  __syncthreads();
  for (int i = lane; i < Lq; i += 64) text[b * Lq + i] = (st == 0 && i < pos) ? s_out[i] : 0;
  if (lane == 0) {
    text_len[b] = st == 0 ? (int32_t)pos : 0;
    status[b] = st;
  }
}

}  // namespace

extern "C" int sam_question_from_utf8(const uint8_t* raw, int64_t nbytes, const int32_t* raw_off, int B, int Lq, const int32_t* uni_block, int uni_n_stage1,
                                      const int32_t* uni_rec, int uni_n_blocks, const int32_t* uni_pool, int uni_n_pool, int32_t* question_text,
                                      int32_t* question_text_len, int32_t* status, void* stream) {
  SAM_REQUIRE(raw_off && question_text && question_text_len && status, "sam_question_from_utf8: null raw_off / question_text / question_text_len / status");
  SAM_REQUIRE(nbytes >= 0 && nbytes <= 0x7fffffffLL, "sam_question_from_utf8: nbytes=%lld must be in [0, 2^31)", (long long)nbytes);
  SAM_REQUIRE(raw || nbytes == 0, "sam_question_from_utf8: null raw with nbytes=%lld", (long long)nbytes);
  SAM_REQUIRE(B >= 1, "sam_question_from_utf8: B=%d questions", B);
  SAM_REQUIRE(Lq >= 1 && Lq <= kMaxLq, "sam_question_from_utf8: Lq=%d must be in [1, %d]", Lq, kMaxLq);
  SAM_REQUIRE(((uintptr_t)raw_off % 4) == 0 && ((uintptr_t)question_text % 4) == 0 && ((uintptr_t)question_text_len % 4) == 0 && ((uintptr_t)status % 4) == 0,
              "sam_question_from_utf8: misaligned raw_off / question_text / question_text_len / status");
  if (int rc = uni_table_check("sam_question_from_utf8", uni_block, uni_n_stage1, uni_rec, uni_n_blocks, uni_pool, uni_n_pool)) return rc;
  const UniTable ut{uni_block, (const int2*)uni_rec, uni_pool, uni_n_blocks, uni_n_pool};
  question_from_utf8_kernel<<<dim3((unsigned)B), dim3(64), 0, (hipStream_t)stream>>>(raw, nbytes, raw_off, Lq, ut, question_text, question_text_len, status);
  SAM_LAUNCH_CHECK();
  return SAM_OK;
}

// PHOC of the OCR tokens straight from their text (gfx950): one launch per batch.
//   phoc_from_text  <- build_phoc of the dataset (sam/phoc/build_phoc.py: lower, keep a-z 0-9; sam/phoc/cphoc.c: the 604-column pyramidal histogram of
//                      characters, unigram levels 2..5 and the 50 most frequent bigrams at level 2), which PhocProcessor (sam/datasets/processors.py:407-440)
//                      runs per token on the host and ships as fp32 [50, 604] with every sample.
// The batch carries the tokens as code points (int32 [B * n_max, ld_text] + a length per slot: the layout of the score table's "ocr" / "ocr_len"); the
// kernel folds and compacts them and writes the 604 columns -- 0/1, or scaled as l2norm_row (rowwise.h) scales a 0/1 row -- as fp32 or bf16 at a column
// offset of a wider destination row, as a part of sam_ragged_expand would.
//
// ARITHMETIC.  The reference's region test is not the exact rational one: it forms index/n, (index+1)/n, region/level and (region+1)/level as fp32
// quotients, takes their fp32 max / min, one fp32 subtraction each for the numerator and the denominator, ONE fp32 division, and compares with 0.5.  That
// differs from the exact test for everyday tokens (first at n = 3, index = 1: the middle letter of "the"), so region_hit below performs the same
// operations in the same order.  It relies on IEEE correctly rounded fp32 division, which is hipcc's default at this build's flags (-O3, no fast-math, no
// -fno-hip-fp32-correctly-rounded-divide-sqrt): keep it that way for this file, and use no reciprocal-multiply.  The sequence holds no multiply followed
// by an add, so -ffp-contract has nothing to fuse.  phoc.py's phoc_host is the host twin (numpy float32, the same sequence).
//
// One wave per slot, four slots per 256-thread block like the other row-wise kernels; one code point per lane (Lw <= 64).  The kept characters are
// compacted with a ballot and a prefix count, every kept character ORs its (at most 14 + 2) bits into the slot's 604-bit row in LDS, and the row leaves
// with 16-byte (fp32) / 8-byte (bf16) stores.  No global atomics, no workspace, nothing read by the host.
#include "common.h"
#include "rowwise.h"
#include "sam_hip_text.h"

namespace {

constexpr int PHOC_DIM = 604, PHOC_UNI = 504, PHOC_WORDS = 19, PHOC_CHUNKS = PHOC_DIM / 4;   // 14 regions x 36 | 2 regions x 50; 19 x 32 bits >= 604

// The non-ASCII code points whose Python str.lower() contains a kept character (phoc.py: FOLD_TABLE, re-derived over all code points by the CPU test,
// which also reads these lines).
#define PHOC_FOLD(X) X(0x0130, 'i') X(0x212A, 'k')
// The 50 bigrams in column order, two characters each (phoc.py: BIGRAMS, from the golden fixture's name list; the CPU test compares this string).
__device__ const char PHOC_BIGRAMS[101] = "thheineranreesonstntenatedndtooreatiartengalitasishaetseouoflesaverorarihinemedecotaecsillsonalilael";

// alphabet index (a-z -> 0..25, 0-9 -> 26..35) of a code point after folding, -1 = dropped
__device__ __forceinline__ int fold_char(int cp) {
  if (cp >= 'a' && cp <= 'z') return cp - 'a';
  if (cp >= 'A' && cp <= 'Z') return cp - 'A';
  if (cp >= '0' && cp <= '9') return 26 + cp - '0';
#define X(CP, CH) if (cp == CP) return CH - 'a';
  PHOC_FOLD(X)
#undef X
  return -1;
}

// cphoc.c's overlap test: occupancy [lo / n, hi / n] of a character (hi = lo + 1) or bigram (hi = lo + 2) against region `region` of `level`
__device__ __forceinline__ bool region_hit(int lo, int hi, int n, int region, int level) {
  const float occ0 = (float)lo / (float)n, occ1 = (float)hi / (float)n;
  const float reg0 = (float)region / (float)level, reg1 = (float)(region + 1) / (float)level;
  const float ov0 = occ0 > reg0 ? occ0 : reg0, ov1 = occ1 < reg1 ? occ1 : reg1;
  return (ov1 - ov0) / (occ1 - occ0) >= 0.5f;
}

template <typename DstT>
__device__ __forceinline__ void store_row(DstT* drow, const unsigned* bits, float one, bool vec, int lane) {
  if (vec) {
    for (int c = lane; c < PHOC_CHUNKS; c += 64) {
      const unsigned w = bits[c >> 3] >> ((c & 7) * 4);               // 4 columns never straddle a word
      const float v[4] = {(w & 1u) ? one : 0.f, (w & 2u) ? one : 0.f, (w & 4u) ? one : 0.f, (w & 8u) ? one : 0.f};
      st4(drow + 4 * c, v);
    }
  } else {
    for (int c = lane; c < PHOC_DIM; c += 64) {
      const float v = ((bits[c >> 5] >> (c & 31)) & 1u) ? one : 0.f;
      if constexpr (std::is_same<DstT, float>::value) drow[c] = v; else drow[c] = f2bf(v);
    }
  }
}

// grid ceil(B * n_max / 4): wave = slot.  Every wave reaches every barrier (a wave past the last slot works on an empty token and stores nothing).
__global__ __launch_bounds__(256) void phoc_from_text_kernel(const int32_t* __restrict__ text, int64_t ld_text, const int32_t* __restrict__ text_len,
                                                             const int32_t* __restrict__ counts, int rows, int n_max, int Lw, void* dst, int64_t ld_dst, int col0,
                                                             int dst_f32, int normalize, float eps, int vec) {
  __shared__ unsigned s_bits[4][PHOC_WORDS + 1];
  __shared__ signed char s_chars[4][64];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, row = blockIdx.x * 4 + wv;
  const bool in_range = row < rows;
  int len = 0;
  if (in_range) {
    len = text_len[row];
    len = len < 0 ? 0 : (len > Lw ? Lw : len);                        // clamped, never trusted
    if (counts) {
      const int b = row / n_max, i = row - b * n_max;
      int cnt = counts[b];
      cnt = cnt < 0 ? 0 : (cnt > n_max ? n_max : cnt);                // as sam_ragged_expand clamps
      if (i >= cnt) len = 0;                                          // padding slot: an all-zero row whatever its text holds
    }
  }
  int ch = -1;
  if (lane < len) ch = fold_char(text[(int64_t)row * ld_text + lane] & 0x3fffffff);      // (bit 30: the score table's NO_GLUE flag on an "s", not part of the code point)
  const unsigned long long kept = __ballot(ch >= 0);
  const int n = __popcll(kept), index = __popcll(kept & ((1ull << lane) - 1ull));
  if (lane < PHOC_WORDS + 1) s_bits[wv][lane] = 0u;
  if (ch >= 0) s_chars[wv][index] = (signed char)ch;
  __syncthreads();
  if (ch >= 0) {
    // unigrams: level 2..5, block of level L starts at region row 0, 2, 5, 9
    int base = 0;
    for (int level = 2; level <= 5; ++level) {
      for (int region = 0; region < level; ++region)
        if (region_hit(index, index + 1, n, region, level)) {
          const int col = (base + region) * 36 + ch;
          atomicOr(&s_bits[wv][col >> 5], 1u << (col & 31));
        }
      base += level;
    }
    // the bigram starting at this character, level 2
    if (index + 1 < n) {
      const int nx = s_chars[wv][index + 1];
      int bg = -1;
      for (int k = 0; k < 50; ++k)
        if (PHOC_BIGRAMS[2 * k] - 'a' == ch && PHOC_BIGRAMS[2 * k + 1] - 'a' == nx) { bg = k; break; }     // (every listed bigram is two letters)
      if (bg >= 0)
        for (int region = 0; region < 2; ++region)
          if (region_hit(index, index + 2, n, region, 2)) {
            const int col = PHOC_UNI + region * 50 + bg;
            atomicOr(&s_bits[wv][col >> 5], 1u << (col & 31));
          }
    }
  }
  __syncthreads();
  float one = 1.f;
  if (normalize) {
    // l2norm_row on a 0/1 row: the sum of squares is the number of ones (exact in fp32 in any order), then the same scale formula
    const float q = wave_sum(lane < PHOC_WORDS ? (float)__popc(s_bits[wv][lane]) : 0.f);
    one = 1.f * (1.0f / fmaxf(sqrtf(q), eps));
  }
  if (!in_range) return;
  if (dst_f32) store_row((float*)dst + (int64_t)row * ld_dst + col0, s_bits[wv], one, vec, lane);
  else store_row((bf16_t*)dst + (int64_t)row * ld_dst + col0, s_bits[wv], one, vec, lane);
}

}  // namespace

extern "C" int sam_phoc_from_text(const int32_t* text, int64_t ld_text, const int32_t* text_len, const int32_t* counts, int B, int n_max, int Lw, void* dst,
                                  int64_t ld_dst, int col0, int dst_f32, int normalize, float eps, void* stream) {
  SAM_REQUIRE(text && text_len && dst, "sam_phoc_from_text: null text / text_len / dst");
  SAM_REQUIRE(B > 0 && n_max > 0 && (int64_t)B * n_max < (int64_t)1 << 31, "sam_phoc_from_text: bad shape B=%d n_max=%d", B, n_max);
  SAM_REQUIRE(Lw >= 1, "sam_phoc_from_text: Lw must be at least 1 (Lw=%d)", Lw);
  if (Lw > 64) {
    sam_set_error("sam_phoc_from_text: Lw=%d: one code point per lane, at most 64", Lw);
    return SAM_ERR_UNSUPPORTED;
  }
  SAM_REQUIRE(ld_text >= Lw, "sam_phoc_from_text: need ld_text >= Lw (ld_text=%ld Lw=%d)", (long)ld_text, Lw);
  SAM_REQUIRE(col0 >= 0 && (int64_t)col0 + PHOC_DIM <= ld_dst, "sam_phoc_from_text: need 0 <= col0 and col0 + 604 <= ld_dst (col0=%d ld_dst=%ld)", col0, (long)ld_dst);
  SAM_REQUIRE(eps > 0.f, "sam_phoc_from_text: eps must be positive");
  const int esz = dst_f32 ? 4 : 2;
  SAM_REQUIRE(((uintptr_t)text % 4) == 0 && ((uintptr_t)text_len % 4) == 0 && ((uintptr_t)counts % 4) == 0 && ((uintptr_t)dst % esz) == 0,
              "sam_phoc_from_text: misaligned text / text_len / counts / dst");
  const int vec = ld_dst % 4 == 0 && col0 % 4 == 0 && ((uintptr_t)dst % (4 * esz)) == 0;       // 16-byte fp32 / 8-byte bf16 stores
  const int64_t rows = (int64_t)B * n_max;
  phoc_from_text_kernel<<<dim3((unsigned)((rows + 3) / 4)), dim3(256), 0, (hipStream_t)stream>>>(text, ld_text, text_len, counts, (int)rows, n_max, Lw, dst, ld_dst,
                                                                                                col0, dst_f32, normalize, eps, vec);
  SAM_LAUNCH_CHECK();
  return SAM_OK;
}

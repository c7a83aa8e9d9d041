// FastText vectors of the OCR tokens straight from their text (gfx950): one launch per batch, one wave per slot.
//   fasttext_from_text  <- FastTextProcessor (sam/datasets/processors.py:181-226): np.mean([model.get_word_vector(w) for w in token.split(" ")], axis=0)
//                          (processors.py:96-102), run per token on the host in every DataLoader worker and shipped as fp32 [50, 300] with every sample.
// The batch carries the tokens as code points (the layout of csrc/phoc.hip), the run keeps the model's input matrix (nwords dictionary rows, then `bucket`
// n-gram rows) and an exact-match hash index of the dictionary words on the device (fasttext.model_index; index_lookup_wave of csrc/text.h).
// include/sam_hip_fasttext.h states the rules; fasttext.vectors_host_text is the host twin and the outputs equal it bit for bit.
//
// ARITHMETIC.  A word vector is the sum of its rows IN LIST ORDER, fp32, times (float)(1.0 / count); a token is the sum of its pieces' vectors in order
// divided once by their number.  None of this may be reassociated or contracted: the unit is built without fast-math, and fp contraction is switched off
// below for everything this file defines (the multiply by the reciprocal is followed by the add of the next piece).  l2norm_row (rowwise.h, included
// above the pragma) keeps the contraction it has in every other unit, so normalize = 1 writes the bits of sam_l2norm_pack_bf16.
//
// One 64-lane block per slot: every branch that holds a barrier, a ballot or a shuffle is wave-uniform.  Per piece:
//   probe     every lane hashes the piece's code points, the wave walks the slots together and compares a candidate with one code point per lane;
//   n-grams   lane j owns the n-grams that start at character j of "<piece>" (up to 66 starts: two trips), extends the byte hash character by
//             character and writes its ids to LDS behind a wave prefix count, which is the canonical start-major, length-minor order;
//   gather    all lanes walk the id list in order with 8 row loads in flight per trip (unconditional, at clamped list positions), the row in registers
//             (chunk c of 4 columns on lane c & 63, as l2norm_row assigns them), adding strictly in list order.
// No global atomics, no workspace, nothing read by the host.
#include "common.h"
#include "rowwise.h"
#include "text.h"
#include "sam_hip_fasttext.h"

#pragma clang fp contract(off)

namespace {

constexpr int kMaxLw = 64, kMaxDim = 512, kMaxN = 8, kInFlight = 8;
constexpr int kMaxIds = 1 + (kMaxLw + 2) * kMaxN;      // the word's own row + every n-gram of "<" 64 characters ">"
constexpr unsigned kCpMask = 0x1FFFFFu;                 // 21 bits: what four UTF-8 bytes carry; the flag bits 30 / 31 are never part of a code point

// one FNV-1a step; the byte enters as a SIGNED char, as the library's hash takes it
__device__ __forceinline__ unsigned fnv_byte(unsigned h, unsigned byte) { return (h ^ (unsigned)(int)(signed char)byte) * 16777619u; }
// ... over the UTF-8 bytes of one code point (arithmetic encoding, 1-4 bytes)
__device__ __forceinline__ unsigned fnv_char(unsigned h, unsigned c) {
  if (c < 0x80u) return fnv_byte(h, c);
  if (c < 0x800u) return fnv_byte(fnv_byte(h, 0xC0u | (c >> 6)), 0x80u | (c & 0x3Fu));
  if (c < 0x10000u) return fnv_byte(fnv_byte(fnv_byte(h, 0xE0u | (c >> 12)), 0x80u | ((c >> 6) & 0x3Fu)), 0x80u | (c & 0x3Fu));
  return fnv_byte(fnv_byte(fnv_byte(fnv_byte(h, 0xF0u | (c >> 18)), 0x80u | ((c >> 12) & 0x3Fu)), 0x80u | ((c >> 6) & 0x3Fu)), 0x80u | (c & 0x3Fu));
}

// grid B * n_max, block 64: wave = slot.  NCH chunks of 4 columns per lane (dim <= 256 * NCH).
template <int NCH, typename DstT>
__global__ __launch_bounds__(64) void fasttext_from_text_kernel(const int32_t* __restrict__ text, int64_t ld_text, const int32_t* __restrict__ text_len,
                                                                const int32_t* __restrict__ counts, int n_max, int Lw, const float* __restrict__ matrix,
                                                                int64_t ld_matrix, const int32_t* __restrict__ index_cp, int64_t ld_index,
                                                                const int32_t* __restrict__ index_len, const int32_t* __restrict__ slots, int Lv, int n_slots,
                                                                int minn, int maxn, int bucket, int nwords, int eos_id, int dim, DstT* __restrict__ dst,
                                                                int64_t ld_dst, int col0, int normalize, float eps) {
  __shared__ unsigned s_cp[kMaxLw];
  __shared__ int s_ids[kMaxIds + kInFlight];
  __shared__ __attribute__((aligned(16))) float s_row[kMaxDim];
  const int row = blockIdx.x, lane = threadIdx.x;
  const int nchunk = dim >> 2;
  const WordIndex index{index_cp, ld_index, index_len, slots, nwords, n_slots};
  DstT* drow = dst + (int64_t)row * ld_dst + col0;
  int len = text_len[row];
  len = len < 0 ? 0 : (len > Lw ? Lw : len);                          // clamped, never trusted
  if (counts) {
    const int b = row / n_max, i = row - b * n_max;
    int cnt = counts[b];
    cnt = cnt < 0 ? 0 : (cnt > n_max ? n_max : cnt);                  // as sam_ragged_expand clamps
    if (i >= cnt) {                                                   // padding slot: an all-zero row whatever its text holds
      const float z[4] = {0.f, 0.f, 0.f, 0.f};
      for (int c = lane; c < nchunk; c += 64) st4(drow + 4 * c, z);
      return;
    }
  }
  unsigned cp = 0u;
  if (lane < len) cp = (unsigned)text[(int64_t)row * ld_text + lane] & kCpMask;
  s_cp[lane] = cp;
  const unsigned long long spaces = __ballot(lane < len && cp == 0x20u);
  __syncthreads();

  int chunk[NCH];
#pragma unroll
  for (int k = 0; k < NCH; ++k) chunk[k] = min(lane + 64 * k, nchunk - 1);
  float sum[NCH][4] = {};
  int n_pieces = 0;
  for (int p = 0;;) {                                                 // the pieces of token.split(" "): [p, e), e the next space or the end
    const unsigned long long m = p < 64 ? spaces & (~0ull << p) : 0ull;
    const int e = m ? __ffsll((long long)m) - 1 : len;
    const int L = e - p, M = L + 2;                                   // M characters in "<" piece ">"

    // ---- the dictionary word with exactly these code points, or -1
    int wid = -1;
    if (L <= Lv) wid = index_lookup_wave(index, L, lane, [&](int i) { return s_cp[p + i]; });

    // ---- the id list in LDS: the word's own row, then the n-grams of "<" piece ">" (not for the end-of-sentence word)
    int n_ids = 0;
    if (wid >= 0) {
      if (lane == 0) s_ids[0] = wid;
      n_ids = 1;
    }
    if (maxn > 0 && !(wid >= 0 && wid == eos_id)) {
      const int n_lo = minn > 1 ? minn : 1;
      for (int trip = 0; trip * 64 < M; ++trip) {
        const int j = trip * 64 + lane;
        const bool edge = j == 0 || j + 1 == M;                       // a single character at either end of the word is skipped
        int hi = 0, cnt = 0;
        if (j < M) {
          hi = min(maxn, M - j);
          cnt = max(0, hi - n_lo + 1) - ((n_lo == 1 && edge) ? 1 : 0);
        }
        int inc = cnt;                                                // inclusive prefix count over the lanes
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
          const int t = __shfl_up(inc, d);
          if (lane >= d) inc += t;
        }
        int at = n_ids + inc - cnt;
        unsigned h = 2166136261u;
        for (int n = 1; n <= hi; ++n) {
          const int k = j + n - 1;
          h = fnv_char(h, k == 0 ? (unsigned)'<' : (k == M - 1 ? (unsigned)'>' : s_cp[p + k - 1]));
          if (n >= n_lo && !(n == 1 && edge)) s_ids[at++] = nwords + (int)(h % (unsigned)bucket);
        }
        n_ids += __shfl(inc, 63);
      }
    }
    __syncthreads();

    // ---- v = sum of the rows in list order, times 1 / count
    float v[NCH][4];
#pragma unroll
    for (int k = 0; k < NCH; ++k)
#pragma unroll
      for (int q = 0; q < 4; ++q) v[k][q] = 0.f;
    for (int t = 0; t < n_ids; t += kInFlight) {
      float x[kInFlight][NCH][4];
#pragma unroll
      for (int u = 0; u < kInFlight; ++u) {
        const float* r = matrix + (int64_t)s_ids[min(t + u, n_ids - 1)] * ld_matrix;
#pragma unroll
        for (int k = 0; k < NCH; ++k) ld4(r + 4 * chunk[k], x[u][k]);
      }
#pragma unroll
      for (int u = 0; u < kInFlight; ++u)
        if (t + u < n_ids) {
#pragma unroll
          for (int k = 0; k < NCH; ++k)
#pragma unroll
            for (int q = 0; q < 4; ++q) v[k][q] = v[k][q] + x[u][k][q];
        }
    }
    if (n_ids > 0) {
      const float inv = (float)(1.0 / (double)n_ids);
#pragma unroll
      for (int k = 0; k < NCH; ++k)
#pragma unroll
        for (int q = 0; q < 4; ++q) v[k][q] = v[k][q] * inv;
    }
#pragma unroll
    for (int k = 0; k < NCH; ++k)
#pragma unroll
      for (int q = 0; q < 4; ++q) sum[k][q] = n_pieces == 0 ? v[k][q] : sum[k][q] + v[k][q];
    ++n_pieces;
    __syncthreads();                                                  // the id list is free for the next piece
    if (e >= len) break;
    p = e + 1;
  }
  const float np = (float)n_pieces;
#pragma unroll
  for (int k = 0; k < NCH; ++k)
    if (lane + 64 * k < nchunk) {
#pragma unroll
      for (int q = 0; q < 4; ++q) s_row[4 * (lane + 64 * k) + q] = sum[k][q] / np;
    }
  __syncthreads();
  l2norm_row<NCH>((const float*)s_row, drow, dim, normalize != 0, eps, lane);
}

}  // namespace

extern "C" int sam_fasttext_from_text(const int32_t* text, int64_t ld_text, const int32_t* text_len, const int32_t* counts, int B, int n_max, int Lw,
                                      const float* matrix, int64_t ld_matrix, const int32_t* index_cp, int64_t ld_index, const int32_t* index_len,
                                      const int32_t* slots, int Lv, int n_slots, int minn, int maxn, int bucket, int nwords, int eos_id, int dim, void* dst,
                                      int64_t ld_dst, int col0, int dst_f32, int normalize, float eps, void* stream) {
  SAM_REQUIRE(text && text_len && dst, "sam_fasttext_from_text: null text / text_len / dst");
  SAM_REQUIRE(matrix, "sam_fasttext_from_text: null matrix");
  if (const int rc = word_index_check("sam_fasttext_from_text", "ld_index", index_cp, ld_index, index_len, slots, Lv, kMaxLw, n_slots)) return rc;
  SAM_REQUIRE(B > 0 && n_max > 0 && (int64_t)B * n_max < (int64_t)1 << 31, "sam_fasttext_from_text: bad shape B=%d n_max=%d", B, n_max);
  SAM_REQUIRE(Lw >= 1 && dim >= 4 && minn >= 0 && maxn >= minn, "sam_fasttext_from_text: need Lw >= 1, dim >= 4, 0 <= minn <= maxn (Lw=%d dim=%d minn=%d maxn=%d)", Lw,
              dim, minn, maxn);
  const int esz = dst_f32 ? 4 : 2;
  if (Lw > kMaxLw || dim % 4 != 0 || dim > kMaxDim || maxn > kMaxN || col0 % 4 != 0 || ld_dst % 4 != 0 || ((uintptr_t)dst % (4 * esz)) != 0) {
    sam_set_error("sam_fasttext_from_text: Lw=%d dim=%d maxn=%d col0=%d ld_dst=%ld: this build takes Lw <= %d, dim %% 4 == 0, dim <= %d, maxn <= %d and a "
                  "destination of 4-element alignment (col0 %% 4 == 0, ld_dst %% 4 == 0)", Lw, dim, maxn, col0, (long)ld_dst, kMaxLw, kMaxDim, kMaxN);
    return SAM_ERR_UNSUPPORTED;
  }
  SAM_REQUIRE(ld_text >= Lw, "sam_fasttext_from_text: need ld_text >= Lw (ld_text=%ld Lw=%d)", (long)ld_text, Lw);
  SAM_REQUIRE(nwords >= 1 && bucket >= 0 && (bucket >= 1 || maxn == 0) && (int64_t)nwords + bucket < (int64_t)1 << 31,
              "sam_fasttext_from_text: need nwords >= 1 and bucket >= 1 (bucket = 0 only with maxn = 0); nwords=%d bucket=%d maxn=%d", nwords, bucket, maxn);
  SAM_REQUIRE(eos_id >= -1 && eos_id < nwords, "sam_fasttext_from_text: eos_id=%d outside [-1, %d)", eos_id, nwords);
  SAM_REQUIRE(ld_matrix >= dim && ld_matrix % 4 == 0 && ((uintptr_t)matrix % 16) == 0, "sam_fasttext_from_text: the matrix rows must be 16-byte aligned with "
              "ld_matrix >= dim (ld_matrix=%ld dim=%d)", (long)ld_matrix, dim);
  SAM_REQUIRE(col0 >= 0 && (int64_t)col0 + dim <= ld_dst, "sam_fasttext_from_text: need 0 <= col0 and col0 + dim <= ld_dst (col0=%d dim=%d ld_dst=%ld)", col0, dim,
              (long)ld_dst);
  SAM_REQUIRE(eps > 0.f, "sam_fasttext_from_text: eps must be positive");
  SAM_REQUIRE(((uintptr_t)text | (uintptr_t)text_len | (uintptr_t)counts) % 4 == 0, "sam_fasttext_from_text: misaligned text / text_len / counts");
  const dim3 grid((unsigned)((int64_t)B * n_max)), blk(64);
  hipStream_t st = (hipStream_t)stream;
#define FT_LAUNCH(NCH_, T_) fasttext_from_text_kernel<NCH_, T_><<<grid, blk, 0, st>>>(text, ld_text, text_len, counts, n_max, Lw, matrix, ld_matrix, index_cp, ld_index, \
      index_len, slots, Lv, n_slots, minn, maxn, bucket, nwords, eos_id, dim, (T_*)dst, ld_dst, col0, normalize, eps)
  if (dim <= 256) { if (dst_f32) FT_LAUNCH(1, float); else FT_LAUNCH(1, bf16_t); }
  else { if (dst_f32) FT_LAUNCH(2, float); else FT_LAUNCH(2, bf16_t); }
#undef FT_LAUNCH
  SAM_LAUNCH_CHECK();
  return SAM_OK;
}

// Evaluation results collected by question index: a results board resident in device memory (gfx950).
//   evalboard_collect  <- the per-batch bookkeeping of Evaluator.evaluate (evaluator.py:67-135: the running sums, the question-id and answer lists): a
//                         batch's sam_eval_beams rows are scattered to board[sample_idx[b]] where valid[b] is set, first write wins, `seen` counts.
//   evalboard_reduce   <- the means' numerators, over the board's distinct rows in score_totals_kernel's fixed order (score_walk.h).
//   evalboard_merge    <- two ranks' boards, row by row.
// collect is laid out as store_gather_fixed_kernel: one wave per slot, four waves per 256-thread block; a wave finds whether its slot owns the question
// and how many live slots hold it from a lane-strided scan of sample_idx / valid (B is small).  Distinct owners write distinct rows: no atomics, no
// cross-block communication.  Nothing read from device memory is trusted: include/sam_hip_evalboard.h.
#include "common.h"
#include "sam_hip_evalboard.h"

namespace {

constexpr int BOARD_THREADS = 256;
enum { ST_BAD_INDEX = 1 };

struct Board {
  float *scores, *oracle;
  int32_t *flags, *best, *answer, *answer_len, *seen, *status;
};
struct Rows {                                                                // a batch's sam_eval_beams outputs, or another board
  const float *scores, *oracle;
  const int32_t *flags, *best, *answer, *answer_len;
};
struct Slots {
  const int32_t *sample_idx, *valid;
  int B;
};

__device__ __forceinline__ bool slot_valid(const Slots& s, int b) { return !s.valid || s.valid[b] != 0; }
__device__ __forceinline__ bool in_range(int q, int64_t n) { return q >= 0 && (int64_t)q < n; }

// row `from` of src -> row q of the board, by one wave; len_cap >= 0: answer_len clamped to [0, len_cap]
__device__ __forceinline__ void copy_row(const Board& d, int64_t q, const Rows& s, int64_t from, int P, int len_cap, int lane) {
  if (lane < 3) d.scores[3 * q + lane] = s.scores[3 * from + lane];
  else if (lane < 6) d.oracle[3 * q + lane - 3] = s.oracle[3 * from + lane - 3];
  else if (lane == 6) d.flags[q] = s.flags[from];
  else if (lane == 7) d.best[q] = s.best[from];
  else if (lane == 8) {
    int len = s.answer_len[from];
    if (len_cap >= 0) len = len < 0 ? 0 : (len > len_cap ? len_cap : len);
    d.answer_len[q] = len;
  }
  const int32_t* sa = s.answer + from * (int64_t)P;
  int32_t* da = d.answer + q * (int64_t)P;
  for (int c = lane; c < P; c += 64) da[c] = sa[c];
}

// grid ceil(B / 4): wave = slot
__global__ __launch_bounds__(BOARD_THREADS) void evalboard_collect_kernel(Slots sl, Rows in, Board bd, int64_t n, int P) {
  const int lane = threadIdx.x & 63, b = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (b >= sl.B) return;                                                    // (wave-uniform, as every branch around a wave sum below)
  if (b == 0) {                                                             // one wave looks for valid slots out of range: one writer of the status word
    int bad = 0;
    for (int s = lane; s < sl.B; s += 64) bad += (slot_valid(sl, s) && !in_range(sl.sample_idx[s], n)) ? 1 : 0;
    bad = wave_sum_i(bad);
    if (bad && lane == 0) *bd.status |= ST_BAD_INDEX;
  }
  const int q = sl.sample_idx[b];
  if (!slot_valid(sl, b) || !in_range(q, n)) return;
  int before = 0, m = 0;
  for (int s = lane; s < sl.B; s += 64) {
    const int hit = (slot_valid(sl, s) && sl.sample_idx[s] == q) ? 1 : 0;    // (q is in range, so the slot is live)
    m += hit;
    before += (s < b) ? hit : 0;
  }
  before = wave_sum_i(before);
  m = wave_sum_i(m);                                                        // 1 <= m <= B
  if (before) return;                                                       // an earlier live slot owns q
  const int was = bd.seen[q];                                               // read by every lane in front of lane 0's store below
  if (was == 0) copy_row(bd, q, in, b, P, P, lane);
  if (lane == 0) bd.seen[q] = was == 0 ? m : (int)((unsigned)was + (unsigned)m);
}

// one workgroup: score_totals_kernel's order over the board's rows
__global__ __launch_bounds__(BOARD_THREADS) void evalboard_reduce_kernel(const float* __restrict__ scores, const float* __restrict__ oracle,
                                                                         const int32_t* __restrict__ seen, int64_t n, double* __restrict__ out) {
  __shared__ double red[6][BOARD_THREADS];
  __shared__ long long cnt[2][BOARD_THREADS];
  const int tid = threadIdx.x;
  double acc[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
  long long rows = 0, total = 0;
  for (int64_t r = tid; r < n; r += BOARD_THREADS) {
    const int s = seen[r];
    if (s <= 0) continue;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      acc[c] += (double)scores[3 * r + c];
      acc[3 + c] += (double)oracle[3 * r + c];
    }
    rows += 1;
    total += s;
  }
#pragma unroll
  for (int c = 0; c < 6; ++c) red[c][tid] = acc[c];
  cnt[0][tid] = rows;
  cnt[1][tid] = total;
  __syncthreads();
  for (int o = BOARD_THREADS / 2; o >= 1; o >>= 1) {
    if (tid < o) {
#pragma unroll
      for (int c = 0; c < 6; ++c) red[c][tid] += red[c][tid + o];
      cnt[0][tid] += cnt[0][tid + o];
      cnt[1][tid] += cnt[1][tid + o];
    }
    __syncthreads();
  }
  if (tid < 3) out[tid] = red[tid][0];
  else if (tid == 3) out[3] = (double)cnt[0][0];
  else if (tid < 7) out[tid] = red[tid - 1][0];
  else if (tid == 7) out[7] = (double)cnt[1][0];                            // < 2^31 * 2^31: exact below 2^53
}

// grid ceil(n / 4): wave = row
__global__ __launch_bounds__(BOARD_THREADS) void evalboard_merge_kernel(Board dst, Rows src, const int32_t* __restrict__ src_seen,
                                                                        const int32_t* __restrict__ src_status, int64_t n, int P) {
  const int lane = threadIdx.x & 63;
  const int64_t q = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (q >= n) return;
  if (q == 0 && lane == 0) *dst.status |= *src_status;
  const int s = src_seen[q];
  if (s <= 0) return;
  const int was = dst.seen[q];
  if (was == 0) copy_row(dst, q, src, q, P, -1, lane);
  if (lane == 0) dst.seen[q] = (int)((unsigned)was + (unsigned)s);
}

bool aligned(const void* p, unsigned a) { return ((uintptr_t)p % a) == 0; }

int check_size(const char* who, int64_t n, int P) {
  SAM_REQUIRE(n >= 1 && n < (int64_t)1 << 31, "%s: bad size n=%ld (need 1 <= n < 2^31)", who, (long)n);
  SAM_REQUIRE(P >= 1, "%s: bad answer width P=%d (need P >= 1)", who, P);
  return SAM_OK;
}

}  // namespace

extern "C" int sam_evalboard_collect(const int32_t* sample_idx, const int32_t* valid, int B, const float* best_scores, const float* oracle,
                                     const int32_t* best_flags, const int32_t* best, const int32_t* answer, const int32_t* answer_len, int64_t n, int P,
                                     float* board_scores, float* board_oracle, int32_t* board_flags, int32_t* board_best, int32_t* board_answer,
                                     int32_t* board_answer_len, int32_t* board_seen, int32_t* board_status, void* stream) {
  const char* who = "sam_evalboard_collect";
  SAM_REQUIRE(sample_idx && best_scores && oracle && best_flags && best && answer && answer_len,
              "%s: null pointer (sample_idx, best_scores, oracle, best_flags, best, answer, answer_len)", who);
  SAM_REQUIRE(board_scores && board_oracle && board_flags && board_best && board_answer && board_answer_len && board_seen && board_status,
              "%s: null board pointer (scores, oracle, flags, best, answer, answer_len, seen, status)", who);
  const void* ptrs[] = {sample_idx, valid, best_scores, oracle, best_flags, best, answer, answer_len, board_scores, board_oracle, board_flags, board_best,
                        board_answer, board_answer_len, board_seen, board_status};
  for (const void* p : ptrs) SAM_REQUIRE(aligned(p, 4), "%s: misaligned pointer %p (every tensor holds 4-byte elements)", who, p);
  SAM_REQUIRE(B >= 1, "%s: bad shape B=%d (need B >= 1)", who, B);
  if (const int rc = check_size(who, n, P)) return rc;
  const Slots sl{sample_idx, valid, B};
  const Rows in{best_scores, oracle, best_flags, best, answer, answer_len};
  const Board bd{board_scores, board_oracle, board_flags, board_best, board_answer, board_answer_len, board_seen, board_status};
  evalboard_collect_kernel<<<dim3((unsigned)(((int64_t)B + 3) / 4)), dim3(BOARD_THREADS), 0, (hipStream_t)stream>>>(sl, in, bd, n, P);
  SAM_LAUNCH_CHECK();
  return SAM_OK;
}

extern "C" int sam_evalboard_reduce(const float* board_scores, const float* board_oracle, const int32_t* board_seen, int64_t n, double* out, void* stream) {
  const char* who = "sam_evalboard_reduce";
  SAM_REQUIRE(board_scores && board_oracle && board_seen && out, "%s: null pointer (scores, oracle, seen, out)", who);
  SAM_REQUIRE(aligned(board_scores, 4) && aligned(board_oracle, 4) && aligned(board_seen, 4) && aligned(out, 8),
              "%s: misaligned scores / oracle / seen / out pointer", who);
  if (const int rc = check_size(who, n, 1)) return rc;
  evalboard_reduce_kernel<<<dim3(1), dim3(BOARD_THREADS), 0, (hipStream_t)stream>>>(board_scores, board_oracle, board_seen, n, out);
  SAM_LAUNCH_CHECK();
  return SAM_OK;
}

extern "C" int sam_evalboard_merge(float* dst_scores, float* dst_oracle, int32_t* dst_flags, int32_t* dst_best, int32_t* dst_answer,
                                   int32_t* dst_answer_len, int32_t* dst_seen, int32_t* dst_status, const float* src_scores, const float* src_oracle,
                                   const int32_t* src_flags, const int32_t* src_best, const int32_t* src_answer, const int32_t* src_answer_len,
                                   const int32_t* src_seen, const int32_t* src_status, int64_t n, int P, void* stream) {
  const char* who = "sam_evalboard_merge";
  SAM_REQUIRE(dst_scores && dst_oracle && dst_flags && dst_best && dst_answer && dst_answer_len && dst_seen && dst_status,
              "%s: null dst pointer (scores, oracle, flags, best, answer, answer_len, seen, status)", who);
  SAM_REQUIRE(src_scores && src_oracle && src_flags && src_best && src_answer && src_answer_len && src_seen && src_status,
              "%s: null src pointer (scores, oracle, flags, best, answer, answer_len, seen, status)", who);
  const void* dst[8] = {dst_scores, dst_oracle, dst_flags, dst_best, dst_answer, dst_answer_len, dst_seen, dst_status};
  const void* src[8] = {src_scores, src_oracle, src_flags, src_best, src_answer, src_answer_len, src_seen, src_status};
  for (int k = 0; k < 8; ++k)
    SAM_REQUIRE(aligned(dst[k], 4) && aligned(src[k], 4), "%s: misaligned pointer (tensor %d of the board; every tensor holds 4-byte elements)", who, k);
  if (const int rc = check_size(who, n, P)) return rc;
  const uint64_t bytes[8] = {12u * (uint64_t)n, 12u * (uint64_t)n, 4u * (uint64_t)n, 4u * (uint64_t)n, 4u * (uint64_t)n * (uint64_t)P, 4u * (uint64_t)n,
                             4u * (uint64_t)n, 4u};
  for (int i = 0; i < 8; ++i)
    for (int j = 0; j < 8; ++j) {
      const uintptr_t d = (uintptr_t)dst[i], s = (uintptr_t)src[j];
      SAM_REQUIRE(d + bytes[i] <= s || s + bytes[j] <= d, "%s: the boards overlap (dst tensor %d, src tensor %d): merge needs two boards", who, i, j);
    }
  const Board bd{dst_scores, dst_oracle, dst_flags, dst_best, dst_answer, dst_answer_len, dst_seen, dst_status};
  const Rows in{src_scores, src_oracle, src_flags, src_best, src_answer, src_answer_len};
  evalboard_merge_kernel<<<dim3((unsigned)((n + 3) / 4)), dim3(BOARD_THREADS), 0, (hipStream_t)stream>>>(bd, in, src_seen, src_status, n, P);
  SAM_LAUNCH_CHECK();
  return SAM_OK;
}

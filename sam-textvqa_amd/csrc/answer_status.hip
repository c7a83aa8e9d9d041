// The sticky record of the answer-table build's status (include/sam_hip_step.h): sam_answer_table_from_text leaves one status word per
// sample; a build that runs in front of every step without a read-back (a captured one could not raise at all) needs a record, so a launch of ONE wave right
// behind the build folds the vector into four int64 words that outlive the step: OR of the bits, number of flagged samples, step and batch index of the
// first one.  The caller reads them when it wants to (answers.fold_status_host is the host twin).
//
// The wave walks the vector 64 samples at a time.  Count and lowest flagged index of a chunk come from one ballot (popcount / find-first-set of the
// mask: uniform over the wave, nothing to reduce); the OR of the words is a six-step xor butterfly once at the end.  Lane 0 then does the
// read-modify-write of the four words with ordinary stores: launches on a stream are ordered, so no atomics and no workspace.
#include "common.h"
#include "sam_hip_step.h"

namespace {

constexpr int kWave = 64;
constexpr long long kCountCap = 1ll << 62;

__global__ __launch_bounds__(kWave) void answer_status_fold_kernel(const int32_t* __restrict__ status, int B, const int64_t* step_dev, long long step,
                                                                   int64_t* __restrict__ state) {
  const int lane = threadIdx.x;
  unsigned bits = 0;
  long long flagged = 0, first = -1;
  for (long long base = 0; base < B; base += kWave) {         // (64-bit: base + lane must not wrap for B near 2^31; every lane runs every trip: ballot)
    const long long i = base + lane;
    const unsigned st = i < B ? (unsigned)status[i] : 0u;
    bits |= st;
    const unsigned long long m = __ballot(st != 0u);
    flagged += __popcll(m);
    if (first < 0 && m) first = base + __ffsll((long long)m) - 1;
  }
  for (int o = kWave / 2; o > 0; o >>= 1) bits |= (unsigned)__shfl_xor((int)bits, o);
  if (lane != 0) return;
  state[0] |= (int64_t)bits;                                   // (zero-extended: the word never goes negative)
  if (!flagged) return;
  const long long seen = state[1];
  state[1] = seen >= kCountCap - flagged ? kCountCap : seen + flagged;      // min(seen + flagged, 2^62); flagged <= 2^31: no overflow on either side
  if (state[3] < 0) {
    state[2] = (step_dev ? (long long)*step_dev : 0ll) + step;
    state[3] = first;
  }
}

}  // namespace

extern "C" int sam_answer_status_fold(const int32_t* status, int B, const int64_t* step_dev, int64_t step, int64_t* state, void* stream) {
  SAM_REQUIRE(status && state, "sam_answer_status_fold: null status / state pointer");
  SAM_REQUIRE(B >= 1, "sam_answer_status_fold: batch %d must be at least 1", B);
  SAM_REQUIRE(((uintptr_t)status % 4) == 0 && ((uintptr_t)state % 8) == 0 && ((uintptr_t)step_dev % 8) == 0, "sam_answer_status_fold: misaligned operand");
  answer_status_fold_kernel<<<dim3(1), dim3(kWave), 0, (hipStream_t)stream>>>(status, B, step_dev, (long long)step, state);
  SAM_LAUNCH_CHECK();
  return SAM_OK;
}

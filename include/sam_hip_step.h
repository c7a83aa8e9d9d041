/* sam_hip_step.h -- entry points of libsam_hip.so that keep a record of the training step in device memory, across steps and graph replays.
 *
 * The conventions of sam_hip_pipeline.h hold: plain C, every function returns 0 or a SAM_ERR_* code of sam_hip.h with a message in sam_last_error(),
 * arguments are checked before any device call, launches go to the caller's stream and nothing synchronises, no workspace, no global atomics; the
 * model's ABI (sam_hip.h, sam_abi_version()) is untouched.  The declarations live in a file of their own because the ctypes binding keeps one table per
 * header and the tables of the other four headers are pinned by the tests of the entry points they were written for.
 */
#ifndef SAM_HIP_STEP_H
#define SAM_HIP_STEP_H
#include "sam_hip.h"
#ifdef __cplusplus
extern "C" {
#endif

/* ---- fold the status vector of one sam_answer_table_from_text launch into a sticky four-word record, one launch of one wave ----
 * A captured step cannot raise for a flagged sample and a read-back per eager step would synchronise; the build already gives a flagged sample an
 * all-zero table ("no candidate" for sam_answer_sample).  This keeps what outlives the step.  state int64 [4]:
 *   [0] the OR of every status word seen (each taken as an unsigned 32-bit value)             reset: 0
 *   [1] the number of flagged samples (status != 0), saturating at 2^62                      reset: 0
 *   [2] the step of the first flagged sample                                                  reset: -1
 *   [3] the batch index of that sample, the lowest flagged index of that step                 reset: -1
 * Words 2 and 3 are written once, by the first launch that meets a flagged sample while word 3 is negative.  The step is step_dev[0] + step when
 * step_dev is not NULL (int64 [1] in device memory: the Trainer's step counter, so that a replay records its own step), else step -- the convention of
 * sam_answer_sample.  status int32 [B], B >= 1.  Launches on one stream are ordered: the read-modify-write of the four words is done by one lane with
 * ordinary stores, without atomics. */
int sam_answer_status_fold(const int32_t* status, int B, const int64_t* step_dev, int64_t step, int64_t* state /*[4]*/, void* stream);

#ifdef __cplusplus
}
#endif
#endif

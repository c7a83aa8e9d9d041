/* sam_hip_sampler.h -- each step's sample indices drawn on the device: shuffled, sharded epochs from a resident state.  An
 * extension of the model's ABI: additive (sam_abi_version() stays what it was), declared here and in no other header; a C caller includes this file,
 * which includes sam_hip.h.  Same conventions as there.
 *
 * state int64 [4] in DEVICE memory: {seed, epoch, step_in_epoch, batches_drawn}.  One launch writes batch t = step_in_epoch of epoch `epoch` for rank
 * `rank` of `world` -- torch.utils.data.DistributedSampler's semantics (shuffle per epoch, pad by wrapping to a multiple of the world size, rank r
 * takes every world-th position; world = 1 is a RandomSampler) -- and advances the state:
 *   num_samples     = ceil(n / world)            (flags & 2, drop_last:       floor(n / world), which must be >= 1)
 *   steps_per_epoch = ceil(num_samples / B)      (flags & 4, drop_last_batch: floor(num_samples / B), which must be >= 1)
 *   slot i:  j = t * B + i,  p = j * world + rank  (64-bit),  valid[i] = (j < num_samples),
 *            sample_idx[i] = flags & 1 (shuffle) ? perm(seed, epoch, n)[p mod n] : p mod n
 *   A slot past the shard's end (valid 0) still holds an in-range index computed the same way: a gather needs no special case.
 *   Then, unless flags & 8 (peek): step_in_epoch += 1; at steps_per_epoch it becomes 0 and epoch += 1; batches_drawn += 1.
 * perm(seed, epoch, n) is a keyed bijection on [0, n) evaluated per element: a balanced Feistel network of 8 rounds on the smallest even bit width 2k
 * with 2^(2k) >= n, followed by a keyed swap of the values 0 and 1 (so that odd permutations of the domain are drawn too), cycle-walked back into
 * [0, n); the round function is mix32 of the half-word xor a round key, the round keys chain mix32 over the seed's and the epoch's 32-bit halves, the
 * round number and a constant of this sampler's own.  sampler.py holds the host twin, which is the definition bit for bit; the order is this
 * project's own, not torch.randperm's.
 *
 * Nothing read from device memory is trusted: a state with epoch < 0, step_in_epoch < 0 or step_in_epoch >= steps_per_epoch gives all-zero sample_idx
 * and valid, status[0] |= 2 (bit 1; bit 0 is not used), and stays as it was.  status int32 [1] is only ever OR-ed into: zero it before the first call.
 *
 * Arguments are checked on the host in front of the launch (SAM_ERR_ARG with a message): null or misaligned pointers, n outside [1, 2^31), B < 1,
 * world < 1, rank outside [0, world), flag bits above 8, drop_last with n < world, drop_last_batch with num_samples < B.
 *
 * One workgroup of 256 threads striding over B; every thread reads the state in front of a block barrier and thread 0 writes the advanced state
 * behind it: no atomics, no workspace, nothing read back by the host. */
#ifndef SAM_HIP_SAMPLER_H
#define SAM_HIP_SAMPLER_H
#include "sam_hip.h"
#ifdef __cplusplus
extern "C" {
#endif

int sam_sample_batch(int64_t* state, int64_t n, int B, int rank, int world, int flags, int32_t* sample_idx, int32_t* valid, int32_t* status,
                     void* stream);

#ifdef __cplusplus
}
#endif
#endif

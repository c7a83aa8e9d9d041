// Each step's sample indices from a state resident in device memory: shuffled, sharded epochs (gfx950).
//   sample_batch  <- RandomSampler / DistributedSampler + the DataLoader's batching (sam/task_utils.py:138-166; torch.utils.data.distributed): shuffle
//                    per epoch, pad by wrapping to a multiple of the world size, rank r takes every world-th position.  In place of randperm(n) on the
//                    host, a slice and a copy of int32 [B] per step: perm(seed, epoch, n)[p] is evaluated per element (a keyed Feistel bijection,
//                    cycle-walked into [0, n)), so there is no permutation array and nothing comes from the host.
// One workgroup; every thread reads the four state words in front of the barrier, thread 0 writes the advanced state behind it.  sampler.py holds the
// host twin (perm_at, batch_host): the same integer arithmetic, bit for bit.  Nothing read from device memory is trusted: include/sam_hip_sampler.h.
#include "common.h"
#include "sam_hip_sampler.h"

namespace {

constexpr int SAMPLER_THREADS = 256;
constexpr int SAMPLER_ROUNDS = 8;
constexpr unsigned SAMPLER_DOMAIN = 0x53414D50u;                           // the key chain's own constant: no other mix32 user starts from it
constexpr unsigned SAMPLER_ROUND_STEP = 0x9E3779B1u;
enum { FLAG_SHUFFLE = 1, FLAG_DROP_LAST = 2, FLAG_DROP_LAST_BATCH = 4, FLAG_PEEK = 8, FLAG_ALL = 15 };
enum { ST_BAD_STATE = 2 };

struct Args {
  int64_t* state;
  int32_t *sample_idx, *valid, *status;
  uint64_t n, num_samples, steps;                                           // n < 2^31; num_samples, steps <= n
  int B, rank, world, flags, half_bits;                                     // half_bits = k: the Feistel network permutes [0, 2^(2k))
};

struct Keys { unsigned k[SAMPLER_ROUNDS]; unsigned swap; };                  // swap: 1 when values 0 and 1 change places behind the network

__device__ __forceinline__ Keys round_keys(uint64_t seed, uint64_t epoch) {
  unsigned h = mix32((unsigned)seed ^ SAMPLER_DOMAIN);
  h = mix32(h ^ (unsigned)(seed >> 32));
  h = mix32(h ^ (unsigned)epoch);
  h = mix32(h ^ (unsigned)(epoch >> 32));
  Keys ks;
#pragma unroll
  for (int r = 0; r < SAMPLER_ROUNDS; ++r) ks.k[r] = mix32(h ^ ((unsigned)(r + 1) * SAMPLER_ROUND_STEP));
  ks.swap = mix32(h ^ ((unsigned)(SAMPLER_ROUNDS + 1) * SAMPLER_ROUND_STEP)) & 1u;
  return ks;
}

// perm[p] for p < n <= 2^(2k).  A balanced Feistel network with k >= 2 is always an EVEN permutation of [0, 2^(2k)) (every round is the half swap and
// an xor, both products of an even number of transpositions), which would leave the even orderings of a small n likelier than the odd ones (by 1/12
// at n = 5); so a key bit decides whether the transposition (0 1) follows the network, and both parities are drawn.
// The network and the swap together are a permutation of [0, 2^(2k)), and p lies on one of its cycles: following the cycle from p comes
// back to p, which is below n, so a value below n is met after finitely many steps (at the latest p itself).  Hence no iteration cap: a cap could only
// return a wrong value.  2^(2k) < 4n, so a walk takes fewer than four network evaluations on average.
__device__ __forceinline__ unsigned perm_at(const Keys& ks, int k, uint64_t n, unsigned p) {
  if (n == 1) return 0;
  const unsigned mask = (1u << k) - 1u;
  unsigned x = p;
  do {
    unsigned l = x >> k, r = x & mask;
#pragma unroll
    for (int i = 0; i < SAMPLER_ROUNDS; ++i) {
      const unsigned t = l ^ (mix32(r ^ ks.k[i]) >> (32 - k));
      l = r;
      r = t;
    }
    x = (l << k) | r;
    x ^= (x < 2u) ? ks.swap : 0u;
  } while ((uint64_t)x >= n);
  return x;
}

__global__ __launch_bounds__(SAMPLER_THREADS) void sample_batch_kernel(Args a) {
  const int tid = threadIdx.x;
  const int64_t seed = a.state[0], epoch = a.state[1], step = a.state[2], drawn = a.state[3];
  __syncthreads();                                                          // every read of the state is in front of the one write below
  if (epoch < 0 || step < 0 || (uint64_t)step >= a.steps) {                 // (block-uniform)
    for (int i = tid; i < a.B; i += SAMPLER_THREADS) { a.sample_idx[i] = 0; a.valid[i] = 0; }
    if (tid == 0) *a.status |= ST_BAD_STATE;
    return;
  }
  const bool shuffle = a.flags & FLAG_SHUFFLE;
  const Keys ks = round_keys((uint64_t)seed, (uint64_t)epoch);
  // j = step * B + i < num_samples + B < 2^32 and world < 2^31: p = j * world + rank < 2^63.  One 64-bit division per thread; the next slot of this
  // thread lies SAMPLER_THREADS * world positions on, so p mod n moves by that product mod n.
  uint64_t j = (uint64_t)step * (uint64_t)a.B + (uint64_t)tid;
  uint64_t m = (j * (uint64_t)a.world + (uint64_t)a.rank) % a.n;
  const uint64_t delta = ((uint64_t)SAMPLER_THREADS * (uint64_t)a.world) % a.n;
  for (int i = tid; i < a.B; i += SAMPLER_THREADS) {
    a.sample_idx[i] = (int32_t)(shuffle ? perm_at(ks, a.half_bits, a.n, (unsigned)m) : (unsigned)m);
    a.valid[i] = j < a.num_samples ? 1 : 0;
    j += SAMPLER_THREADS;
    m += delta;                                                             // both below n < 2^31
    if (m >= a.n) m -= a.n;
  }
  if (tid == 0 && !(a.flags & FLAG_PEEK)) {
    const bool last = (uint64_t)step + 1 == a.steps;
    a.state[1] = (int64_t)((uint64_t)epoch + (last ? 1u : 0u));
    a.state[2] = last ? 0 : step + 1;
    a.state[3] = (int64_t)((uint64_t)drawn + 1u);
  }
}

}  // namespace

extern "C" int sam_sample_batch(int64_t* state, int64_t n, int B, int rank, int world, int flags, int32_t* sample_idx, int32_t* valid, int32_t* status,
                                void* stream) {
  const char* who = "sam_sample_batch";
  SAM_REQUIRE(state && sample_idx && valid && status, "%s: null pointer (state, sample_idx, valid, status)", who);
  SAM_REQUIRE(((uintptr_t)state % 8) == 0 && ((uintptr_t)sample_idx % 4) == 0 && ((uintptr_t)valid % 4) == 0 && ((uintptr_t)status % 4) == 0,
              "%s: misaligned state / index / valid / status pointer", who);
  SAM_REQUIRE(n >= 1 && n < (int64_t)1 << 31, "%s: bad size n=%ld (need 1 <= n < 2^31)", who, (long)n);
  SAM_REQUIRE(B >= 1, "%s: bad shape B=%d (need B >= 1)", who, B);
  SAM_REQUIRE(world >= 1 && rank >= 0 && rank < world, "%s: bad shard rank=%d world=%d (need world >= 1 and 0 <= rank < world)", who, rank, world);
  SAM_REQUIRE((flags & ~FLAG_ALL) == 0, "%s: unknown flag bits 0x%x (1 shuffle, 2 drop_last, 4 drop_last_batch, 8 peek)", who, flags & ~FLAG_ALL);
  SAM_REQUIRE(!(flags & FLAG_DROP_LAST) || n >= world, "%s: drop_last with n=%ld < world=%d leaves no sample", who, (long)n, world);
  Args a;
  a.state = state; a.sample_idx = sample_idx; a.valid = valid; a.status = status;
  a.n = (uint64_t)n;
  a.num_samples = (flags & FLAG_DROP_LAST) ? a.n / (uint64_t)world : (a.n + (uint64_t)world - 1) / (uint64_t)world;
  SAM_REQUIRE(!(flags & FLAG_DROP_LAST_BATCH) || a.num_samples >= (uint64_t)B, "%s: drop_last_batch with num_samples=%ld < B=%d leaves no batch", who,
              (long)a.num_samples, B);
  a.steps = (flags & FLAG_DROP_LAST_BATCH) ? a.num_samples / (uint64_t)B : (a.num_samples + (uint64_t)B - 1) / (uint64_t)B;
  a.B = B; a.rank = rank; a.world = world; a.flags = flags;
  a.half_bits = 1;
  while (((uint64_t)1 << (2 * a.half_bits)) < a.n) ++a.half_bits;           // at most 16: n < 2^31 <= 2^32
  sample_batch_kernel<<<dim3(1), dim3(SAMPLER_THREADS), 0, (hipStream_t)stream>>>(a);
  SAM_LAUNCH_CHECK();
  return SAM_OK;
}

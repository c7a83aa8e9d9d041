"""Each step's sample indices drawn on the device: shuffled, sharded epochs from a resident state.

The reference draws its batches with RandomSampler / DistributedSampler (sam/task_utils.py:138-166): torch.randperm(n) on the host, a slice per step and
a copy of int32 [B].  Here the record of where training is in its epoch is four int64 words in device memory,

    state = {seed, epoch, step_in_epoch, batches_drawn}

and one launch (ops.sample_batch, csrc/sampler.hip) reads it, writes this rank's sample_idx int32 [B] and valid int32 [B], and advances it.  The
semantics are DistributedSampler's: shuffle per epoch, pad by wrapping to a multiple of the world size, rank r takes every world-th position; world = 1
is a RandomSampler.  The shuffle is perm(seed, epoch, n), a keyed bijection on [0, n) evaluated per element: a balanced Feistel network on the smallest
even bit width 2k with 2^(2k) >= n, followed by a keyed swap of the values 0 and 1 (the network alone is always an even permutation of its domain,
which would leave the even orderings of a small n likelier than the odd ones), cycle-walked back into [0, n).  There is no permutation array.  The
order is this project's own (as its dropout streams are), not torch.randperm's.

This file is the definition: perm / perm_at / batch_host are the host twin the kernel equals bit for bit.  store.gather(s, sample_idx, into) consumes
the indices unchanged; a slot past the shard's end (valid 0) holds an in-range index like any other and the consumer weights it by `valid`."""
import numpy as np
import torch

from .wordindex import mix32 as _mix32

ROUNDS = 8                                      # Feistel rounds (csrc/sampler.hip: SAMPLER_ROUNDS)
DOMAIN = 0x53414D50                             # the key chain's own constant
ROUND_STEP = 0x9E3779B1
SHUFFLE, DROP_LAST, DROP_LAST_BATCH, PEEK = 1, 2, 4, 8          # flags of sam_sample_batch
BAD_STATE = 2                                   # status bit 1 (include/sam_hip_sampler.h); bit 0 is not used
STATE_KEYS = ("seed", "epoch", "step_in_epoch", "batches_drawn")
_CONFIG_KEYS = ("n", "batch_size", "rank", "world", "shuffle", "drop_last", "drop_last_batch")
_M64 = (1 << 64) - 1


def half_bits(n):
    """k: the Feistel network permutes [0, 2^(2k)), the smallest even width (at least 2 bits) that holds n; 2^(2k) < 4n for n >= 2"""
    k = 1
    while (1 << (2 * k)) < n:
        k += 1
    return k


def round_keys(seed, epoch):
    """the ROUNDS round keys of (seed, epoch) and one more word (its lowest bit is the parity swap of perm_at): mix32 chained over the seed's and the
    epoch's 32-bit halves (two's complement), then the round number"""
    u = np.uint32
    seed, epoch = int(seed) & _M64, int(epoch) & _M64
    with np.errstate(over="ignore"):
        h = _mix32(u((seed & 0xFFFFFFFF) ^ DOMAIN))
        h = _mix32(h ^ u(seed >> 32))
        h = _mix32(h ^ u(epoch & 0xFFFFFFFF))
        h = _mix32(h ^ u(epoch >> 32))
        return [_mix32(h ^ u(((r + 1) * ROUND_STEP) & 0xFFFFFFFF)) for r in range(ROUNDS + 1)]


def perm_at(seed, epoch, n, p):
    """perm(seed, epoch, n) at the positions p (integers in [0, n)) -> int64 array of p's shape.  The walk needs no iteration cap: the network is a
    permutation of [0, 2^(2k)), so the cycle through p comes back to p < n, and a value below n is met at the latest there."""
    n = int(n)
    if not 1 <= n < 1 << 31:
        raise ValueError("sampler: n = %d (need 1 <= n < 2^31)" % n)
    p = np.asarray(p, dtype=np.int64)
    if p.size and (int(p.min()) < 0 or int(p.max()) >= n):
        raise ValueError("sampler: a position outside [0, %d)" % n)
    if n == 1:
        return np.zeros(p.shape, np.int64)
    k, keys = half_bits(n), round_keys(seed, epoch)
    ku, mask, top = np.uint32(k), np.uint32((1 << k) - 1), np.uint32(32 - k)
    swap = keys.pop() & np.uint32(1)
    x = p.astype(np.uint32).reshape(-1)
    todo = np.arange(x.size)
    with np.errstate(over="ignore"):
        while todo.size:
            v = x[todo]
            l, r = v >> ku, v & mask
            for key in keys:
                l, r = r, l ^ (_mix32(r ^ key) >> top)
            v = (l << ku) | r
            v = v ^ ((v < 2) * swap).astype(np.uint32)          # the parity swap: values 0 and 1 change places when the key's bit is set
            x[todo] = v
            todo = todo[v.astype(np.int64) >= n]
    return x.astype(np.int64).reshape(p.shape)


def perm(seed, epoch, n):
    """the whole permutation of [0, n) of (seed, epoch), int64 [n]"""
    return perm_at(seed, epoch, n, np.arange(int(n), dtype=np.int64))


def plan(n, batch_size, rank=0, world=1, drop_last=False, drop_last_batch=False):
    """(num_samples, steps_per_epoch) of a shard; ValueError for what sam_sample_batch refuses"""
    n, B, rank, world = int(n), int(batch_size), int(rank), int(world)
    if not 1 <= n < 1 << 31:
        raise ValueError("sampler: n = %d (need 1 <= n < 2^31)" % n)
    if B < 1:
        raise ValueError("sampler: batch_size = %d (need >= 1)" % B)
    if world < 1 or not 0 <= rank < world:
        raise ValueError("sampler: rank %d of world %d (need world >= 1 and 0 <= rank < world)" % (rank, world))
    if drop_last and n < world:
        raise ValueError("sampler: drop_last with n = %d < world = %d leaves no sample" % (n, world))
    num_samples = n // world if drop_last else -(-n // world)
    if drop_last_batch and num_samples < B:
        raise ValueError("sampler: drop_last_batch with num_samples = %d < batch_size = %d leaves no batch" % (num_samples, B))
    return num_samples, (num_samples // B if drop_last_batch else -(-num_samples // B))


def flags_of(shuffle=True, drop_last=False, drop_last_batch=False, peek=False):
    return (SHUFFLE if shuffle else 0) | (DROP_LAST if drop_last else 0) | (DROP_LAST_BATCH if drop_last_batch else 0) | (PEEK if peek else 0)


def batch_host(state, n, B, rank=0, world=1, shuffle=True, drop_last=False, drop_last_batch=False):
    """the host twin of one launch, and its specification: state = (seed, epoch, step_in_epoch, batches_drawn) as integers
    -> (sample_idx int32 [B], valid int32 [B], new_state).  A state the kernel flags (epoch < 0, step < 0, step >= steps_per_epoch) raises ValueError."""
    seed, epoch, step, drawn = (int(v) for v in state)
    n, B, rank, world = int(n), int(B), int(rank), int(world)
    num_samples, steps = plan(n, B, rank, world, drop_last, drop_last_batch)
    if epoch < 0 or step < 0 or step >= steps:
        raise ValueError("sampler: bad state epoch = %d, step_in_epoch = %d (%d steps per epoch)" % (epoch, step, steps))
    j = step * B + np.arange(B, dtype=np.int64)                 # Python / int64: j < 2^32, j * world + rank < 2^63
    m = (j * world + rank) % n
    idx = perm_at(seed, epoch, n, m) if shuffle else m
    last = step + 1 == steps
    return idx.astype(np.int32), (j < num_samples).astype(np.int32), (seed, epoch + 1 if last else epoch, 0 if last else step + 1, drawn + 1)


class Sampler:
    """The resident sampler of one rank.  next() is one launch: it takes no host-side value per call, allocates nothing when `out` is given and never
    synchronises.  The four state integers are read back only by state_dict() (and status() reads the status word)."""

    def __init__(self, n, batch_size, seed=0, rank=0, world=1, shuffle=True, drop_last=False, drop_last_batch=False, device="cuda"):
        self.n, self.batch_size, self.rank, self.world = int(n), int(batch_size), int(rank), int(world)
        self.shuffle, self.drop_last, self.drop_last_batch = bool(shuffle), bool(drop_last), bool(drop_last_batch)
        self.num_samples, self.steps_per_epoch = plan(self.n, self.batch_size, self.rank, self.world, self.drop_last, self.drop_last_batch)
        self.flags = flags_of(self.shuffle, self.drop_last, self.drop_last_batch)
        seed = int(seed)
        if not -(1 << 63) <= seed < 1 << 63:
            raise ValueError("sampler: the seed must fit an int64")
        self.device = torch.device(device)
        self.state = torch.tensor([seed, 0, 0, 0], dtype=torch.int64).to(self.device)
        self._status = torch.zeros(1, dtype=torch.int32, device=self.device)

    def _out(self, out):
        if out is None:
            return (torch.empty(self.batch_size, dtype=torch.int32, device=self.device), torch.empty(self.batch_size, dtype=torch.int32, device=self.device))
        idx, valid = out
        if idx.numel() != self.batch_size or valid.numel() != self.batch_size:
            raise ValueError("sampler: out must be (sample_idx, valid), int32 [%d] each" % self.batch_size)
        return idx, valid

    def _draw(self, out, flags):
        from . import ops
        idx, valid = self._out(out)
        ops.sample_batch(self.state, self.n, self.rank, self.world, flags, idx, valid, self._status)
        return idx, valid

    def next(self, out=None):
        """-> (sample_idx int32 [B], valid int32 [B]) of this rank's next batch, written into `out` when given; advances the resident state"""
        return self._draw(out, self.flags)

    def peek(self, out=None):
        """the batch next() would return, with the state left as it is"""
        return self._draw(out, self.flags | PEEK)

    def seek(self, epoch, step=0):
        """continue at batch `step` of `epoch` (host values: a copy of two words; batches_drawn stays)"""
        epoch, step = int(epoch), int(step)
        if epoch < 0 or not 0 <= step < self.steps_per_epoch:
            raise ValueError("sampler: seek(%d, %d) outside epoch >= 0, 0 <= step < %d" % (epoch, step, self.steps_per_epoch))
        self.state[1:3].copy_(torch.tensor([epoch, step], dtype=torch.int64))

    def status(self, check=True):
        """the status word (read back: synchronises).  check=True raises ValueError naming the bit"""
        st = int(self._status.item())
        if check and st:
            raise ValueError("sampler: status %d: %s" % (st, "bit 1: bad state (epoch < 0, step_in_epoch < 0 or step_in_epoch >= %d): nothing was drawn"
                                                         % self.steps_per_epoch if st & BAD_STATE else "unknown bits"))
        return st

    def state_dict(self):
        """the four state integers (read back here and nowhere else) and the constructor's arguments"""
        d = dict(zip(STATE_KEYS, self.state.tolist()))
        d.update({k: getattr(self, k) for k in _CONFIG_KEYS})
        return d

    def load_state_dict(self, d):
        """resume at the exact sample: ValueError when the shard the state was saved for is not this one, or the state is out of range"""
        for k in _CONFIG_KEYS:
            if k not in d or d[k] != getattr(self, k):
                raise ValueError("sampler: the saved state has %s = %r, this sampler %r" % (k, d.get(k), getattr(self, k)))
        vals = [int(d[k]) for k in STATE_KEYS]
        if vals[1] < 0 or not 0 <= vals[2] < self.steps_per_epoch:
            raise ValueError("sampler: the saved state has epoch = %d, step_in_epoch = %d (%d steps per epoch)" % (vals[1], vals[2], self.steps_per_epoch))
        self.state.copy_(torch.tensor(vals, dtype=torch.int64))


def for_store(s, batch_size, **kw):
    """a Sampler over the questions of a store (store.build / store.to); the device defaults to the store's"""
    kw.setdefault("device", s["obj"]["row_off"].device)
    return Sampler(s["n_questions"], batch_size, **kw)

"""CPU: the resident sampler (sam_textvqa_amd/sampler.py) without a GPU -- the definition the kernel is compared against: the
keyed bijection, DistributedSampler's structure with and without shuffle, the quality conditions on fixed seeds, the state machine, the header registry
and the entry point's argument checks."""
import ctypes
import itertools
import math
import os

import numpy as np
import pytest
import torch

BIJECTION_N = (1, 2, 3, 4, 5, 15, 16, 17, 63, 64, 65, 255, 256, 257, 1000, 4097, 65537)
SEEDS = (0, 1, -1, 0x123456789ABCDEF, 1 << 40)              # both halves of the seed matter; a negative seed is its two's complement
EPOCHS = (0, 1, 7, 1 << 33)
QUALITY_SEED = 0
Z999 = 3.0902323061678                                      # the 0.999 quantile of the standard normal


def chi2_q999(df):
    """the 0.999 quantile of chi-square with df degrees of freedom (Wilson-Hilferty; 0.4 % above the exact 39.25 at df = 16, within 0.03 % of 172.42
    and 331.66 at df = 119 and 256)"""
    return df * (1.0 - 2.0 / (9.0 * df) + Z999 * math.sqrt(2.0 / (9.0 * df))) ** 3


def _epoch(n, B, W, r, seed=0, epoch=0, drawn=0, **kw):
    """a whole epoch of one rank through batch_host -> (indices of the valid slots, all indices, all valid flags, the state after it)"""
    from sam_textvqa_amd import sampler as S
    _, steps = S.plan(n, B, r, W, kw.get("drop_last", False), kw.get("drop_last_batch", False))
    state, idx, valid = (seed, epoch, 0, drawn), [], []
    for t in range(steps):
        i, v, state = S.batch_host(state, n, B, r, W, **kw)
        assert i.dtype == np.int32 and v.dtype == np.int32 and i.shape == (B,) and v.shape == (B,)
        assert state[2] == (t + 1) % steps and state[3] == drawn + t + 1
        idx.append(i)
        valid.append(v)
    idx, valid = np.concatenate(idx), np.concatenate(valid)
    assert idx.min() >= 0 and idx.max() < n                                     # the invalid slots too
    return idx[valid == 1], idx, valid, state


# ---------------------------------------------------------------------------------------------- the keyed bijection
@pytest.mark.parametrize("n", BIJECTION_N)
def test_perm_is_a_bijection(n):
    from sam_textvqa_amd import sampler as S
    assert 1 << (2 * S.half_bits(n)) >= n and (n <= 4 or 1 << (2 * S.half_bits(n)) < 4 * n)
    pairs = list(itertools.product(SEEDS, EPOCHS)) if n <= 4097 else [(0, 0), (-1, 1 << 33)]
    for seed, epoch in pairs:
        p = S.perm(seed, epoch, n)
        assert p.dtype == np.int64 and p.shape == (n,)
        assert np.array_equal(np.sort(p), np.arange(n)), (seed, epoch)
        at = np.array([n - 1, 0, n // 2, 0])
        assert np.array_equal(S.perm_at(seed, epoch, n, at), p[at])                 # evaluated per element, in any order, repeats included
    assert S.perm(3, 0, 1).tolist() == [0]


def test_perm_at_the_largest_n_stays_in_range_and_is_injective_on_a_sample():
    from sam_textvqa_amd import sampler as S
    n = (1 << 31) - 1
    assert S.half_bits(n) == 16 and S.half_bits(1 << 30) == 15 and S.half_bits((1 << 30) + 1) == 16
    at = np.concatenate([np.arange(2000), n - 1 - np.arange(2000), np.arange(1 << 19, n - (1 << 19), 1 << 19)])
    p = S.perm_at(5, 2, n, at)
    assert p.min() >= 0 and p.max() < n and len(set(p.tolist())) == len(at)
    for bad in (0, 1 << 31):
        with pytest.raises(ValueError):
            S.perm_at(0, 0, bad, [0])
    with pytest.raises(ValueError):
        S.perm_at(0, 0, 5, [5])


def test_perm_depends_on_seed_and_epoch_and_on_nothing_else():
    from sam_textvqa_amd import sampler as S
    for n in (5, 17, 64, 1000):
        seen = {}
        for seed, epoch in itertools.product(SEEDS, EPOCHS):
            p = S.perm(seed, epoch, n)
            assert np.array_equal(p, S.perm(seed, epoch, n))
            seen[(seed, epoch)] = tuple(p)
        if n >= 17:                                             # 20 draws from n! orderings: all distinct (at n = 5, 120 orderings, repeats are expected)
            assert len(set(seen.values())) == len(seen)
    # n = 5: consecutive epochs and neighbouring seeds still differ somewhere
    assert len({tuple(S.perm(0, e, 5)) for e in range(12)}) > 6 and len({tuple(S.perm(s, 0, 5)) for s in range(12)}) > 6
    # every word of the key chain matters: the seed's high half, the epoch's high half
    assert not np.array_equal(S.perm(1, 0, 1000), S.perm(1 | 1 << 32, 0, 1000)) and not np.array_equal(S.perm(1, 1, 1000), S.perm(1, 1 | 1 << 32, 1000))
    assert len(S.round_keys(0, 0)) == S.ROUNDS + 1 and S.ROUNDS >= 6


# ---------------------------------------------------------------------------------------------- DistributedSampler's structure
@pytest.mark.parametrize("W", [1, 2, 3, 8])
@pytest.mark.parametrize("n", [1, 5, 17, 64, 1000])
def test_without_shuffle_an_epoch_is_distributed_samplers_list(n, W):
    from torch.utils.data import DistributedSampler
    for drop_last in (False, True):
        for B in sorted({1, 4, 64 if n >= 64 else 3}):          # n < W * B at every n for some B; n < W at n = 1, 5
            for r in range(W):
                want = list(DistributedSampler(range(n), num_replicas=W, rank=r, shuffle=False, drop_last=drop_last))
                if drop_last and n < W:                          # torch yields an empty shard; the launch refuses the shape
                    assert want == []
                    with pytest.raises(ValueError, match="leaves no sample"):
                        _epoch(n, B, W, r, shuffle=False, drop_last=True)
                    continue
                got, _, valid, _ = _epoch(n, B, W, r, shuffle=False, drop_last=drop_last)
                assert got.tolist() == want, (n, W, r, B, drop_last)
                assert valid.tolist() == [1] * len(want) + [0] * (len(valid) - len(want)) and len(valid) - len(want) < B


@pytest.mark.parametrize("W", [1, 2, 3, 8])
@pytest.mark.parametrize("n", [1, 5, 17, 64, 1000])
def test_with_shuffle_the_ranks_valid_slots_are_perm_padded_by_wrapping(n, W):
    from sam_textvqa_amd import sampler as S
    seed, epoch, B = 11, 3, 4
    p = S.perm(seed, epoch, n)
    for drop_last in (False, True):
        if drop_last and n < W:
            continue
        ns, _ = S.plan(n, B, 0, W, drop_last)
        shards = [_epoch(n, B, W, r, seed=seed, epoch=epoch, shuffle=True, drop_last=drop_last)[0] for r in range(W)]
        assert all(len(s) == ns for s in shards)
        merged = np.stack(shards, 1).reshape(-1)                # position j * W + r
        assert np.array_equal(merged, p[np.arange(ns * W) % n])
        counts = np.bincount(merged, minlength=n)
        if not drop_last:
            pad = ns * W - n
            assert 0 <= pad < W and counts.min() >= 1 and counts.max() - counts.min() <= pad and counts.sum() == n + pad
        else:
            assert counts.max() == 1 and counts.sum() == ns * W > n - W
        if W == 1:
            assert np.array_equal(merged, p)                    # a RandomSampler: exactly a permutation
    # the invalid slots of the last batch go on in the same sequence
    _, idx, valid, _ = _epoch(17, 4, 3, 2, seed=seed, epoch=epoch, shuffle=True)
    assert valid.tolist() == [1] * 6 + [0] * 2 and np.array_equal(idx, S.perm(seed, epoch, 17)[(np.arange(8) * 3 + 2) % 17])


# ---------------------------------------------------------------------------------------------- quality: conditions on fixed seeds, not measurements
@pytest.fixture(scope="module")
def perms_small():
    from sam_textvqa_amd import sampler as S
    return {n: np.stack([S.perm(QUALITY_SEED, e, n) for e in range(4000)]) for n in (5, 17)}


@pytest.mark.parametrize("n", [5, 17])
def test_position_by_value_table_is_uniform(perms_small, n):
    """4000 epochs: the n x n table of (position, value) counts against 4000 / n each.  Rows and columns both sum to 4000, so the table has (n - 1)^2
    degrees of freedom.  For uniform permutations the plain Pearson sum used here is n / (n - 1) times a chi-square variable of that many degrees
    (its mean is n (n - 1), not (n - 1)^2), so holding it below the chi-square quantile is stricter than the nominal 0.999."""
    P = perms_small[n]
    table = np.zeros((n, n))
    for pos in range(n):
        table[pos] = np.bincount(P[:, pos], minlength=n)
    expect = len(P) / n
    chi2 = float(((table - expect) ** 2 / expect).sum())
    print("n = %d: chi-square %.1f, bound %.1f at %d degrees of freedom" % (n, chi2, chi2_q999((n - 1) ** 2), (n - 1) ** 2))
    assert chi2 < chi2_q999((n - 1) ** 2)


def test_all_120_orderings_of_five_are_reached_uniformly(perms_small):
    """The network alone is an even permutation of its 16 values, which would leave the 60 even orderings of n = 5 likelier than the 60 odd ones by
    1/12; with the keyed swap both parities are drawn and the reachable set is all 120."""
    P = perms_small[5]
    code = (P * 5 ** np.arange(5)).sum(1)
    _, counts = np.unique(code, return_counts=True)
    assert len(counts) == 120
    expect = len(P) / 120
    chi2 = float(((counts - expect) ** 2 / expect).sum())
    sign = np.array([(-1) ** sum(p[i] > p[j] for i in range(5) for j in range(i + 1, 5)) for p in P])
    even = int((sign == 1).sum())
    print("orderings: chi-square %.1f, bound %.1f at 119 degrees of freedom; %d even of %d" % (chi2, chi2_q999(119), even, len(P)))
    assert chi2 < chi2_q999(119)
    assert abs(even - len(P) / 2) < 3.2905 * math.sqrt(len(P)) / 2          # two-sided 0.999 of a fair coin (104 of 4000); without the swap the excess is 1/24 of the draws (167)


def test_consecutive_epochs_are_uncorrelated_in_rank():
    """n = 1000, 50 epochs, 49 consecutive pairs: under independence Spearman's rho is near N(0, 1 / (n - 1)), so |rho| has mean sqrt(2 / pi) sigma and
    variance (1 - 2 / pi) sigma^2, and the mean of 49 of them is near normal."""
    from sam_textvqa_amd import sampler as S
    n = 1000
    P = np.stack([S.perm(QUALITY_SEED, e, n) for e in range(50)]).astype(np.float64)
    P -= (n - 1) / 2.0
    rho = np.abs((P[:-1] * P[1:]).sum(1) / (P[0] ** 2).sum())
    sigma = 1.0 / math.sqrt(n - 1)
    bound = math.sqrt(2 / math.pi) * sigma + Z999 * math.sqrt((1 - 2 / math.pi) / len(rho)) * sigma
    print("mean |rho| %.5f over %d pairs, bound %.5f" % (rho.mean(), len(rho), bound))
    assert len(rho) == 49 and rho.mean() < bound


# ---------------------------------------------------------------------------------------------- the state machine
def test_steps_per_epoch_and_what_plan_refuses():
    from sam_textvqa_amd import sampler as S
    assert S.plan(23, 4) == (23, 6) and S.plan(23, 4, drop_last_batch=True) == (23, 5)
    assert S.plan(23, 4, 1, 2) == (12, 3) and S.plan(23, 4, 1, 2, drop_last=True) == (11, 3) and S.plan(23, 4, 1, 2, drop_last=True, drop_last_batch=True) == (11, 2)
    assert S.plan(24, 4, 0, 2, drop_last=True, drop_last_batch=True) == (12, 3) and S.plan(1, 64, 7, 8) == (1, 1)
    assert S.plan(35000, 64) == (35000, 547) and S.plan((1 << 31) - 1, 64, 7, 8) == (1 << 28, 1 << 22)
    for kw in (dict(n=0), dict(n=1 << 31), dict(batch_size=0), dict(world=0), dict(rank=2, world=2), dict(rank=-1), dict(n=3, world=4, rank=0, drop_last=True),
               dict(n=23, world=2, batch_size=12, drop_last=True, drop_last_batch=True)):
        args = dict(n=23, batch_size=4)
        args.update(kw)
        with pytest.raises(ValueError):
            S.plan(**args)
    assert S.flags_of() == 1 and S.flags_of(False, True, True, True) == 14 and (S.SHUFFLE, S.DROP_LAST, S.DROP_LAST_BATCH, S.PEEK, S.BAD_STATE) == (1, 2, 4, 8, 2)


def test_batch_host_rolls_over_into_the_next_epoch():
    from sam_textvqa_amd import sampler as S
    n, B = 23, 4
    state = (9, 0, 0, 0)
    for t in range(13):
        i, v, new = S.batch_host(state, n, B)
        epoch, step = divmod(t, 6)
        assert state == (9, epoch, step, t) and new == (9, (t + 1) // 6, (t + 1) % 6, t + 1)
        want = S.perm(9, epoch, n)[(step * B + np.arange(B)) % n]
        assert np.array_equal(i, want) and v.tolist() == [int(step * B + k < n) for k in range(B)]
        state = new
    assert S.batch_host((9, 1, 4, 0), n, B, drop_last_batch=True)[2] == (9, 2, 0, 1)
    for bad in ((9, -1, 0, 0), (9, 0, -1, 0), (9, 0, 6, 0)):
        with pytest.raises(ValueError, match="bad state"):
            S.batch_host(bad, n, B)
    with pytest.raises(ValueError, match="bad state"):
        S.batch_host((9, 0, 5, 0), n, B, drop_last_batch=True)


def test_sampler_object_seek_state_dict_and_mismatched_load():
    from sam_textvqa_amd import _capi
    from sam_textvqa_amd import sampler as S
    a = S.Sampler(23, 4, seed=5, rank=1, world=2, device="cpu")
    assert a.steps_per_epoch == 3 and a.num_samples == 12 and a.state.dtype == torch.int64 and a.state.tolist() == [5, 0, 0, 0]
    assert S.Sampler(23, 4, rank=1, world=2, drop_last=True, drop_last_batch=True, device="cpu").steps_per_epoch == 2
    a.seek(4, 2)
    d = a.state_dict()
    assert d == dict(seed=5, epoch=4, step_in_epoch=2, batches_drawn=0, n=23, batch_size=4, rank=1, world=2, shuffle=True, drop_last=False, drop_last_batch=False)
    b = S.Sampler(23, 4, seed=77, rank=1, world=2, device="cpu")
    b.load_state_dict(d)
    assert b.state.tolist() == [5, 4, 2, 0] and b.state_dict() == d
    for kw in (dict(n=24), dict(batch_size=5), dict(rank=0), dict(world=3, rank=1), dict(shuffle=False), dict(drop_last=True), dict(drop_last_batch=True)):
        args = dict(n=23, batch_size=4, rank=1, world=2)
        args.update(kw)
        other = S.Sampler(device="cpu", **args)
        with pytest.raises(ValueError, match="saved state"):
            other.load_state_dict(d)
        assert other.state.tolist() == [0, 0, 0, 0]
    for bad in (dict(d, epoch=-1), dict(d, step_in_epoch=3)):
        with pytest.raises(ValueError, match="saved state"):
            b.load_state_dict(bad)
    for e, t in ((-1, 0), (0, 3), (0, -1)):
        with pytest.raises(ValueError, match="seek"):
            a.seek(e, t)
    assert a.state.tolist() == [5, 4, 2, 0] and a.status() == 0
    with pytest.raises(ValueError):
        S.Sampler(23, 4, rank=2, world=2, device="cpu")
    with pytest.raises(_capi.SamHipError):                      # the draw has no CPU path: batch_host is the twin, not a fallback
        a.next()
    s = {"n_questions": 23, "obj": {"row_off": torch.zeros(8, dtype=torch.int64)}}
    f = S.for_store(s, 4, seed=3, rank=1, world=2)
    assert (f.n, f.batch_size, f.rank, f.world, f.device.type, f.state.tolist()) == (23, 4, 1, 2, "cpu", [3, 0, 0, 0])


# ---------------------------------------------------------------------------------------------- registry and C ABI
def test_the_header_parses_into_the_open_table_and_the_library_holds_the_kernel():
    from sam_textvqa_amd import _build, _capi
    vp, i, i64 = ctypes.c_void_p, ctypes.c_int, ctypes.c_int64
    assert "sampler" in _build.ABI_ADDITIONS and _build.ABI_ADDITIONS["sampler"] in _build.public_headers()
    assert _capi.ADDITION_SIGNATURES["sampler"] == {"sam_sample_batch": [vp, i64, i, i, i, i, vp, vp, vp, vp]}
    assert _capi.ADDITION_RESTYPES["sampler"] == {"sam_sample_batch": i}
    assert "sam_sample_batch" not in open(_build.ABI_ADDITIONS["store"]).read()
    assert os.path.join(_build.CSRC, "sampler.hip") in _build.sources()
    lib = _capi.lib()                                           # builds sampler.hip for gfx950 with the rest when the tree changed
    assert lib.sam_build_digest().decode() == _build._digest()
    assert lib.sam_sample_batch.argtypes == _capi.ADDITION_SIGNATURES["sampler"]["sam_sample_batch"] and lib.sam_sample_batch.restype is i


def test_entry_point_rejects_bad_arguments_without_a_gpu():
    from sam_textvqa_amd import _capi, ops
    fake = 1 << 20                                              # never dereferenced: the checks reject the call before any launch

    def call(state=fake, n=23, b=4, rank=0, world=1, flags=1, idx=fake, valid=fake, status=fake):
        return _capi.call("sam_sample_batch", state, n, b, rank, world, flags, idx, valid, status, None)

    for kw in (dict(state=None), dict(idx=None), dict(valid=None), dict(status=None)):
        with pytest.raises(_capi.SamHipError, match="null pointer"):
            call(**kw)
    for kw in (dict(state=fake + 4), dict(idx=fake + 2)):
        with pytest.raises(_capi.SamHipError, match="misaligned"):
            call(**kw)
    for n in (0, -1, 1 << 31, 1 << 40):
        with pytest.raises(_capi.SamHipError, match="bad size"):
            call(n=n)
    for b in (0, -3):
        with pytest.raises(_capi.SamHipError, match="bad shape"):
            call(b=b)
    for kw in (dict(world=0), dict(rank=-1), dict(rank=1), dict(rank=2, world=2)):
        with pytest.raises(_capi.SamHipError, match="bad shard"):
            call(**kw)
    for flags in (16, 1 | 32, -1):
        with pytest.raises(_capi.SamHipError, match="unknown flag bits"):
            call(flags=flags)
    with pytest.raises(_capi.SamHipError, match="leaves no sample"):
        call(n=3, world=4, flags=1 | 2)
    with pytest.raises(_capi.SamHipError, match="leaves no batch") as e:
        call(n=23, world=2, b=12, flags=1 | 2 | 4)
    assert "rc=-1" in str(e.value)                              # SAM_ERR_ARG
    with pytest.raises(_capi.SamHipError, match="leaves no batch"):
        call(n=23, b=24, flags=4)
    # the Python wrapper: CPU tensors are refused, there is no fallback
    with pytest.raises(_capi.SamHipError):
        ops.sample_batch(torch.zeros(4, dtype=torch.int64), 23, 0, 1, 1, torch.zeros(4, dtype=torch.int32), torch.zeros(4, dtype=torch.int32), torch.zeros(1, dtype=torch.int32))

"""GPU: the resident sampler (csrc/sampler.hip, sam_textvqa_amd/sampler.py) on the MI355X -- the launch against the host twin
sampler.batch_host bit for bit (which tests/test_sampler_cpu.py judges), drawn from device state alone across epoch boundaries, the 64-bit positions,
peek, states out of range, resuming, and an epoch of two ranks through store.gather.  No test captures a graph."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

GRID_N = (1, 2, 3, 5, 17, 64, 65, 257, 1000, 65537)
GRID_B = (1, 3, 64, 257)                                    # 257: more than one pass of the 256 threads, and no multiple of 64
GRID_SHARDS = ((1, 0), (2, 1), (3, 2), (8, 7))
MAX_STEPS = 48                                              # the pruning rule: shapes whose epoch is longer are left out (2 * steps + 1 launches each)
SENTINEL = 0x5A5A5A5A


def _grid(W, r):
    """(n, B, flags) of this shard: every flag combination the shape allows, epochs of at most MAX_STEPS batches"""
    from sam_textvqa_amd import sampler as S
    out = []
    for n in GRID_N:
        for B in GRID_B:
            for flags in range(8):
                try:
                    _, steps = S.plan(n, B, r, W, bool(flags & S.DROP_LAST), bool(flags & S.DROP_LAST_BATCH))
                except ValueError:
                    continue
                if steps <= MAX_STEPS:
                    out.append((n, B, flags, steps))
    return out


def test_the_pruned_grid_keeps_every_n_every_b_and_every_flag_combination():
    cases = [c + (W,) for W, r in GRID_SHARDS for c in _grid(W, r)]
    assert {c[0] for c in cases} == set(GRID_N) and {c[1] for c in cases} == set(GRID_B) and {c[2] for c in cases} == set(range(8))
    assert {(c[0], c[4]) for c in cases} >= {(n, 8) for n in GRID_N}                 # n < W and n < W * B are in
    assert any(c[1] == 257 and c[3] > 1 for c in cases) and sum(2 * c[3] + 1 for c in cases) < 20000


def _draw_log(smp, calls):
    """`calls` consecutive next() with nothing but device state between them -> (idx [calls, B], valid [calls, B], state after each [calls, 4]) on the CPU"""
    B = smp.batch_size
    idx = torch.full((calls, B), SENTINEL, dtype=torch.int32, device="cuda")
    valid = torch.full((calls, B), SENTINEL, dtype=torch.int32, device="cuda")
    states = torch.empty((calls, 4), dtype=torch.int64, device="cuda")
    for c in range(calls):
        got = smp.next(out=(idx[c], valid[c]))
        assert got[0].data_ptr() == idx[c].data_ptr()
        states[c].copy_(smp.state)
    return idx.cpu().numpy(), valid.cpu().numpy(), states.cpu().tolist()


def _twin_log(state, calls, n, B, r, W, flags):
    from sam_textvqa_amd import sampler as S
    idx, valid, states = [], [], []
    for _ in range(calls):
        i, v, state = S.batch_host(state, n, B, r, W, bool(flags & S.SHUFFLE), bool(flags & S.DROP_LAST), bool(flags & S.DROP_LAST_BATCH))
        idx.append(i)
        valid.append(v)
        states.append(list(state))
    return np.stack(idx), np.stack(valid), states


@pytest.mark.parametrize("W,r", GRID_SHARDS)
def test_batches_and_state_equal_the_twin_across_the_epoch_boundary(W, r):
    from sam_textvqa_amd import sampler as S
    for k, (n, B, flags, steps) in enumerate(_grid(W, r)):
        seed = (-3, 0, 1 << 40 | 7, 12345)[k % 4]
        smp = S.Sampler(n, B, seed=seed, rank=r, world=W, shuffle=bool(flags & S.SHUFFLE), drop_last=bool(flags & S.DROP_LAST),
                        drop_last_batch=bool(flags & S.DROP_LAST_BATCH))
        assert smp.steps_per_epoch == steps and smp.state.is_cuda
        calls = 2 * steps + 1
        idx, valid, states = _draw_log(smp, calls)
        w_idx, w_valid, w_states = _twin_log((seed, 0, 0, 0), calls, n, B, r, W, flags)
        where = (n, B, W, r, flags)
        assert np.array_equal(idx, w_idx), where
        assert np.array_equal(valid, w_valid), where
        assert states == w_states and states[-1] == [seed, calls // steps, calls % steps, calls], where
        assert smp.status() == 0


@pytest.mark.parametrize("W,r,B,step,reach", [(8, 7, 64, (1 << 22) - 1, (1 << 31) - 1), (1 << 24, (1 << 24) - 1, 257, 0, (1 << 32) + 1)],
                         ids=["issue-shape-last-step", "positions-past-2^32"])
def test_largest_n_takes_the_64_bit_path(W, r, B, step, reach):
    """n = 2^31 - 1.  With W = 8 and B = 64 a position j * W + r stays below n + W * B whatever the step (an epoch ends there), so it cannot pass 2^32:
    the last step of the epoch takes it to 2^31 - 1, past what signed 32-bit arithmetic holds, and there the padding wraps.  The second shape does
    pass 2^32: the 257 slots of rank 2^24 - 1 in a world of 2^24 reach position 256 * 2^24 + 2^24 - 1 (the slots from the 128th on are invalid and
    still hold an in-range index)."""
    from sam_textvqa_amd import sampler as S
    n = (1 << 31) - 1
    assert ((step + 1) * B - 1) * W + r >= reach and step == S.plan(n, B, r, W)[1] - 1
    for shuffle in (True, False):
        smp = S.Sampler(n, B, seed=99, rank=r, world=W, shuffle=shuffle)
        smp.seek(5, step)
        idx, valid, states = _draw_log(smp, 1)
        w_idx, w_valid, w_states = _twin_log((99, 5, step, 0), 1, n, B, r, W, S.flags_of(shuffle))
        assert np.array_equal(idx, w_idx) and np.array_equal(valid, w_valid) and states == w_states == [[99, 6, 0, 1]]
        assert idx.min() >= 0 and smp.status() == 0
        if not shuffle:                                         # the positions in Python integers, whatever the twin's int64 arithmetic does
            assert idx[0].tolist() == [((step * B + i) * W + r) % n for i in range(B)]
            assert valid[0].tolist() == [int(step * B + i < -(-n // W)) for i in range(B)]


def test_peek_leaves_the_state_and_equals_the_following_draw():
    from sam_textvqa_amd import sampler as S
    smp = S.Sampler(65, 3, seed=4, rank=1, world=2)
    smp.seek(2, 9)
    before = smp.state.tolist()
    p_idx, p_valid = smp.peek()
    assert smp.state.tolist() == before == [4, 2, 9, 0]
    p2 = smp.peek(out=(torch.empty_like(p_idx), torch.empty_like(p_valid)))
    n_idx, n_valid = smp.next()
    assert torch.equal(p_idx, n_idx) and torch.equal(p_valid, n_valid) and torch.equal(p2[0], n_idx) and torch.equal(p2[1], n_valid)
    assert smp.state.tolist() == [4, 2, 10, 1]
    w_idx, w_valid, _ = S.batch_host(before, 65, 3, 1, 2)
    assert n_idx.cpu().tolist() == w_idx.tolist() and n_valid.cpu().tolist() == w_valid.tolist()
    smp.seek(2, 10)                                             # the last batch of the shard (33 samples, 11 steps): peek does not roll over either
    smp.peek()
    assert smp.state.tolist() == [4, 2, 10, 1]
    smp.next()
    assert smp.state.tolist() == [4, 3, 0, 2] and smp.status() == 0


@pytest.mark.parametrize("bad", [[7, -1, 0, 5], [7, 0, 6, 5], [7, 0, -2, 5], [7, -(1 << 62), 1 << 40, 5]],
                         ids=["negative-epoch", "step-at-steps-per-epoch", "negative-step", "far-out"])
def test_a_state_out_of_range_is_flagged_and_nothing_moves(bad):
    from sam_textvqa_amd import sampler as S
    smp = S.Sampler(23, 4, seed=7)                              # 6 steps per epoch
    good = smp.next()
    assert smp.status() == 0
    smp.state.copy_(torch.tensor(bad, dtype=torch.int64))       # written behind the object's back: device memory is not trusted
    idx = torch.full((4,), SENTINEL, dtype=torch.int32, device="cuda")
    valid = torch.full((4,), SENTINEL, dtype=torch.int32, device="cuda")
    for draw in (smp.next, smp.peek):
        idx.fill_(SENTINEL)
        valid.fill_(SENTINEL)
        draw(out=(idx, valid))
        assert idx.tolist() == [0] * 4 and valid.tolist() == [0] * 4 and smp.state.tolist() == bad
        assert smp.status(check=False) == S.BAD_STATE
    with pytest.raises(ValueError, match="bit 1: bad state"):
        smp.status()
    smp.seek(0, 0)                                              # the sampler goes on once the state is good; the status word is sticky
    again = smp.next()
    assert torch.equal(again[0], good[0]) and torch.equal(again[1], good[1]) and smp.status(check=False) == S.BAD_STATE


def test_same_arguments_same_sequence_and_a_loaded_state_continues_identically():
    from sam_textvqa_amd import sampler as S
    kw = dict(n=257, batch_size=64, seed=31, rank=2, world=3)
    a, b = S.Sampler(**kw), S.Sampler(**kw)                     # 86 samples per shard, 2 steps per epoch
    la, lb = _draw_log(a, 3), _draw_log(b, 3)
    assert np.array_equal(la[0], lb[0]) and np.array_equal(la[1], lb[1]) and la[2] == lb[2]
    d = a.state_dict()                                          # mid-epoch: epoch 1, step 1
    assert (d["epoch"], d["step_in_epoch"], d["batches_drawn"]) == (1, 1, 3)
    c = S.Sampler(**dict(kw, seed=0))
    c.load_state_dict(d)
    la, lc = _draw_log(a, 4), _draw_log(c, 4)
    assert np.array_equal(la[0], lc[0]) and np.array_equal(la[1], lc[1]) and la[2] == lc[2] and la[2][-1] == [31, 3, 1, 7]
    other = S.Sampler(**dict(kw, seed=32))
    assert not np.array_equal(_draw_log(other, 3)[0], lb[0])
    with pytest.raises(ValueError, match="saved state"):
        S.Sampler(**dict(kw, rank=1)).load_state_dict(d)


def _small_store():
    """7 images, 23 questions, rows of width 16, one question table"""
    from sam_textvqa_amd import store
    g = torch.Generator().manual_seed(5)
    obj_counts, ocr_counts = [0, 1, 4, 6, 2, 3, 5], [3, 0, 4, 5, 1, 2, 2]

    def group(counts):
        return store.build_group_from_rows([torch.randn(c, 16, generator=g) for c in counts], [torch.rand(c, 5, generator=g) for c in counts])

    ioq = torch.randint(0, 7, (23,), generator=g, dtype=torch.int32)
    return store.build(group(obj_counts), group(ocr_counts), question_tables={"question_indices": torch.randint(0, 30000, (23, 20), generator=g)},
                       image_of_question=ioq)


def test_an_epoch_of_two_ranks_through_the_store():
    from sam_textvqa_amd import sampler as S
    from sam_textvqa_amd import store
    s_host = _small_store()
    s_dev = store.to(s_host, "cuda")
    B, n_max = 4, 4
    shape, _ = store.gather_host(s_host, torch.zeros(B, dtype=torch.int32), max_obj_num=n_max, max_ocr_num=n_max)
    seen = []
    for r in range(2):
        smp = S.for_store(s_dev, B, seed=8, rank=r, world=2)
        assert smp.n == 23 and smp.steps_per_epoch == 3 and smp.state.is_cuda
        state = (8, 0, 0, 0)
        for _ in range(smp.steps_per_epoch):
            into_d = {k: torch.zeros_like(v, device="cuda") for k, v in shape.items()}
            into_h = {k: torch.zeros_like(v) for k, v in shape.items()}
            idx, valid = smp.next()
            store.gather(s_dev, idx, into_d, max_obj_num=n_max, max_ocr_num=n_max, check=True)
            w_idx, w_valid, state = S.batch_host(state, 23, B, r, 2)
            assert idx.cpu().tolist() == w_idx.tolist() and valid.cpu().tolist() == w_valid.tolist()
            store.gather_host(s_host, torch.from_numpy(w_idx), into=into_h, max_obj_num=n_max, max_ocr_num=n_max, check=True)
            assert set(into_d) == set(into_h)
            for k in into_h:
                assert torch.equal(into_d[k].cpu().view(-1).view(torch.uint8), into_h[k].view(-1).view(torch.uint8)), k
            seen += idx.cpu()[valid.cpu() == 1].tolist()
        assert smp.state.tolist() == [8, 1, 0, 3] and smp.status() == 0
    counts = np.bincount(seen, minlength=23)
    assert len(seen) == 24 and counts.min() == 1 and sorted(counts.tolist())[-2:] == [1, 2]       # all 23 questions, exactly the one padded repeat

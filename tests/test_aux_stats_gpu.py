"""GPU: the spatial aux heads' confusion counts (csrc/aux_stats.hip) on the MI355X -- constructed inputs with hand-computed tables,
exact equality with the twin on the dense launch's scores (both kernels compile aux_pair.h's pair_scores), the float64 host twin within the count of
near-ties, accumulation, the code histogram and the loss's pair count, peak memory and SAM4C.spatial_aux_stats.

Shapes: the counting tile is 64 j x 16 i.  n = 1, 17 (one past a row tile), 63 / 64 / 65 (around a wave of j), 150 (the c3 shape: 3 x 10 tiles per sample).
B = 3: sample 2 has no valid row; rows that are not valid hold NaN in O and D; codes run to 15 (above 12: class 0).

No test here captures a graph: the eval forward of the module test takes the eager decoding loop."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

FUSIONS = ("mul", "add")
NAN = float("nan")


def _case(n, seed, b=3, nan_rows=True):
    """CPU tensors: O, D, W, bias, codes (0..15), valid (about 70 % of the rows; the last sample of a B = 3 case has none)"""
    g = torch.Generator().manual_seed(seed)
    o, d = torch.randn(b, n, 32, generator=g), torch.randn(b, n, 32, generator=g)
    w, bias = torch.randn(12, 32, generator=g) * 0.2, torch.randn(12, generator=g) * 0.1
    codes = torch.randint(0, 16, (b, n, n), generator=g).to(torch.uint8)
    valid = (torch.rand(b, n, generator=g) < 0.7).to(torch.uint8)
    valid[0, 0] = 1
    if b == 3:
        valid[2] = 0
    if nan_rows:
        o[valid == 0] = NAN
        d[valid == 0] = NAN
    return o, d, w, bias, codes, valid


def _cuda(*ts):
    return [t.cuda() for t in ts]


def near_ties(s64, valid):
    """(L, K, pairs, delta) of float64 scores [B, n, n, 12]: delta = 1e-5 max|S| over the valid pairs; L = valid pairs whose winning margin -- the gap
    between the two largest of (0, S_0 .. S_11) -- is below delta; K = (valid pair, channel) entries with |S| < delta"""
    v = valid != 0
    s = s64[v.unsqueeze(2) & v.unsqueeze(1)]
    if s.numel() == 0:
        return 0, 0, 0, 0.0
    delta = 1e-5 * float(s.abs().max())
    top = torch.cat([torch.zeros(s.shape[0], 1, dtype=s.dtype), s], 1).topk(2, dim=1).values
    return int(((top[:, 0] - top[:, 1]) < delta).sum()), int((s.abs() < delta).sum()), s.shape[0], delta


# ---------------------------------------------------------------------------------------------- 1. constructed, exact
@pytest.mark.parametrize("fusion", FUSIONS)
def test_constructed_integer_scores_give_the_hand_computed_tables(fusion):
    """O rows one-hot at k_i = i mod 32, D all ones (mul) / zeros (add), W and bias small integers: S[b, i, j, r] = W[r, k_i] + bias[r], an exact integer
    in every arithmetic.  The expected tables are counted in integer numpy, pair by pair."""
    from sam_textvqa_amd import ops
    b, n = 2, 70
    g = torch.Generator().manual_seed(5)
    k = torch.arange(n) % 32
    o = torch.zeros(b, n, 32)
    o[:, torch.arange(n), k] = 1.0
    d = torch.ones(b, n, 32) if fusion == "mul" else torch.zeros(b, n, 32)
    w = torch.randint(-3, 3, (12, 32), generator=g).float()
    bias = torch.randint(-1, 2, (12,), generator=g).float()
    w[:, 0] = -bias                                           # row k = 0: every score an exact 0 -> p = 0, nothing fires
    w[:, 1] = 2 - bias                                        # row k = 1: a twelve-way tie at 2 -> p = 1, everything fires
    codes = torch.randint(0, 16, (b, n, n), generator=g).to(torch.uint8)
    valid = (torch.rand(b, n, generator=g) < 0.8).to(torch.uint8)
    valid[:, :2] = 1
    o[valid == 0] = NAN
    d[valid == 0] = NAN
    si = (w[:, k].t() + bias).long().numpy()                  # [n, 12] integer scores of row i (any j)
    assert (si == 0).any() and any((row == row.max()).sum() > 1 and row.max() > 0 for row in si)          # zeros and ties are in the case
    conf, fired = np.zeros((13, 13), np.int64), np.zeros((13, 12), np.int64)
    vn, cn = valid.numpy(), codes.numpy()
    for bb in range(b):
        for i in range(n):
            if not vn[bb, i]:
                continue
            p = int(np.argmax(si[i])) + 1 if si[i].max() > 0 else 0          # (numpy's argmax: the first maximum)
            for j in range(n):
                if vn[bb, j]:
                    c = int(cn[bb, i, j]) if 1 <= cn[bb, i, j] <= 12 else 0
                    conf[c, p] += 1
                    fired[c] += si[i] > 0
    got_c, got_f = ops.aux_pair_stats(*_cuda(o, d, w, bias, codes, valid), fusion)
    assert got_c.dtype == got_f.dtype == torch.int64 and tuple(got_c.shape) == (13, 13) and tuple(got_f.shape) == (13, 12)
    assert np.array_equal(got_c.cpu().numpy(), conf) and np.array_equal(got_f.cpu().numpy(), fired)
    assert conf[:, 0].sum() > 0 and conf[:, 1].sum() > 0 and conf.sum() == int((valid.long().sum(1) ** 2).sum())


# ---------------------------------------------------------------------------------------------- 2. against the dense launch
@pytest.mark.parametrize("fusion", FUSIONS)
@pytest.mark.parametrize("n", [1, 17, 63, 64, 65, 150])
def test_counts_equal_the_twin_on_the_dense_launchs_scores_exactly(fusion, n):
    from sam_textvqa_amd import ops
    for b in (1, 3):
        o, d, w, bias, codes, valid = _cuda(*_case(n, 100 * n + b, b))
        got = ops.aux_pair_stats(o, d, w, bias, codes, valid, fusion)
        dense = ops.aux_pair_fwd(o, d, w, bias, fusion)
        want = ops.aux_stats_from_logits(dense, codes, valid)
        pairs = int((valid.long().sum(1) ** 2).sum())
        print("n %d B %d %s: %d pairs, accuracy %.4f, confusion diff %d fired diff %d" % (n, b, fusion, pairs, float(got[0].diagonal().sum()) / max(pairs, 1),
              int((got[0] - want[0]).abs().sum()), int((got[1] - want[1]).abs().sum())))
        assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])
        assert int(got[0].sum()) == pairs
        if b == 3:
            assert int(valid[2].sum()) == 0 and int(got[0].sum()) == int((valid[:2].long().sum(1) ** 2).sum())          # the sample with no valid row
        if n > 1:
            assert int(codes.max()) > 12 and bool(torch.isnan(o).any()) and bool(torch.isnan(dense).any())          # the dense tensor holds NaN where the counts never look


def test_a_batch_without_a_valid_pair_gives_zeros_and_overwrites():
    from sam_textvqa_amd import ops
    o, d, w, bias, codes, valid = _cuda(*_case(65, 7, 2))
    valid.zero_()
    o.fill_(NAN)
    d.fill_(NAN)
    conf, fired = ops.aux_pair_stats(o, d, w, bias, codes, valid, "mul")                  # (fresh outputs come from torch.empty: the launch stores every cell)
    assert int(conf.abs().sum()) == 0 and int(fired.abs().sum()) == 0


# ---------------------------------------------------------------------------------------------- 3. against float64
_HOST = {}


def _host(n, seed, b, fusion):
    key = (n, seed, b, fusion)
    if key not in _HOST:
        from sam_textvqa_amd import ops
        o, d, w, bias, codes, valid = _case(n, seed, b)
        s64, _ = ops._aux_scores_host(o, d, w, bias, valid, fusion)
        _HOST[key] = ops.aux_stats_host(o, d, w, bias, codes, valid, fusion) + near_ties(s64, valid)
    return _HOST[key]


@pytest.mark.parametrize("fusion", FUSIONS)
def test_counts_vs_the_float64_twin_within_the_near_ties(fusion):
    """delta = 1e-5 max|S|: fp32 scores of 32 products (error about 32 * 2^-24 * max|S| = 2e-6 max|S|) can move a pair across a decision only where the
    float64 margin is below delta.  A pair that changes its predicted class moves two confusion cells; a channel that changes sign one fired cell.
    Seed 21, B = 3, n = 150 (23812 valid pairs), counted by the float64 twin alone on the CPU: mul L = 3, K = 15 (delta 6.8e-5); add L = 2, K = 12
    (delta 9.1e-5) -- all under the cap of 0.1 % of the pairs (23)."""
    from sam_textvqa_amd import ops
    n, seed, b = 150, 21, 3
    want_c, want_f, L, K, pairs, delta = _host(n, seed, b, fusion)
    got_c, got_f = ops.aux_pair_stats(*_cuda(*_case(n, seed, b)), fusion)
    dc, df = int((got_c.cpu() - want_c).abs().sum()), int((got_f.cpu() - want_f).abs().sum())
    print("float64 twin %s: %d pairs, delta %.3g, L %d K %d, confusion diff %d fired diff %d" % (fusion, pairs, delta, L, K, dc, df))
    assert pairs > 20000 and L < 1e-3 * pairs and K < 1e-3 * pairs
    assert int(got_c.sum()) == pairs
    assert dc <= 2 * L and df <= K


# ---------------------------------------------------------------------------------------------- 4. accumulation, histogram, the loss's count
@pytest.mark.parametrize("fusion", FUSIONS)
def test_into_accumulates_and_the_rows_are_the_code_histogram(fusion):
    from sam_textvqa_amd import ops
    o, d, w, bias, codes, valid = _cuda(*_case(65, 11, 3))
    once = ops.aux_pair_stats(o, d, w, bias, codes, valid, fusion)
    again = ops.aux_pair_stats(o, d, w, bias, codes, valid, fusion)
    assert torch.equal(once[0], again[0]) and torch.equal(once[1], again[1])              # bit-identical from run to run
    totals = ops.new_aux_stats()
    for k in (1, 2):
        ret = ops.aux_pair_stats(o, d, w, bias, codes, valid, fusion, into=totals)
        assert ret[0] is totals[0] and ret[1] is totals[1]
        assert torch.equal(totals[0], once[0] * k) and torch.equal(totals[1], once[1] * k)
    v = valid.bool()
    m = v.unsqueeze(2) & v.unsqueeze(1)
    cls = codes[m].long()
    cls = torch.where(cls <= 12, cls, torch.zeros_like(cls))
    assert torch.equal(once[0].sum(1), torch.bincount(cls, minlength=13))
    assert bool((once[1] <= once[0].sum(1, keepdim=True)).all())                         # a channel fires at most once per pair of the class
    _, count = ops.aux_pair_loss(o, d, w, bias, torch.where(codes <= 12, codes, torch.zeros_like(codes)), valid, fusion)
    assert int(once[0].sum()) == int(count.item()) == int(m.sum())
    with pytest.raises(Exception, match="int64"):
        ops.aux_pair_stats(o, d, w, bias, codes, valid, fusion, into=(totals[0].int(), totals[1]))


def test_torch_op_equals_the_ctypes_route():
    from sam_textvqa_amd import ops, torchops
    ns = torchops.ns()
    o, d, w, bias, codes, valid = _cuda(*_case(65, 13, 3))
    for fusion in FUSIONS:
        want = ops.aux_pair_stats(o, d, w, bias, codes, valid, fusion)
        conf, fired = ops.new_aux_stats()
        conf.fill_(-5)
        ns.aux_pair_stats(o, d, w, bias, codes, valid, ops.AUX_FUSIONS[fusion], conf, fired, False)
        assert torch.equal(conf, want[0]) and torch.equal(fired, want[1])
        ns.aux_pair_stats(o, d, w, bias, codes, valid, ops.AUX_FUSIONS[fusion], conf, fired, True)
        assert torch.equal(conf, want[0] * 2) and torch.equal(fired, want[1] * 2)
    with pytest.raises(RuntimeError):
        ns.aux_pair_stats(o, d, w, bias, codes, valid, 0, conf.float(), fired, False)


# ---------------------------------------------------------------------------------------------- 5. memory
def test_peak_allocation_stays_below_the_dense_tensor():
    from sam_textvqa_amd import ops
    b, n = 8, 150
    o, d, w, bias, codes, valid = _cuda(*_case(n, 3, b, nan_rows=False))
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    conf, fired = ops.aux_pair_stats(o, d, w, bias, codes, valid, "mul")
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - before
    print("peak allocation of aux_pair_stats at B = %d, n = %d: %d bytes (dense tensor %d)" % (b, n, peak, b * n * n * 12 * 4))
    assert peak < b * n * n * 12 * 4 and int(conf.sum()) == int((valid.long().sum(1) ** 2).sum())


# ---------------------------------------------------------------------------------------------- 6. module surface
def _model(fusion="mul", **kw):
    import sam_textvqa_amd.modules as M
    from sam_textvqa_amd.synthetic import mmt_config_dict, text_bert_config_dict
    md = mmt_config_dict(3, ("n", "s"), n_dec=3, T=7, n_obj=20, n_ocr=9)
    md.update(hidden_dropout_prob=0.0, attention_probs_dropout_prob=0.0, obj_drop=0.0, ocr_drop=0.0, use_aux_heads=True, aux_spatial_fusion=fusion)
    torch.manual_seed(0)
    td = dict(text_bert_config_dict(), num_hidden_layers=1, hidden_dropout_prob=0.0, attention_probs_dropout_prob=0.0)
    return M.SAM4C(M.BertConfig.from_dict(md), M.BertConfig.from_dict(td), num_answers=60, bos_idx=1, **kw).cuda().train()


def _batch(spatial="adjacency"):
    from sam_textvqa_amd import ops
    from sam_textvqa_amd.synthetic import make_batch
    bd = make_batch(3, 7, 20, 9, 3, vocab=60, context=3, device="cuda", seed=4, spatial=spatial)
    if spatial == "adjacency":
        boxes = torch.cat([bd["pad_obj_bboxes"][..., :4], bd["pad_ocr_bboxes"][..., :4]], 1).double().contiguous()
        bd["spatial_adj_matrices"]["1"] = ops.spatial_relation_tensor(boxes, 1)
    return bd


@pytest.mark.parametrize("spatial", ["adjacency", "boxes"])
def test_module_counts_after_a_training_and_after_an_eval_forward(spatial, monkeypatch):
    from sam_textvqa_amd import ops
    from sam_textvqa_amd.params import prepare
    from sam_textvqa_amd.synthetic import clone_batch
    monkeypatch.setenv("SAM_DECODE_SESSION", "0")             # the eval forward as the eager decoding loop: no graph capture in this file
    model = _model("mul", materialize_spatial_head_out=False)
    prepare(model)
    batch = _batch(spatial)
    bd = clone_batch(batch)
    model(bd)
    assert "spatial_head_out" not in bd and "_sam_aux_od" in bd
    keys = set(bd)
    train = model.spatial_aux_stats(bd)
    assert set(bd) == keys and "spatial_head_out" not in bd                              # no new key, no dense tensor
    assert not train[0].requires_grad and train[0].dtype == torch.int64
    valid = torch.cat([bd["pad_obj_mask"], bd["pad_ocr_mask"]], -1).ne(0)
    pairs = int((valid.long().sum(1) ** 2).sum())
    assert int(train[0].sum()) == pairs and pairs > 0
    # the row sums are the batch's code histogram, whichever form carried the relations
    boxes = torch.cat([batch["pad_obj_bboxes"][..., :4], batch["pad_ocr_bboxes"][..., :4]], 1).double().contiguous()
    codes = ops.codes_from_relation_tensor(ops.spatial_relation_tensor(boxes, 1))
    m = valid.unsqueeze(2) & valid.unsqueeze(1)
    assert torch.equal(train[0].sum(1), torch.bincount(codes[m].long(), minlength=13))
    model.eval()
    bd_e = clone_batch(batch)
    with torch.no_grad():
        model(bd_e)
    assert "_sam_aux_od" not in bd_e
    keys = set(bd_e)
    ev = model.spatial_aux_stats(bd_e)
    assert set(bd_e) == keys                                                             # an eval forward still leaves no new key
    dense = ops.aux_stats_from_logits(bd_e["spatial_head_out"], codes, valid.to(torch.uint8))
    print("module %s: %d pairs, train/eval confusion diff %d fired diff %d" % (spatial, pairs, int((train[0] - ev[0]).abs().sum()), int((train[1] - ev[1]).abs().sum())))
    assert torch.equal(ev[0], dense[0]) and torch.equal(ev[1], dense[1])                 # the eval forward's own dense scores, counted by the twin
    assert torch.equal(train[0], ev[0]) and torch.equal(train[1], ev[1])
    totals = ops.new_aux_stats()
    model.spatial_aux_stats(bd_e, into=totals)
    model.spatial_aux_stats(bd, into=totals)
    assert torch.equal(totals[0], train[0] * 2) and torch.equal(totals[1], train[1] * 2)
    with pytest.raises(ValueError, match="forward"):
        model.spatial_aux_stats(clone_batch(batch))

"""GPU: beam-search output to per-question results (csrc/eval_beams.hip, sam_eval_beams) against the reference-written golden (the bounds
of tests/test_eval_beams_cpu.py) and, bit for bit and in all nine outputs, against its host twin metrics.evaluate_beams_host: random batches at the shapes
where the kernels change path (one beam, one sample, 64 beams = every lane of the selecting wave, more samples than a wave), frequent ties, NaN scores,
out-of-range ids, "<pad>" slots, no OCR slots; sam_score_answers on the repeated table; the float64 accumulator; both op routes; evaluator.evaluate end
to end on the smallest model of tests/test_decode_gpu.py."""
import numpy as np
import pytest
import torch

from sam_textvqa_amd import answers as A
from sam_textvqa_amd import metrics as M
from sam_textvqa_amd import ops
from tests.test_eval_beams_cpu import check_against_golden, load_golden

pytestmark = pytest.mark.gpu
S = 12
CUM_POOL = np.array([-3.0, -1.5, -1.5 + 2.0 ** -20, -0.25, -0.0, 0.0, 0.5], np.float32)       # seven values: ties in most samples


def on_gpu(d):
    return {k: (v.cuda() if torch.is_tensor(v) else v) for k, v in d.items()}


def to_numpy(res):
    return {k: v.cpu().numpy() for k, v in res.items()}


def assert_same(got, want, what=""):
    """all nine outputs, bit for bit, the padding of `answer` included"""
    assert set(got) == set(M.EVAL_BEAMS_KEYS) == set(want)
    for k in M.EVAL_BEAMS_KEYS:
        g, w = got[k], want[k]
        assert g.dtype == w.dtype and g.shape == w.shape, (what, k, g.dtype, w.dtype, g.shape, w.shape)
        gi, wi = (a.view(np.int32) if a.dtype == np.float32 else a for a in (g, w))
        bad = np.argwhere(gi != wi)
        assert bad.size == 0, (what, k, bad[:4].tolist(), g[tuple(bad[0])], w[tuple(bad[0])])


def random_beams(B, K, seed, n_ocr=20, num_vocab=120):
    """tests/test_metrics_gpu.random_batch's draw with K rows per sample and the BOS column in front: ids from the normaliser-exercising words, the last
    vocabulary words, every OCR slot and EOS; a third of the rows spell one of their sample's answers.  Cumulative scores from CUM_POOL."""
    voc, answers, tokens = M.make_score_text(B, num_vocab=num_vocab, n_ocr=max(n_ocr, 1), seed=seed, rich=True)
    s_tabs = [M.build_score_table(a, t[:n_ocr], max_ocr_tokens=n_ocr) for a, t in zip(answers, tokens)]       # (n_ocr = 0: no slot at all)
    vt, table = M.vocab_text(voc), M.collate_score_tables(s_tabs)
    rng = np.random.RandomState(seed + 1)
    V, L = len(voc), S - 1
    pool = np.concatenate([np.arange(4, 4 + len(M._RICH)), np.arange(V - 6, V), V + np.arange(max(n_ocr, 1)), [voc.EOS_IDX] * 8])
    ids = pool[rng.randint(0, len(pool), (B * K, L))]
    for r in range(0, B * K, 3):
        t = s_tabs[r // K]
        words = t["gt_raw"][rng.randint(len(t["gt_raw"]))].split()
        toks = ["".join(chr(c & ~M.NO_GLUE) for c in o) for o in t["ocr"]]
        row = [V + toks.index(w) if w in toks else voc.word2idx_dict.get(w, -1) for w in words][:L - 1]
        if row and min(row) >= 0:
            ids[r] = (row + [voc.EOS_IDX] * L)[:L]
    seqs = np.concatenate([np.full((B * K, 1), 1, np.int64), ids.astype(np.int64)], 1)
    cum = CUM_POOL[rng.randint(0, len(CUM_POOL), B * K)]
    return seqs, cum, table, vt


def run(seqs, cum, table, vt, K, **kw):
    return to_numpy(M.evaluate_beams(torch.as_tensor(seqs).cuda(), torch.as_tensor(cum).cuda(), table, vt, K, **kw))


def test_kernel_equals_the_golden():
    g = load_golden()
    res = run(g["seqs"], g["cum"], g["table"], g["vt"], g["K"])
    check_against_golden(res, g)
    assert_same(res, M.evaluate_beams_host(g["seqs"], g["cum"], g["table"], g["vt"], g["K"]), "golden")


@pytest.mark.parametrize("B,K", [(1, 1), (3, 5), (2, 64), (67, 3)])
def test_kernel_equals_the_host_twin_on_random_batches(B, K):
    seqs, cum, table, vt = random_beams(B, K, seed=20 + B + K)
    res = run(seqs, cum.reshape(-1, 1), table, vt, K)
    want = M.evaluate_beams_host(seqs, cum, table, vt, K)
    assert_same(res, want, (B, K))
    if K > 1:
        ties = sum(np.sum(cum[b * K:(b + 1) * K] == cum[b * K:(b + 1) * K].max()) > 1 for b in range(B))
        assert ties >= 1 and (want["best"] != 0).any()
    if B * K >= 128:
        assert (want["beam_scores"][:, 1] > 0).any() and (want["beam_scores"][:, 2] > 0).any() and (want["oracle"] > want["best_scores"]).any()
    # CONTRACT: the beams' scores are sam_score_answers' on the table repeated K times
    tab = on_gpu(table)
    rep = {k: v.repeat_interleave(K, dim=0).contiguous() for k, v in tab.items()}
    sc, fl = ops.score_answers(torch.as_tensor(seqs[:, 1:]).contiguous().cuda(), rep, vt["cp"].cuda(), vt["len"].cuda(), vt["eos"])
    assert np.array_equal(sc.cpu().numpy().view(np.int32), res["beam_scores"].view(np.int32)) and np.array_equal(fl.cpu().numpy(), res["beam_flags"])


def corner_batch():
    """six samples of five beams: NaN scores, infinities, a winner with an out-of-range id, a winner that points at "<pad>" slots"""
    B, K = 6, 5
    seqs, cum, table, vt = random_beams(B, K, seed=5)
    V, No, eos = vt["len"].numel(), table["ocr"].shape[1], vt["eos"]
    cum = cum.copy()
    cum[0 * K + 3] = np.nan                                  # one NaN: it wins
    cum[1 * K + 2] = cum[1 * K + 4] = np.nan                 # two: the first wins
    cum[2 * K:3 * K] = [-np.inf, -np.inf, np.inf, np.inf, 0.0]
    cum[3 * K:4 * K] = -np.inf
    cum[4 * K:5 * K] = [-1.0, 7.0, -1.0, -1.0, -1.0]         # sample 4's winner, beam 1, holds an out-of-range id behind two words
    seqs[4 * K + 1, 1:] = [5, V, V + No, 6, eos] + [eos] * 6
    cum[5 * K:6 * K] = [-1.0, -1.0, -1.0, -1.0, 7.0]         # sample 5's winner, beam 4, points at slots behind the sample's tokens: "<pad>"
    n_tok = int((table["ocr_len"][5] > 0).sum())
    pad = [o for o in range(No) if "".join(map(chr, table["ocr"][5, o, :5].tolist())) == "<pad>"]
    assert pad and pad[-1] == No - 1 and n_tok <= No
    seqs[5 * K + 4, 1:] = [V + pad[-1], 6, V + pad[0], eos] + [eos] * 7
    return seqs, cum, table, vt, K


def test_nan_scores_bad_ids_pad_slots():
    seqs, cum, table, vt, K = corner_batch()
    res = run(seqs, cum, table, vt, K)
    assert_same(res, M.evaluate_beams_host(seqs, cum, table, vt, K), "corner")
    assert res["best"].tolist()[:4] == [3, 2, 2, 0] and res["best"][4] == 1 and res["best"][5] == 4
    assert res["best_flags"][4] & 1 and not res["best_flags"][5] & 1
    text = M.answer_strings(res["answer"], res["answer_len"])
    assert text[5].startswith("<pad> ") and text[5].endswith(" <pad>")
    V = vt["len"].numel()                                    # the string of the flagged winner holds the two words in front of the bad id, and no more
    two, bad = M.assemble_prediction([5, V, vt["eos"]], table["ocr"][4].numpy(), table["ocr_len"][4].numpy(), vt["cp"].numpy(), vt["len"].numpy(), vt["eos"])
    assert not bad and text[4] == M._strip(two) != ""


def test_no_ocr_slots():
    B, K = 3, 4
    seqs, cum, table, vt = random_beams(B, K, seed=9, n_ocr=0)
    assert table["ocr"].shape[1] == 1 and not table["ocr_len"].any()        # collate_score_tables keeps one empty slot
    res = run(seqs, cum, table, vt, K)
    assert_same(res, M.evaluate_beams_host(seqs, cum, table, vt, K), "No = 0")


def test_totals_accumulate_over_two_calls_and_runs_are_bit_identical():
    B, K = 67, 3
    seqs, cum, table, vt = random_beams(B, K, seed=31)
    tab, vtg = on_gpu(table), on_gpu(vt)
    seqs2, cum2 = seqs[::-1].copy(), cum[::-1].copy()
    runs = []
    for _ in range(2):
        tot = M.new_totals()
        r1 = run(seqs, cum, tab, vtg, K, totals=tot)
        r2 = run(seqs2, cum2, tab, vtg, K, totals=tot)
        runs.append((r1, r2, tot.cpu().numpy()))
    want = np.zeros(4)
    want += M.host_totals(runs[0][0]["best_scores"])
    want += M.host_totals(runs[0][1]["best_scores"])
    np.testing.assert_array_equal(runs[0][2], want)
    assert want[3] == 2 * B
    assert_same(runs[0][0], runs[1][0]), assert_same(runs[0][1], runs[1][1])
    np.testing.assert_array_equal(runs[0][2], runs[1][2])


def test_both_op_routes_agree(monkeypatch):
    g = load_golden()
    out = {}
    for route in ("1", "0"):
        monkeypatch.setenv("SAM_COARSE_OPS", route)
        tot = M.new_totals()
        out[route] = (run(g["seqs"], g["cum"], g["table"], g["vt"], g["K"], totals=tot), tot.cpu().numpy())
    assert_same(out["1"][0], out["0"][0], "routes")
    np.testing.assert_array_equal(out["1"][1], out["0"][1])
    tab, B, K = on_gpu(g["table"]), len(g["questions"]), g["K"]
    bufs = ops.eval_beams_outputs(B, K, S - 1, g["vt"]["cp"].shape[1], "cuda")
    torch.ops.sam_hip.eval_beams(torch.as_tensor(g["seqs"]).cuda(), torch.as_tensor(g["cum"]).reshape(-1).cuda(), [tab[k] for k in ops.SCORE_TABLE_KEYS],
                                 g["vt"]["cp"].cuda(), g["vt"]["len"].cuda(), g["vt"]["eos"], K, 1, [bufs[k] for k in ops.EVAL_BEAMS_KEYS], None)
    assert_same(to_numpy(bufs), out["0"][0], "torch op")
    with pytest.raises(ops.capi.SamHipError, match="K = 4"):
        ops.eval_beams(torch.as_tensor(g["seqs"]).cuda(), torch.as_tensor(g["cum"]).reshape(-1).cuda(), tab, g["vt"]["cp"].cuda(), g["vt"]["len"].cuda(), 2, 4)


def test_evaluator_end_to_end_equals_the_host_on_the_same_beams(tmp_path):
    """evaluator.evaluate over two batches of the smallest synthetic model at beam 3, one with a shipped score table and one with its table built from the
    batch's text: accuracies and answers equal evaluate_beams_host on the complete_seqs and topkscores the search left"""
    import json
    from sam_textvqa_amd import evaluator as E, phoc as P
    from sam_textvqa_amd.registry import registry
    from tests.test_decode_gpu import _batch, _models
    model, _, shapes = _models(layers=("n", "s"))
    registry.EOS_IDX, registry.BOS_IDX = 2, 1
    beam, n, n_ocr = 3, 3, shapes[2]
    voc, answers, tokens = M.make_score_text(2 * n, num_vocab=300, n_ocr=n_ocr, seed=4)
    assert len(voc) == 300 and voc.EOS_IDX == 2
    vt = M.vocab_text(voc)
    host_tabs = [M.collate_score_tables([M.build_score_table(a, t, max_ocr_tokens=n_ocr) for a, t in zip(answers[i * n:(i + 1) * n], tokens[i * n:(i + 1) * n])])
                 for i in range(2)]
    batches = []
    for i in range(2):
        bd = _batch(n, shapes, 300, 40 + i, "cuda")
        bd["train_prev_inds"] = torch.zeros_like(bd["train_prev_inds"]); bd["train_prev_inds"][:, 0] = 1
        bd["question_id"] = torch.tensor([70, 5, 33], device="cuda") + 100 * i
        if i == 0:
            bd["score_table"] = host_tabs[0]                                   # shipped (on the host: moved by evaluate_beams)
        else:                                                                  # the text schema: answers and OCR tokens as code points, no ocr_phoc, no table
            bd.update(on_gpu(A.pack_answer_text(answers[n:])))
            bd.update(on_gpu(P.pack_ocr_text(tokens[n:], max_ocr_tokens=n_ocr)))
            cnt = M.ocr_counts(tokens[n:], n_ocr).cuda()
            bd["pad_ocr_mask"] = (torch.arange(n_ocr, device="cuda")[None, :] < cnt[:, None]).to(bd["pad_ocr_mask"].dtype)
            del bd["ocr_phoc"]
        batches.append(bd)
    seen = []

    def feed():
        for bd in batches:
            yield bd
            seen.append((bd["complete_seqs"].reshape(n * beam, S).cpu().numpy().copy(), bd["topkscores"].reshape(-1).cpu().numpy().copy()))
    res = E.evaluate(model, feed(), vt, beam)
    assert len(seen) == 2 and not model.training
    tot, oracle, want_answers = np.zeros(4), np.zeros(3), []
    for (seqs, cum), tab, qid in zip(seen, host_tabs, ([70, 5, 33], [170, 105, 133])):
        h = M.evaluate_beams_host(seqs, cum, tab, vt, beam, totals=tot)
        oracle += h["oracle"].astype(np.float64).sum(0)
        want_answers += [{"question_id": q, "answer": s} for q, s in zip(qid, M.answer_strings(h["answer"], h["answer_len"]))]
    assert res["count"] == 2 * n and res["answers"] == want_answers
    assert (res["vqa_accuracy"], res["stvqa_accuracy"], res["anls"]) == tuple(tot[:3] / tot[3])
    assert np.abs(np.array(res["oracle"]) - oracle / (2 * n)).max() <= 1e-12
    E.write_evalai(res, str(tmp_path / "evalai.json"))
    assert json.load(open(tmp_path / "evalai.json")) == want_answers

"""GPU: the metrics kernel (csrc/score.hip, sam_score_answers) against the reference-written goldens (same bounds as
tests/test_metrics_cpu.py: stored scores exact, ANLS within 2^-22, batch means within B * 2^-24) and, bit for bit, against its host twin
metrics.score_answers_host: random batches across the reduction's wave / block boundaries, every combination of string lengths around the 64-column
chunks of the distance rows, the float64 accumulator, determinism, out-of-range ids, both op routes, and Trainer(metric=...)."""
import numpy as np
import pytest
import torch

from sam_textvqa_amd import answers as A
from sam_textvqa_amd import metrics as M
from sam_textvqa_amd import ops
from tests.test_metrics_cpu import CAPS, check_scores, golden  # noqa: F401

pytestmark = pytest.mark.gpu


def on_gpu(d):
    return {k: (v.cuda() if torch.is_tensor(v) else v) for k, v in d.items()}


def run(ids, table, vt, totals=None):
    sc, fl = M.score_predictions(torch.as_tensor(np.asarray(ids), dtype=torch.int64).cuda(), table, vt, totals=totals, return_flags=True)
    return sc.cpu().numpy(), fl.cpu().numpy()


def assert_equals_twin(ids, table, vt):
    sc, fl = run(ids, table, vt)
    want, wfl = M.score_answers_host(ids, table, vt, return_flags=True)
    bad = np.flatnonzero((sc.view(np.int32) != want.view(np.int32)).any(1) | (fl != wfl))
    assert bad.size == 0, (bad[:8], sc[bad[:8]], want[bad[:8]], fl[bad[:8]], wfl[bad[:8]])
    return sc, fl


def test_kernel_equals_the_goldens(golden):
    sc, fl = run(golden["ids"], golden["table"], golden["vt"])
    assert not fl.any()
    check_scores(sc, golden["cases"])
    B = len(golden["cases"])
    for m, e in zip(sc.astype(np.float64).mean(0), golden["batch_means"]):
        assert abs(m - e) <= B * 2.0 ** -24
    assert_equals_twin(golden["ids"], golden["table"], golden["vt"])


def random_batch(B, seed, L=12, n_ocr=20, num_vocab=120):
    voc, _, s_tabs = M.make_score_tables(B, num_vocab=num_vocab, n_ocr=n_ocr, seed=seed, rich=True)
    vt = M.vocab_text(voc)
    table = M.collate_score_tables(s_tabs)
    rng = np.random.RandomState(seed + 1)
    V = len(voc)
    pool = np.concatenate([np.arange(4, 4 + len(M._RICH)), np.arange(V - 6, V), V + np.arange(n_ocr), [voc.EOS_IDX] * 8])
    ids = pool[rng.randint(0, len(pool), (B, L))]
    for b in range(0, B, 3):                                 # a third predict one of their own answers, word by word, where the words are known
        words = s_tabs[b]["gt_raw"][rng.randint(len(s_tabs[b]["gt_raw"]))].split()
        toks = ["".join(chr(c & ~M.NO_GLUE) for c in o) for o in s_tabs[b]["ocr"]]
        row = [V + toks.index(w) if w in toks else voc.word2idx_dict.get(w, -1) for w in words][:L - 1]
        if row and min(row) >= 0:
            ids[b] = (row + [voc.EOS_IDX] * L)[:L]
    return ids, table, vt


@pytest.mark.parametrize("B", [1, 3, 64, 67])
def test_kernel_equals_the_host_twin_on_random_batches(B):
    ids, table, vt = random_batch(B, seed=10 + B)
    sc, _ = assert_equals_twin(ids, table, vt)
    if B >= 64:
        assert (sc[:, 1] > 0).any() and (sc[:, 2] > 0).any() and (sc[:, 1] == 0).any()


LENGTHS = (0, 1, 63, 64, 65, 129)


def length_cases(n_answers, seed=0):
    """one sample per (prediction length, ground-truth length): predictions of 1-3 vocabulary words joined with blanks, ground truths derived from them by
    random edits (so that the distances land on both sides of the threshold), cut or padded to the wanted length"""
    rng = np.random.RandomState(seed)
    letters = "bcdefghk"
    words = [A.PAD_TOKEN, A.BOS_TOKEN, A.EOS_TOKEN, A.UNK_TOKEN]
    split = {0: (), 1: (1,), 63: (31, 31), 64: (31, 32), 65: (32, 32), 129: (64, 64)}

    def mutate(s, m):
        s = [c if rng.rand() > 0.2 else letters[rng.randint(8)] for c in s.replace(" ", "a")]
        s = (s + [letters[rng.randint(8)] for _ in range(m)])[:m]
        return "".join(s)

    tabs = [(n, m) for n in LENGTHS for m in LENGTHS]
    rows = []
    for n, m in tabs:
        row = []
        for ln in split[n]:
            w = "".join(letters[i] for i in rng.randint(0, 8, ln))
            while w in words:
                w = "".join(letters[i] for i in rng.randint(0, 8, ln))
            words.append(w)
            row.append(len(words) - 1)
        rows.append(row)
    voc = A.AnswerVocab(words)
    recs = []
    for (n, m), row in zip(tabs, rows):
        pred = " ".join(words[i] for i in row)
        assert len(pred) == n
        gts = [mutate(pred, m)] + [mutate(pred, LENGTHS[(k + LENGTHS.index(m)) % 6]) for k in range(1, n_answers)]
        gts = list(dict.fromkeys(gts))
        recs.append({"gt_norm": gts, "gt_score": np.linspace(0.1, 1.0, len(gts)).astype(np.float32), "gt_raw": gts, "ocr": [[ord("o")]]})
    L = 3
    ids = np.array([(r + [voc.EOS_IDX] * L)[:L] for r in rows], np.int64)
    return ids, M.collate_score_tables(recs, M.ScoreTableCaps(n_answers, 64, 129)), M.vocab_text(voc, max_word=64)


@pytest.mark.parametrize("n_answers", [1, 10])
def test_distances_at_every_length_combination(n_answers):
    ids, table, vt = length_cases(n_answers)
    sc, fl = assert_equals_twin(ids, table, vt)
    assert fl[0] == 2 and (n_answers > 1 or not fl[1:].any())      # (0, 0): empty against empty (with ten answers every empty prediction meets one)
    assert ((sc[:, 2] > 0) & (sc[:, 2] < 1)).sum() >= 5     # the equal-length pairs are a few edits apart


def test_totals_accumulate_in_float64_and_runs_are_bit_identical():
    ids, table, vt = random_batch(67, seed=3)
    tab, vtg = on_gpu(table), on_gpu(vt)
    tot = M.new_totals()
    s1, f1 = run(ids, tab, vtg, totals=tot)
    ids2 = ids[::-1].copy()
    s2, f2 = run(ids2, tab, vtg, totals=tot)
    want = np.concatenate([s1.astype(np.float64).sum(0) + s2.astype(np.float64).sum(0), [134.0]])
    np.testing.assert_array_equal(tot.cpu().numpy(), want)
    tot_b = M.new_totals()
    s1b, f1b = run(ids, tab, vtg, totals=tot_b)
    s2b, f2b = run(ids2, tab, vtg, totals=tot_b)
    assert np.array_equal(s1.view(np.int32), s1b.view(np.int32)) and np.array_equal(s2.view(np.int32), s2b.view(np.int32))
    assert np.array_equal(f1, f1b) and torch.equal(tot, tot_b)


def test_out_of_range_ids_set_flag_bit_0(golden):
    V, No, eos = len(golden["vocab"]), golden["max_ocr_tokens"], golden["vt"]["eos"]
    ids = golden["ids"][:4].copy()
    ids[0, 0] = V + No
    ids[1, 1] = -1
    ids[2, 0] = 2 ** 40
    ids[3, :] = [eos] + [V + No + 5] * 11                    # after EOS: never read
    table = {k: v[:4] for k, v in golden["table"].items()}
    sc, fl = assert_equals_twin(ids, table, golden["vt"])
    assert fl.tolist() == [1, 1, 1, 0]


def test_both_op_routes_agree(golden, monkeypatch):
    out = {}
    for route in ("1", "0"):
        monkeypatch.setenv("SAM_COARSE_OPS", route)
        tot = M.new_totals()
        sc, fl = run(golden["ids"], golden["table"], golden["vt"], totals=tot)
        out[route] = (sc, fl, tot.cpu().numpy())
    for a, b in zip(out["1"], out["0"]):
        np.testing.assert_array_equal(a, b)
    tab = on_gpu(golden["table"])
    sc = torch.empty(len(golden["cases"]), 3, device="cuda")
    fl = torch.empty(len(golden["cases"]), dtype=torch.int32, device="cuda")
    torch.ops.sam_hip.score_answers(torch.as_tensor(golden["ids"]).cuda(), [tab[k] for k in ops.SCORE_TABLE_KEYS], golden["vt"]["cp"].cuda(),
                                    golden["vt"]["len"].cuda(), golden["vt"]["eos"], sc, fl, None)
    np.testing.assert_array_equal(sc.cpu().numpy(), out["0"][0])


_TRAINER_RUNS = {}


def trainer_runs():
    """three steps (eager warm-up, capture + replay, replay) of the smallest model of tests/test_answers_gpu.py, with and without metric=: computed once,
    shared by the two tests below"""
    if _TRAINER_RUNS:
        return _TRAINER_RUNS
    from sam_textvqa_amd.trainer import Trainer
    from tests.test_answers_gpu import batches, small_model, with_inputs
    bd, table = batches()
    voc, a_tabs, s_tabs = M.make_score_tables(4, num_vocab=200, n_ocr=50, seed=5)
    assert all(torch.equal(v, A.collate_answer_tables(a_tabs)[k]) for k, v in table.items())       # the same samples
    vt, stab = M.vocab_text(voc), M.collate_score_tables(s_tabs)
    for name, extra in (("metric", dict(metric="textvqa", metric_vocab=vt)), ("plain", {})):
        tr = Trainer(small_model(), seed=7, base_lr=1e-3, use_graph=True, pipeline_update=False, answer_targets="table", predictions=True, **extra)
        losses, host_sum = [], np.zeros(3)
        for step in range(3):
            inputs = with_inputs(bd, answer_table=table, **({"score_table": stab} if name == "metric" else {}))
            losses.append(tr.step(inputs).clone())
            if name == "metric":
                want, wfl = M.score_answers_host(tr.predictions().cpu().numpy(), stab, vt, return_flags=True)
                got = tr.batch_scores().cpu().numpy()
                assert np.array_equal(got.view(np.int32), want.view(np.int32)) and np.array_equal(tr.score_flags().cpu().numpy(), wfl)
                host_sum += want.astype(np.float64).sum(0)
                np.testing.assert_array_equal(tr.metric_totals().cpu().numpy(), np.concatenate([host_sum, [4.0 * (step + 1)]]))
        assert tr._graph is not None
        torch.cuda.synchronize()
        _TRAINER_RUNS[name] = (torch.stack(losses).cpu(), tr.flat.flat.clone().cpu())
        if name == "plain":                                   # the comparison below means something only if the loss is reproducible at all
            again = Trainer(small_model(), seed=7, base_lr=1e-3, use_graph=True, pipeline_update=False, answer_targets="table", predictions=True)
            l2 = torch.stack([again.step(with_inputs(bd, answer_table=table)).clone() for _ in range(3)]).cpu()
            _TRAINER_RUNS["plain_again"] = (l2, again.flat.flat.clone().cpu())
        if name == "metric":
            assert abs(tr.metric_value() - host_sum[0] / 12.0) < 1e-12
            old = tr.metric_totals(reset=True)
            assert old[3].item() == 12.0 and not tr.metric_totals().any()
        else:
            assert tr.batch_scores() is None and tr.metric_totals() is None
    with pytest.raises(ValueError, match="score_table"):
        Trainer(small_model(), seed=7, answer_targets="table", predictions=True, metric="stvqa_anls", metric_vocab=vt).step(with_inputs(bd, answer_table=table))
    return _TRAINER_RUNS


def test_trainer_metric_scores_inside_the_step_and_leaves_the_parameters_bit_identical():
    """batch_scores() equals the host twin on predictions() in the eager, the capturing and the replayed step, metric_totals() accumulates and resets, and
    the parameters after three steps are bit-identical to a Trainer without metric="""
    runs = trainer_runs()
    print("parameters differ in %d places (max %.3g)" % ((runs["metric"][1] != runs["plain"][1]).sum().item(),
                                                         (runs["metric"][1] - runs["plain"][1]).abs().max().item()))
    assert torch.equal(runs["metric"][1], runs["plain"][1])


def test_trainer_metric_leaves_the_loss_bit_identical():
    """the three losses of a Trainer with metric= equal those of a Trainer without, bit for bit (the table loss adds its blocks' parts in a fixed order:
    csrc/bce_table.hip)"""
    runs = trainer_runs()
    print("losses with metric %s, without %s, without again %s" % (runs["metric"][0].tolist(), runs["plain"][0].tolist(), runs["plain_again"][0].tolist()))
    assert torch.equal(runs["plain"][0], runs["plain_again"][0]) and torch.equal(runs["plain"][1], runs["plain_again"][1])
    assert torch.equal(runs["metric"][0], runs["plain"][0])

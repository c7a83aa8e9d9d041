"""GPU: beam-search answers chosen by string (csrc/beam_merge.hip, sam_eval_beams_merged) against the host twin
metrics.evaluate_beams_merged_host, whose definition tests/test_beam_merge_cpu.py pins.  The fixtures make duplicates frequent: a few base answers per
question, every beam one of them spelled another way (a vocabulary id or an OCR slot of the same text, "joe's" or "joe" + "'s", ids behind EOS).

What is compared, on whole tensors written over 0x7F bytes: every integer output and beam_scores / best_scores / oracle bit for bit; mass and best_mass bit
for bit where the group has one member, else within 1e-5 + 2.4e-7 |mass| of the twin's float64 value (DESIGN.md §3.29 derives it: at most 64 terms in
[0, 1] of 1 ulp each and 64 roundings of the sum give 65 * 2^-24 = 3.9e-6 relative in s, hence absolute in log s; logf adds 1 ulp of at most 4.16, the final
add one rounding at |mass|: 4.4e-6 + 6e-8 |mass|; the absolute term is doubled and the relative one quadrupled for a library expf / logf worse than 1 ulp).
The discrete outputs can be exact only where the fp32 and the float64 masses rank the groups alike, so every fixture satisfies, and every test asserts:
the two largest group masses of the twin differ by more than 1e-3 unless both groups have a single member (such masses are the beams' own cum on both
sides, a tie between them is exact and goes to the lower leader)."""
import functools

import numpy as np
import pytest
import torch

from sam_textvqa_amd import evalboard as EB
from sam_textvqa_amd import metrics as M
from sam_textvqa_amd import ops

pytestmark = pytest.mark.gpu
N_OCR = 12
INT_KEYS = ("beam_flags", "best", "best_ids", "best_flags", "answer", "answer_len", "beam_answer", "beam_answer_len", "group", "n_groups", "plain_best")
EXACT_FLOAT_KEYS = ("beam_scores", "best_scores", "oracle")
# (B, K, S, skip) -> the seed at which the fixture condition holds for every question (chosen on the CPU: the twin alone decides it)
CASES = {(1, 1, 2, 1): 0, (7, 5, 13, 1): 0, (3, 33, 13, 1): 0, (2, 64, 13, 1): 0, (2, 4, 64, 0): 0, (5, 3, 2, 1): 0}


def world(B, L, seed):
    """metrics.make_score_tables(rich=True) for B questions; the last OCR slot of every question is overwritten with "joe", whose possessive the rich
    vocabulary holds as the single token "joe's".  Words of at most 12 code points when L is large, so that L = 64 stays within the LDS bound."""
    caps = M.ScoreTableCaps(10, 12 if L > 16 else 32, 128)
    voc, _, s_tabs = M.make_score_tables(B, num_vocab=120, n_ocr=N_OCR, seed=seed, rich=True)
    for t in s_tabs:
        t["ocr"][-1] = M._lower_word("joe")
    return voc, s_tabs, M.collate_score_tables(s_tabs, caps), M.vocab_text(voc, max_word=caps.Lw)


def spellings(word, voc, toks):
    """every id sequence of one or two ids that spells `word` for this question: its vocabulary id, every OCR slot with that text, and for "joe's" also
    "joe" (a slot) followed by the vocabulary's "'s\""""
    V = len(voc)
    out = [[voc.word2idx_dict[word]]] if word in voc.word2idx_dict else []
    out += [[V + o] for o, t in enumerate(toks) if t == word]
    if word == "joe's":
        out += [[V + o, voc.word2idx_dict["'s"]] for o, t in enumerate(toks) if t == "joe"]
    return out


def merged_beams(B, K, S, skip, seed):
    """-> (seqs int64 [B * K, S], cum fp32 [B * K], table, vt).  Per question 3 + K // 8 base answers (at most K) of one to three words; a beam is a base with every
    word spelled one of its ways, then EOS, then arbitrary ids.  cum is the log of a random distribution over the beams, some of them -inf."""
    L = S - skip
    voc, s_tabs, table, vt = world(B, L, seed)
    rng = np.random.RandomState(seed + 1000)
    V, eos = len(voc), voc.EOS_IDX
    rows = []
    for b in range(B):
        toks = ["".join(chr(c & ~M.NO_GLUE) for c in o) for o in s_tabs[b]["ocr"]]
        words = sorted(set(toks)) + ["joe's", "w1", "w2", "stop" if "stop" in voc.word2idx_dict else "w3"]
        words = [w for w in words if spellings(w, voc, toks)]
        bases = [[words[i] for i in rng.randint(0, len(words), rng.randint(1, 4))] for _ in range(min(K, 3 + K // 8))]
        for k in range(K):
            ids = [i for w in bases[rng.randint(len(bases))] for i in (lambda sp: sp[rng.randint(len(sp))])(spellings(w, voc, toks))]
            rows.append((ids + [eos] + rng.randint(0, V + N_OCR, L).tolist())[:L])
    seqs = np.concatenate([np.full((B * K, skip), 1, np.int64), np.array(rows, np.int64)], 1)
    p = rng.dirichlet(np.ones(K), B).reshape(-1)
    if K >= 3:
        p[rng.rand(B * K) < 0.08] = 0.0
    with np.errstate(divide="ignore"):
        cum = np.log(p).astype(np.float32)
    return seqs, cum, table, vt


@functools.lru_cache(maxsize=None)
def fixture(B, K, S, skip):
    """the case's inputs and the twin's result, computed once and shared (callers copy what they change)"""
    seqs, cum, table, vt = merged_beams(B, K, S, skip, CASES[B, K, S, skip])
    return seqs, cum, table, vt, M.evaluate_beams_merged_host(seqs, cum, table, vt, K, skip=skip)


def sizes(want, K):
    """members of every beam's group, int [B * K]"""
    g = want["group"].reshape(-1, K)
    return np.stack([np.bincount(row, minlength=K)[row] for row in g]).reshape(-1)


def undecided(want, K, nan_decides=False):
    """the questions the fixture condition does not cover: the two largest group masses of the twin are within 1e-3 and not both single members.
    nan_decides: a NaN mass is a NaN on both sides (no arithmetic decides it) and the first one wins, exactly: such a question is covered."""
    n, bad = sizes(want, K).reshape(-1, K), []
    for b, (g, m) in enumerate(zip(want["group"].reshape(-1, K), want["mass"].reshape(-1, K).astype(np.float64))):
        lead = [k for k in range(K) if g[k] == k]
        if nan_decides and np.isnan(m[lead]).any():
            continue
        assert not np.isnan(m[lead]).any()
        top = sorted(lead, key=lambda k: -m[k])[:2]
        if len(top) == 2 and not (n[b, top[0]] == 1 and n[b, top[1]] == 1) and not abs(m[top[0]] - m[top[1]]) > 1e-3:          # (inf - inf is NaN: undecided)
            bad.append(b)
    return bad


def run(seqs, cum, table, vt, K, skip, **kw):
    """the kernel on buffers pre-filled with 0x7F bytes -> numpy"""
    B, L = table["meta"].shape[0], seqs.shape[1] - skip
    out = ops.eval_beams_merged_outputs(B, K, L, table["ocr"].shape[2], "cuda")
    for t in out.values():
        t.view(torch.uint8).fill_(0x7F)
    res = M.evaluate_beams_merged(torch.as_tensor(seqs).cuda(), torch.as_tensor(cum).cuda(), table, vt, K, skip=skip, out=out, **kw)
    assert all(res[k] is out[k] for k in M.EVAL_MERGED_KEYS)
    return {k: v.cpu().numpy() for k, v in res.items()}


def assert_same(got, want, K, what=""):
    assert tuple(got) == M.EVAL_MERGED_KEYS == tuple(want)
    for k in M.EVAL_MERGED_KEYS:
        assert got[k].dtype == want[k].dtype and got[k].shape == want[k].shape, (what, k, got[k].dtype, want[k].dtype, got[k].shape, want[k].shape)
    for k in INT_KEYS + EXACT_FLOAT_KEYS:
        g, w = (a.view(np.int32) if a.dtype == np.float32 else a for a in (got[k], want[k]))
        bad = np.argwhere(g != w)
        assert bad.size == 0, (what, k, bad[:4].tolist(), got[k][tuple(bad[0])], want[k][tuple(bad[0])])
    n = sizes(want, K)
    for key, members in (("mass", n), ("best_mass", n.reshape(-1, K)[np.arange(len(want["best"])), want["best"]])):
        g, w = got[key], want[key]
        one = members == 1
        assert np.array_equal(g[one].view(np.int32), w[one].view(np.int32)), (what, key, "single members", g[one], w[one])
        g, w = g[~one].astype(np.float64), w[~one].astype(np.float64)
        fin = np.isfinite(w)
        assert np.array_equal(np.isnan(g), np.isnan(w)) and np.array_equal(g[~fin & ~np.isnan(w)], w[~fin & ~np.isnan(w)]), (what, key, g, w)
        err = np.abs(g[fin] - w[fin])
        print(what, key, "groups of several members:", int((~one).sum()), "largest error", err.max() if err.size else 0.0)
        assert (err <= 1e-5 + 2.4e-7 * np.abs(w[fin])).all(), (what, key, err.max())


@pytest.mark.parametrize("B,K,S,skip", list(CASES))
def test_kernel_equals_the_twin(B, K, S, skip):
    seqs, cum, table, vt, want = fixture(B, K, S, skip)
    assert undecided(want, K) == []                            # the fixture condition, for every question
    got = run(seqs, cum, table, vt, K, skip)
    assert_same(got, want, K, (B, K, S, skip))
    if K >= 3:                                                 # the fixture does what it is for: beams merge, and merging changes answers
        assert (want["n_groups"] < K).any() and (sizes(want, K) >= 2).any()
    if (B, K) == (7, 5):
        assert (want["best"] != want["plain_best"]).any() and np.isneginf(cum).any()
    assert M.answer_strings(got["beam_answer"], got["beam_answer_len"]) == M.answer_strings(want["beam_answer"], want["beam_answer_len"])


def corner_batch():
    """(7, 5, 13, 1) with six questions rewritten: an exact tie of two single-member groups at the top; NaN inside a group; a NaN single beam behind it;
    a group of -inf members only beside a finite beam; a flagged beam whose partial string equals its neighbours'; every beam the empty string"""
    seqs, cum, table, vt, _ = fixture(7, 5, 13, 1)
    seqs, cum = seqs.copy(), cum.copy()
    K, V, eos, L = 5, vt["len"].numel(), vt["eos"], 12
    w = [int(i) for i in np.arange(V - 10, V)]                 # ten plain vocabulary words: ten distinct strings

    def put(b, rows, scores):
        for k, row in enumerate(rows):
            seqs[b * K + k, 1:] = (list(row) + [eos] * L)[:L]
        cum[b * K:(b + 1) * K] = scores

    put(0, [[w[0]], [w[1]], [w[2]], [w[3]], [w[3], eos, w[4]]], [-3.0, -0.5, -0.5, -5.0, -5.0])
    put(1, [[w[0]], [w[1]], [w[1], eos, 5], [w[2]], [w[3]]], [0.0, -1.0, np.nan, -0.25, -2.0])
    put(2, [[w[0]], [w[1]], [w[1]], [w[2]], [w[3]]], [np.nan, -1.0, np.nan, np.nan, -2.0])
    put(3, [[w[0]], [w[0]], [w[1]], [w[0]], [w[2]]], [-np.inf, -np.inf, -7.0, -np.inf, -np.inf])
    put(4, [[w[0], V + N_OCR, w[5]], [w[0]], [w[0], -1], [w[0]], [w[1]]], [-0.7, -1.3, -0.7, -1.3, -0.8])
    put(5, [[eos], [eos, w[0]], [eos] * 3, [eos, -1], [eos, V + N_OCR]], [-1.0, -2.0, -3.0, -1.5, -2.5])
    return seqs, cum, table, vt, K


def test_exact_ties_nan_minus_infinity_flagged_and_empty_beams():
    seqs, cum, table, vt, K = corner_batch()
    want = M.evaluate_beams_merged_host(seqs, cum, table, vt, K, skip=1)
    # questions 1 and 2 hold NaN masses: NaN on both sides whatever the arithmetic, and the first NaN wins exactly; every other question meets the condition
    assert undecided(want, K, nan_decides=True) == [] and np.isnan(want["best_mass"]).tolist() == [False, True, True] + [False] * 4
    assert want["group"][:30].reshape(6, K).tolist() == [[0, 1, 2, 3, 3], [0, 1, 1, 3, 4], [0, 1, 1, 3, 4], [0, 0, 2, 0, 4], [0, 1, 2, 1, 4], [0, 0, 0, 0, 0]]
    assert want["best"][:6].tolist() == [1, 2, 0, 2, 1, 0] and want["plain_best"][:6].tolist() == [1, 2, 0, 2, 0, 0]
    assert want["best_mass"][0] == np.float32(-0.5) and np.isneginf(want["mass"][15]) and (want["beam_flags"][20:25] & 1).tolist() == [1, 0, 1, 0, 0]
    assert want["beam_answer_len"][25:30].tolist() == [0] * 5 and want["n_groups"][5] == 1
    assert_same(run(seqs, cum, table, vt, K, 1), want, K, "corners")


def test_two_calls_agree_bit_for_bit_and_leave_the_inputs_alone():
    B, K, S, skip = 3, 33, 13, 1
    seqs, cum, table, vt, want = fixture(B, K, S, skip)
    tab, vtg = {k: v.cuda() for k, v in table.items()}, {"cp": vt["cp"].cuda(), "len": vt["len"].cuda(), "eos": vt["eos"]}
    sg, cg = torch.as_tensor(seqs).cuda(), torch.as_tensor(cum).cuda()
    runs, tots = [], []
    for _ in range(2):
        tot = M.new_totals()
        runs.append({k: v.cpu().numpy() for k, v in M.evaluate_beams_merged(sg, cg, tab, vtg, K, skip=skip, totals=tot).items()})
        tots.append(tot.cpu().numpy())
    for k in M.EVAL_MERGED_KEYS:
        assert runs[0][k].tobytes() == runs[1][k].tobytes(), k
    assert tots[0].tobytes() == tots[1].tobytes() and np.array_equal(tots[0], M.host_totals(want["best_scores"])) and tots[0][3] == B
    assert np.array_equal(sg.cpu().numpy(), seqs) and cg.cpu().numpy().tobytes() == cum.tobytes()
    assert all(np.array_equal(tab[k].cpu().numpy(), table[k].numpy()) for k in M.SCORE_TABLE_KEYS)
    assert np.array_equal(vtg["cp"].cpu().numpy(), vt["cp"].numpy()) and np.array_equal(vtg["len"].cpu().numpy(), vt["len"].numpy())


def test_distinct_strings_give_evaluate_beams_in_the_nine_shared_outputs():
    B, K, S = 6, 5, 12
    voc, _, table, vt = world(B, S - 1, seed=3)
    rng = np.random.RandomState(8)
    V, eos = len(voc), voc.EOS_IDX
    seqs = np.full((B * K, S), eos, np.int64)
    seqs[:, 0] = 1
    for b in range(B):                                         # K different plain vocabulary words first: K different strings, whatever follows
        seqs[b * K:(b + 1) * K, 1] = V - 1 - rng.permutation(20)[:K]
        seqs[b * K:(b + 1) * K, 2:5] = rng.randint(0, V + N_OCR, (K, 3))
    cum = np.array([-3.0, -1.5, -1.5, -0.25, 0.5], np.float32)[rng.randint(0, 5, B * K)]          # ties in most questions
    want = M.evaluate_beams_merged_host(seqs, cum, table, vt, K)
    assert (want["n_groups"] == K).all() and undecided(want, K) == []
    got = run(seqs, cum, table, vt, K, 1)
    assert_same(got, want, K, "distinct")
    plain = {k: v.cpu().numpy() for k, v in M.evaluate_beams(torch.as_tensor(seqs).cuda(), torch.as_tensor(cum).cuda(), table, vt, K).items()}
    for k in M.EVAL_BEAMS_KEYS:
        assert got[k].dtype == plain[k].dtype and got[k].tobytes() == plain[k].tobytes(), k
    assert np.array_equal(got["plain_best"], plain["best"]) and got["mass"].tobytes() == cum.tobytes()


def test_a_merged_result_goes_through_the_board():
    B, K, S, skip = 7, 5, 13, 1
    seqs, cum, table, vt, want = fixture(B, K, S, skip)
    n, P = 11, (S - skip) * (table["ocr"].shape[2] + 1)
    idx, valid = np.array([4, 9, 0, 7, 10, 2, 9], np.int32), np.array([1, 1, 1, 0, 1, 1, 1], np.int32)          # a slot left out, a question met twice
    res = M.evaluate_beams_merged(torch.as_tensor(seqs).cuda(), torch.as_tensor(cum).cuda(), table, vt, K, skip=skip)
    board, host = EB.Board(n, P), EB.new_host(n, P)
    board.collect(res, torch.from_numpy(idx).cuda(), torch.from_numpy(valid).cuda())
    EB.collect_host(host, want, idx, valid)
    assert board.result() == EB.result_host(host)
    assert {k: v.cpu().numpy().tobytes() for k, v in board.t.items()} == {k: v.tobytes() for k, v in host.items()}


def test_evaluator_with_merge_equals_the_twin_on_the_searchs_own_beams():
    """evaluator.evaluate(merge="string") over two batches of the smallest synthetic model at beam 3 (the model of tests/test_eval_beams_gpu.py); the OCR
    slots of every question spell two words in turn, both in the vocabulary, so that beams which differ in a slot often spell the same answer.  Answers,
    means, "changed" and "groups" equal the twin's on the complete_seqs / topkscores the search left.  The search's scores are not under this test's
    control: where a question's two largest masses are within 1e-3 (and not both of single beams) its string may be either candidate's -- at most one
    such question is tolerated, and then the means and "changed" are not compared.  Then: evaluate without merge has no new field, and
    evaluate_indexed on the greedy route gives one result with and without merge."""
    from sam_textvqa_amd import evaluator as E
    from sam_textvqa_amd.registry import registry
    from tests.test_decode_gpu import _batch, _models
    model, _, shapes = _models(layers=("n", "s"))
    registry.EOS_IDX, registry.BOS_IDX = 2, 1
    beam, n, n_ocr, S = 3, 3, shapes[2], 12
    voc, answers, _ = M.make_score_text(2 * n, num_vocab=300, n_ocr=n_ocr, seed=4)
    assert len(voc) == 300 and voc.EOS_IDX == 2
    vt = M.vocab_text(voc)
    tokens = [[("w%d" % (5 + q), "w%d" % (40 + q))[o % 2] for o in range(n_ocr)] for q in range(2 * n)]
    tabs = [M.collate_score_tables([M.build_score_table(a, t, max_ocr_tokens=n_ocr) for a, t in zip(answers[i * n:(i + 1) * n], tokens[i * n:(i + 1) * n])])
            for i in range(2)]

    def make_batches():                                        # (the search rewrites a batch in place: fresh ones per pass)
        batches = []
        for i in range(2):
            bd = _batch(n, shapes, 300, 40 + i, "cuda")
            bd["train_prev_inds"] = torch.zeros_like(bd["train_prev_inds"]); bd["train_prev_inds"][:, 0] = 1
            bd["question_id"] = torch.tensor([70, 5, 33], device="cuda") + 100 * i
            bd["score_table"] = tabs[i]
            batches.append(bd)
        return batches
    batches, seen = make_batches(), []

    def feed():
        for bd in batches:
            yield bd
            seen.append((bd["complete_seqs"].reshape(n * beam, S).cpu().numpy().copy(), bd["topkscores"].reshape(-1).cpu().numpy().copy()))
    res = E.evaluate(model, feed(), vt, beam, merge="string")
    assert len(seen) == 2 and not model.training
    tot, close, qid, answers_got = np.zeros(4), 0, [70, 5, 33, 170, 105, 133], res["answers"]
    changed = groups = 0
    for i, ((seqs, cum), tab) in enumerate(zip(seen, tabs)):
        h = M.evaluate_beams_merged_host(seqs, cum, tab, vt, beam, totals=tot)
        text, nbest = M.answer_strings(h["answer"], h["answer_len"]), M.answer_strings(h["beam_answer"], h["beam_answer_len"])
        und = undecided(h, beam)
        print("batch", i, "groups", h["n_groups"].tolist(), "best", h["best"].tolist(), "plain", h["plain_best"].tolist(), "undecided", und)
        for b in range(n):
            got = answers_got[i * n + b]
            assert got["question_id"] == qid[i * n + b]
            lead = [k for k in range(beam) if h["group"][b * beam + k] == k]          # too close to call: either of the two heaviest groups' strings
            two = {nbest[b * beam + k] for k in sorted(lead, key=lambda k: -float(h["mass"][b * beam + k]))[:2]}
            assert got["answer"] in ([text[b]] if b not in und else two), (i, b, got, text[b])
        close += len(und)
        changed += int((h["best"] != h["plain_best"]).sum())
        groups += int(h["n_groups"].sum())
    assert close <= 1                                          # the cap on questions too close to call
    assert res["count"] == 2 * n and res["groups"] == groups / (2 * n)
    if close == 0:
        assert [a["answer"] for a in answers_got] == [s for (seqs, cum), tab in zip(seen, tabs)
                                                      for s in (lambda h: M.answer_strings(h["answer"], h["answer_len"]))(M.evaluate_beams_merged_host(seqs, cum, tab, vt, beam))]
        assert (res["vqa_accuracy"], res["stvqa_accuracy"], res["anls"]) == tuple(tot[:3] / tot[3]) and res["changed"] == changed
    plain = E.evaluate(model, iter(make_batches()), vt, beam)   # without merge the result has no new field
    assert "changed" not in plain and "groups" not in plain and plain["count"] == 2 * n
    # evaluate_indexed: the greedy route has one beam per question, so merge="string" is legal and changes nothing
    greedy = []
    for merge in (None, "string"):
        bs = make_batches()
        for i, bd in enumerate(bs):
            bd["sample_idx"] = torch.arange(n, dtype=torch.int32, device="cuda") + n * i
        greedy.append(E.evaluate_indexed(model, iter(bs), vt, 0, EB.Board(2 * n, S * (vt["cp"].shape[1] + 1)), merge=merge))
    assert greedy[0] == greedy[1] and greedy[0]["count"] == 2 * n

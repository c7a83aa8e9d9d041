#!/usr/bin/env python
"""The results board, device-event timing around host-issued calls, eager (no graph is captured):

  a. per batch at B = 64, P = 12 * 65 (12 scored steps of words of up to 64 code points): Board.collect against the per-batch bookkeeping of
     evaluator.evaluate that it replaces -- sam_eval_beams' totals launch (measured as evaluate_beams with and without totals), `oracle_sum +=`, and
     the pass's final torch.cat calls spread over its batches -- in one process, the routes taking turns;
  b. Board.reduce at n = 5000 and n = 35 000;
  c. the read-back of a pass of 5000 questions: evaluate's (totals, oracle sums, the concatenated ids and answers, answer_strings) against
     Board.result(), host wall time;
  d. a whole pass of the smallest model (one TextBert layer, two MMT layers) at beam 3 over the same batches: evaluator.evaluate against
     evaluator.evaluate_indexed.

    python tools/bench_evalboard.py [--iters 300] [--passes 3] [--batch 64] [--out profiles/evalboard_bench.txt]      (--out is rewritten)
"""
import os
import sys

import numpy as np
import measure
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from sam_textvqa_amd import evalboard as E  # noqa: E402
from sam_textvqa_amd import evaluator as Ev  # noqa: E402
from sam_textvqa_amd import metrics as M  # noqa: E402
from sam_textvqa_amd import ops  # noqa: E402

K, S, LW, N_OCR, VOCAB = 5, 13, 64, 50, 5000                    # L = S - 1 = 12 scored steps, P = 12 * (64 + 1) = 780


def beams(B, seed):
    """one batch of beam-search output with its score table on the device, at word capacity LW"""
    voc, _, s_tabs = M.make_score_tables(B, num_vocab=VOCAB, n_ocr=N_OCR, seed=seed, rich=True)
    rng = np.random.RandomState(seed + 100)
    V = len(voc)
    pool = np.concatenate([np.arange(4, V, 37), V + np.arange(N_OCR), [voc.EOS_IDX] * 12])
    seqs = np.concatenate([np.ones((B * K, 1), np.int64), pool[rng.randint(0, len(pool), (B * K, S - 1))].astype(np.int64)], 1)
    vt = M.vocab_text(voc, max_word=LW)
    return {"seqs": torch.from_numpy(seqs).cuda(), "cum": torch.from_numpy(-rng.rand(B * K).astype(np.float32) * 8).cuda(),
            "table": {k: v.cuda() for k, v in M.collate_score_tables(s_tabs, caps=(10, LW, 128)).items()},
            "vt": {"cp": vt["cp"].cuda(), "len": vt["len"].cuda(), "eos": vt["eos"]}}


def host_ms(fn):
    """median wall time of fn followed by a synchronise, 5 runs"""
    torch.cuda.synchronize()
    return measure.host_ms(lambda _: (fn(), torch.cuda.synchronize()), 5)[0]


def small_pass(n_batches, B, beam):
    """the smallest model and n_batches batches of B questions with shipped score tables and sample_idx"""
    import sam_textvqa_amd.modules as Mod
    from sam_textvqa_amd.params import prepare
    from sam_textvqa_amd.registry import registry
    from sam_textvqa_amd.synthetic import make_batch, mmt_config_dict, text_bert_config_dict
    md = mmt_config_dict(3, ("n", "s"))
    md.update(hidden_dropout_prob=0.0, attention_probs_dropout_prob=0.0, obj_drop=0.0, ocr_drop=0.0)
    td = dict(text_bert_config_dict(), num_hidden_layers=1, hidden_dropout_prob=0.0, attention_probs_dropout_prob=0.0, vocab_size=500)
    torch.manual_seed(0)
    model = Mod.SAM4C(Mod.BertConfig.from_dict(md), Mod.BertConfig.from_dict(td), num_answers=300, bos_idx=1)
    model.cuda().eval()
    prepare(model)
    registry.EOS_IDX, registry.BOS_IDX = 2, 1
    voc, _, s_tabs = M.make_score_tables(n_batches * B, num_vocab=300, n_ocr=N_OCR, seed=4)
    inputs = []
    for i in range(n_batches):
        bd = make_batch(B, vocab=300, context=3, device="cuda", seed=40 + i)
        bd["question_indices"] = (bd["question_indices"] % 499 + 1) * bd["question_mask"]
        bd["train_prev_inds"] = torch.zeros_like(bd["train_prev_inds"])
        bd["train_prev_inds"][:, 0] = 1
        bd["score_table"] = {k: v.cuda() for k, v in M.collate_score_tables(s_tabs[i * B:(i + 1) * B]).items()}
        bd["sample_idx"] = torch.arange(i * B, (i + 1) * B, dtype=torch.int32, device="cuda")
        inputs.append(bd)

    def fresh():                                                 # SAM4C.forward mutates its batch: every pass gets shallow copies
        return [dict(bd, spatial_adj_matrices=dict(bd["spatial_adj_matrices"])) for bd in inputs]
    return model, M.vocab_text(voc), fresh


def main():
    ap = measure.arg_parser()
    ap.add_argument("--iters", type=int, default=300)
    ap.add_argument("--passes", type=int, default=3)
    ap.add_argument("--batch", type=int, default=64)
    a = ap.parse_args()
    measure.require_gpu("bench_evalboard.py")
    B, n = a.batch, 5000
    L, P = S - 1, (S - 1) * (LW + 1)
    sets = [beams(B, 60 + i) for i in range(4)]
    bufs = ops.eval_beams_outputs(B, K, L, LW, "cuda")
    totals, oracle_sum = M.new_totals("cuda"), torch.zeros(3, dtype=torch.float64, device="cuda")
    board = E.Board(n, P)
    idx = [torch.from_numpy(np.random.RandomState(i).permutation(n)[:B].astype(np.int32)).cuda() for i in range(4)]
    valid = torch.ones(B, dtype=torch.int32, device="cuda")
    turn = [0, 0, 0, 0, 0]

    def pick(r):
        turn[r] += 1
        return turn[r] % 4

    def beams_with_totals():
        s = sets[pick(0)]
        return M.evaluate_beams(s["seqs"], s["cum"], s["table"], s["vt"], K, totals=totals, out=bufs)

    def beams_alone():
        s = sets[pick(1)]
        return M.evaluate_beams(s["seqs"], s["cum"], s["table"], s["vt"], K, out=bufs)

    def parent_batch():
        res = beams_with_totals()
        oracle_sum.add_(res["oracle"].double().sum(0))

    def board_batch():
        board.collect(beams_alone(), idx[pick(2)], valid)

    res = beams_alone()
    assert res["answer"].shape == (B, P)
    t_tot, t_no, t_parent, t_board, t_collect, t_osum = measure.timed_alternating(
        [beams_with_totals, beams_alone, parent_batch, board_batch, lambda: board.collect(res, idx[pick(3)], valid),
         lambda: oracle_sum.add_(res["oracle"].double().sum(0))], a.iters)
    board.status()
    steps = -(-n // B)
    answers, lens, qids = [res["answer"].clone() for _ in range(steps)], [res["answer_len"].clone() for _ in range(steps)], [idx[0].clone() for _ in range(steps)]
    t_cat = measure.timed_alternating([lambda: (torch.cat(qids), torch.cat(answers), torch.cat(lens))], 20)[0] / steps

    def parent_readback():
        totals.cpu().tolist(), oracle_sum.cpu().tolist()
        torch.cat(qids).cpu().tolist()
        return [s for an, ln in zip(answers, lens) for s in M.answer_strings(an, ln)]

    full = E.Board(n, P)
    for i in range(steps):
        full.collect(res, torch.arange(i * B, (i + 1) * B, dtype=torch.int32, device="cuda").remainder(n), valid)
    ms_parent, ms_board = host_ms(parent_readback), host_ms(full.result)
    lines = ["# tools/bench_evalboard.py --iters %d --passes %d --batch %d on one MI355X; K = %d beams, %d scored steps, Lw = %d: P = %d" % (a.iters, a.passes, B, K, L, LW, P),
             "# device events around host-issued calls, 3 alternating windows per route, median window; eager calls, no graph is captured",
             "evaluate_beams with totals (3 launches) / without (2 launches):      %8.1f / %8.1f us per eager call: the totals launch costs %.1f us" % (t_tot, t_no, t_tot - t_no),
             "Board.collect alone (one sam_evalboard_collect launch):              %8.1f us per eager call" % t_collect,
             "`oracle_sum += oracle.double().sum(0)` alone:                        %8.1f us per eager call; the final torch.cat of ids, answers and lengths: %.1f us per batch of a %d-batch pass"
             % (t_osum, t_cat, steps),
             "per batch, evaluate's route (beams with totals, oracle_sum +=):      %8.1f us" % t_parent,
             "per batch, the board's route (beams without totals, collect):        %8.1f us   (%+.1f %%)" % (t_board, 100.0 * (t_board - t_parent) / t_parent)]
    for m in (5000, 35000):
        bd = E.Board(m, 4)
        bd.t["seen"].fill_(1)
        bd.t["scores"].uniform_()
        out = torch.empty(8, dtype=torch.float64, device="cuda")
        lines.append("Board.reduce at n = %5d (one workgroup, fixed order):               %8.1f us per eager call" % (m, measure.timed_alternating([lambda: bd.reduce(out)], a.iters)[0]))
    lines.append("read-back of a %d-question pass, host wall time: evaluate's (two sums, cat, answer_strings) %.1f ms; Board.result() (reduce, the used answer columns, answer_strings) %.1f ms"
                 % (n, ms_parent, ms_board))

    beam, nb, Bs = 3, 8, 32
    model, vt, fresh = small_pass(nb, Bs, beam)
    small = E.Board(nb * Bs, 11 * 33)

    def pass_parent():
        return Ev.evaluate(model, fresh(), vt, beam)

    def pass_board():
        small.reset()
        return Ev.evaluate_indexed(model, fresh(), vt, beam, small)

    r_parent, r_board = pass_parent(), pass_board()
    same = all(r_parent[k] == r_board[k] for k in ("count", "answers")) and max(abs(r_parent[k] - r_board[k]) for k in ("vqa_accuracy", "stvqa_accuracy", "anls")) < 1e-12
    t_p, t_b = measure.timed_alternating([pass_parent, pass_board], a.passes, warm=1)
    lines += ["# the smallest model (1 TextBert layer, 2 MMT layers), beam %d, %d batches of %d questions with shipped score tables" % (beam, nb, Bs),
              "evaluator.evaluate, whole pass with its read-back:          %8.2f ms" % (t_p / 1e3),
              "evaluator.evaluate_indexed, whole pass with its read-back:  %8.2f ms   (%+.1f %%; the box-to-box spread is +-3 %%); same count, answers and means: %s"
              % (t_b / 1e3, 100.0 * (t_b - t_p) / t_p, same)]
    measure.finish(lines, a.out)


if __name__ == "__main__":
    main()

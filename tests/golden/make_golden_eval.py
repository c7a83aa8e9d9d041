#!/usr/bin/env python3
"""Generate tests/golden/eval_beams.json by running the REFERENCE's evaluate_predictions (evaluator.py:304-356) on CPU, for acc_type "vqa" and "anls", on a
hand-built eval_df and results_df: a handful of questions with K = 5 beams of S = 12 ids each, as Evaluator.evaluate (:67-135) feeds it after beam search.

Runs ONLY in the build container (the reference never travels to the GPU box) and is never imported by a test.  It reuses make_golden_metrics' shims
(import_metrics: the stub sam.datasets package, the Levenshtein stand-in for `editdistance`), its vocabulary and its token list; a stub `sam.task_utils`
module is installed before `evaluator` is imported, so that the model stack is not pulled in.  The fixture holds data only.

eval_beams.json: vocab (word list), max_ocr_tokens, K, S, questions [{name, question_id, ocr_tokens, answers, complete_seqs [K][S], topkscores [K], best,
answer, vqa, anls}] in the order the batch holds them (question ids are NOT sorted: evaluate_predictions' groupby sorts them), means {vqa, anls}.

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_eval.py
"""
import json
import os
import sys
import types

sys.dont_write_bytecode = True

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
from tests.golden.make_golden import REF  # noqa: E402
from tests.golden.make_golden_metrics import MAX_OCR, T0, VOCAB, import_metrics, pred_row  # noqa: E402

K, S = 5, 12
BOS = VOCAB.index("<s>")
T_LOW = [t.lower() for t in T0]                     # (the answer text is compared: lower-case tokens, as Processors.word_cleaner leaves them)
T_WS = ["joe", "'s", " bar\t", "\u3000lead", "sign"]
SOFT = ["one"] + ["two"] * 2 + ["three"] * 3 + ["four"] * 4

# (name, question id, OCR tokens, ten answers, K beams of (prediction, cumulative score)); a prediction entry is a vocabulary word, ("ocr", slot), or None
# for EOS, as in make_golden_metrics.CASES
QUESTIONS = [
    ("top_beam_is_not_the_most_accurate", 907, T_LOW, ["stop sign"] * 10,
     [(["hello", None], -0.5), ([("ocr", 0), ("ocr", 1), None], -0.9), ([("ocr", 0), None], -1.25), (["world", None], -2.0), ([("ocr", 1), None], -2.5)]),
    ("exact_tie_first_wins", 12, T_LOW, ["coca cola"] * 6 + ["cocacola"] * 4,
     [(["red", None], -1.0), ([("ocr", 7), None], -0.25), (["apple", None], -0.25), (["hello", None], -2.0), (["world", None], -3.0)]),
    ("all_scores_equal", 455, ["one", "two", "four"], SOFT,
     [([("ocr", 1), None], -1.5), ([("ocr", 2), None], -1.5), ([("ocr", 0), None], -1.5), (["3", None], -1.5), (["hello", None], -1.5)]),
    ("negative_and_zero_mixed", 3, T_LOW, ["abcy"] * 10,
     [(["abcd", "w", None], -0.75), (["abcd", None], 0.0), (["hello", None], -0.125), (["abcd", "abcd", None], 0.0), (["w", None], -3.0)]),
    ("all_scores_zero", 78, T_LOW, ["3 don't"] * 8 + ["three dont"] * 2,
     [(["three", "dont", None], 0.0), (["three", None], 0.0), (["dont", None], 0.0), (["ten", None], 0.0), (["none", None], 0.0)]),
    ("winner_ends_at_step_0", 1001, ["one"], SOFT,
     [([("ocr", 0), None], -4.0), (["hello", None], -3.5), ([None], -0.0625), (["world", None], -5.0), (["red", None], -6.0)]),
    ("glue_and_whitespace_to_strip", 64, T_WS, ["lead joe's bar"] * 7 + ["joe's bar"] * 3,
     [([("ocr", 0), ("ocr", 1), ("ocr", 2), None], -1.0), ([("ocr", 0), ("ocr", 1), None], -1.5), (["hello", None], -2.0), (["it", "'s", None], -2.5),
      ([("ocr", 3), ("ocr", 0), ("ocr", 1), ("ocr", 2), None], -0.5)]),
    ("positive_scores_last_beam_wins", 250, T_LOW, ["1.5 x.5"] * 10,
     [(["1.5", None], 0.5), (["x.5", None], 1.0), (["u.s.a.", None], -1.0), (["1.5", "x.5", "1.5", None], 0.0), (["1.5", "x.5", None], 2.0)]),
]


def main():
    import_metrics()
    stub = types.ModuleType("sam.task_utils")
    stub.forward_model = None
    sys.modules["sam.task_utils"] = stub
    if REF not in sys.path:
        sys.path.insert(0, REF)
    import pandas as pd
    from tools.registry import registry
    registry.EOS_IDX = VOCAB.index("</s>")
    import evaluator as E

    rows = {"question_id": [], "topkscores": [], "complete_seqs": []}
    seqs = []
    for _, qid, _, _, beams in QUESTIONS:
        assert len(beams) == K
        seqs.append([([BOS] + pred_row(p))[:S] for p, _ in beams])
        for row, (_, score) in zip(seqs[-1], beams):
            rows["question_id"].append(qid)
            rows["topkscores"].append([score])          # Evaluator.evaluate's .tolist() of a [N, 1] array
            rows["complete_seqs"].append(row)
    results_df = pd.DataFrame.from_dict(rows, orient="columns")
    padded = [list(t)[:MAX_OCR] + ["<pad>"] * (MAX_OCR - len(t)) for _, _, t, _, _ in QUESTIONS]
    eval_df = pd.DataFrame({"question_id": [q[1] for q in QUESTIONS], "answers": [list(q[3]) for q in QUESTIONS], "ocr_tokens": padded})
    res = {t: E.evaluate_predictions(eval_df, results_df, VOCAB, acc_type=t) for t in ("vqa", "anls")}

    first = {q[1]: i * K for i, q in enumerate(QUESTIONS)}
    picked = {}
    for t in ("vqa", "anls"):
        for label, row in res[t]["best_result_df"].iterrows():
            qid = int(row["question_id"])
            picked.setdefault(qid, {})[t] = (int(label) - first[qid], row["pred_answer"].strip(), float(row["accuracy"]))
    questions, n_oracle = [], 0
    for i, (name, qid, tokens, answers, beams) in enumerate(QUESTIONS):
        (kv, sv, av), (ka, sa, aa) = picked[qid]["vqa"], picked[qid]["anls"]
        assert kv == ka and sv == sa
        acc = res["vqa"]["accuracies_df"]
        per_beam = [float(a) for a in acc[acc["question_id"] == qid]["accuracy"].tolist()]
        n_oracle += max(per_beam) > av
        questions.append({"name": name, "question_id": qid, "ocr_tokens": list(tokens), "answers": list(answers), "complete_seqs": seqs[i],
                          "topkscores": [s for _, s in beams], "best": kv, "answer": sv, "vqa": av, "anls": aa})
        print("%-36s qid %4d best %d %-20r vqa %.2f anls %.4f (beams' vqa %s)" % (name, qid, kv, sv, av, aa, per_beam))
    assert sum(q["best"] != 0 for q in questions) >= 2 and n_oracle >= 1
    means = {"vqa": float(res["vqa"]["vqa_accuracy"]), "anls": float(res["anls"]["vqa_accuracy"])}
    with open(os.path.join(HERE, "eval_beams.json"), "w") as f:
        json.dump({"vocab": VOCAB, "max_ocr_tokens": MAX_OCR, "K": K, "S": S, "questions": questions, "means": means}, f, indent=1, ensure_ascii=True)
        f.write("\n")
    print("eval_beams.json: %d questions, means %s, %d with best != 0, %d where another beam scores higher" % (
        len(questions), means, sum(q["best"] != 0 for q in questions), n_oracle))


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""Generate tests/golden/metrics.json by running the REFERENCE's metrics (sam/datasets/metrics.py) on CPU: EvalAIAnswerProcessor on a list of strings, and
TextVQAAccuracy / STVQAAccuracy / STVQAANLS .calculate (hence TextVQAAccuracyEvaluator, STVQAAccuracyEvaluator, STVQAANLSEvaluator and the index -> word
walk of :39-51) on one hand-built batch.

Runs ONLY in the build container (the reference never travels to the GPU box).  Besides make_golden.py's shims: a stub `sam.datasets` package module (its
__init__ imports the lmdb / h5py dataset classes); Tensor.cuda is the identity while calculate runs (:65 moves the batch mean to a GPU); `editdistance` is
not installed, so a module of that name is installed whose eval is the plain two-row Levenshtein below.  The fixture holds data only.

metrics.json: vocab (word list), max_ocr_tokens, L, pairs [[input, normalised]], cases [{name, ocr_tokens, answers, pred_ids, answer, scores [vqa, acc,
anls]}], batch_means [vqa, acc, anls].

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_metrics.py
"""
import json
import os
import sys
import types

sys.dont_write_bytecode = True
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
from tests.golden.make_golden import REF, install_shims  # noqa: E402

MAX_OCR, L = 50, 12
DOTS = "." * 33 + "z"
VOCAB = ["<pad>", "<s>", "</s>", "<unk>", "red", "apple", "the", "a", "an", "three", "3", "dont", "coca-cola", "it", "'s", "'stop", "st.", "1.5", "x.5",
         "u.s.a.", "joe's", "hello", "world", "abcd", "(stop)", "- go", DOTS, "w@x", "none", "Stop", "he'dve", "ten", "w"]

PAIRS_IN = ["a.b 1.5 x. <=.", "Coca-Cola", "coca -cola", "coca- cola and pepsi-cola", "(stop) (go )", "what?", "1,000", "joe's bar", "joe 's bar", "it's",
            "'stop sign", "go 'stop", "the a an", "The End", "three", "none of ten", "dont", "hed've", "he'dve gone", "she's", "let's", "Im", "x.5", ".5", "5.",
            "u.s.a.", DOTS, ".".join("x" * 34), "a\tb\nc", " \t lead and trail \n", "tab\tdash -", "e\x0bf", "nb sp", "Über STRASSE", "ΣΑΣ", "a / b", "a/b",
            "w@x", "100%", "no.", "no.7", "st. 5", "..5", "5..", "[x] {y}", "a_b_c _", "\"q\"", "back\\slash", "x=y+z", "<=>", "`tick`", "hi!", "hi !", "",
            "   ", "an apple a day", "twas", "'ows'at", "yall'd've", "somebody'd", "3 's", "s's's", "?,", "a,b", "- go", "e-mail me - now"]

# (name, OCR tokens, ten answers, prediction): a prediction entry is a vocabulary word, ("ocr", slot), or None for EOS; padded with <pad> ids to L
T0 = ["stop", "sign", "Main", "st.", "joe", "'s", "e\tf\ng", "coca-cola"] + ["t%d" % i for i in range(8, 49)] + ["last"]
SOFT = ["one"] + ["two"] * 2 + ["three"] * 3 + ["four"] * 4
CASES = [
    ("soft_0.3", ["one", "two", "four"], SOFT, [("ocr", 0), None]),
    ("soft_0.6", ["one", "two", "four"], SOFT, [("ocr", 1), None]),
    ("soft_0.9_after_normalisation", ["one", "two", "four"], SOFT, ["3", None]),
    ("soft_1.0", ["one", "two", "four"], SOFT, [("ocr", 2), None]),
    ("matches_nothing", ["one", "two", "four"], SOFT, ["hello", "world", None]),
    ("eos_at_step_0", ["one"], SOFT, [None]),
    ("no_eos_in_12_steps", ["red"], ["red " * 11 + "red"] * 10, ["red"] * 12),
    ("ocr_first_last_padded", T0, ["stop last"] * 6 + ["stop"] * 4, [("ocr", 0), ("ocr", 49), None]),
    ("padded_slot", ["stop"], ["stop <pad>"] * 10, [("ocr", 0), ("ocr", 7), None]),
    ("glue_s", T0, ["joe's sign"] * 7 + ["joe 's sign"] * 3, [("ocr", 4), ("ocr", 5), ("ocr", 1), None]),
    ("word_starting_with_s_after_blank", T0, ["go 'stop"] * 10, ["hello", "'stop", None]),
    ("capital_S_not_glued", ["'S", "joe"], ["joe's"] * 10, [("ocr", 1), ("ocr", 0), None]),
    ("tabs_newlines_in_token", T0, ["e f g"] * 10, [("ocr", 6), None]),
    ("punct_not_touching", T0, ["coca cola"] * 6 + ["cocacola"] * 4, ["coca-cola", None]),
    ("punct_touching", T0, ["go"] * 5 + ["- go"] * 5, ["- go", None]),
    ("periods_33", T0, [".z"] * 4 + ["z"] * 6, [DOTS, None]),
    ("period_before_digit", T0, ["1.5 x.5"] * 10, ["1.5", "x.5", None]),
    ("period_dropped", T0, ["usa main st"] * 10, ["u.s.a.", ("ocr", 2), ("ocr", 3), None]),
    ("number_word_and_contraction", T0, ["3 don't"] * 8 + ["three dont"] * 2, ["three", "dont", None]),
    ("contraction_with_apostrophe", T0, ["he'd've"] * 10, ["he'dve", None]),
    ("articles_only_answers", T0, ["the"] * 4 + ["a an"] * 3 + ["red"] * 3, ["the", "a", "an", None]),
    ("articles_only_prediction_vs_words", T0, ["red"] * 10, ["the", None]),
    ("none_is_zero", T0, ["0"] * 10, ["none", None]),
    ("case_folding", T0, ["STOP"] * 10, ["Stop", None]),
    ("anls_tie", T0, ["abxy"] * 10, ["abcd", None]),
    ("anls_one_edit_above", T0, ["abcy"] * 10, ["abcd", None]),
    ("anls_one_edit_below", T0, ["axyz"] * 10, ["abcd", None]),
    ("anls_max_over_answers", T0, ["abcd efgh"] * 3 + ["abcd"] * 3 + ["zzzz"] * 4, ["abcd", "w", None]),
    ("at_sign", T0, ["w x"] * 10, ["w@x", None]),
    ("eos_then_garbage", T0, ["red"] * 10, ["red", None, "apple", ("ocr", 3)]),
]


def levenshtein(a, b):
    prev = list(range(len(b) + 1))
    for i in range(1, len(a) + 1):
        cur = [i] + [0] * len(b)
        for j in range(1, len(b) + 1):
            cur[j] = min(prev[j] + 1, cur[j - 1] + 1, prev[j - 1] + (a[i - 1] != b[j - 1]))
        prev = cur
    return prev[len(b)]


def import_metrics():
    install_shims()
    if REF not in sys.path:
        sys.path.insert(0, REF)
    import sam  # noqa: F401
    pkg = types.ModuleType("sam.datasets")
    pkg.__path__ = [os.path.join(REF, "sam", "datasets")]
    sys.modules["sam.datasets"] = pkg
    ed = types.ModuleType("editdistance")
    ed.eval = levenshtein
    sys.modules["editdistance"] = ed
    from sam.datasets import metrics as M
    from tools.objects_to_byte_tensor import enc_obj2bytes
    from tools.registry import registry
    return M, registry, enc_obj2bytes


class Vocab:
    def __init__(self, words):
        self.words = words

    def __len__(self):
        return len(self.words)

    def idx2word(self, i):
        return self.words[i]


def pred_row(pred):
    V, row = len(VOCAB), []
    for p in pred:
        row.append(VOCAB.index("</s>") if p is None else (V + p[1] if isinstance(p, tuple) else VOCAB.index(p)))
    return row + [0] * (L - len(row))


def main():
    M, registry, enc = import_metrics()
    proc = M.EvalAIAnswerProcessor()
    pairs = [[s, proc(s)] for s in PAIRS_IN]
    registry.answer_vocab = Vocab(VOCAB)
    registry.EOS_IDX = VOCAB.index("</s>")
    rows = [pred_row(p) for _, _, _, p in CASES]
    padded = [list(t)[:MAX_OCR] + ["<pad>"] * (MAX_OCR - len(t)) for _, t, _, _ in CASES]
    batch = {"pred_answer_rd": torch.tensor(rows), "ocr_tokens": torch.stack([enc(t) for t in padded]),
             "answers": torch.stack([enc(list(a)) for _, _, a, _ in CASES]), "question_id": torch.arange(len(CASES))}
    orig_cuda = torch.Tensor.cuda
    torch.Tensor.cuda = lambda self, *a, **k: self
    try:
        res = []
        for cls in (M.TextVQAAccuracy, M.STVQAAccuracy, M.STVQAANLS):
            m = cls()
            m.accuracies = []
            acc, scores, preds = m.calculate(batch, None)
            res.append((float(acc), [float(s) for s in scores], preds))
    finally:
        torch.Tensor.cuda = orig_cuda
    cases = []
    for i, (name, tokens, answers, _) in enumerate(CASES):
        cases.append({"name": name, "ocr_tokens": list(tokens), "answers": list(answers), "pred_ids": rows[i], "answer": res[0][2][i]["pred_answer"],
                      "scores": [res[0][1][i], res[1][1][i], res[2][1][i]]})
        print("%-36s %-28r vqa %.2f acc %.0f anls %.4f" % (name, cases[-1]["answer"], *cases[-1]["scores"]))
    with open(os.path.join(HERE, "metrics.json"), "w") as f:
        json.dump({"vocab": VOCAB, "max_ocr_tokens": MAX_OCR, "L": L, "pairs": pairs, "cases": cases, "batch_means": [r[0] for r in res]}, f, indent=1,
                  ensure_ascii=True)
        f.write("\n")
    print("metrics.json: %d pairs, %d cases, batch means %s" % (len(pairs), len(cases), [r[0] for r in res]))


if __name__ == "__main__":
    main()

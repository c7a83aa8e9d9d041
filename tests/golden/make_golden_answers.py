#!/usr/bin/env python3
"""Generate tests/golden/answers.npz + answers.json by running the REFERENCE's M4CAnswerProcessor (sam/datasets/processors.py:501-707) on CPU.

Runs ONLY in the build container (the reference never travels to the GPU box).  Importing the processor needs, besides make_golden.py's shims: a stub
`sam.datasets` package module (its __init__ imports the lmdb / h5py dataset classes) and a stub `sam.phoc` (cphoc.so is built for another Python).  The
answer vocabulary is a toy word list written to a temporary file: <pad> first, <unk> present (the processor's asserts, :530-536).

For each hand-built case and each k in range(len(all_idx_seq_list)), np.random.choice is patched to return k (:667) and the processor's outputs are
recorded; a case without candidates is recorded once with k = -1.  Cases on which the reference fails one of its own assertions are listed with the
draws that fail.

Contents of answers.npz (R records, L = 12 steps):
  rec_case, rec_k int32 [R]       case index / forced draw
  n_cand int32 [C]                len(all_idx_seq_list) per case
  nz_off int32 [R + 1]            record r's non-zeros of targets are nz_idx / nz_val[nz_off[r]:nz_off[r + 1]] (flat t * W + j, value)
  nz_idx int32, nz_val float32
  prev int64 [R, L], loss_mask / acc_mask float32 [R, L]
answers.json: vocab word list, W, max_ocr_tokens, the cases {name, answers, context_tokens}, the failing cases {name, answers, context_tokens, failing_k}.

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_answers.py
"""
import json
import os
import sys
import tempfile
import types

sys.dont_write_bytecode = True
import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
from tests.golden.make_golden import REF, install_shims  # noqa: E402

VOCAB = ["<pad>", "<s>", "</s>", "<unk>", "red", "apple", "flag", "stop", "coca", "cola", "the", "a"]
MAX_OCR = 50
L = 12

CASES = [
    ("soft_scores", ["red"] * 4 + ["apple"] * 3 + ["flag"] * 2 + ["stop"], ["red", "sign"]),
    ("multi_word", ["red apple"] * 5 + ["red flag"] * 3 + ["coca cola"] * 2, ["apple", "red", "cola"]),
    ("vocab_and_ocr", ["coca cola"] * 6 + ["cola"] * 4, ["coca", "cola", "zero"]),
    ("repeated_ocr", ["stop"] * 6 + ["stop go"] * 4, ["stop", "go", "stop", "go", "stop"]),
    ("ocr_in_vocab", ["the end"] * 7 + ["end"] * 3, ["the", "end", "a"]),
    ("no_match", ["xyzzy"] * 7 + ["plugh"] * 3, ["abc", "def"]),
    ("long_answer", ["the a b c d e f g h i j k l m"] * 3 + ["b"] * 7, list("bcdefghijklm")),
    ("many_matches", ["stop stop stop"] * 2 + ["stop"] * 8, ["stop", "stop", "stop", "go"]),
    ("ocr_cut", ["w55 red"] * 5 + ["w3"] * 5, ["w%d" % i for i in range(60)]),
    ("one_word_eos", ["cola"] * 10, ["pepsi"]),
    ("partial_match", ["red", "zzz", "red", "yyy", "apple", "red", "qqq", "flag", "apple", "xxx"], ["flag"]),
    ("empty_ocr", ["red flag", "red", "flag", "red flag", "a", "a", "the", "red", "red", "flag"], []),
]
FAILING = [
    ("unk_at_step1", ["go <unk>"] * 10, ["go"]),
    ("pad_ocr_at_step1", ["go <pad>"] * 10, ["go", "<pad>"]),
]


def import_processor():
    install_shims()
    if REF not in sys.path:
        sys.path.insert(0, REF)
    import sam  # noqa: F401
    pkg = types.ModuleType("sam.datasets")
    pkg.__path__ = [os.path.join(REF, "sam", "datasets")]
    sys.modules["sam.datasets"] = pkg
    phoc = types.ModuleType("sam.phoc")
    phoc.build_phoc = lambda *a, **k: None
    sys.modules["sam.phoc"] = phoc
    from sam.datasets import processors as P
    from tools.registry import registry
    return P, registry


def run(P, proc, answers, tokens, k):
    orig = P.np.random.choice
    seen = []

    def choice(n):
        seen.append(n)
        return k
    P.np.random.choice = choice
    try:
        out = proc({"answers": list(answers), "context_tokens": list(tokens)})
    finally:
        P.np.random.choice = orig
    return out, (seen[0] if seen else 0)


def main():
    P, registry = import_processor()
    with tempfile.TemporaryDirectory() as tmp:
        vf = os.path.join(tmp, "vocab.txt")
        with open(vf, "w") as f:
            f.write("\n".join(VOCAB) + "\n")
        registry["Vocabs"] = {"vocab5k": vf}
        from easydict import EasyDict
        proc = P.M4CAnswerProcessor(EasyDict(vocab_type="5k", num_answers=10, max_ocr_tokens=MAX_OCR, max_copy_steps=L))
    W = proc.get_vocab_size()
    rec_case, rec_k, n_cand, nz_off, nz_idx, nz_val, prev, loss, acc = [], [], [], [0], [], [], [], [], []
    for c, (name, answers, tokens) in enumerate(CASES):
        _, n = run(P, proc, answers, tokens, 0)
        n_cand.append(n)
        for k in (range(n) if n > 0 else [-1]):
            out, _ = run(P, proc, answers, tokens, k)
            tg = out["targets"].numpy().reshape(-1)
            nz = np.flatnonzero(tg)
            nz_idx.extend(nz.tolist())
            nz_val.extend(tg[nz].tolist())
            nz_off.append(len(nz_idx))
            rec_case.append(c)
            rec_k.append(k)
            prev.append(out["train_prev_inds"].numpy())
            loss.append(out["train_loss_mask"].numpy())
            acc.append(out["train_acc_mask"].numpy())
        print("%-16s %3d candidates" % (name, n))
    failing = []
    for name, answers, tokens in FAILING:
        cnt = [0]

        def counting(n_):                                        # the candidate count: stop at the draw itself
            cnt[0] = n_
            raise AssertionError("count only")
        orig = P.np.random.choice
        P.np.random.choice = counting
        try:
            proc({"answers": list(answers), "context_tokens": list(tokens)})
        except AssertionError:
            pass
        finally:
            P.np.random.choice = orig
        bad = []
        for k in range(cnt[0]):
            try:
                run(P, proc, answers, tokens, k)
            except AssertionError:
                bad.append(k)
        assert bad, name
        failing.append({"name": name, "answers": answers, "context_tokens": tokens, "n_cand": cnt[0], "failing_k": bad})
        print("%-16s %3d candidates, draws %s fail the reference's assertions" % (name, cnt[0], bad))
    np.savez_compressed(os.path.join(HERE, "answers.npz"), rec_case=np.array(rec_case, np.int32), rec_k=np.array(rec_k, np.int32),
                        n_cand=np.array(n_cand, np.int32), nz_off=np.array(nz_off, np.int32), nz_idx=np.array(nz_idx, np.int32),
                        nz_val=np.array(nz_val, np.float32), prev=np.stack(prev).astype(np.int64), loss_mask=np.stack(loss).astype(np.float32),
                        acc_mask=np.stack(acc).astype(np.float32))
    with open(os.path.join(HERE, "answers.json"), "w") as f:
        json.dump({"vocab": VOCAB, "W": W, "max_ocr_tokens": MAX_OCR, "max_copy_steps": L,
                   "cases": [{"name": n, "answers": a, "context_tokens": t} for n, a, t in CASES], "failing": failing}, f, indent=1)
        f.write("\n")
    print("answers.npz: %d records, %.1f KB" % (len(rec_case), os.path.getsize(os.path.join(HERE, "answers.npz")) / 1024))


if __name__ == "__main__":
    main()

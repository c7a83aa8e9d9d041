#!/usr/bin/env python3
"""Host time of the batch's text packers, the only speed the batchtext refactor can move (CPU only; no GPU is touched):

  pack_ocr_text        B = 64 samples of 50 tokens        pack_answer_text     B = 64 samples of 10 answers
  pack_question_text   B = 64 questions                   answers.vocab_index  5000 words

The same fixed inputs on every run.  --runs fresh child processes per checkout (fresh: the parent commit's package and this tree's cannot share one
interpreter), each timing REPS calls per packer with measure.host_ms; the parent's children and this tree's alternate.  The bound is the parent's own
run-to-run spread: a packer passes when this tree's best median is no further above the parent's best median than the parent's medians lie apart.

    python tools/bench_batchtext.py --parent <checkout of the parent commit> --out profiles/batchtext_host_bench.txt"""
import json
import os
import subprocess
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import measure  # noqa: E402

B, REPS, WARM = 64, 41, 5
PACKERS = ("pack_ocr_text", "pack_answer_text", "pack_question_text", "vocab_index")


def child():
    import numpy as np
    from sam_textvqa_amd import answers, metrics, phoc, wordpiece
    voc, ans, tokens = metrics.make_score_text(B, num_vocab=5000, n_ocr=50, seed=7, rich=True)
    tokens = [(t * 50)[:50] for t in tokens]                                  # every slot holds a token
    rng = np.random.RandomState(3)
    questions = ["what does the %s sign next to the %s say%s" % (t[0], t[-1], "?" * int(rng.randint(1, 3))) for t in tokens]
    calls = {"pack_ocr_text": lambda r: phoc.pack_ocr_text(tokens), "pack_answer_text": lambda r: answers.pack_answer_text(ans),
             "pack_question_text": lambda r: wordpiece.pack_question_text(questions), "vocab_index": lambda r: answers.vocab_index(voc)}
    out = {}
    for name in PACKERS:
        measure.host_ms(calls[name], WARM)
        out[name] = measure.host_ms(calls[name], REPS)
    print(json.dumps(out))


def run(root):
    env = dict(os.environ, PYTHONPATH=root + os.pathsep + os.environ.get("PYTHONPATH", ""))
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", "-", "--root", root], env=env, stdout=subprocess.PIPE, check=True, cwd=root)
    return json.loads(r.stdout.decode().strip().splitlines()[-1])


def main():
    ap = measure.arg_parser(parent=True, child=True)
    ap.add_argument("--runs", type=int, default=2)
    args = ap.parse_args()
    sys.path.insert(0, args.root)
    if args.child:
        return child()
    roots = ([("parent", args.parent)] if args.parent else []) + [("this tree", measure.ROOT)]
    runs = {name: [] for name, _ in roots}
    for _ in range(args.runs):
        for name, root in roots:
            runs[name].append(run(root))
    lines = ["host packers, B = %d, ms per call: median (min .. max) of %d calls, %d fresh processes per checkout, alternating" % (B, REPS, args.runs)]
    ok = True
    for p in PACKERS:
        lines.append(p)
        for name, rs in runs.items():
            lines += ["  %-10s run %d  %8.3f (%.3f .. %.3f)" % (name, i + 1, r[p][0], r[p][1], r[p][2]) for i, r in enumerate(rs)]
        if args.parent:
            base, new = [r[p][0] for r in runs["parent"]], [r[p][0] for r in runs["this tree"]]
            spread = max(base) - min(base)
            good = min(new) <= min(base) + spread
            ok = ok and good
            lines.append("  parent's spread %.3f ms (%.1f %%); this tree's best median %+.1f %% against the parent's best: %s" % (
                spread, 100 * spread / min(base), 100 * (min(new) / min(base) - 1), "within it or faster" if good else "SLOWER than the spread"))
    if not args.parent:
        lines.append(measure.NO_PARENT.replace("step", "packers"))
    measure.finish(lines, args.out, ok, "a packer is slower than the parent's own spread allows")


if __name__ == "__main__":
    main()

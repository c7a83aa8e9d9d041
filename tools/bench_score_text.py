#!/usr/bin/env python3
"""Score tables from text at B = 64, the default capacities (10 answers, 50 OCR slots, Lw = 32, Lg = 128): what the launch costs, what the
host functions it replaces cost, what a batch ships either way, and the eager training step with the build in front against the same step fed the
host-built table.

  kernel     sam_score_table_from_text: ROUNDS launches captured in one graph, cycling over COPIES distinct batches, replayed REPS times with HIP events
             around each replay; median (min .. max) per launch.  The last batch's table is compared with the host twin.
  host       wall time of build_score_table per sample + collate_score_tables of the 64 samples (the strings in, the collated CPU table out), one
             thread of this machine's host, median of HOST_REPS runs over the same COPIES batches.
  bytes      per batch: the collated score table, against the answers' text (which answers.tables_from_text ships already) and the OCR count; the OCR
             text is shipped either way, for PHOC, and the table's copy of it ("ocr" / "ocr_len") goes.
  step       Trainer(use_graph=False, metric="textvqa") at bench.py's default shapes (c3 model, B = 64, 5000 words): STEP_REPS steps timed one by one
             with HIP events, median.  Every variant runs in a fresh child process of this script, the variants alternating, CHILD_ROUNDS times each:
               text          this tree, metrics.score_tables_from_text(check=False) builds the batch's score_table on the GPU inside the timed region,
                             in front of Trainer.step
               host table    this tree, the batch carries the collated score_table (the code a batch without the new call always ran)
               parent        --parent DIR: a built checkout of the parent commit, the same host-table batch (read from a file this script writes)

    python tools/bench_score_text.py [--parent DIR] [--out profiles/score_text_bench.txt]"""
import argparse
import json
import os
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

B, N_OCR, VOCAB = 64, 50, 5000
ROUNDS, COPIES, REPS, HOST_REPS = 20, 4, 15, 5
STEP_REPS, CHILD_ROUNDS = 40, 2
TEXT_KEYS = ("answer_text", "answer_text_len", "ocr_count")


def time_kernel():
    import numpy as np
    import torch
    from sam_textvqa_amd import answers as A, metrics as M, phoc as P
    sets, packed = [], []
    for i in range(COPIES):
        _, ans, tok = M.make_score_text(B, num_vocab=VOCAB, n_ocr=N_OCR, seed=50 + i, rich=True)
        bd = dict(A.pack_answer_text(ans), **P.pack_ocr_text(tok, N_OCR), ocr_count=M.ocr_counts(tok, N_OCR))
        packed.append(bd)
        sets.append({k: v.cuda() for k, v in bd.items()})
    out = M.score_table_outputs(B, N_OCR, M.DEFAULT_SCORE_CAPS, "cuda")
    fn = lambda s: M.score_tables_from_text(s, out=out, check=False)
    for s in sets:
        fn(s)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        for i in range(ROUNDS):
            fn(sets[i % COPIES])
    g.replay()
    torch.cuda.synchronize()
    us = []
    for _ in range(REPS):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        g.replay()
        e1.record()
        torch.cuda.synchronize()
        us.append(1e3 * e0.elapsed_time(e1) / ROUNDS)
    last = packed[(ROUNDS - 1) % COPIES]
    want, want_status = M.score_tables_from_text_host(last)
    same = all(torch.equal(out[k].cpu().view(torch.int32), want[k].view(torch.int32)) for k in M.SCORE_TABLE_KEYS) and torch.equal(out["status"].cpu(), want_status)
    nbytes = {"text": sum(last[k].numel() * 4 for k in TEXT_KEYS), "table": sum(want[k].numel() * want[k].element_size() for k in M.SCORE_TABLE_KEYS),
              "ocr": sum(want[k].numel() * 4 for k in ("ocr", "ocr_len"))}
    return (float(np.median(us)), min(us), max(us)), same, nbytes


def time_host():
    import numpy as np
    from sam_textvqa_amd import metrics as M
    ms = []
    for r in range(HOST_REPS):
        _, ans, tok = M.make_score_text(B, num_vocab=VOCAB, n_ocr=N_OCR, seed=50 + r % COPIES, rich=True)
        t0 = time.perf_counter()
        M.collate_score_tables([M.build_score_table(a, t, max_ocr_tokens=N_OCR) for a, t in zip(ans, tok)])
        ms.append(1e3 * (time.perf_counter() - t0))
    return float(np.median(ms)), min(ms), max(ms)


def write_batches(path):
    """the step's batch in both forms, on the CPU, into `path` (the parent's child reads the host-table form from it), with the vocabulary's text"""
    import torch
    from sam_textvqa_amd import answers as A, metrics as M, phoc as P
    from sam_textvqa_amd.synthetic import make_batch
    bd = make_batch(B, vocab=VOCAB, device="cpu", seed=77)
    for k in ("targets", "train_prev_inds", "train_loss_mask"):
        del bd[k]
    voc, ans, tok = M.make_score_text(B, num_vocab=VOCAB, n_ocr=N_OCR, seed=9)
    _, a_tabs, s_tabs = M.make_score_tables(B, num_vocab=VOCAB, n_ocr=N_OCR, seed=9)           # the same samples: the metric reads the table loss's predictions
    bd["answer_table"] = A.collate_answer_tables(a_tabs)
    stab = M.collate_score_tables(s_tabs)
    text = dict(A.pack_answer_text(ans), **P.pack_ocr_text(tok, N_OCR), ocr_count=M.ocr_counts(tok, N_OCR))
    torch.save({"host table": dict(bd, score_table=stab), "text": dict(bd, score_text=text), "vocab_text": M.vocab_text(voc)}, path)


def child(path, form):
    """eager step of the package importable from sys.path[0], on the batch `form` of the file: prints one JSON line"""
    import numpy as np
    import torch
    import sam_textvqa_amd.modules as MD
    from sam_textvqa_amd import metrics as M
    from sam_textvqa_amd.synthetic import clone_batch, mmt_config_dict, text_bert_config_dict
    from sam_textvqa_amd.trainer import Trainer
    blob = torch.load(path, weights_only=False)
    to_gpu = lambda d: {k: (v.cuda() if torch.is_tensor(v) else to_gpu(v) if isinstance(v, dict) else v) for k, v in d.items()}
    bd, vt = to_gpu(blob[form]), to_gpu(blob["vocab_text"])
    torch.manual_seed(0)
    model = MD.SAM4C(MD.BertConfig.from_dict(mmt_config_dict(3)), MD.BertConfig.from_dict(text_bert_config_dict()), num_answers=VOCAB, bos_idx=1)
    tr = Trainer(model, base_lr=1e-4, seed=1, use_graph=False, answer_targets="table", predictions=True, metric="textvqa", metric_vocab=vt)
    if form == "text":
        out = M.score_table_outputs(B, N_OCR, M.DEFAULT_SCORE_CAPS, "cuda")

        def step(batch):
            batch["score_table"], _ = M.score_tables_from_text(batch.pop("score_text"), out=out, check=False)
            return tr.step(batch)
    else:
        step = tr.step
    for _ in range(8):
        step(clone_batch(bd))
    torch.cuda.synchronize()
    ms = []
    for _ in range(STEP_REPS):
        batch = clone_batch(bd)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        loss = step(batch)
        e1.record()
        torch.cuda.synchronize()
        ms.append(e0.elapsed_time(e1))
    print(json.dumps({"form": form, "median_ms": float(np.median(ms)), "min_ms": min(ms), "max_ms": max(ms), "loss": float(loss),
                      "metric": float(tr.metric_value())}))


def run_child(root, path, form):
    env = dict(os.environ, PYTHONPATH=root + os.pathsep + os.environ.get("PYTHONPATH", ""))
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", path, "--form", form, "--root", root], env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                       timeout=600, cwd=root)
    if r.returncode != 0:
        raise SystemExit("child (%s, %s) failed with %d:\n%s" % (root, form, r.returncode, r.stderr.decode(errors="replace")[-2000:]))
    return json.loads(r.stdout.decode().strip().splitlines()[-1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--parent", default=None, help="a built checkout of the parent commit")
    ap.add_argument("--child", default=None)
    ap.add_argument("--form", default="text")
    ap.add_argument("--root", default=ROOT)
    args = ap.parse_args()
    sys.path.insert(0, args.root)
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_score_text.py measures on the GPU; none found")
    if args.child:
        return child(args.child, args.form)
    (m, a, z), same, nbytes = time_kernel()
    hm, ha, hz = time_host()
    lines = ["score tables from text, B = %d, 10 answers of up to 128 code points, %d OCR slots, capacities A = 10, Lw = 32, Lg = 128" % (B, N_OCR),
             "kernel output equals the host twin: %s" % same,
             "launch time: us per launch, median (min .. max) of %d replays of %d launches over %d batches" % (REPS, ROUNDS, COPIES),
             "  sam_score_table_from_text                              %8.2f us (%.2f .. %.2f)" % (m, a, z),
             "host functions for the same %d samples: ms per batch, median (min .. max) of %d runs, one host thread" % (B, HOST_REPS),
             "  build_score_table x %d + collate_score_tables          %8.2f ms (%.2f .. %.2f)" % (B, hm, ha, hz),
             "bytes per batch:",
             "  collated score table at the default capacities         %9d   (of which its copy of the OCR text: %d)" % (nbytes["table"], nbytes["ocr"]),
             "  answers' text + lengths + OCR counts instead           %9d   (shipped already where answers.tables_from_text runs: then 0 more)" % nbytes["text"]]
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, "batches.pt")
        write_batches(path)
        variants = [("text", ROOT, "text"), ("host table", ROOT, "host table")] + ([("parent, host table", os.path.abspath(args.parent), "host table")] if args.parent else [])
        runs = {name: [] for name, _, _ in variants}
        for _ in range(CHILD_ROUNDS):
            for name, root, form in variants:
                runs[name].append(run_child(root, path, form))
    lines.append("eager training step with metric=\"textvqa\", c3 model, B = %d: ms per step, median (min .. max) of %d steps, one line per fresh process, variants alternating"
                 % (B, STEP_REPS))
    for name, rs in runs.items():
        for r in rs:
            lines.append("  %-20s %8.3f ms (%.3f .. %.3f)   loss %.6f   metric %.6f" % (name, r["median_ms"], r["min_ms"], r["max_ms"], r["loss"], r["metric"]))
    base = "parent, host table" if args.parent else "host table"
    best = lambda n: min(r["median_ms"] for r in runs[n])
    ratio = best("text") / best(base)
    inside = abs(ratio - 1) <= 0.03
    lines.append("text against %s (best median of each): %+.2f %%  -- %s" % (base, 100 * (ratio - 1), "no change in step time (inside the pool's box-to-box spread of +-3 %)"
                                                                            if inside else ("SLOWER than the spread of +-3 %" if ratio > 1 else "faster than the spread of +-3 %")))
    if not args.parent:
        lines.append("(no --parent checkout given: the parent commit's step was not measured)")
    text = "\n".join(lines)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")
    if not same:
        raise SystemExit("the kernel and the host twin disagree")


if __name__ == "__main__":
    main()

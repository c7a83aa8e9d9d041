#!/usr/bin/env python3
"""Answer tables from text at B = 64, the 5000-word vocabulary, 50 OCR slots: what the launch costs, what the host functions it replaces
cost, what a batch ships either way, and the eager training step with answer text against the same step fed the host-built table.

  kernel     sam_answer_table_from_text: ROUNDS launches captured in one graph, cycling over COPIES distinct batches, replayed REPS times with HIP events
             around each replay; median (min .. max) per launch.  The last batch's table is compared with the host twin.
  host       wall time of build_answer_table per sample + collate_answer_tables of the 64 samples (the strings in, the collated CPU table out), one
             thread of this machine's host, median of HOST_REPS runs over the same COPIES batches.
  bytes      per batch: the answers' text (int32 code points + lengths) and the collated table at the default capacities.
  step       Trainer(use_graph=False) at bench.py's default shapes (c3 model, B = 64, 5000 words): STEP_REPS steps timed one by one with HIP events,
             median.  Every variant runs in a fresh child process of this script, the variants alternating, CHILD_ROUNDS times each:
               text          this tree, the batch carries answer_text / answer_text_len; answers.tables_from_text(check=False) builds its answer_table on
                             the GPU inside the timed region, in front of Trainer.step
               host table    this tree, the batch carries the collated answer_table (the code a batch without the new keys always ran)
               parent        --parent DIR: a built checkout of the parent commit, the same host-table batch (read from a file this script writes)

    python tools/bench_answer_text.py [--parent DIR] [--out profiles/answer_text_bench.txt]"""
import argparse
import json
import os
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

B, N_OCR, LW, VOCAB = 64, 50, 32, 5000
ROUNDS, COPIES, REPS, HOST_REPS = 20, 4, 15, 5
STEP_REPS, CHILD_ROUNDS = 40, 2


def samples(seed):
    """answers.make_answer_tables' synthetic samples as strings: (answers per sample, tokens per sample) over the VOCAB-word vocabulary"""
    import numpy as np
    rng = np.random.RandomState(seed)
    answers, tokens = [], []
    for _ in range(B):
        n_tok = rng.randint(1, N_OCR + 1)
        pool = ["w%d" % i for i in rng.randint(0, VOCAB - 4, 8)] + ["oov%d" % i for i in rng.randint(0, 40, 8)]
        toks = [pool[i] for i in rng.randint(0, len(pool), n_tok)]
        cands = []
        for _ in range(4):
            src = toks if rng.rand() < 0.6 else ["w%d" % i for i in rng.randint(0, VOCAB - 4, 3)]
            cands.append(" ".join(src[i] for i in rng.randint(0, len(src), rng.randint(1, 4))))
        cands.append("unmatched%d" % rng.randint(1000))
        answers.append([cands[i] for i in rng.choice(len(cands), 10, p=[0.4, 0.25, 0.15, 0.1, 0.1])])
        tokens.append(toks)
    return answers, tokens


def vocabulary():
    from sam_textvqa_amd import answers as A
    return A.AnswerVocab([A.PAD_TOKEN, A.BOS_TOKEN, A.EOS_TOKEN, A.UNK_TOKEN] + ["w%d" % i for i in range(VOCAB - 4)])


def time_kernel(voc):
    import numpy as np
    import torch
    from sam_textvqa_amd import answers as A, phoc as P
    index = A.index_to(A.vocab_index(voc), "cuda")
    sets, packed = [], []
    for i in range(COPIES):
        ans, tok = samples(50 + i)
        bd = dict(A.pack_answer_text(ans), **P.pack_ocr_text(tok, N_OCR, LW))
        packed.append(bd)
        sets.append({k: v.cuda() for k, v in bd.items()})
    out = A.table_outputs(B, A.DEFAULT_CAPS, "cuda")
    fn = lambda s: A.tables_from_text(s, index, out=out, check=False)
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
    want, want_status = A.tables_from_text_host(last["answer_text"], last["answer_text_len"], last["ocr_text"], last["ocr_text_len"], voc)
    same = all(torch.equal(out[k].cpu(), want[k]) for k in A.TABLE_KEYS) and torch.equal(out["status"].cpu(), want_status)
    nbytes = {"text": sum(last[k].numel() * 4 for k in A.ANSWER_TEXT_KEYS), "table": sum(want[k].numel() * want[k].element_size() for k in A.TABLE_KEYS)}
    return (float(np.median(us)), min(us), max(us)), same, nbytes


def time_host(voc):
    import numpy as np
    from sam_textvqa_amd import answers as A
    ms = []
    for r in range(HOST_REPS):
        ans, tok = samples(50 + r % COPIES)
        t0 = time.perf_counter()
        A.collate_answer_tables([A.build_answer_table(a, t, voc, max_ocr_tokens=N_OCR) for a, t in zip(ans, tok)])
        ms.append(1e3 * (time.perf_counter() - t0))
    return float(np.median(ms)), min(ms), max(ms)


def write_batches(path, voc):
    """the step's batch in both forms, on the CPU, into `path` (the parent's child reads the host-table form from it)"""
    import torch
    from sam_textvqa_amd import answers as A, phoc as P
    from sam_textvqa_amd.synthetic import make_batch
    bd = make_batch(B, vocab=VOCAB, device="cpu", seed=77)
    for k in ("targets", "train_prev_inds", "train_loss_mask", "ocr_phoc"):
        del bd[k]
    ans, tok = samples(9)
    bd.update(P.pack_ocr_text(tok, N_OCR, LW))
    table = A.collate_answer_tables([A.build_answer_table(a, t, voc, max_ocr_tokens=N_OCR) for a, t in zip(ans, tok)])
    torch.save({"host table": dict(bd, answer_table=table), "text": dict(bd, **A.pack_answer_text(ans))}, path)


def child(path, form):
    """eager step of the package importable from sys.path[0], on the batch `form` of the file: prints one JSON line"""
    import numpy as np
    import torch
    import sam_textvqa_amd.modules as M
    from sam_textvqa_amd.synthetic import clone_batch, mmt_config_dict, text_bert_config_dict
    from sam_textvqa_amd.trainer import Trainer
    bd = torch.load(path, weights_only=False)[form]
    bd = {k: (v.cuda() if torch.is_tensor(v) else {kk: (vv.cuda() if torch.is_tensor(vv) else vv) for kk, vv in v.items()} if isinstance(v, dict) else v)
          for k, v in bd.items()}
    torch.manual_seed(0)
    model = M.SAM4C(M.BertConfig.from_dict(mmt_config_dict(3)), M.BertConfig.from_dict(text_bert_config_dict()), num_answers=VOCAB, bos_idx=1)
    from sam_textvqa_amd import answers as A
    tr = Trainer(model, base_lr=1e-4, seed=1, use_graph=False)
    if form == "text":
        index, out = A.index_to(A.vocab_index(vocabulary()), "cuda"), A.table_outputs(B, A.DEFAULT_CAPS, "cuda")

        def step(batch):
            text = {k: batch.pop(k) for k in A.ANSWER_TEXT_KEYS}
            batch["answer_table"], _ = A.tables_from_text(dict(text, ocr_text=batch["ocr_text"], ocr_text_len=batch["ocr_text_len"]), index, out=out, check=False)
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
    print(json.dumps({"form": form, "median_ms": float(np.median(ms)), "min_ms": min(ms), "max_ms": max(ms), "loss": float(loss)}))


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
        raise SystemExit("bench_answer_text.py measures on the GPU; none found")
    if args.child:
        return child(args.child, args.form)
    voc = vocabulary()
    (m, a, z), same, nbytes = time_kernel(voc)
    hm, ha, hz = time_host(voc)
    lines = ["answer tables from text, B = %d, %d-word vocabulary, %d OCR slots, Lw = %d, 10 answers of up to 128 code points" % (B, VOCAB, N_OCR, LW),
             "kernel output equals the host twin: %s" % same,
             "launch time: us per launch, median (min .. max) of %d replays of %d launches over %d batches" % (REPS, ROUNDS, COPIES),
             "  sam_answer_table_from_text                             %8.2f us (%.2f .. %.2f)" % (m, a, z),
             "host functions for the same %d samples: ms per batch, median (min .. max) of %d runs, one host thread" % (B, HOST_REPS),
             "  build_answer_table x %d + collate_answer_tables        %8.2f ms (%.2f .. %.2f)" % (B, hm, ha, hz),
             "bytes per batch:",
             "  answers' text: int32 code points + lengths             %9d" % nbytes["text"],
             "  collated answer table at the default capacities        %9d" % nbytes["table"]]
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, "batches.pt")
        write_batches(path, voc)
        variants = [("text", ROOT, "text"), ("host table", ROOT, "host table")] + ([("parent, host table", os.path.abspath(args.parent), "host table")] if args.parent else [])
        runs = {name: [] for name, _, _ in variants}
        for _ in range(CHILD_ROUNDS):
            for name, root, form in variants:
                runs[name].append(run_child(root, path, form))
    lines.append("eager training step, c3 model, B = %d: ms per step, median (min .. max) of %d steps, one line per fresh process, variants alternating" % (B, STEP_REPS))
    for name, rs in runs.items():
        for r in rs:
            lines.append("  %-20s %8.3f ms (%.3f .. %.3f)   loss %.6f" % (name, r["median_ms"], r["min_ms"], r["max_ms"], r["loss"]))
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

#!/usr/bin/env python3
"""Question ids from text at B = 64, T = 20, a 30 522-entry synthetic WordPiece vocabulary: what the launch costs, what the host work it
replaces costs, and the training step -- eager and captured -- with the question's text against the same step fed the host twin's ids.

  kernel     sam_wordpiece_from_text: ROUNDS launches captured in one graph, cycling over COPIES distinct batches, replayed REPS times with HIP events around
             each replay; median (min .. max) per launch.  The last batch's output is compared with the host twin.
  host       wall time per batch of 64 questions, one thread of this machine's host, median of HOST_REPS runs: wordpiece.encode_questions (the packer + the
             host twin, plain Python), wordpiece.pack_question_text alone (what a text batch still does on the host), and -- when transformers imports --
             its BertTokenizer(vocab, do_lower_case=True).encode per question.
  step       Trainer at bench.py's default shapes (c3 model, B = 64, 5000 answer words), use_graph False and True: STEP_REPS steps timed one by one with HIP
             events, median.  Every variant runs in a fresh child process of this script, the variants alternating, CHILD_ROUNDS times each:
               text          this tree, the batch carries question_text / question_text_len; the launch is part of the model's forward (a node of the graph)
               host ids      this tree, the batch carries question_indices / question_mask (the code a batch without the new keys always ran)
               parent        --parent DIR: a built checkout of the parent commit, the same host-ids batch (read from a file this script writes)

    python tools/bench_question_text.py [--parent DIR] [--out profiles/question_text_bench.txt]"""
import argparse
import json
import os
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

B, T, VOCAB, ANSWERS = 64, 20, 30522, 5000
ROUNDS, COPIES, REPS, HOST_REPS = 20, 4, 15, 5
STEP_REPS, CHILD_ROUNDS = 40, 2


def vocabulary():
    """30 522 entries in the proportions of an uncased BERT vocabulary: specials, single characters, whole words, a fifth of them "##" pieces"""
    words = ["[PAD]"] + ["[unused%d]" % i for i in range(99)] + ["[UNK]", "[CLS]", "[SEP]", "[MASK]"]
    words += [chr(c) for c in range(33, 127) if not ("A" <= chr(c) <= "Z")]
    words += ["##" + chr(c) for c in range(ord("a"), ord("z") + 1)] + ["##" + str(d) for d in range(10)]
    k, seen = 0, set(words)
    syll = [a + b for a in "bcdfghjklmnprstvwz" for b in "aeiou"]
    while len(words) < VOCAB:
        w = "".join(syll[(k // len(syll) ** i) % len(syll)] for i in range(2 + k % 3))
        w = "##" + w if k % 5 == 4 else w
        if w not in seen:
            seen.add(w)
            words.append(w)
        k += 1
    return words


def questions(words, seed):
    import random
    rng = random.Random(seed)
    plain = [w for w in words[300:] if not w.startswith("##")]
    tails = [w[2:] for w in words[300:] if w.startswith("##")]
    out = []
    for _ in range(B):
        ws = [rng.choice(plain) + (rng.choice(tails) if rng.random() < 0.3 else "") for _ in range(rng.randint(5, 14))]
        q = " ".join(ws) + rng.choice(["?", " ?", ""])
        out.append(q.capitalize() if rng.random() < 0.5 else q)
    return out


def time_kernel(words):
    import numpy as np
    import torch
    from sam_textvqa_amd import answers as A, wordpiece as W
    host_index = W.vocab_index(words)
    index = A.index_to(host_index, "cuda")
    packed = [W.pack_question_text(questions(words, 50 + i)) for i in range(COPIES)]
    sets = [{k: v.cuda() for k, v in p.items()} for p in packed]
    out = W.outputs(B, T, "cuda")
    fn = lambda s: W.from_text(s["question_text"], s["question_text_len"], index, T, out=out)
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
    want = W.encode_host(last["question_text"], last["question_text_len"], host_index, T)
    same = all(torch.equal(out[k].cpu(), want[k]) for k in W.QUESTION_KEYS)
    return (float(np.median(us)), min(us), max(us)), same, host_index, float(want["num_question_tokens"].float().mean())


def time_host(words, index):
    import numpy as np
    from sam_textvqa_amd import wordpiece as W

    def timed(fn):
        ms = []
        for r in range(HOST_REPS):
            qs = questions(words, 50 + r % COPIES)
            t0 = time.perf_counter()
            fn(qs)
            ms.append(1e3 * (time.perf_counter() - t0))
        return float(np.median(ms)), min(ms), max(ms)
    res = {"encode_questions (packer + host twin)": timed(lambda qs: W.encode_questions(qs, index, T)), "pack_question_text alone": timed(W.pack_question_text)}
    try:
        os.environ.setdefault("HF_HUB_OFFLINE", "1")
        os.environ.setdefault("TRANSFORMERS_OFFLINE", "1")
        from transformers import BertTokenizer
    except Exception:
        return res, None
    with tempfile.TemporaryDirectory() as d:
        path = os.path.join(d, "vocab.txt")
        with open(path, "w", encoding="utf-8") as f:
            f.write("\n".join(words) + "\n")
        tok = BertTokenizer(path, do_lower_case=True)
        qs = questions(words, 50)
        agree = [tok.encode(q, add_special_tokens=True)[:T] for q in qs] == [r[:int(n)].tolist() for r, n in zip(*(lambda e: (e["question_indices"], e["num_question_tokens"]))(
            W.encode_questions(qs, index, T)))]
        res["transformers BertTokenizer.encode x %d" % B] = timed(lambda qs: [tok.encode(q, add_special_tokens=True)[:T] for q in qs])
    return res, agree


def write_batches(path, words, index):
    """the step's batch in both forms, on the CPU, into `path` (the parent's child reads the host-ids form from it)"""
    import torch
    from sam_textvqa_amd import wordpiece as W
    from sam_textvqa_amd.synthetic import make_batch
    bd = make_batch(B, vocab=ANSWERS, device="cpu", seed=77)
    packed = W.pack_question_text(questions(words, 9))
    enc = W.encode_host(packed["question_text"], packed["question_text_len"], index, T)
    text = {k: v for k, v in bd.items() if k not in ("question_indices", "question_mask")}
    torch.save({"host ids": dict(bd, question_indices=enc["question_indices"], question_mask=enc["question_mask"]), "text": dict(text, **packed),
                "index": {k: index[k] for k in ("cp", "len", "slots", "V", "PAD", "UNK", "CLS", "SEP")}}, path)


def child(path, form, use_graph):
    """training steps of the package importable from sys.path[0], on the batch `form` of the file: prints one JSON line"""
    import numpy as np
    import torch
    import sam_textvqa_amd.modules as M
    from sam_textvqa_amd.synthetic import clone_batch, mmt_config_dict, text_bert_config_dict
    from sam_textvqa_amd.trainer import Trainer
    blob = torch.load(path, weights_only=False)
    bd = blob[form]
    bd = {k: (v.cuda() if torch.is_tensor(v) else {kk: (vv.cuda() if torch.is_tensor(vv) else vv) for kk, vv in v.items()} if isinstance(v, dict) else v)
          for k, v in bd.items()}
    torch.manual_seed(0)
    model = M.SAM4C(M.BertConfig.from_dict(mmt_config_dict(3)), M.BertConfig.from_dict(text_bert_config_dict()), num_answers=ANSWERS, bos_idx=1)
    if form == "text":
        model.set_question_vocab(blob["index"])
    tr = Trainer(model, base_lr=1e-4, seed=1, use_graph=use_graph)
    for _ in range(8):
        tr.step(clone_batch(bd))
    torch.cuda.synchronize()
    if use_graph and tr._graph is None:
        raise SystemExit("the step was not captured")
    ms = []
    for _ in range(STEP_REPS):
        batch = clone_batch(bd)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        loss = tr.step(batch)
        e1.record()
        torch.cuda.synchronize()
        ms.append(e0.elapsed_time(e1))
    print(json.dumps({"form": form, "graph": bool(use_graph), "median_ms": float(np.median(ms)), "min_ms": min(ms), "max_ms": max(ms), "loss": float(loss)}))


def run_child(root, path, form, use_graph):
    env = dict(os.environ, PYTHONPATH=root + os.pathsep + os.environ.get("PYTHONPATH", ""))
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", path, "--form", form, "--root", root] + (["--graph"] if use_graph else []), env=env,
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=600, cwd=root)
    if r.returncode != 0:
        raise SystemExit("child (%s, %s, graph=%s) failed with %d:\n%s" % (root, form, use_graph, r.returncode, r.stderr.decode(errors="replace")[-2000:]))
    return json.loads(r.stdout.decode().strip().splitlines()[-1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--parent", default=None, help="a built checkout of the parent commit")
    ap.add_argument("--child", default=None)
    ap.add_argument("--form", default="text")
    ap.add_argument("--graph", action="store_true")
    ap.add_argument("--root", default=ROOT)
    args = ap.parse_args()
    sys.path.insert(0, args.root)
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_question_text.py measures on the GPU; none found")
    if args.child:
        return child(args.child, args.form, args.graph)
    words = vocabulary()
    (m, a, z), same, index, mean_tokens = time_kernel(words)
    host, agree = time_host(words, index)
    lines = ["question ids from text, B = %d, T = %d, %d-entry synthetic vocabulary, Lq = 256, %.1f tokens per question" % (B, T, VOCAB, mean_tokens),
             "kernel output equals the host twin: %s" % same,
             "host twin equals the installed BertTokenizer on one batch: %s" % ("transformers not importable, not compared" if agree is None else agree),
             "launch time: us per launch, median (min .. max) of %d replays of %d launches over %d batches" % (REPS, ROUNDS, COPIES),
             "  sam_wordpiece_from_text                                %8.2f us (%.2f .. %.2f)" % (m, a, z),
             "host work for the same %d questions: ms per batch, median (min .. max) of %d runs, one host thread" % (B, HOST_REPS)]
    for name, (hm, ha, hz) in host.items():
        lines.append("  %-52s %8.2f ms (%.2f .. %.2f)" % (name, hm, ha, hz))
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, "batches.pt")
        write_batches(path, words, index)
        variants = [("text", ROOT, "text"), ("host ids", ROOT, "host ids")] + ([("parent, host ids", os.path.abspath(args.parent), "host ids")] if args.parent else [])
        runs = {(name, g): [] for g in (False, True) for name, _, _ in variants}
        for _ in range(CHILD_ROUNDS):
            for g in (False, True):
                for name, root, form in variants:
                    runs[(name, g)].append(run_child(root, path, form, g))
                    print("%s, %s: %.3f ms" % (name, "captured" if g else "eager", runs[(name, g)][-1]["median_ms"]), file=sys.stderr, flush=True)
    base = "parent, host ids" if args.parent else "host ids"
    best = lambda n, g: min(r["median_ms"] for r in runs[(n, g)])
    for g in (False, True):
        lines.append("%s training step, c3 model, B = %d: ms per step, median (min .. max) of %d steps, one line per fresh process, variants alternating" % (
            "captured" if g else "eager", B, STEP_REPS))
        for name, _, _ in variants:
            for r in runs[(name, g)]:
                lines.append("  %-20s %8.3f ms (%.3f .. %.3f)   loss %.6f" % (name, r["median_ms"], r["min_ms"], r["max_ms"], r["loss"]))
        ratio = best("text", g) / best(base, g)
        lines.append("  text against %s (best median of each): %+.2f %%  -- %s" % (base, 100 * (ratio - 1), "no change in step time (inside the pool's box-to-box spread of +-3 %)"
                                                                                  if abs(ratio - 1) <= 0.03 else ("SLOWER than the spread of +-3 %" if ratio > 1 else "faster than the spread of +-3 %")))
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

#!/usr/bin/env python3
"""Question ids from text at B = 64, T = 20, a 30 522-entry synthetic WordPiece vocabulary: what the launch costs, what the host work it
replaces costs, and the training step -- eager and captured -- with the question's text against the same step fed the host twin's ids.

  kernel     sam_wordpiece_from_text over COPIES distinct batches (measure.replay_us).  The last batch's output is compared with the host twin.
  host       wall time per batch of 64 questions, one thread of this machine's host, HOST_REPS runs (measure.host_ms): wordpiece.encode_questions (the packer + the
             host twin, plain Python), wordpiece.pack_question_text alone (what a text batch still does on the host), and -- when transformers imports --
             its BertTokenizer(vocab, do_lower_case=True).encode per question.
  step       Trainer at bench.py's default shapes (c3 model, B = 64, 5000 answer words), use_graph False and True; the captured step too is fed a
             clone of the batch (in_place=False: its staging copies are inside the timed region).  CHILD_ROUNDS fresh processes per variant (measure.step_ab):
               text          this tree, the batch carries question_text / question_text_len; the launch is part of the model's forward (a node of the graph)
               host ids      this tree, the batch carries question_indices / question_mask (the code a batch without the new keys always ran)
               parent        --parent DIR: a built checkout of the parent commit, the same host-ids batch (read from a file this script writes)

How each number is taken: tools/measure.py.

    python tools/bench_question_text.py [--parent DIR] [--out profiles/question_text_bench.txt]"""
import os
import sys
import tempfile

import measure

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
    import torch
    from sam_textvqa_amd import answers as A, wordpiece as W
    host_index = W.vocab_index(words)
    index = A.index_to(host_index, "cuda")
    packed = [W.pack_question_text(questions(words, 50 + i)) for i in range(COPIES)]
    sets = [{k: v.cuda() for k, v in p.items()} for p in packed]
    out = W.outputs(B, T, "cuda")
    us, _ = measure.replay_us(lambda s: W.from_text(s["question_text"], s["question_text_len"], index, T, out=out), sets, ROUNDS, REPS)
    last = packed[(ROUNDS - 1) % COPIES]
    want = W.encode_host(last["question_text"], last["question_text_len"], host_index, T)
    same = all(torch.equal(out[k].cpu(), want[k]) for k in W.QUESTION_KEYS)
    return us, same, host_index, float(want["num_question_tokens"].float().mean())


def time_host(words, index):
    from sam_textvqa_amd import wordpiece as W
    batches = [questions(words, 50 + r % COPIES) for r in range(HOST_REPS)]
    timed = lambda fn: measure.host_ms(lambda r: fn(batches[r]), HOST_REPS)
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
    def make_step(trainer, batch, form):
        if form == "text":
            import torch
            trainer.model.set_question_vocab(torch.load(path, weights_only=False)["index"])
        return trainer.step
    measure.step_child(path, form, make_step, use_graph=use_graph, warm=8, reps=STEP_REPS, num_answers=ANSWERS, in_place=False, extra=lambda tr: {"graph": bool(use_graph)})


def main():
    ap = measure.arg_parser(parent=True, child=True)
    ap.add_argument("--graph", action="store_true")
    args = ap.parse_args()
    sys.path.insert(0, args.root)
    measure.require_gpu("bench_question_text.py")
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
        modes = {"eager": [], "captured": ["--graph"]}
        runs = measure.step_ab(__file__, [((name, mode), root, form, flag) for mode, flag in modes.items() for name, root, form in variants], path, CHILD_ROUNDS)
    for mode in modes:
        lines.append("%s training step, c3 model, B = %d: ms per step, median (min .. max) of %d steps, one line per fresh process, variants alternating" % (mode, B, STEP_REPS))
        of_g = {name: runs[(name, mode)] for name, _, _ in variants}
        lines += measure.step_lines(of_g) + ["  " + measure.verdict("text", "host ids", of_g)[0]]
    if not args.parent:
        lines.append(measure.NO_PARENT)
    measure.finish(lines, args.out, same, "the kernel and the host twin disagree")


if __name__ == "__main__":
    main()

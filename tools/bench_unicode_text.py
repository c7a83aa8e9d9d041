#!/usr/bin/env python3
"""Lowering and normalising Unicode text on the device at B = 64, 50 OCR slots of Lw = 32, 10 answers of La = 128 and one question of Lq = 256 (DESIGN.md
§3.21): what the three launches cost, what the host work they replace costs, what the table lookup adds to a launch, and the eager training step with
textprep.materialize(unicode=...) in front against the parent commit's step on host-packed text.  NON_ASCII of the strings are not ASCII (accented
capitals, Greek with final sigmas, U+0130, CJK in the questions); the rest is tools/bench_textprep.py's text.

  kernel     materialize(unicode=...)'s three launches (sam_text_from_utf8_unicode for the OCR slots and the answers, sam_question_from_utf8): ROUNDS
             triples captured in one graph, cycling over COPIES distinct batches, replayed REPS times with HIP events around each replay; median
             (min .. max) per triple.  The same for the two text launches alone, with and without the table, on the SAME host-lowered bytes: the
             difference is the table's lookup cost.  The last batch's tensors are compared with the host route's.
  host       wall time, one host thread, median of HOST_REPS runs over the same batches: wordpiece.pack_question_text, and the str.lower() pass of
             textprep.pack_utf8 (pack_utf8 with host lowering minus pack_utf8(host_lower=False)).
  step       Trainer(use_graph=False) at bench.py's default shapes (c3 model, B = 64, 5000 words) with answers.tables_from_text in front, as
             tools/bench_textprep.py runs it: STEP_REPS steps timed one by one with HIP events, median.  Every variant runs in a fresh child process of
             this script, the variants alternating, CHILD_ROUNDS times each:
               unicode       this tree, materialize(unicode=table, check=False) of unlowered bytes and the raw questions inside the timed region (the
                             question text it writes is set aside: the step reads the batch's question_indices, as the parent's does)
               parent        --parent DIR: a built checkout of the parent commit, materialize(check=False) of the host-lowered bytes inside the timed
                             region (the parent's route for the same strings; its question packing is host work and is listed under `host`)

    python tools/bench_unicode_text.py [--parent DIR] [--out profiles/unicode_text_bench.txt]"""
import argparse
import json
import os
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from bench_textprep import raw_strings, word_cleaner        # noqa: E402  (the same dirty strings as §3.20's measurement)

B, N_OCR, N_ANS, LW, LA, LQ, VOCAB = 64, 50, 10, 32, 128, 256, 5000
NON_ASCII = 0.25
ROUNDS, COPIES, REPS, HOST_REPS = 20, 4, 15, 5
STEP_REPS, CHILD_ROUNDS = 40, 2
_ACCENT = str.maketrans("aeiouAEIOUsScCnN", "áéíóúÁÉÍÓÚßẞçÇñÑ")
_GREEK = ["ΟΔΟΣ", "ΣΟΦΟΣ", "ΑΘΗΝΑ", "İstanbul", "STRAẞE"]
_QUESTIONS = ["What is the name of this store?", "what does the sign say", "Which BRAND is on the bottle?", "what time is it on the clock?", "who is the author"]
_QUESTIONS_NA = ["Quel est le nom du CAFÉ?", "Τι γράφει η ΠΙΝΑΚΙΔΑ ΤΗΣ ΟΔΟΥ;", "この看板は何と書いてありますか", "¿QUÉ dice el LETRERO de la señal?", "Was steht auf dem STRAẞENSCHILD?"]


def strings(seed):
    """(raw answers, raw OCR tokens, questions) per sample, NON_ASCII of each not ASCII"""
    import numpy as np
    answers, tokens = raw_strings(seed)
    rng = np.random.RandomState(seed + 11)

    def some(s):
        if rng.rand() >= NON_ASCII:
            return s
        return _GREEK[rng.randint(len(_GREEK))] if rng.rand() < 0.2 or s.translate(_ACCENT) == s else s.translate(_ACCENT)
    questions = [(_QUESTIONS_NA if rng.rand() < NON_ASCII else _QUESTIONS)[rng.randint(5)] for _ in range(B)]
    return [[some(a) for a in ans] for ans in answers], [[some(t) for t in tok] for tok in tokens], questions


def raw_route(answers, tokens, questions=None, host_lower=True):
    from sam_textvqa_amd import textprep as T
    po, pa = T.pack_utf8(tokens, N_OCR, host_lower=host_lower), T.pack_utf8(answers, N_ANS, host_lower=host_lower)
    out = {"ocr_raw": po["raw"], "ocr_raw_off": po["raw_off"], "ocr_count": po["count"], "answer_raw": pa["raw"], "answer_raw_off": pa["raw_off"]}
    if questions is not None:
        from sam_textvqa_amd import wordpiece as W
        out.update(W.pack_question_utf8(questions))
    return out


def replay_us(fn, sets):
    import numpy as np
    import torch
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
    return float(np.median(us)), min(us), max(us)


def time_kernels():
    import torch
    from sam_textvqa_amd import ops, unicode_table as U, wordpiece as W
    table_host = U.build()
    table = U.to(table_host, "cuda")
    strs = [strings(50 + i) for i in range(COPIES)]
    unlowered = [{k: v.cuda() for k, v in raw_route(*s, host_lower=False).items()} for s in strs]
    lowered = [{k: v.cuda() for k, v in raw_route(s[0], s[1]).items()} for s in strs]
    outs = [{"text": torch.empty((B * n, L), dtype=torch.int32, device="cuda"), "text_len": torch.empty(B * n, dtype=torch.int32, device="cuda"),
             "status": torch.empty(B * n, dtype=torch.int32, device="cuda")} for n, L in ((N_OCR, LW), (N_ANS, LA))]
    qout = {"question_text": torch.empty((B, LQ), dtype=torch.int32, device="cuda"), "question_text_len": torch.empty(B, dtype=torch.int32, device="cuda"),
            "status": torch.empty(B, dtype=torch.int32, device="cuda")}

    def text_pair(s, unicode):
        ops.text_from_utf8(s["ocr_raw"], s["ocr_raw_off"], LW, 15, out=outs[0], unicode=unicode)
        ops.text_from_utf8(s["answer_raw"], s["answer_raw_off"], LA, 15, out=outs[1], unicode=unicode)

    def triple(s):
        text_pair(s, table)
        ops.question_from_utf8(s["question_raw"], s["question_raw_off"], LQ, table, out=qout)
    ascii_pair = replay_us(lambda s: text_pair(s, None), lowered)
    table_pair = replay_us(lambda s: text_pair(s, table), lowered)
    question = replay_us(lambda s: ops.question_from_utf8(s["question_raw"], s["question_raw_off"], LQ, table, out=qout), unlowered)
    all_three = replay_us(triple, unlowered)
    ans, tok, qs = strs[(ROUNDS - 1) % COPIES]
    want_q = W.pack_question_text(qs, max_chars=LQ)
    clean = lambda groups, n, L: [[word_cleaner(x) for x in g] for g in groups]
    from sam_textvqa_amd import answers as A, phoc as P
    want = dict(P.pack_ocr_text(clean(tok, N_OCR, LW), N_OCR, max_chars=LW), **A.pack_answer_text(clean(ans, N_ANS, LA), N_ANS, max_chars=LA))
    same = torch.equal(outs[0]["text"].cpu().view(B, N_OCR, LW), want["ocr_text"]) and torch.equal(outs[0]["text_len"].cpu().view(B, N_OCR), want["ocr_text_len"]) and \
        torch.equal(outs[1]["text"].cpu().view(B, N_ANS, LA), want["answer_text"]) and torch.equal(outs[1]["text_len"].cpu().view(B, N_ANS), want["answer_text_len"]) and \
        torch.equal(qout["question_text"].cpu(), want_q["question_text"]) and torch.equal(qout["question_text_len"].cpu(), want_q["question_text_len"]) and \
        not any(o["status"].any().item() for o in outs + [qout])
    share = sum(not x.isascii() for s in strs for grp in s[0] + s[1] for x in grp) / float(sum(len(grp) for s in strs for grp in s[0] + s[1]))
    return dict(ascii_pair=ascii_pair, table_pair=table_pair, question=question, all_three=all_three), same, share, U.nbytes(table_host)


def time_host():
    import numpy as np
    from sam_textvqa_amd import wordpiece as W
    q, low, plain = [], [], []
    for r in range(HOST_REPS):
        ans, tok, qs = strings(50 + r % COPIES)
        t0 = time.perf_counter()
        W.pack_question_text(qs, max_chars=LQ)
        t1 = time.perf_counter()
        raw_route(ans, tok)
        t2 = time.perf_counter()
        raw_route(ans, tok, host_lower=False)
        t3 = time.perf_counter()
        q.append(1e3 * (t1 - t0))
        low.append(1e3 * (t2 - t1))
        plain.append(1e3 * (t3 - t2))
    stat = lambda v: (float(np.median(v)), min(v), max(v))
    return stat(q), stat(low), stat(plain)


def write_batches(path):
    """the step's batch in both forms, on the CPU, into `path` (the parent's child reads the host-lowered form from it)"""
    import torch
    from sam_textvqa_amd.synthetic import make_batch
    bd = make_batch(B, vocab=VOCAB, device="cpu", seed=77)
    for k in ("targets", "train_prev_inds", "train_loss_mask", "ocr_phoc"):
        del bd[k]
    ans, tok, qs = strings(9)
    torch.save({"parent": dict(bd, **raw_route(ans, tok)), "unicode": dict(bd, **raw_route(ans, tok, qs, host_lower=False))}, path)


def child(path, form):
    """eager step of the package importable from sys.path[0], on the batch `form` of the file: prints one JSON line"""
    import numpy as np
    import torch
    import sam_textvqa_amd.modules as MD
    from sam_textvqa_amd import answers as A, metrics as M, textprep as T
    from sam_textvqa_amd.synthetic import clone_batch, mmt_config_dict, text_bert_config_dict
    from sam_textvqa_amd.trainer import Trainer
    to_gpu = lambda d: {k: (v.cuda() if torch.is_tensor(v) else to_gpu(v) if isinstance(v, dict) else v) for k, v in d.items()}
    bd = to_gpu(torch.load(path, weights_only=False)[form])
    voc = M.make_score_text(1, num_vocab=VOCAB, n_ocr=N_OCR, seed=9, rich=True)[0]
    index, out = A.index_to(A.vocab_index(voc), "cuda"), A.table_outputs(B, A.DEFAULT_CAPS, "cuda")
    torch.manual_seed(0)
    model = MD.SAM4C(MD.BertConfig.from_dict(mmt_config_dict(3)), MD.BertConfig.from_dict(text_bert_config_dict()), num_answers=VOCAB, bos_idx=1)
    tr = Trainer(model, base_lr=1e-4, seed=1, use_graph=False)
    kw = {}
    if form == "unicode":
        from sam_textvqa_amd import unicode_table as U
        kw = dict(unicode=U.to(U.build(), "cuda"), question_chars=LQ)

    def step(batch):
        ids = {k: batch.pop(k) for k in ("question_indices", "question_mask")} if kw else {}       # (raw questions next to their ids are refused)
        T.materialize(batch, ocr_chars=LW, answer_chars=LA, check=False, **kw)
        batch.pop("question_text", None), batch.pop("question_text_len", None)
        batch.update(ids)
        text = {k: batch.pop(k) for k in A.ANSWER_TEXT_KEYS}
        batch["answer_table"], _ = A.tables_from_text(dict(text, ocr_text=batch["ocr_text"], ocr_text_len=batch["ocr_text_len"]), index, out=out, check=False)
        return tr.step(batch)
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
    """this file's child against the package under `root` (the parent's tree has no such script; its form touches nothing new)"""
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
    ap.add_argument("--form", default="unicode")
    ap.add_argument("--root", default=ROOT)
    args = ap.parse_args()
    sys.path.insert(0, args.root)
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_unicode_text.py measures on the GPU; none found")
    if args.child:
        return child(args.child, args.form)
    k, same, share, resident = time_kernels()
    hq, hlow, hplain = time_host()
    f = lambda t: "%8.2f us (%.2f .. %.2f)" % t
    lines = ["Unicode text on the device, B = %d: %d OCR slots of Lw = %d, %d answers of La = %d, one question of Lq = %d; %.1f %% of the OCR / answer strings are not ASCII"
             % (B, N_OCR, LW, N_ANS, LA, LQ, 100 * share),
             "resident table: %d bytes" % resident,
             "kernel output equals the host route's (word_cleaner + packers, pack_question_text): %s" % same,
             "launch time: us, median (min .. max) of %d replays of %d rounds over %d batches" % (REPS, ROUNDS, COPIES),
             "  sam_text_from_utf8 x 2, host-lowered bytes (the parent's launches)       " + f(k["ascii_pair"]),
             "  sam_text_from_utf8_unicode x 2, the same bytes                           " + f(k["table_pair"]),
             "  -> the table's lookup cost per pair of launches                          %8.2f us" % (k["table_pair"][0] - k["ascii_pair"][0]),
             "  sam_question_from_utf8 (%d questions)                                    " % B + f(k["question"]),
             "  all three launches of materialize(unicode=...), unlowered bytes          " + f(k["all_three"]),
             "host work they replace, ms per batch, median (min .. max) of %d runs, one host thread" % HOST_REPS,
             "  wordpiece.pack_question_text                                             %8.3f ms (%.3f .. %.3f)" % hq,
             "  pack_utf8 x 2 with the str.lower() pass                                  %8.3f ms (%.3f .. %.3f)" % hlow,
             "  pack_utf8 x 2, host_lower=False                                          %8.3f ms (%.3f .. %.3f)" % hplain,
             "  -> the str.lower() pass                                                  %8.3f ms" % (hlow[0] - hplain[0])]
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, "batches.pt")
        write_batches(path)
        variants = [("unicode", ROOT, "unicode")] + ([("parent", os.path.abspath(args.parent), "parent")] if args.parent else [])
        runs = {name: [] for name, _, _ in variants}
        for _ in range(CHILD_ROUNDS):
            for name, root, form in variants:
                runs[name].append(run_child(root, path, form))
    lines.append("eager training step with materialize in front, c3 model, B = %d: ms per step, median (min .. max) of %d steps, one line per fresh process, variants alternating"
                 % (B, STEP_REPS))
    for name, rs in runs.items():
        for r in rs:
            lines.append("  %-20s %8.3f ms (%.3f .. %.3f)   loss %.6f" % (name, r["median_ms"], r["min_ms"], r["max_ms"], r["loss"]))
    if args.parent:
        best = lambda n: min(r["median_ms"] for r in runs[n])
        ratio = best("unicode") / best("parent")
        inside = abs(ratio - 1) <= 0.03
        lines.append("unicode against parent (best median of each): %+.2f %%  -- %s" % (100 * (ratio - 1), "no change in step time (inside the pool's box-to-box spread of +-3 %)"
                                                                                      if inside else ("SLOWER than the spread of +-3 %" if ratio > 1 else "faster than the spread of +-3 %")))
    else:
        lines.append("(no --parent checkout given: the parent commit's step was not measured)")
    text = "\n".join(lines)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(text + "\n")
    if not same:
        raise SystemExit("the kernels and the host route disagree")


if __name__ == "__main__":
    main()

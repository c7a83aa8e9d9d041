#!/usr/bin/env python3
"""Lowering and normalising Unicode text on the device at B = 64, 50 OCR slots of Lw = 32, 10 answers of La = 128 and one question of Lq = 256 (DESIGN.md
§3.21): what the three launches cost, what the host work they replace costs, what the table lookup adds to a launch, and the eager training step with
textprep.materialize(unicode=...) in front against the parent commit's step on host-packed text.  NON_ASCII of the strings are not ASCII (accented
capitals, Greek with final sigmas, U+0130, CJK in the questions); the rest is tools/bench_textprep.py's text.

  kernel     materialize(unicode=...)'s three launches (sam_text_from_utf8_unicode for the OCR slots and the answers, sam_question_from_utf8), per
             triple, over COPIES distinct batches (measure.replay_us, one form at a time).  The same for the two text launches alone, with and
             without the table, on the SAME host-lowered bytes: the difference is the table's lookup cost.  The last batch's tensors are compared
             with the host route's.
  host       wall time, one host thread, HOST_REPS runs over the same batches (measure.host_ms): wordpiece.pack_question_text, and the str.lower() pass of
             textprep.pack_utf8 (pack_utf8 with host lowering minus pack_utf8(host_lower=False)).
  step       Trainer(use_graph=False) at bench.py's default shapes (c3 model, B = 64, 5000 words) with answers.tables_from_text in front, as
             tools/bench_textprep.py runs it, CHILD_ROUNDS fresh processes per variant (measure.step_ab):
               unicode       this tree, materialize(unicode=table, check=False) of unlowered bytes and the raw questions inside the timed region (the
                             question text it writes is set aside: the step reads the batch's question_indices, as the parent's does)
               parent        --parent DIR: a built checkout of the parent commit, materialize(check=False) of the host-lowered bytes inside the timed
                             region (the parent's route for the same strings; its question packing is host work and is listed under `host`)

How each number is taken: tools/measure.py.

    python tools/bench_unicode_text.py [--parent DIR] [--out profiles/unicode_text_bench.txt]"""
import os
import sys
import tempfile

import measure
from bench_textprep import raw_strings, word_cleaner        # (the same dirty strings as §3.20's measurement)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

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
    replay_us = lambda fn, sets: measure.replay_us(fn, sets, ROUNDS, REPS)[0]
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
    from sam_textvqa_amd import wordpiece as W
    strs = [strings(50 + r % COPIES) for r in range(HOST_REPS)]
    return (measure.host_ms(lambda r: W.pack_question_text(strs[r][2], max_chars=LQ), HOST_REPS), measure.host_ms(lambda r: raw_route(*strs[r][:2]), HOST_REPS),
            measure.host_ms(lambda r: raw_route(*strs[r][:2], host_lower=False), HOST_REPS))


def write_batches(path):
    """the step's batch in both forms, on the CPU, into `path` (the parent's child reads the host-lowered form from it)"""
    import torch
    from sam_textvqa_amd.synthetic import make_batch
    bd = make_batch(B, vocab=VOCAB, device="cpu", seed=77)
    for k in ("targets", "train_prev_inds", "train_loss_mask", "ocr_phoc"):
        del bd[k]
    ans, tok, qs = strings(9)
    torch.save({"parent": dict(bd, **raw_route(ans, tok)), "unicode": dict(bd, **raw_route(ans, tok, qs, host_lower=False))}, path)


def make_step(trainer, batch, form):
    from sam_textvqa_amd import answers as A, metrics as M, textprep as T
    voc = M.make_score_text(1, num_vocab=VOCAB, n_ocr=N_OCR, seed=9, rich=True)[0]
    index, out = A.index_to(A.vocab_index(voc), "cuda"), A.table_outputs(B, A.DEFAULT_CAPS, "cuda")
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
        return trainer.step(batch)
    return step


def main():
    args = measure.arg_parser(parent=True, child=True, form="unicode").parse_args()
    sys.path.insert(0, args.root)
    measure.require_gpu("bench_unicode_text.py")
    if args.child:
        return measure.step_child(args.child, args.form, make_step, use_graph=False, warm=8, reps=STEP_REPS, num_answers=VOCAB)
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
        runs = measure.step_ab(__file__, variants, path, CHILD_ROUNDS)        # (the parent's tree has no such script: this file's child runs against its package)
    lines.append("eager training step with materialize in front, c3 model, B = %d: ms per step, median (min .. max) of %d steps, one line per fresh process, variants alternating"
                 % (B, STEP_REPS))
    lines += measure.step_lines(runs) + measure.verdict("unicode", None, runs)
    measure.finish(lines, args.out, same, "the kernels and the host route disagree")


if __name__ == "__main__":
    main()

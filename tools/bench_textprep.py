#!/usr/bin/env python3
"""Raw strings to cleaned code points at B = 64, 50 OCR slots of Lw = 32 plus 10 answers of La = 128: what the two launches cost, what the
host route they replace costs, what a batch ships either way, and the eager training step with textprep.materialize in front against the same step on
host-packed text.

  kernel     sam_text_from_utf8 for the OCR slots and for the answers (textprep.materialize's two launches), per pair, over COPIES distinct batches
             (measure.replay_us).  The last batch's tensors are compared with the host packers' on the host-cleaned strings.
  host       wall time of word_cleaner on every string + phoc.pack_ocr_text + answers.pack_answer_text (the strings in, the CPU tensors out), against
             textprep.pack_utf8 twice, one thread of this machine's host, HOST_REPS runs over the same COPIES batches (measure.host_ms).
  bytes      per batch: the four packed text tensors, against raw bytes + offsets + counts.
  step       Trainer(use_graph=False) at bench.py's default shapes (c3 model, B = 64, 5000 words) with answers.tables_from_text in front, as
             tools/bench_answer_text.py runs it, CHILD_ROUNDS fresh processes per variant (measure.step_ab):
               raw           this tree, textprep.materialize(check=False) inside the timed region, in front of Trainer.step
               host text     this tree, the batch carries the host-packed text (the code a batch without the new keys always ran)
               parent        --parent DIR: a built checkout of the parent commit, the same host-packed batch (read from a file this script writes)

How each number is taken: tools/measure.py.

    python tools/bench_textprep.py [--parent DIR] [--out profiles/textprep_bench.txt]"""
import os
import sys
import tempfile

import measure

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

B, N_OCR, N_ANS, LW, LA, VOCAB = 64, 50, 10, 32, 128, 5000
ROUNDS, COPIES, REPS, HOST_REPS = 20, 4, 15, 5
STEP_REPS, CHILD_ROUNDS = 40, 2
TEXT_KEYS = ("ocr_text", "ocr_text_len", "answer_text", "answer_text_len")


def word_cleaner(w):
    return w.lower().replace(",", "").replace("?", "").replace("'s", " 's").strip()


def raw_strings(seed):
    """metrics.make_score_text's samples with the dirt the cleaner removes put back: (raw answers, raw OCR tokens) per sample"""
    import numpy as np
    from sam_textvqa_amd import metrics as M
    _, answers, tokens = M.make_score_text(B, num_vocab=VOCAB, n_ocr=N_OCR, seed=seed, rich=True)
    rng = np.random.RandomState(seed + 7)

    def dirty(s):
        return (s.upper(), "  " + s + "\t", s + "?", s.replace(" ", ", "), s.capitalize() + ",", s)[rng.randint(6)]
    return [[dirty(a) for a in ans] for ans in answers], [[dirty(t) for t in tok] for tok in tokens]


def host_route(answers, tokens):
    from sam_textvqa_amd import answers as A, phoc as P
    out = dict(P.pack_ocr_text([[word_cleaner(t) for t in tok] for tok in tokens], N_OCR, max_chars=LW))
    out.update(A.pack_answer_text([[word_cleaner(a) for a in ans] for ans in answers], N_ANS, max_chars=LA))
    return out


def raw_route(answers, tokens):
    from sam_textvqa_amd import textprep as T
    po, pa = T.pack_utf8(tokens, N_OCR), T.pack_utf8(answers, N_ANS)
    return {"ocr_raw": po["raw"], "ocr_raw_off": po["raw_off"], "ocr_count": po["count"], "answer_raw": pa["raw"], "answer_raw_off": pa["raw_off"]}


def time_kernel():
    import torch
    from sam_textvqa_amd import ops
    strings = [raw_strings(50 + i) for i in range(COPIES)]
    sets = [{k: v.cuda() for k, v in raw_route(*s).items()} for s in strings]
    outs = [{"text": torch.empty((B * n, L), dtype=torch.int32, device="cuda"), "text_len": torch.empty(B * n, dtype=torch.int32, device="cuda"),
             "status": torch.empty(B * n, dtype=torch.int32, device="cuda")} for n, L in ((N_OCR, LW), (N_ANS, LA))]

    def fn(s):
        ops.text_from_utf8(s["ocr_raw"], s["ocr_raw_off"], LW, 15, out=outs[0])
        ops.text_from_utf8(s["answer_raw"], s["answer_raw_off"], LA, 15, out=outs[1])
    us, _ = measure.replay_us(fn, sets, ROUNDS, REPS)
    last = (ROUNDS - 1) % COPIES
    want = host_route(*strings[last])
    same = torch.equal(outs[0]["text"].cpu().view(B, N_OCR, LW), want["ocr_text"]) and torch.equal(outs[0]["text_len"].cpu().view(B, N_OCR), want["ocr_text_len"]) and \
        torch.equal(outs[1]["text"].cpu().view(B, N_ANS, LA), want["answer_text"]) and torch.equal(outs[1]["text_len"].cpu().view(B, N_ANS), want["answer_text_len"]) and \
        not outs[0]["status"].any().item() and not outs[1]["status"].any().item()
    raw = raw_route(*strings[last])
    nbytes = {"text": sum(want[k].numel() * 4 for k in TEXT_KEYS), "raw": sum(v.numel() * v.element_size() for v in raw.values()),
              "payload": raw["ocr_raw"].numel() + raw["answer_raw"].numel()}
    return us, same, nbytes


def time_host():
    strings = [raw_strings(50 + r % COPIES) for r in range(HOST_REPS)]
    return measure.host_ms(lambda r: host_route(*strings[r]), HOST_REPS), measure.host_ms(lambda r: raw_route(*strings[r]), HOST_REPS)


def write_batches(path):
    """the step's batch in both forms, on the CPU, into `path` (the parent's child reads the host-packed form from it)"""
    import torch
    from sam_textvqa_amd.synthetic import make_batch
    bd = make_batch(B, vocab=VOCAB, device="cpu", seed=77)
    for k in ("targets", "train_prev_inds", "train_loss_mask", "ocr_phoc"):
        del bd[k]
    ans, tok = raw_strings(9)
    torch.save({"host text": dict(bd, **host_route(ans, tok)), "raw": dict(bd, **raw_route(ans, tok))}, path)          # (a padded batch: materialize drops ocr_count)


def make_step(trainer, batch, form):
    """Both forms build the answer table from the text in front of the step (answers.tables_from_text, check=False); the raw form runs
    textprep.materialize in front of that."""
    from sam_textvqa_amd import answers as A, metrics as M
    if form == "raw":
        from sam_textvqa_amd import textprep as T          # (the host-text form runs against a parent without this module)
    voc = M.make_score_text(1, num_vocab=VOCAB, n_ocr=N_OCR, seed=9, rich=True)[0]          # (the vocabulary depends on num_vocab and rich alone)
    index, out = A.index_to(A.vocab_index(voc), "cuda"), A.table_outputs(B, A.DEFAULT_CAPS, "cuda")

    def step(batch):
        if form == "raw":
            T.materialize(batch, ocr_chars=LW, answer_chars=LA, check=False)
        text = {k: batch.pop(k) for k in A.ANSWER_TEXT_KEYS}
        batch["answer_table"], _ = A.tables_from_text(dict(text, ocr_text=batch["ocr_text"], ocr_text_len=batch["ocr_text_len"]), index, out=out, check=False)
        return trainer.step(batch)
    return step


def main():
    args = measure.arg_parser(parent=True, child=True, form="raw").parse_args()
    sys.path.insert(0, args.root)
    measure.require_gpu("bench_textprep.py")
    if args.child:
        return measure.step_child(args.child, args.form, make_step, use_graph=False, warm=8, reps=STEP_REPS, num_answers=VOCAB)
    (m, a, z), same, nbytes = time_kernel()
    (hm, ha, hz), (pm, pa, pz) = time_host()
    lines = ["raw strings to cleaned code points, B = %d, %d OCR slots of Lw = %d and %d answers of La = %d, mode 15 (word_cleaner)" % (B, N_OCR, LW, N_ANS, LA),
             "kernel output equals the host packers' on the host-cleaned strings: %s" % same,
             "launch time: us per pair of launches, median (min .. max) of %d replays of %d pairs over %d batches" % (REPS, ROUNDS, COPIES),
             "  sam_text_from_utf8 (%d slots) + sam_text_from_utf8 (%d slots)      %8.2f us (%.2f .. %.2f)" % (B * N_OCR, B * N_ANS, m, a, z),
             "host work for the same %d samples: ms per batch, median (min .. max) of %d runs, one host thread" % (B, HOST_REPS),
             "  word_cleaner + pack_ocr_text + pack_answer_text                    %8.2f ms (%.2f .. %.2f)" % (hm, ha, hz),
             "  pack_utf8 x 2 (what the host still does)                           %8.2f ms (%.2f .. %.2f)" % (pm, pa, pz),
             "bytes per batch, host to device:",
             "  ocr_text + ocr_text_len + answer_text + answer_text_len            %9d" % nbytes["text"],
             "  raw bytes + offsets + counts instead                               %9d   (of which UTF-8 payload: %d)" % (nbytes["raw"], nbytes["payload"])]
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, "batches.pt")
        write_batches(path)
        variants = [("raw", ROOT, "raw"), ("host text", ROOT, "host text")] + ([("parent, host text", os.path.abspath(args.parent), "host text")] if args.parent else [])
        runs = measure.step_ab(__file__, variants, path, CHILD_ROUNDS)
    lines.append("eager training step with the answer table built from text, c3 model, B = %d: ms per step, median (min .. max) of %d steps, one line per fresh process, variants alternating"
                 % (B, STEP_REPS))
    lines += measure.step_lines(runs) + measure.verdict("raw", "host text", runs)
    measure.finish(lines, args.out, same, "the kernel and the host packers disagree")


if __name__ == "__main__":
    main()

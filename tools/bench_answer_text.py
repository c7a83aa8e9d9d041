#!/usr/bin/env python3
"""Answer tables from text at B = 64, the 5000-word vocabulary, 50 OCR slots: what the launch costs, what the host functions it replaces
cost, what a batch ships either way, and the eager training step with answer text against the same step fed the host-built table.

  kernel     sam_answer_table_from_text over COPIES distinct batches (measure.replay_us).  The last batch's table is compared with the host twin.
  host       wall time of build_answer_table per sample + collate_answer_tables of the 64 samples (the strings in, the collated CPU table out), one
             thread of this machine's host, HOST_REPS runs over the same COPIES batches (measure.host_ms).
  bytes      per batch: the answers' text (int32 code points + lengths) and the collated table at the default capacities.
  step       Trainer(use_graph=False) at bench.py's default shapes (c3 model, B = 64, 5000 words), CHILD_ROUNDS fresh processes per variant
             (measure.step_ab):
               text          this tree, the batch carries answer_text / answer_text_len; answers.tables_from_text(check=False) builds its answer_table on
                             the GPU inside the timed region, in front of Trainer.step
               host table    this tree, the batch carries the collated answer_table (the code a batch without the new keys always ran)
               parent        --parent DIR: a built checkout of the parent commit, the same host-table batch (read from a file this script writes)

How each number is taken: tools/measure.py.

    python tools/bench_answer_text.py [--parent DIR] [--out profiles/answer_text_bench.txt]"""
import os
import sys
import tempfile

import measure

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
    us, _ = measure.replay_us(lambda s: A.tables_from_text(s, index, out=out, check=False), sets, ROUNDS, REPS)
    last = packed[(ROUNDS - 1) % COPIES]
    want, want_status = A.tables_from_text_host(last["answer_text"], last["answer_text_len"], last["ocr_text"], last["ocr_text_len"], voc)
    same = all(torch.equal(out[k].cpu(), want[k]) for k in A.TABLE_KEYS) and torch.equal(out["status"].cpu(), want_status)
    nbytes = {"text": sum(last[k].numel() * 4 for k in A.ANSWER_TEXT_KEYS), "table": sum(want[k].numel() * want[k].element_size() for k in A.TABLE_KEYS)}
    return us, same, nbytes


def time_host(voc):
    from sam_textvqa_amd import answers as A
    strings = [samples(50 + r % COPIES) for r in range(HOST_REPS)]
    return measure.host_ms(lambda r: A.collate_answer_tables([A.build_answer_table(a, t, voc, max_ocr_tokens=N_OCR) for a, t in zip(*strings[r])]), HOST_REPS)


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


def make_step(trainer, batch, form):
    """the text form builds its answer table on the GPU in front of Trainer.step, inside the timed region"""
    if form != "text":
        return trainer.step
    from sam_textvqa_amd import answers as A
    index, out = A.index_to(A.vocab_index(vocabulary()), "cuda"), A.table_outputs(B, A.DEFAULT_CAPS, "cuda")

    def step(batch):
        text = {k: batch.pop(k) for k in A.ANSWER_TEXT_KEYS}
        batch["answer_table"], _ = A.tables_from_text(dict(text, ocr_text=batch["ocr_text"], ocr_text_len=batch["ocr_text_len"]), index, out=out, check=False)
        return trainer.step(batch)
    return step


def main():
    args = measure.arg_parser(parent=True, child=True).parse_args()
    sys.path.insert(0, args.root)
    measure.require_gpu("bench_answer_text.py")
    if args.child:
        return measure.step_child(args.child, args.form, make_step, use_graph=False, warm=8, reps=STEP_REPS, num_answers=VOCAB)
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
        runs = measure.step_ab(__file__, variants, path, CHILD_ROUNDS)
    lines.append("eager training step, c3 model, B = %d: ms per step, median (min .. max) of %d steps, one line per fresh process, variants alternating" % (B, STEP_REPS))
    lines += measure.step_lines(runs) + measure.verdict("text", "host table", runs)
    measure.finish(lines, args.out, same, "the kernel and the host twin disagree")


if __name__ == "__main__":
    main()

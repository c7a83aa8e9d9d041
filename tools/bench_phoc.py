#!/usr/bin/env python3
"""PHOC from the OCR tokens' text at B = 64, 50 OCR slots, Lw = 32: what the launch costs, what a batch ships either way, and the captured
ragged training step with text against the same step fed host-built PHOC rows.

  kernel     sam_phoc_from_text in the two forms the model uses: normalised bf16 into columns 300..903 of the OCR operand [3200, 3008] (ragged batch), and the
             fp32 0/1 tensor [64, 50, 604] (padded batch), over COPIES distinct token sets (measure.replay_us, the forms alternating).
  bytes      per batch: the text (int32 code points + lengths), the padded fp32 PHOC the reference ships, the fp16 rows of a ragged batch.
  step       Trainer(use_graph=True) on a ragged fp16 batch (c3 model, synthetic.make_batch), fed its own input buffers (measure.step_ab), CHILD_ROUNDS fresh
             processes per variant:
               text          this tree, the batch carries ocr_text / ocr_text_len
               host rows     this tree, the batch carries ocr_phoc_rows (the code a batch without the new keys always ran)
               parent        --parent DIR: a built checkout of the parent commit, the same host-rows batch (read from a file this script writes)

How each number is taken: tools/measure.py.

    python tools/bench_phoc.py [--parent DIR] [--out profiles/phoc_bench.txt]"""
import os
import random
import sys
import tempfile

import measure

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

B, N_OCR, LW = 64, 50, 32
ROUNDS, COPIES, REPS = 20, 4, 15
STEP_REPS, CHILD_ROUNDS = 40, 2


def tokens(seed):
    rng = random.Random(seed)
    return [["".join(rng.choice("etaoinshrdlu" * 3 + "abcdefghijklmnopqrstuvwxyz0123456789-'") for _ in range(rng.randint(1, 14))) for _ in range(N_OCR)] for _ in range(B)]


def time_kernel():
    import numpy as np
    import torch
    from sam_textvqa_amd import ops, phoc as P
    sets = []
    for i in range(COPIES):
        t = P.pack_ocr_text(tokens(50 + i), N_OCR, LW)
        sets.append((t["ocr_text"].cuda(), t["ocr_text_len"].cuda(), torch.randint(1, N_OCR + 1, (B,), dtype=torch.int32).cuda()))
    operand = torch.zeros((B * N_OCR, 3008), dtype=torch.bfloat16, device="cuda")
    dense = torch.zeros((B * N_OCR, 604), dtype=torch.float32, device="cuda")
    forms = {"bf16, normalised, columns 300..903 of [3200, 3008]": lambda s: ops.phoc_from_text(s[0], s[1], s[2], operand, 300, True),
             "fp32 0/1 [64, 50, 604]": lambda s: ops.phoc_from_text(s[0], s[1], s[2], dense, 0, False)}
    us, _ = measure.replay_us(forms, sets, ROUNDS, REPS)
    same = bool(np.array_equal(dense.view(B, N_OCR, 604).cpu().numpy(), P.phoc_host_text(sets[(ROUNDS - 1) % COPIES][0], sets[(ROUNDS - 1) % COPIES][1], sets[(ROUNDS - 1) % COPIES][2])))
    return us, same


def write_batches(path):
    """the ragged fp16 batch in both forms, on the CPU, into `path` (the parent's child reads the host-rows form from it: it has no phoc.py)"""
    import torch
    from sam_textvqa_amd import phoc as P, ragged as R
    from sam_textvqa_amd.synthetic import make_batch
    bd = make_batch(B, device="cpu", seed=77)
    toks = [t[:int(c)] for t, c in zip(tokens(9), bd["pad_ocr_mask"].sum(1).tolist())]
    ph = torch.zeros(B, N_OCR, 604)
    for b, t in enumerate(toks):
        ph[b, :len(t)] = torch.from_numpy(P.phoc_host(t))
    host = R.from_padded(dict(bd, ocr_phoc=ph))
    text = R.from_padded(dict({k: v for k, v in bd.items() if k != "ocr_phoc"}, **P.pack_ocr_text(toks, N_OCR, LW)))
    torch.save({"host rows": host, "text": text}, path)
    valid = int(bd["pad_ocr_mask"].sum())
    return valid


def main():
    args = measure.arg_parser(parent=True, child=True).parse_args()
    sys.path.insert(0, args.root)
    measure.require_gpu("bench_phoc.py")
    if args.child:
        return measure.step_child(args.child, args.form, use_graph=True, warm=12, reps=STEP_REPS)
    kernel, same = time_kernel()
    lines = ["PHOC from text, B = %d, %d OCR slots, Lw = %d" % (B, N_OCR, LW),
             "kernel output equals the host twin: %s" % same,
             "launch times: us per launch, median (min .. max) of %d replays of %d launches over %d token sets, forms alternating" % (REPS, ROUNDS, COPIES)]
    for name, (m, a, z) in kernel.items():
        lines.append("  %-56s %8.2f us (%.2f .. %.2f)" % (name, m, a, z))
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, "batches.pt")
        valid = write_batches(path)
        lines += ["bytes per batch (%d of %d OCR slots valid):" % (valid, B * N_OCR),
                  "  text: int32 code points + lengths, every slot          %9d" % (B * N_OCR * (LW + 1) * 4),
                  "  padded fp32 PHOC, as the reference ships it            %9d" % (B * N_OCR * 604 * 4),
                  "  fp16 PHOC rows of a ragged batch, valid rows only      %9d" % (valid * 604 * 2)]
        variants = [("text", ROOT, "text"), ("host rows", ROOT, "host rows")] + ([("parent, host rows", os.path.abspath(args.parent), "host rows")] if args.parent else [])
        runs = measure.step_ab(__file__, variants, path, CHILD_ROUNDS)
    lines.append("captured ragged training step, c3 model, fp16 rows: ms per replay, median (min .. max) of %d replays, one line per fresh process, variants alternating" % STEP_REPS)
    lines += measure.step_lines(runs) + measure.verdict("text", "host rows", runs)
    measure.finish(lines, args.out, same, "the kernel and the host twin disagree")


if __name__ == "__main__":
    main()

#!/usr/bin/env python
"""Answer-space upper bounds, device-event timing around host-issued calls, eager (no graph is captured; nothing here runs in
the training step, so no step time is claimed), at the 5000-word vocabulary, A = 10 answers, 50 OCR slots of up to 32 code points, L = 12:

  a. coverage.witness (one sam_answer_witness launch into preallocated outputs) at B = 64 and at a dataset-scale B;
  b. the three metrics.evaluate_beams calls that turn the witnesses into bounds (K = 10 "beams" per sample), and coverage.upper_bounds as a whole
     (score table from text, witnesses, three evaluations, masking);
  c. the host twin on one thread for the same batches (coverage.witness_host with the vocabulary dict built beforehand: wall time), and the whole host
     route at B = 64 (score table, witnesses, three evaluate_beams_host);
  d. what the pass reports for these synthetic samples (coverage.measure), as a check that the routes timed above computed the bounds.

    python tools/bench_coverage.py [--iters 2000] [--batch 64] [--big 4096] [--out profiles/coverage_bench.txt]      (--out is rewritten)
"""
import os
import sys

import measure
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from sam_textvqa_amd import answers as A  # noqa: E402
from sam_textvqa_amd import coverage as C  # noqa: E402
from sam_textvqa_amd import metrics as M  # noqa: E402
from sam_textvqa_amd import ops  # noqa: E402
from sam_textvqa_amd import phoc as P  # noqa: E402
from sam_textvqa_amd.wordindex import index_to  # noqa: E402

VOCAB, N_ANS, N_OCR, LW, L = 5000, 10, 50, 32, 12
CAPS = (N_ANS, LW, 128)


def batch(B, seed):
    """B synthetic questions as the text a batch ships, on the CPU: (vocabulary, batch dict)"""
    voc, answers, tokens = M.make_score_text(B, num_vocab=VOCAB, n_ocr=N_OCR, seed=seed, rich=True)
    bd = A.pack_answer_text(answers, num_answers=N_ANS)
    bd.update(P.pack_ocr_text(tokens, max_ocr_tokens=N_OCR, max_chars=LW))
    bd["ocr_count"] = M.ocr_counts(tokens, N_OCR)
    return voc, bd


def main():
    ap = measure.arg_parser()
    ap.add_argument("--iters", type=int, default=2000)
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--big", type=int, default=4096)
    ap.set_defaults(out=os.path.join(ROOT, "profiles", "coverage_bench.txt"))
    a = ap.parse_args()
    measure.require_gpu("bench_coverage.py")
    torch.set_num_threads(1)
    lines = ["# tools/bench_coverage.py --iters %d --batch %d --big %d on one MI355X; V = %d words (T = 16384 slots), A = %d, No = %d, Lw = %d, L = %d"
             % (a.iters, a.batch, a.big, VOCAB, N_ANS, N_OCR, LW, L),
             "# device events around host-issued calls, 3 alternating windows per route, median window; eager calls, no graph is captured; host: wall time, one thread"]
    report = None
    for B in (a.batch, a.big):
        voc, host = batch(B, 60)
        index = A.vocab_index(voc)
        vt = M.vocab_text(voc, max_word=LW)
        dev = {k: v.cuda() for k, v in host.items()}
        dev_index = index_to(index, "cuda")
        dev_vt = {"cp": vt["cp"].cuda(), "len": vt["len"].cuda(), "eos": vt["eos"]}
        table, _ = M.score_tables_from_text(dev, caps=CAPS, check=False)
        out = C.WITNESS.empty("cuda", B=B, A=N_ANS, L=L)
        wit = C.witness(dev, dev_index, L, out=out)
        zeros = torch.zeros(B * N_ANS, dtype=torch.float32, device="cuda")
        bufs = [ops.eval_beams_outputs(B, N_ANS, L, LW, "cuda") for _ in range(3)]

        def three_evaluations():
            return [M.evaluate_beams(wit["seqs"][s], zeros, table, dev_vt, beam=N_ANS, skip=0, out=bufs[s]) for s in range(3)]

        iters = a.iters if B <= 256 else max(a.iters // 10, 10)
        t_wit, t_eval, t_all = measure.timed_alternating([lambda: C.witness(dev, dev_index, L, out=out), three_evaluations,
                                                  lambda: C.upper_bounds(dev, dev_index, dev_vt, caps=CAPS, L=L)], iters)
        vocab = C.vocab_dict(index)
        ms_twin = measure.host_ms(lambda _: C.witness_host(host, index, L, vocab=vocab), 3 if B <= 256 else 1)[0]
        want = C.witness_host(host, index, L, vocab=vocab)
        equal = all(wit[k].cpu().numpy().tobytes() == want[k].tobytes() for k in C.KEYS)
        lines += ["B = %d:" % B,
                  "  coverage.witness (one launch, outputs preallocated):                 %9.1f us per eager call   (equals the host twin in all five tensors: %s)" % (t_wit, equal),
                  "  three metrics.evaluate_beams calls on the witnesses (K = %d):         %9.1f us" % (N_ANS, t_eval),
                  "  coverage.upper_bounds (score table from text, witnesses, 3 evaluations, masks): %9.1f us" % t_all,
                  "  coverage.witness_host, one thread, vocabulary dict prebuilt:         %9.1f ms wall   (%.0f x the launch)" % (ms_twin, 1e3 * ms_twin / t_wit)]
        if B <= 256:
            ms_host = measure.host_ms(lambda _: C.upper_bounds_host(host, index, vt, caps=CAPS, L=L), 3)[0]
            lines.append("  coverage.upper_bounds_host (host score table, twin, 3 evaluate_beams_host): %6.1f ms wall   (%.0f x upper_bounds)" % (ms_host, 1e3 * ms_host / t_all))
        else:
            report = C.measure([dev], dev_index, dev_vt, caps=CAPS, L=L)
    if report is not None:
        src = report["sources"]
        lines.append("coverage.measure over the %d synthetic questions (make_score_text(rich=True); not a dataset): VQA bound vocab %.4f / OCR %.4f / both %.4f; reachable %d / %d / %d; "
                     "words %d, in vocabulary %.3f, among OCR %.3f, in neither %.3f"
                     % (report["count"], src["vocab"]["vqa_accuracy"], src["ocr"]["vqa_accuracy"], src["both"]["vqa_accuracy"], src["vocab"]["reachable"],
                        src["ocr"]["reachable"], src["both"]["reachable"], report["words"]["words"], report["words"]["in_vocab_share"], report["words"]["in_ocr_share"],
                        report["words"]["in_neither_share"]))
    measure.finish(lines, a.out)


if __name__ == "__main__":
    main()

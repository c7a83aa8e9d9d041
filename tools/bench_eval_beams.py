#!/usr/bin/env python3
"""Beam-search output to per-question results at B = 64, K = 5, S = 12, the default capacities (10 answers, 50 OCR slots, Lw = 32, Lg = 128; DESIGN.md
§3.19): the new call against the composition the package offered before it, and against the host route.

  eval_beams   metrics.evaluate_beams (sam_eval_beams: two launches): every beam scored against the table of the 64 samples, the best beam chosen, its ids,
               scores, flags and answer string gathered.
  composition  what a caller could build before: repeat_interleave of the eight table tensors K times, ops.score_answers on the 320 rows, then torch
               argmax over the cumulative scores and gathers of the chosen ids and scores (no answer string: there was no device route to it).
  host         answers.decode_predictions of the chosen beams plus metrics.score_answers_host on all beams and numpy's argmax, one thread, wall time.
Both device variants: measure.replay_us over COPIES distinct batches, one variant after the other (how the number is taken: tools/measure.py).  The new
call's outputs are compared with the composition's and with the host twin.  bytes: the table traffic either way.

    python tools/bench_eval_beams.py [--out profiles/eval_beams_bench.txt]"""
import os
import sys

import measure

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

B, K, S, N_OCR, VOCAB = 64, 5, 12, 50, 5000
ROUNDS, COPIES, REPS, HOST_REPS = 20, 4, 15, 3


def make_sets():
    import numpy as np
    import torch
    from sam_textvqa_amd import metrics as M
    sets = []
    for i in range(COPIES):
        voc, _, s_tabs = M.make_score_tables(B, num_vocab=VOCAB, n_ocr=N_OCR, seed=60 + i, rich=True)
        rng = np.random.RandomState(160 + i)
        V = len(voc)
        pool = np.concatenate([np.arange(4, V, 37), V + np.arange(N_OCR), [voc.EOS_IDX] * 12])
        ids = pool[rng.randint(0, len(pool), (B * K, S - 1))]
        for r in range(0, B * K, 2):                          # half the beams spell one of their sample's answers from the OCR tokens
            t = s_tabs[r // K]
            toks = ["".join(chr(c & ~M.NO_GLUE) for c in o) for o in t["ocr"]]
            row = [V + toks.index(w) for w in t["gt_raw"][rng.randint(len(t["gt_raw"]))].split() if w in toks][:S - 2]
            ids[r] = (row + [voc.EOS_IDX] * S)[:S - 1]
        seqs = np.concatenate([np.ones((B * K, 1), np.int64), ids.astype(np.int64)], 1)
        cum = -rng.rand(B * K).astype(np.float32) * 8
        sets.append({"seqs": torch.from_numpy(seqs), "cum": torch.from_numpy(cum), "table": M.collate_score_tables(s_tabs), "vt": M.vocab_text(voc), "voc": voc,
                     "tokens": [["".join(chr(c & ~M.NO_GLUE) for c in o) for o in t["ocr"]] for t in s_tabs]})
    return sets


def main():
    args = measure.arg_parser().parse_args()
    sys.path.insert(0, ROOT)
    import numpy as np
    import torch
    from sam_textvqa_amd import answers as A, metrics as M, ops
    os.environ["SAM_COARSE_OPS"] = "0"                     # the ctypes route for both variants: the same call overhead outside the graph, none inside
    sets = make_sets()
    gsets = []
    for s in sets:
        gsets.append({"seqs": s["seqs"].cuda(), "cum": s["cum"].cuda(), "pred": s["seqs"][:, 1:].contiguous().cuda(), "table": {k: v.cuda() for k, v in s["table"].items()},
                      "vt": {"cp": s["vt"]["cp"].cuda(), "len": s["vt"]["len"].cuda(), "eos": s["vt"]["eos"]}})
    bufs = ops.eval_beams_outputs(B, K, S - 1, M.DEFAULT_SCORE_CAPS.Lw, "cuda")
    new = lambda s: M.evaluate_beams(s["seqs"], s["cum"], s["table"], s["vt"], K, out=bufs)
    sc_out = (torch.empty((B * K, 3), device="cuda"), torch.empty((B * K,), dtype=torch.int32, device="cuda"))

    def composition(s):
        rep = {k: v.repeat_interleave(K, dim=0) for k, v in s["table"].items()}
        sc, fl = ops.score_answers(s["pred"], rep, s["vt"]["cp"], s["vt"]["len"], s["vt"]["eos"], out=sc_out)
        best = s["cum"].view(B, K).argmax(1)
        rows = best + torch.arange(B, device="cuda") * K
        return {"best": best, "best_ids": s["pred"][rows], "best_scores": sc[rows], "best_flags": fl[rows], "oracle": sc.view(B, K, 3).amax(1), "beam_scores": sc}

    t_new, o_new = measure.replay_us(new, gsets, ROUNDS, REPS)
    o_new = {k: v.clone() for k, v in o_new.items()}
    t_old, o_old = measure.replay_us(composition, gsets, ROUNDS, REPS)
    last = sets[(ROUNDS - 1) % COPIES]
    twin = M.evaluate_beams_host(last["seqs"], last["cum"], last["table"], last["vt"], K)
    same_twin = all(np.array_equal(o_new[k].cpu().numpy().view(np.int32) if o_new[k].dtype == torch.float32 else o_new[k].cpu().numpy(),
                                   twin[k].view(np.int32) if twin[k].dtype == np.float32 else twin[k]) for k in M.EVAL_BEAMS_KEYS)
    same_old = all(torch.equal(o_new[k].to(o_old[k].dtype), o_old[k]) for k in o_old)

    def host_route(r):
        s = sets[r % COPIES]
        rep = {k: v.repeat_interleave(K, dim=0) for k, v in s["table"].items()}
        sc = M.score_answers_host(s["seqs"][:, 1:], rep, s["vt"], return_flags=True)[0]
        best = s["cum"].numpy().reshape(B, K).argmax(1)
        rows = best + np.arange(B) * K
        A.decode_predictions(s["seqs"][:, 1:][rows].tolist(), s["voc"], s["tokens"])
        sc[rows].astype(np.float64).mean(0)
    table_bytes = sum(v.numel() * v.element_size() for v in last["table"].values())
    lines = ["beam-search output to per-question results, B = %d, K = %d, S = %d, %d OCR slots, capacities %s" % (B, K, S, N_OCR, tuple(M.DEFAULT_SCORE_CAPS)),
             "%d calls per graph replay over %d distinct batches, %d replays, HIP events; median (min .. max) per call" % (ROUNDS, COPIES, REPS),
             "  eval_beams (sam_eval_beams, 2 launches)                          %8.1f us (%.1f .. %.1f)" % t_new,
             "  composition (repeat_interleave x8, sam_score_answers, argmax, gathers) %8.1f us (%.1f .. %.1f)" % t_old,
             "  host (score_answers_host on %d beams + decode_predictions, 1 thread)  %8.1f ms (%.1f .. %.1f)" % ((B * K,) + measure.host_ms(host_route, HOST_REPS)),
             "  outputs equal the host twin bit for bit: %s; equal the composition's: %s" % (same_twin, same_old),
             "  table read in place: %.2f MB; the composition writes and reads a %d-fold copy: %.2f MB more per batch" % (
                 table_bytes / 1e6, K, K * table_bytes / 1e6),
             "  eval_beams is %s than the composition (%.2fx)" % ("faster" if t_new[0] < t_old[0] else "SLOWER", t_old[0] / t_new[0])]
    measure.finish(lines, args.out and os.path.join(ROOT, args.out))          # (a relative --out is taken from the repository root)


if __name__ == "__main__":
    main()

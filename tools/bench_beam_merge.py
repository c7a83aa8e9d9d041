#!/usr/bin/env python3
"""Beam-search answers chosen by string at B = 64, K = 5, S = 12, the default capacities (10 answers, 50 OCR slots, Lw = 32, Lg = 128):
the merged call against the plain one on the same inputs, and against its host twin.

  merged  metrics.evaluate_beams_merged (sam_eval_beams_merged: two launches): every beam scored and spelled out, equal strings grouped, the groups'
          probabilities added, the heaviest group's best member reported; sixteen outputs.
  plain   metrics.evaluate_beams (sam_eval_beams: two launches), the parent commit's call: the beam with the largest cumulative score; nine outputs.
  host    metrics.evaluate_beams_merged_host, one thread, wall time.
Both device calls: measure.replay_us over COPIES distinct batches, one call after the other (how the number is taken: tools/measure.py).  Half the beams
of a question spell one of two answers from its OCR tokens, through whichever slot holds the word, so groups of several beams are frequent.  The merged
call's outputs are compared with its twin's (masses within the tolerance of DESIGN.md §3.29).

    python tools/bench_beam_merge.py [--out profiles/beam_merge_bench.txt]"""
import os
import sys

import measure

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

B, K, S, N_OCR, VOCAB = 64, 5, 12, 50, 5000
ROUNDS, COPIES, REPS, HOST_REPS = 20, 4, 15, 3
HBM_BYTES_PER_US = 6.3e6                                   # the streaming ceiling the extra strings are priced at


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
        for b in range(B):
            toks = ["".join(chr(c & ~M.NO_GLUE) for c in o) for o in s_tabs[b]["ocr"]]
            bases = [[toks[o] for o in rng.randint(0, N_OCR, rng.randint(1, 4))] for _ in range(2)]
            for k in range(K):
                if rng.rand() < 0.5:
                    continue
                row = [V + int(rng.choice([o for o, t in enumerate(toks) if t == w])) for w in bases[rng.randint(2)]]
                ids[b * K + k] = (row + [voc.EOS_IDX] + ids[b * K + k].tolist())[:S - 1]
        seqs = np.concatenate([np.ones((B * K, 1), np.int64), ids.astype(np.int64)], 1)
        cum = np.log(rng.dirichlet(np.ones(K), B).reshape(-1)).astype(np.float32)
        sets.append({"seqs": torch.from_numpy(seqs), "cum": torch.from_numpy(cum), "table": M.collate_score_tables(s_tabs), "vt": M.vocab_text(voc)})
    return sets


def main():
    args = measure.arg_parser().parse_args()
    sys.path.insert(0, ROOT)
    import numpy as np
    import torch
    from sam_textvqa_amd import metrics as M, ops
    os.environ["SAM_COARSE_OPS"] = "0"                     # the ctypes route for both calls: the same call overhead outside the graph, none inside
    sets = make_sets()
    gsets = [{"seqs": s["seqs"].cuda(), "cum": s["cum"].cuda(), "table": {k: v.cuda() for k, v in s["table"].items()},
              "vt": {"cp": s["vt"]["cp"].cuda(), "len": s["vt"]["len"].cuda(), "eos": s["vt"]["eos"]}} for s in sets]
    Lw = M.DEFAULT_SCORE_CAPS.Lw
    m_bufs, p_bufs = ops.eval_beams_merged_outputs(B, K, S - 1, Lw, "cuda"), ops.eval_beams_outputs(B, K, S - 1, Lw, "cuda")
    t_plain, _ = measure.replay_us(lambda s: M.evaluate_beams(s["seqs"], s["cum"], s["table"], s["vt"], K, out=p_bufs), gsets, ROUNDS, REPS)
    t_merged, o = measure.replay_us(lambda s: M.evaluate_beams_merged(s["seqs"], s["cum"], s["table"], s["vt"], K, out=m_bufs), gsets, ROUNDS, REPS)
    got = {k: v.cpu().numpy() for k, v in o.items()}
    calls = [[sets[(ROUNDS - 1 + r) % COPIES][k] for k in ("seqs", "cum", "table", "vt")] + [K] for r in range(HOST_REPS)]
    host = measure.host_ms(lambda r: M.evaluate_beams_merged_host(*calls[r]), HOST_REPS)
    twin = M.evaluate_beams_merged_host(*calls[0])          # (the batch of the graph's last call)
    exact = all(np.array_equal(got[k].view(np.int32) if got[k].dtype == np.float32 else got[k], twin[k].view(np.int32) if twin[k].dtype == np.float32 else twin[k])
                for k in M.EVAL_MERGED_KEYS if k not in ("mass", "best_mass"))
    err = max(float(np.abs(got[k].astype(np.float64) - twin[k].astype(np.float64)).max()) for k in ("mass", "best_mass"))
    extra = B * K * (S - 1) * (Lw + 1) * 4
    over = t_merged[0] - t_plain[0]
    lines = ["beam-search answers chosen by string, B = %d, K = %d, S = %d, %d OCR slots, capacities %s" % (B, K, S, N_OCR, tuple(M.DEFAULT_SCORE_CAPS)),
             "%d calls per graph replay over %d distinct batches, %d replays, HIP events; median (min .. max) per call" % (ROUNDS, COPIES, REPS),
             "  merged (sam_eval_beams_merged, 2 launches, 16 outputs)        %8.1f us (%.1f .. %.1f)" % t_merged,
             "  plain (sam_eval_beams, 2 launches, 9 outputs; the parent's)   %8.1f us (%.1f .. %.1f)" % t_plain,
             "  host twin (evaluate_beams_merged_host, 1 thread)              %8.1f ms (%.1f .. %.1f)" % host,
             "  merged against plain: %+.1f us per call (%+.1f %%; the box-to-box spread is +-3 %%)" % (over, 100 * over / t_plain[0]),
             "  the strings of all beams: %.2f MB more to write, %.2f us at %.1f TB/s -> the merged call costs %s than plain + streaming them" % (
                 extra / 1e6, extra / HBM_BYTES_PER_US, HBM_BYTES_PER_US / 1e6, "MORE" if over > extra / HBM_BYTES_PER_US else "no more"),
             "  last batch: %.2f groups per question, %d of %d answers differ from the best beam's" % (
                 float(twin["n_groups"].mean()), int((twin["best"] != twin["plain_best"]).sum()), B),
             "  outputs equal the host twin bit for bit (masses apart): %s; largest mass error against float64: %.2e" % (exact, err)]
    measure.finish(lines, args.out and os.path.join(ROOT, args.out))          # (a relative --out is taken from the repository root)


if __name__ == "__main__":
    main()

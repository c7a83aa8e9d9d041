#!/usr/bin/env python3
"""Scoring predictions at B = 64, L = 12 (V = 5000 answer words, 50 OCR slots): what the metrics cost on the GPU, on the host, and inside
the training step.

  kernel      sam_score_answers with the float64 accumulator: 50 launches captured in one graph, replayed 20 times after a warm-up, HIP events around each
              replay; median (min) per launch
  host twin   metrics.score_answers_host on the same batch (pure Python, as a port of sam/datasets/metrics.py runs per step): median of 5 calls.  Needs no
              GPU: `--host-only` measures just this
  step        the c3 training step (captured, answer_targets="table", predictions=True) without and with metric="textvqa", both Trainers alive in one
              process and stepped ALTERNATELY in blocks of 10 steps, 8 rounds, median (min) per step

    python tools/bench_score.py [--host-only] [--out profiles/score_bench.txt]"""
import os
import sys

import measure

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402

B, L, V, NO = 64, 12, 5000, 50


def make_inputs(seed=0):
    from sam_textvqa_amd import answers as A
    from sam_textvqa_amd import metrics as M
    voc, a_tabs, s_tabs = M.make_score_tables(B, num_vocab=V, n_ocr=NO, seed=seed, rich=True)
    rng = np.random.RandomState(seed + 1)
    ids = np.full((B, L), voc.EOS_IDX, np.int64)
    for b in range(B):                                       # predictions as a half-trained model makes them: 1-4 words, half of them one of the answers
        toks = ["".join(chr(c & ~M.NO_GLUE) for c in o) for o in s_tabs[b]["ocr"]]
        words = s_tabs[b]["gt_raw"][rng.randint(len(s_tabs[b]["gt_raw"]))].split()
        row = [V + toks.index(w) if w in toks else voc.word2idx_dict.get(w, -1) for w in words]
        if rng.rand() < 0.5 or not row or min(row) < 0:
            row = [int(rng.randint(4, V)) if rng.rand() < 0.5 else V + int(rng.randint(0, NO)) for _ in range(rng.randint(1, 5))]
        ids[b, :len(row)] = row[:L - 1]
    return voc, A.collate_answer_tables(a_tabs), M.collate_score_tables(s_tabs), M.vocab_text(voc), ids


def host_time(ids, stab, vt):
    from sam_textvqa_amd import metrics as M
    return measure.host_ms(lambda _: M.score_answers_host(ids, stab, vt, return_flags=True), 5)[:2]


def kernel_time(ids, stab, vt):
    from sam_textvqa_amd import metrics as M
    from sam_textvqa_amd import ops
    pred = torch.as_tensor(ids).cuda()
    tab = {k: stab[k].cuda() for k in M.SCORE_TABLE_KEYS}
    cp, ln, tot = vt["cp"].cuda(), vt["len"].cuda(), M.new_totals()
    out = (torch.empty(B, 3, device="cuda"), torch.empty(B, dtype=torch.int32, device="cuda"))
    n = 50
    launches = lambda k: [ops.score_answers(pred, tab, cp, ln, vt["eos"], totals=tot, out=out) for _ in range(k)]
    measure.on_side_stream(lambda: launches(3))
    g, _ = measure.graph_of(lambda: launches(n))
    for _ in range(3):
        g.replay()
    torch.cuda.synchronize()
    return measure.timed_replays({0: g}, 20, n)[0][:2]


def step_time(atab, stab, vt):
    from bench import build_model
    from sam_textvqa_amd.synthetic import clone_batch, make_batch
    from sam_textvqa_amd.trainer import Trainer
    shape = (20, 100, NO, L)
    batch = make_batch(B, *shape, vocab=V, context=3, device="cuda", seed=7)
    for k in ("targets", "train_prev_inds", "train_loss_mask"):
        batch.pop(k, None)
    trainers = {}
    for name, extra in (("without", {}), ("with", dict(metric="textvqa", metric_vocab=vt))):
        tr = Trainer(build_model(3, ("n", "n", "s", "s"), V, shape), seed=1, use_graph=True, answer_targets="table", predictions=True, **extra)
        bd = dict(clone_batch(batch), answer_table={k: v.cuda() for k, v in atab.items()})
        if extra:
            bd["score_table"] = {k: v.cuda() for k, v in stab.items()}
        for _ in range(4):
            tr.step(bd)
        trainers[name] = (tr, tr.input_buffers() or bd)
    torch.cuda.synchronize()
    ms = {k: [] for k in trainers}
    for _ in range(8):
        for name, (tr, bd) in trainers.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(10):
                tr.step(bd)
            e1.record()
            torch.cuda.synchronize()
            ms[name].append(e0.elapsed_time(e1) / 10)
    return {k: (float(np.median(v)), min(v)) for k, v in ms.items()}, trainers["with"][0].metric_value()


def main():
    ap = measure.arg_parser()
    ap.add_argument("--host-only", action="store_true")
    ap.add_argument("--no-step", action="store_true")
    args = ap.parse_args()
    voc, atab, stab, vt, ids = make_inputs()
    lines = ["scoring B = %d predictions of L = %d steps (V = %d, %d OCR slots)" % (B, L, V, NO)]
    hm, hmin = host_time(ids, stab, vt)
    lines.append("host twin  score_answers_host          %8.2f ms per batch (min %.2f)   %.0f samples/s" % (hm, hmin, B / hm * 1e3))
    if not args.host_only:
        km, kmin = kernel_time(ids, stab, vt)
        lines.append("kernel     sam_score_answers + totals  %8.2f us per batch (min %.2f)   host twin / kernel = %.0fx" % (km, kmin, hm * 1e3 / km))
        if not args.no_step:
            st, val = step_time(atab, stab, vt)
            lines.append("step       without metric              %8.3f ms (min %.3f)" % st["without"])
            lines.append("step       with metric=\"textvqa\"       %8.3f ms (min %.3f)   difference %+.1f us; running VQA accuracy %.4f" %
                         (st["with"] + (1e3 * (st["with"][0] - st["without"][0]), val)))
            lines.append("host twin per step / step without metric = %.2f" % (hm / st["without"][0]))
    measure.finish(lines, args.out)


if __name__ == "__main__":
    main()

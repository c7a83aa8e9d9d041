#!/usr/bin/env python3
"""PHOC from the OCR tokens' text at B = 64, 50 OCR slots, Lw = 32: what the launch costs, what a batch ships either way, and the captured
ragged training step with text against the same step fed host-built PHOC rows.

  kernel     sam_phoc_from_text in the two forms the model uses: normalised bf16 into columns 300..903 of the OCR operand [3200, 3008] (ragged batch), and the
             fp32 0/1 tensor [64, 50, 604] (padded batch).  ROUNDS launches captured in one graph, cycling over COPIES distinct token sets, replayed REPS
             times with HIP events around each replay, the forms ALTERNATING; median (min .. max) per launch.
  bytes      per batch: the text (int32 code points + lengths), the padded fp32 PHOC the reference ships, the fp16 rows of a ragged batch.
  step       Trainer(use_graph=True) on a ragged fp16 batch (c3 model, synthetic.make_batch): STEP_REPS replays timed one by one with HIP events, median.
             Every variant runs in a fresh child process of this script, the variants alternating, CHILD_ROUNDS times each:
               text          this tree, the batch carries ocr_text / ocr_text_len
               host rows     this tree, the batch carries ocr_phoc_rows (the code a batch without the new keys always ran)
               parent        --parent DIR: a built checkout of the parent commit, the same host-rows batch (read from a file this script writes)

    python tools/bench_phoc.py [--parent DIR] [--out profiles/phoc_bench.txt]"""
import argparse
import json
import os
import random
import subprocess
import sys
import tempfile

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
    graphs = {}
    for name, fn in forms.items():
        for s in sets:
            fn(s)
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            for i in range(ROUNDS):
                fn(sets[i % COPIES])
        graphs[name] = g
        g.replay()
    torch.cuda.synchronize()
    us = {n: [] for n in graphs}
    for _ in range(REPS):
        for name, g in graphs.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            g.replay()
            e1.record()
            torch.cuda.synchronize()
            us[name].append(1e3 * e0.elapsed_time(e1) / ROUNDS)
    same = bool(np.array_equal(dense.view(B, N_OCR, 604).cpu().numpy(), P.phoc_host_text(sets[(ROUNDS - 1) % COPIES][0], sets[(ROUNDS - 1) % COPIES][1], sets[(ROUNDS - 1) % COPIES][2])))
    return {k: (float(np.median(v)), min(v), max(v)) for k, v in us.items()}, same


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


def child(path, form):
    """captured ragged step of the package importable from sys.path[0], on the batch `form` of the file: prints one JSON line"""
    import numpy as np
    import torch
    import sam_textvqa_amd.modules as M
    from sam_textvqa_amd.synthetic import clone_batch, mmt_config_dict, text_bert_config_dict
    from sam_textvqa_amd.trainer import Trainer
    bd = torch.load(path, weights_only=False)[form]
    bd = {k: (v.cuda() if torch.is_tensor(v) else {kk: vv.cuda() for kk, vv in v.items()} if isinstance(v, dict) else v) for k, v in bd.items()}
    torch.manual_seed(0)
    model = M.SAM4C(M.BertConfig.from_dict(mmt_config_dict(3)), M.BertConfig.from_dict(text_bert_config_dict()), num_answers=5000, bos_idx=1)
    tr = Trainer(model, base_lr=1e-4, seed=1, use_graph=True)
    for _ in range(12):
        tr.step(clone_batch(bd))
    assert tr._graph is not None, "the step was not captured"
    bufs = tr.input_buffers()
    torch.cuda.synchronize()
    ms = []
    for _ in range(STEP_REPS):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        loss = tr.step(bufs)
        e1.record()
        torch.cuda.synchronize()
        ms.append(e0.elapsed_time(e1))
    print(json.dumps({"form": form, "median_ms": float(np.median(ms)), "min_ms": min(ms), "max_ms": max(ms), "loss": float(loss)}))


def run_child(root, path, form):
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
    ap.add_argument("--form", default="text")
    ap.add_argument("--root", default=ROOT)
    args = ap.parse_args()
    sys.path.insert(0, args.root)
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_phoc.py measures on the GPU; none found")
    if args.child:
        return child(args.child, args.form)
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
        runs = {name: [] for name, _, _ in variants}
        for _ in range(CHILD_ROUNDS):
            for name, root, form in variants:
                runs[name].append(run_child(root, path, form))
    lines.append("captured ragged training step, c3 model, fp16 rows: ms per replay, median (min .. max) of %d replays, one line per fresh process, variants alternating" % STEP_REPS)
    for name, rs in runs.items():
        for r in rs:
            lines.append("  %-20s %8.3f ms (%.3f .. %.3f)   loss %.6f" % (name, r["median_ms"], r["min_ms"], r["max_ms"], r["loss"]))
    base = "parent, host rows" if args.parent else "host rows"
    best = lambda n: min(r["median_ms"] for r in runs[n])
    ratio = best("text") / best(base)
    lines.append("text against %s (best median of each): %+.2f %%  -- %s the pool's box-to-box spread of +-3 %%" % (base, 100 * (ratio - 1), "within" if abs(ratio - 1) <= 0.03 else
                                                                                                               ("SLOWER than" if ratio > 1 else "faster than")))
    if not args.parent:
        lines.append("(no --parent checkout given: the parent commit's step was not measured)")
    text = "\n".join(lines)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")
    if not same:
        raise SystemExit("the kernel and the host twin disagree")


if __name__ == "__main__":
    main()

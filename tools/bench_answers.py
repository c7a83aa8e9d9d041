#!/usr/bin/env python3
"""M4C answer targets: the GPU sampler (csrc/answers.hip) against its byte floor, and the per-step host cost and host-to-device bytes of the two ways of
feeding the training step.

  kernel      sam_answer_sample at B = 64 / 96 and W = 5050 (c3: 5000-word vocabulary + 50 OCR slots) / 5100 (stress: 100 OCR slots), timed as 50
              back-to-back launches captured in a graph (no host in the loop).  Floor = bytes / 6.3 TB/s (achievable HBM, MI355X_MICROARCH.md; the
              8 TB/s spec floor is printed too): the dense targets, prev inds and masks written, the table rows the kernel reads.
  host path   what the reference does per step (processors.py:586-692 for every sample), here its torch twin on the host for the whole batch
              (answers.sample_answers_torch on CPU tensors) + the dense [B, 12, W] copy to the device, pageable and pinned.
  table path  collate_answer_tables of cached per-sample tables + their copy to the device (the kernel then runs inside the step).
  string half build_answer_table per sample (cacheable; paid once per sample, not per step).

    python tools/bench_answers.py [--out profiles/answers_bench.txt]"""
import os
import sys

import measure

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402

HBM, HBM_SPEC = 6.3e12, 8.0e12


def kernel_us(tab, W, bos, n_launch=50, reps=20):
    from sam_textvqa_amd import ops
    B, _, L = tab["seq_grp"].shape
    out = ops.answer_outputs(B, L, W, "cuda")
    step_dev = torch.zeros(1, dtype=torch.int64, device="cuda")
    measure.on_side_stream(lambda: [ops.answer_sample(tab, W, bos, 1, step_dev=step_dev, out=out) for _ in range(3)])
    g, _ = measure.graph_of(lambda: [ops.answer_sample(tab, W, bos, 1, step_dev=step_dev, step=i, out=out) for i in range(n_launch)])
    g.replay()
    torch.cuda.synchronize()
    return measure.timed_replays({0: g}, reps, n_launch)[0][:2]


def table_read_bytes(table):
    """bytes the kernel reads: meta, per block the chosen seq_grp row / seq_len, the step-0 list (block t = 0), one group's offsets and indices"""
    B, S, L = table["seq_grp"].shape
    n0 = table["meta"][:, 1].sum().item()
    ne = table["meta"][:, 3].sum().item()
    return B * L * (16 + 4 + 2 * L + 8 + 4 + 4) + n0 * 8 + ne * 4


def host_ms(fn, reps=10):
    fn()
    return measure.host_ms(lambda _: fn(), reps)[0]


def main():
    args = measure.arg_parser().parse_args()
    from sam_textvqa_amd import answers as A
    lines = ["# M4C answer sampler (csrc/answers.hip) -- tools/bench_answers.py on %s" % getattr(torch.cuda.get_device_properties(0), "gcnArchName", "?")]
    lines.append("## kernel: 50 launches per graph replay, median (min) of 20 replays; floor = written + read bytes / 6.3 TB/s (spec 8 TB/s in brackets)")
    for B in (64, 96):
        for name, n_ocr in (("c3", 50), ("stress", 100)):
            _, tabs = A.make_answer_tables(B, num_vocab=5000, n_ocr=n_ocr, seed=B + n_ocr)
            table = A.collate_answer_tables(tabs)
            W, bos = A.table_dims(table)
            tab = {k: table[k].cuda() for k in A.TABLE_KEYS}
            L = tab["seq_grp"].shape[2]
            wr = B * L * W * 4 + B * L * (8 + 4 + 4) + B * 4
            nb = wr + table_read_bytes(table)
            med, mn = kernel_us(tab, W, bos)
            lines.append("B=%-3d %-6s W=%d  %7.2f us (%.2f)  bytes %.2f MB  floor %.2f us [%.2f]  x_floor %.2f  (%.2f TB/s)"
                         % (B, name, W, med, mn, nb / 1e6, nb / HBM * 1e6, nb / HBM_SPEC * 1e6, med / (nb / HBM * 1e6), nb / (med * 1e-6) / 1e12))
    lines.append("## per step, B=64, c3 (W=5050): host time and host-to-device bytes")
    voc, tabs = A.make_answer_tables(64, num_vocab=5000, n_ocr=50, seed=1)
    table = A.collate_answer_tables(tabs)
    W, _ = A.table_dims(table)
    n = table["meta"][:, 0].numpy()
    ch = torch.from_numpy(A.draw_choices(1, 0, n))
    dense = A.sample_answers_torch(table, ch)
    dense_bytes = sum(dense[k].numel() * dense[k].element_size() for k in ("targets", "train_prev_inds", "train_loss_mask", "train_acc_mask"))
    t_twin = host_ms(lambda: A.sample_answers_torch(table, ch))
    dev_t = torch.empty_like(dense["targets"], device="cuda")
    pinned = dense["targets"].pin_memory()

    def h2d(src):
        dev_t.copy_(src, non_blocking=True)
        torch.cuda.synchronize()
    t_copy, t_copy_pin = host_ms(lambda: h2d(dense["targets"])), host_ms(lambda: h2d(pinned))
    tab_bytes = sum(v.numel() * v.element_size() for v in table.values())
    t_collate = host_ms(lambda: A.collate_answer_tables(tabs))
    tab_pin = {k: v.pin_memory() for k, v in table.items()}
    dev_tab = {k: torch.empty_like(v, device="cuda") for k, v in table.items()}

    def tab_h2d(src):
        for k, v in src.items():
            dev_tab[k].copy_(v, non_blocking=True)
        torch.cuda.synchronize()
    t_tcopy, t_tcopy_pin = host_ms(lambda: tab_h2d(table)), host_ms(lambda: tab_h2d(tab_pin))
    lines.append("reference-style (dense targets built on the host every step): twin %.2f ms + copy %.2f ms pageable / %.2f ms pinned; H2D %.2f MB"
                 % (t_twin, t_copy, t_copy_pin, dense_bytes / 1e6))
    lines.append("table path (cached tables, sampled in the step):              collate %.2f ms + copy %.2f ms pageable / %.2f ms pinned; H2D %.3f MB (%.1fx less)"
                 % (t_collate, t_tcopy, t_tcopy_pin, tab_bytes / 1e6, dense_bytes / tab_bytes))
    rng = np.random.RandomState(0)
    samples = []
    for _ in range(64):
        toks = ["w%d" % i for i in rng.randint(0, 4996, rng.randint(1, 51))]
        samples.append(([" ".join(toks[j] for j in rng.randint(0, len(toks), rng.randint(1, 4))) for _ in range(10)], toks))
    t_build = host_ms(lambda: [A.build_answer_table(a, t, voc) for a, t in samples]) / 64
    lines.append("string half (build_answer_table, once per sample, cacheable): %.3f ms per sample; max sequences / groups / target indices in this batch: "
                 "%d / %d / %d (caps S=%d G=%d E=%d)" % (t_build, int(table["meta"][:, 0].max()), int(table["meta"][:, 2].max()), int(table["meta"][:, 3].max()),
                                                       *(A.DEFAULT_CAPS[i] for i in (0, 2, 3))))
    measure.finish(lines, args.out)


if __name__ == "__main__":
    main()

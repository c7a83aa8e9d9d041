#!/usr/bin/env python
"""Batches gathered from the resident feature store at B = 64 with the c3 shapes (100 objects x 2048, up to 50 OCR rows x (2048 | 300 | 604), fp16;
fp32 boxes), device-event timing:

  1. store.gather -- its three launches (two sam_store_gather_ragged, one sam_store_gather_fixed) as EAGER CALLS with rotating index sets over a
     synthetic store that is larger than the 256 MB Infinity Cache, so that random indices read HBM; the bytes moved and the time those bytes take at
     8 TB/s;
  2. the route the gather replaces on the same batches: ragged.collate_ragged(pin_memory=True) of the looked-up samples (host time) and ragged.upload
     of the pinned result;
  3. the eager Trainer step of ONE trainer in one process, the forms taking turns: on a resident batch (no input at all), with ragged.upload of a
     pre-collated pinned batch in front (what the parent commit runs per step), and with store.gather in front.

No graph is captured here.

    python tools/bench_store.py [--images 2400] [--iters 200] [--steps 30] [--batch 64] [--out profiles/store_bench.txt]      (--out is rewritten)
"""
import os
import sys
import time

import measure
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from sam_textvqa_amd import ragged as R  # noqa: E402
from sam_textvqa_amd import store  # noqa: E402

N_OBJ, N_OCR, SETS = 100, 50, 8


def synthetic_store(n_images, template, seed=0):
    """built on the GPU: 100 object rows per image (the TextVQA features have exactly 100), 1..50 OCR rows; four questions per image"""
    g = torch.Generator(device="cuda").manual_seed(seed)
    cpu = torch.Generator().manual_seed(seed)

    def group(counts, keys):
        off = torch.cat([torch.zeros(1, dtype=torch.int64), torch.cumsum(counts, 0)])
        rows = int(off[-1])
        out = {"row_off": off.cuda()}
        for key, batch_key in keys:
            w = template[batch_key].shape[1]
            dt = template[batch_key].dtype
            out[key] = (torch.rand((rows, w), generator=g, device="cuda") if key == "box_rows" else torch.randn((rows, w), generator=g, device="cuda", dtype=dt))
        return out

    obj = group(torch.full((n_images,), N_OBJ, dtype=torch.int64), (("rows", "obj_rows"), ("box_rows", "obj_box_rows")))
    ocr = group(torch.randint(1, N_OCR + 1, (n_images,), generator=cpu),
                tuple((k, bk) for k, bk, _ in store.GROUP_ROWS["ocr"] if bk in template))
    nq = 4 * n_images
    image_of = torch.randint(0, n_images, (nq,), generator=cpu, dtype=torch.int32).cuda()
    B = template["obj_count"].numel()
    tables = {k: template[k][torch.randint(0, B, (nq,), generator=cpu).cuda()].contiguous() for k in ("question_indices", "question_mask") if k in template}
    return store.build(obj, ocr, question_tables=tables, image_of_question=image_of)


def main():
    ap = measure.arg_parser()
    ap.add_argument("--images", type=int, default=2400)
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--batch", type=int, default=64)
    a = ap.parse_args()
    measure.require_gpu("bench_store.py")
    if a.images < 2000:
        raise SystemExit("bench_store.py: at least 2000 images, so that the store is larger than the Infinity Cache")
    import sam_textvqa_amd.modules as M
    from sam_textvqa_amd.synthetic import clone_batch, make_batch, mmt_config_dict, text_bert_config_dict
    from sam_textvqa_amd.trainer import Trainer
    B = a.batch
    batch = R.from_padded(make_batch(B, vocab=5000, device="cuda", seed=3), feature_dtype=torch.float16)
    s = synthetic_store(a.images, batch)
    size = store.nbytes(s)
    cpu = torch.Generator().manual_seed(1)
    idx_sets = [torch.randint(0, s["n_questions"], (B,), generator=cpu, dtype=torch.int32) for _ in range(SETS)]
    dev_sets = [i.cuda() for i in idx_sets]
    into = {k: batch[k] for k in R.RAGGED_KEYS if k in batch}
    into.update({k: batch[k] for k in s["question_tables"]})
    status = torch.zeros(B, dtype=torch.int32, device="cuda")

    # the bytes a gather moves (read once, written once) and the route it replaces, on the same batches
    s_host = store.to(s, "cpu")
    row_bytes = {name: sum(t.shape[1] * t.element_size() for k, t in s[name].items() if k != "row_off") for name in ("obj", "ocr")}
    table_bytes = sum(t[0].numel() * t.element_size() for t in s["question_tables"].values())
    moved, hosts, t_collate = [], [], []
    for idx in idx_sets:
        imgs = s_host["image_of_question"][idx.long()].long()
        samples = []
        for g in imgs.tolist():
            smp = {}
            for name, rows in store.GROUP_ROWS.items():
                lo, hi = int(s_host[name]["row_off"][g]), int(s_host[name]["row_off"][g + 1])
                smp.update({sk: s_host[name][k][lo:hi] for k, _, sk in rows if k in s_host[name]})
            samples.append(smp)
        t0 = time.perf_counter()
        host = R.collate_ragged(samples, max_obj_num=N_OBJ, max_ocr_num=N_OCR, pin_memory=True)
        t_collate.append(1e3 * (time.perf_counter() - t0))
        host.update({k: t[idx.long()].pin_memory() for k, t in s_host["question_tables"].items()})
        hosts.append(host)
        moved.append(sum(int(host[COUNT].sum()) * row_bytes[name] for name, COUNT in store.COUNT_KEYS.items()) + B * table_bytes)
    # the two routes write the same batch
    store.gather(s, dev_sets[0], into, max_obj_num=N_OBJ, max_ocr_num=N_OCR, status=status)
    gathered = {k: v.clone() for k, v in into.items()}
    R.upload(hosts[0], into)
    torch.cuda.synchronize()
    for name, cnt in store.COUNT_KEYS.items():
        n = int(hosts[0][cnt].sum())
        assert all(torch.equal(gathered[bk][:n], into[bk][:n]) for _, bk, _ in store.GROUP_ROWS[name] if bk in into) and torch.equal(gathered[cnt], into[cnt])
    assert not status.any()

    turn = {"gather": 0, "upload": 0}

    def gather():
        turn["gather"] += 1
        store.gather(s, dev_sets[turn["gather"] % SETS], into, max_obj_num=N_OBJ, max_ocr_num=N_OCR, status=status)

    def upload():
        turn["upload"] += 1
        R.upload(hosts[turn["upload"] % SETS], into)

    t_gather, t_upload = measure.timed_alternating([gather, upload], a.iters)
    mb = sum(moved) / len(moved) / 1e6
    lines = ["# tools/bench_store.py --images %d --iters %d --steps %d on one MI355X; B = %d, %d objects x 2048 and 1..%d OCR rows x (2048 | 300 | 604) fp16, fp32 boxes"
             % (a.images, a.iters, a.steps, B, N_OBJ, N_OCR),
             "# synthetic store: %d images, %d questions, %.2f GB resident -- larger than the 256 MB Infinity Cache, so the random indices of the %d rotating index sets read HBM"
             % (s["n_images"], s["n_questions"], size / 1e9, SETS),
             "# device events around host-issued calls, 3 alternating windows per route, median window; no graph is captured",
             "store.gather (2 x sam_store_gather_ragged + sam_store_gather_fixed):  %8.1f us per eager call; %.1f MB read and %.1f MB written per batch = %.1f us at 8 TB/s"
             % (t_gather, mb, mb, 2 * mb * 1e6 / 8e12 * 1e6),
             "ragged.upload of the same batches, pinned and pre-collated:            %8.1f us per eager call (%.1f MB over the host link = %.1f GB/s)"
             % (t_upload, mb, mb * 1e6 / (t_upload * 1e-6) / 1e9),
             "ragged.collate_ragged(pin_memory=True) of the looked-up samples:       %8.2f ms of host time per batch (median of %d; the per-sample copy loop and the pinning)"
             % (sorted(t_collate)[len(t_collate) // 2], len(t_collate))]

    torch.manual_seed(0)
    model = M.SAM4C(M.BertConfig.from_dict(mmt_config_dict(3)), M.BertConfig.from_dict(text_bert_config_dict()), num_answers=5000, bos_idx=1)
    tr = Trainer(model, seed=1, use_graph=False)
    for _ in range(3):
        tr.step(clone_batch(batch))
    torch.cuda.synchronize()

    def step(front):
        def fn():
            if front is not None:
                front()
            return tr.step(clone_batch(batch))
        return fn
    t_res, t_up, t_ga = measure.timed_alternating([step(None), step(upload), step(gather)], a.steps)
    lines += ["eager Trainer step on a resident batch (no input):                     %7.3f ms" % (t_res / 1e3),
              "eager Trainer step behind ragged.upload (the parent commit's step):    %7.3f ms" % (t_up / 1e3),
              "eager Trainer step behind store.gather:                                %7.3f ms   (%+.1f %% against the upload route; the box-to-box spread is +-3 %%)"
              % (t_ga / 1e3, 100.0 * (t_ga - t_up) / t_up)]
    measure.finish(lines, a.out)


if __name__ == "__main__":
    main()

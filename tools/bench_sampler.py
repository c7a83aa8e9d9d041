#!/usr/bin/env python
"""The resident sampler at n = 35 000, B = 64, device-event timing around host-issued calls:

  a. Sampler.next -- one sam_sample_batch launch per eager call, into resident tensors;
  b. what a caller does today for the same indices: a slice of a host torch.randperm(n) (drawn once per epoch, its cost spread over the epoch's
     steps) copied into a pinned int32 [B] and from there to the device, per step; and the alternative of one torch.randperm(n, device=...) per epoch
     with a device slice per step;
  c. the eager Trainer step of ONE trainer in one process, the forms taking turns: behind store.gather with host-made indices (the parent commit's
     step) and behind Sampler.next + store.gather, over the synthetic store of tools/bench_store.py.

No graph is captured here.

    python tools/bench_sampler.py [--n 35000] [--images 2400] [--iters 500] [--steps 30] [--batch 64] [--out profiles/sampler_bench.txt]  (--out is rewritten)
"""
import os
import sys
import time

import measure
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from sam_textvqa_amd import ragged as R  # noqa: E402
from sam_textvqa_amd import sampler as S  # noqa: E402
from sam_textvqa_amd import store  # noqa: E402
from tools.bench_store import N_OBJ, N_OCR, synthetic_store  # noqa: E402


class HostIndices:
    """the route replaced: RandomSampler on the host -- randperm(n) per epoch, a slice per step through a pinned int32 [B] to a resident tensor"""

    def __init__(self, n, B):
        self.n, self.B, self.at, self.perm = n, B, 0, torch.randperm(n)
        self.pinned = torch.empty(B, dtype=torch.int32).pin_memory()
        self.dev = torch.empty(B, dtype=torch.int32, device="cuda")

    def next(self):
        if self.at + self.B > self.n:
            self.perm, self.at = torch.randperm(self.n), 0
        self.pinned.copy_(self.perm[self.at: self.at + self.B])
        self.at += self.B
        self.dev.copy_(self.pinned, non_blocking=True)
        return self.dev


class DevicePermIndices:
    """the alternative: torch.randperm(n, device=...) per epoch (int64 [n] resident), a device slice converted to int32 [B] per step"""

    def __init__(self, n, B):
        self.n, self.B, self.at, self.perm = n, B, 0, torch.randperm(n, device="cuda")
        self.dev = torch.empty(B, dtype=torch.int32, device="cuda")

    def next(self):
        if self.at + self.B > self.n:
            self.perm, self.at = torch.randperm(self.n, device="cuda"), 0
        self.dev.copy_(self.perm[self.at: self.at + self.B])
        self.at += self.B
        return self.dev


def main():
    ap = measure.arg_parser()
    ap.add_argument("--n", type=int, default=35000)
    ap.add_argument("--images", type=int, default=2400)
    ap.add_argument("--iters", type=int, default=500)
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--batch", type=int, default=64)
    a = ap.parse_args()
    measure.require_gpu("bench_sampler.py")
    B, n = a.batch, a.n
    smp = S.Sampler(n, B, seed=1)
    out = (torch.empty(B, dtype=torch.int32, device="cuda"), torch.empty(B, dtype=torch.int32, device="cuda"))
    host, devperm = HostIndices(n, B), DevicePermIndices(n, B)
    t_next, t_host, t_dev = measure.timed_alternating([lambda: smp.next(out=out), host.next, devperm.next], a.iters)
    smp.status()
    t0 = time.perf_counter()
    for _ in range(20):
        torch.randperm(n)
    t_perm = 1e6 * (time.perf_counter() - t0) / 20
    lines = ["# tools/bench_sampler.py --n %d --images %d --iters %d --steps %d on one MI355X; B = %d" % (n, a.images, a.iters, a.steps, B),
             "# device events around host-issued calls, 3 alternating windows per route, median window; no graph is captured",
             "Sampler.next (one sam_sample_batch launch, state resident):                       %8.1f us per eager call; nothing crosses the host link" % t_next,
             "host torch.randperm(%d) slice -> pinned int32 [%d] -> device, per step:        %8.1f us per call (the randperm itself: %.0f us of host time per epoch of %d steps)"
             % (n, B, t_host, t_perm, smp.steps_per_epoch),
             "torch.randperm(%d, device=...) per epoch, device slice -> int32 [%d] per step: %8.1f us per call (%d KB resident per epoch)"
             % (n, B, t_dev, n * 8 // 1024)]

    import sam_textvqa_amd.modules as M
    from sam_textvqa_amd.synthetic import clone_batch, make_batch, mmt_config_dict, text_bert_config_dict
    from sam_textvqa_amd.trainer import Trainer
    batch = R.from_padded(make_batch(B, vocab=5000, device="cuda", seed=3), feature_dtype=torch.float16)
    s = synthetic_store(a.images, batch)
    into = {k: batch[k] for k in R.RAGGED_KEYS if k in batch}
    into.update({k: batch[k] for k in s["question_tables"]})
    status = torch.zeros(B, dtype=torch.int32, device="cuda")
    nq = s["n_questions"]
    st_smp, st_host = S.for_store(s, B, seed=1), HostIndices(nq, B)

    def front_sampler():
        idx, _ = st_smp.next(out=out)
        store.gather(s, idx, into, max_obj_num=N_OBJ, max_ocr_num=N_OCR, status=status)

    def front_host():
        store.gather(s, st_host.next(), into, max_obj_num=N_OBJ, max_ocr_num=N_OCR, status=status)

    torch.manual_seed(0)
    model = M.SAM4C(M.BertConfig.from_dict(mmt_config_dict(3)), M.BertConfig.from_dict(text_bert_config_dict()), num_answers=5000, bos_idx=1)
    tr = Trainer(model, seed=1, use_graph=False)
    for _ in range(3):
        tr.step(clone_batch(batch))
    torch.cuda.synchronize()

    def step(front):
        def fn():
            front()
            return tr.step(clone_batch(batch))
        return fn
    t_h, t_s = measure.timed_alternating([step(front_host), step(front_sampler)], a.steps)
    assert not status.any() and st_smp.status() == 0
    lines += ["# synthetic store of tools/bench_store.py: %d images, %d questions, %.2f GB resident" % (s["n_images"], nq, store.nbytes(s) / 1e9),
              "eager Trainer step behind store.gather with host-made indices (the parent commit's step): %7.3f ms" % (t_h / 1e3),
              "eager Trainer step behind Sampler.next + store.gather:                                    %7.3f ms   (%+.1f %%; the box-to-box spread is +-3 %%)"
              % (t_s / 1e3, 100.0 * (t_s - t_h) / t_h)]
    measure.finish(lines, a.out)


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""Spatial aux heads on the device: the pair kernels (csrc/aux_heads.hip) at B = 64, n = 150 against their byte floor and against the eager torch
composition of the same math (the reference's repeated [B, n, n, 32] pair tensors), and the Trainer step with use_aux_heads on and off.

    python tools/bench_aux_heads.py [--iters 50] [--steps 20] [--batch 64]

Byte floor: the one fp32 [B, n, n, 12] tensor each kernel must write (forward) or read (backward) over 6.3 TB/s, the achievable HBM rate of
MI355X_MICROARCH.md; the [B, n, 32] operands and partials are small beside it."""
import argparse
import json
import os
import sys

import measure

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

HBM = 6.3e12


def timed(fn, iters, warmup=5):
    return measure.timed_alternating([fn], iters, rounds=1, warm=warmup)[0]          # us: one eager window (tools/measure.py)


def eager(o, d, w, b, fusion):
    n = o.shape[1]
    oo = o.unsqueeze(-2).repeat(1, 1, n, 1)
    dd = d.unsqueeze(-3).repeat(1, n, 1, 1)
    return torch.nn.functional.linear(oo * dd if fusion == "mul" else oo + dd, w, b)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--n", type=int, default=150)
    a = ap.parse_args()
    from sam_textvqa_amd import ops
    B, n = a.batch, a.n
    g = torch.Generator(device="cpu").manual_seed(0)
    o, d = torch.randn(B, n, 32, generator=g).cuda(), torch.randn(B, n, 32, generator=g).cuda()
    w, bias = (torch.randn(12, 32, generator=g) * 0.2).cuda(), (torch.randn(12, generator=g) * 0.1).cuda()
    gup = torch.randn(B, n, n, 12, generator=g).cuda()
    dw, db = torch.zeros(12, 32, device="cuda"), torch.zeros(12, device="cuda")
    out_bytes = B * n * n * 12 * 4
    floor_us = out_bytes / HBM * 1e6
    res = {"B": B, "n": n, "out_MB": round(out_bytes / 1e6, 1), "floor_us": round(floor_us, 1)}
    for fusion in ("mul", "add"):
        f = timed(lambda: ops.aux_pair_fwd(o, d, w, bias, fusion), a.iters)
        bw = timed(lambda: ops.aux_pair_bwd(gup, o, d, w, dw, db, fusion, accumulate=False), a.iters)
        oe, de = o.clone().requires_grad_(True), d.clone().requires_grad_(True)
        we, be = w.clone().requires_grad_(True), bias.clone().requires_grad_(True)
        ef = timed(lambda: eager(oe, de, we, be, fusion), max(5, a.iters // 5))
        y = eager(oe, de, we, be, fusion)

        def eb():
            torch.autograd.grad(y, (oe, de, we, be), gup, retain_graph=True)
        ebw = timed(eb, max(5, a.iters // 5))
        res[fusion] = {"fwd_us": round(f, 1), "bwd_us": round(bw, 1), "fwd_x_floor": round(f / floor_us, 2), "bwd_x_floor": round(bw / floor_us, 2),
                       "eager_fwd_us": round(ef, 1), "eager_bwd_us": round(ebw, 1)}
        print("%s: fwd %.1f us (%.2fx floor %.1f us), bwd %.1f us (%.2fx floor); eager torch fwd %.1f us, bwd %.1f us"
              % (fusion, f, f / floor_us, floor_us, bw, bw / floor_us, ef, ebw), flush=True)
    # Trainer step, aux heads on / off (the default bench model shapes at this batch: T 20, 100 objects, 50 OCR tokens, 12 steps)
    import sam_textvqa_amd.modules as M
    from sam_textvqa_amd.synthetic import clone_batch, make_batch, mmt_config_dict, text_bert_config_dict
    from sam_textvqa_amd.trainer import Trainer
    for aux in (False, True):
        md = mmt_config_dict(3, ("n", "n", "s", "s"))
        if aux:
            md.update(use_aux_heads=True)
        torch.manual_seed(0)
        model = M.SAM4C(M.BertConfig.from_dict(md), M.BertConfig.from_dict(dict(text_bert_config_dict(), num_hidden_layers=3)), num_answers=5000, bos_idx=1)
        tr = Trainer(model, seed=1)
        batch = make_batch(B, vocab=5000, device="cuda", seed=2)
        bs = [clone_batch(batch) for _ in range(a.steps + 3)]
        for i in range(3):
            tr.step(bs[i])
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for i in range(a.steps):
            tr.step(bs[3 + i])
        e1.record()
        torch.cuda.synchronize()
        ms = e0.elapsed_time(e1) / a.steps
        res["step_ms_aux_" + ("on" if aux else "off")] = round(ms, 3)
        print("trainer step (4 MMT layers, 3 TextBert layers, B=%d) aux %s: %.3f ms" % (B, "on" if aux else "off", ms), flush=True)
        del tr, model, bs
        torch.cuda.empty_cache()
    print(json.dumps(res))


if __name__ == "__main__":
    main()

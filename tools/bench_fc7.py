#!/usr/bin/env python3
"""Faster R-CNN fc7 fine-tuning on the device: the four new launches of the object / OCR encoders at B = 64 with the c3 shapes (100 objects, 50 OCR
tokens: obj R = 6400, OCR R = 3200 rows, fc6 2048 -> fc7 2048), each against its roofline, and the replayed Trainer step with the switch off and on.

    python tools/bench_fc7.py [--iters 50] [--steps 20] [--batch 64]

Rooflines (MI355X_MICROARCH.md): dense bf16 MFMA peak 2.5 PFLOP/s for the three GEMMs; 6.3 TB/s achievable HBM for the row kernel, whose floor is
its bytes: y and g read, dz written, bf16 (6 B per element)."""
import argparse
import json
import os
import sys

import measure

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

PEAK = 2.5e15
HBM = 6.3e12


def timed(fn, iters, warmup=5):
    return measure.timed_alternating([fn], iters, rounds=1, warm=warmup)[0]          # us: one eager window (tools/measure.py)


def launches(R, col0, k_pad, iters):
    from sam_textvqa_amd import _capi, ops
    g = torch.Generator(device="cpu").manual_seed(0)
    bf = lambda *s, scale=1.0: (torch.randn(*s, generator=g) * scale).to("cuda", torch.bfloat16)
    fc6, w, dza, wa = bf(R, 2048), bf(2048, 2048, scale=0.03), bf(R, 768), bf(768, k_pad, scale=0.03)
    b = (torch.randn(2048, generator=g) * 0.1).cuda()
    feat = torch.zeros(R, k_pad, dtype=torch.bfloat16, device="cuda")
    y = ops.gemm(fc6, w, epilogue=_capi.EPI_BIAS_RELU, bias=b)
    g7 = ops.gemm(dza, wa[:, col0: col0 + 2048], b_kcontig=False)
    dz = ops.fc7_bwd_rows(g7, y, True)
    dw, db = torch.zeros(2048, 2048, device="cuda"), torch.zeros(2048, device="cuda")
    t = {"fwd_gemm": timed(lambda: ops.gemm(fc6, w, epilogue=_capi.EPI_BIAS_RELU, bias=b, out=y), iters),
         "pack": timed(lambda: ops.l2norm_pack_bf16(y, feat, col0, True, zero_upto=k_pad), iters),
         "dgrad": timed(lambda: ops.gemm(dza, wa[:, col0: col0 + 2048], b_kcontig=False, out=g7), iters),
         "rows_bwd": timed(lambda: ops.fc7_bwd_rows(g7, y, True, out=dz), iters),
         "wgrad": timed(lambda: ops.gemm(dz, fc6, a_kcontig=False, b_kcontig=False, out=dw, accumulate=True, split_k=-1, bias_grad=db), iters)}
    flops = {"fwd_gemm": 2.0 * R * 2048 * 2048, "dgrad": 2.0 * R * 768 * 2048, "wgrad": 2.0 * R * 2048 * 2048}
    nbytes = {"pack": 4.0 * R * 2048, "rows_bwd": 6.0 * R * 2048}
    out = {}
    for k, us in t.items():
        if k in flops:
            out[k] = {"us": round(us, 1), "TFLOPs": round(flops[k] / us / 1e6, 1), "frac_bf16_peak": round(flops[k] / (us * 1e-6) / PEAK, 3)}
        else:
            floor = nbytes[k] / HBM * 1e6
            out[k] = {"us": round(us, 1), "floor_us": round(floor, 1), "x_floor": round(us / floor, 2)}
    return out


def step_ms(finetune, B, steps):
    import sam_textvqa_amd.modules as M
    from sam_textvqa_amd.synthetic import clone_batch, make_batch, mmt_config_dict, text_bert_config_dict
    from sam_textvqa_amd.trainer import Trainer
    md = mmt_config_dict(3, ("n", "n", "s", "s"))
    if finetune:
        md.update(frcn_encoder_type="finetune_faster_rcnn_fpn_fc7")
    torch.manual_seed(0)
    model = M.SAM4C(M.BertConfig.from_dict(md), M.BertConfig.from_dict(dict(text_bert_config_dict(), num_hidden_layers=3)), num_answers=5000, bos_idx=1)
    tr = Trainer(model, seed=1, use_graph=True)
    batch = make_batch(B, vocab=5000, device="cuda", seed=2)
    bs = [clone_batch(batch) for _ in range(steps + 3)]
    for i in range(3):
        tr.step(bs[i])
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for i in range(steps):
        tr.step(bs[3 + i])
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / steps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--batch", type=int, default=64)
    a = ap.parse_args()
    B = a.batch
    res = {"B": B}
    for name, R, col0, k_pad in (("obj", B * 100, 0, 2048), ("ocr", B * 50, 904, 3008)):
        res[name] = launches(R, col0, k_pad, a.iters)
        print("%s (R=%d): %s" % (name, R, json.dumps(res[name])), flush=True)
    for ft in (False, True):
        ms = step_ms(ft, B, a.steps)
        res["step_ms_fc7_" + ("on" if ft else "off")] = round(ms, 3)
        print("replayed trainer step (4 MMT layers, 3 TextBert layers, B=%d) fc7 %s: %.3f ms" % (B, "on" if ft else "off", ms), flush=True)
        torch.cuda.empty_cache()
    res["step_delta_ms"] = round(res["step_ms_fc7_on"] - res["step_ms_fc7_off"], 3)
    print(json.dumps(res))


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""FastText from the OCR tokens' text at B = 64, 50 OCR slots, Lw = 32 and a synthetic table of the real size (nwords = 2.5 M, bucket = 2 M, dim = 300,
filled on the device): what the launch costs, what it gathers, and what a batch ships either way.

  kernel     sam_fasttext_from_text in the form a ragged step would use: normalised bf16 into columns 0..299 of the OCR operand [3200, 3008], over
             COPIES distinct token sets (measure.replay_us; how the number is taken: tools/measure.py).  The token-length mix is 1..14 code points, a
             fifth of the tokens dictionary words, one in twenty with a space.  The ids gathered
             are counted by the host twin's word_ids on the same text; bytes gathered = ids * dim * 4, divided by the median time.  No target is set:
             random 1.2 KB row gathers from a 5.4 GB table have no measured ceiling on this part to compare with.
  bytes      per batch: the text (int32 code points + lengths), the padded fp32 FastText the reference ships, the fp16 rows of a ragged batch.
  The training step is not measured: SAM4C.forward does not call the launch yet.

    python tools/bench_fasttext.py [--out profiles/fasttext_bench.txt] [--nwords N --bucket N]"""
import os
import random
import sys

import measure

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

B, N_OCR, LW, DIM = 64, 50, 32, 300
ROUNDS, COPIES, REPS = 20, 4, 15
MINN, MAXN = 3, 6
N_REAL = 4096                                         # dictionary words that tokens are drawn from; the other ids are filler ("w<i>")


def real_words():
    rng = random.Random(3)
    out = set()
    while len(out) < N_REAL:
        out.add("".join(rng.choice("etaoinshrdlu" * 3 + "abcdefghijklmnopqrstuvwxyz") for _ in range(rng.randint(2, 10))))
    return sorted(out)


def tokens(seed, words):
    rng = random.Random(seed)

    def one():
        r = rng.random()
        if r < 0.2:
            return rng.choice(words)
        t = "".join(rng.choice("etaoinshrdlu" * 3 + "abcdefghijklmnopqrstuvwxyz0123456789-'") for _ in range(rng.randint(1, 14)))
        return t[:len(t) // 2] + " " + t[len(t) // 2:] if r > 0.95 and len(t) > 3 else t
    return [[one() for _ in range(N_OCR)] for _ in range(B)]


def big_index(nwords, bucket, device):
    """model_index of a dictionary of nwords words (N_REAL drawn words spread over the id range, filler between them) with the matrix [nwords + bucket, DIM]
    allocated and filled on the device: the host never holds it"""
    import numpy as np
    import torch
    from sam_textvqa_amd import fasttext as FT
    words = ["w%d" % i for i in range(nwords)]
    real = real_words()
    for k, w in enumerate(real):
        words[(k * (nwords // len(real))) % nwords] = w
    stub = FT.make_model(words, np.zeros((nwords, 4), np.float32), 0, 0, 0)          # the index needs the words only
    index = FT.model_index(stub)
    g = torch.Generator(device=device).manual_seed(1)
    matrix = torch.empty((nwords + bucket, DIM), dtype=torch.float32, device=device)
    for at in range(0, nwords + bucket, 1 << 18):
        matrix[at: at + (1 << 18)].normal_(generator=g)
    index = dict(FT.index_to(dict(index, matrix=torch.zeros(1, 4)), device), matrix=matrix, minn=MINN, maxn=MAXN, bucket=bucket, dim=DIM)
    return index, real


def time_kernel(nwords, bucket):
    import numpy as np
    import torch
    from sam_textvqa_amd import fasttext as FT, ops, phoc as P
    index, real = big_index(nwords, bucket, "cuda")
    sets, n_ids, n_valid = [], [], []
    host_index = dict(index, matrix=None, cp=index["cp"].cpu(), len=index["len"].cpu(), slots=index["slots"].cpu())
    for i in range(COPIES):
        toks = tokens(50 + i, real)
        t = P.pack_ocr_text(toks, N_OCR, LW)
        counts = torch.randint(1, N_OCR + 1, (B,), dtype=torch.int32)
        sets.append((t["ocr_text"].cuda(), t["ocr_text_len"].cuda(), counts.cuda()))
        if i == 0:
            for b in range(B):
                for tok in toks[b][:int(counts[b])]:
                    n_ids.append(sum(len(FT.word_ids(p, host_index)) for p in tok.split(" ")))
            n_valid.append(int(counts.sum()))
    operand = torch.zeros((B * N_OCR, 3008), dtype=torch.bfloat16, device="cuda")
    us, _ = measure.replay_us(lambda s: ops.fasttext_from_text(s[0], s[1], s[2], index, operand, 0, True), sets, ROUNDS, REPS)
    # the twin on a sample of the first set's rows, against the fp32 form of the same launch
    dense = torch.zeros((B * N_OCR, DIM), dtype=torch.float32, device="cuda")
    ops.fasttext_from_text(sets[0][0], sets[0][1], sets[0][2], index, dense, 0, False)
    torch.cuda.synchronize()
    rows = [0, 1, 2, 3, N_OCR, N_OCR + 1, 2 * N_OCR]
    ids = sorted({i for r in rows for p in _pieces(sets[0][0][r // N_OCR, r % N_OCR, :int(sets[0][1][r // N_OCR, r % N_OCR])].tolist()) for i in FT.word_ids(p, host_index)})
    small = dict(host_index, matrix=_RowsOnDemand(index["matrix"], ids))
    same = all(np.array_equal(dense[r].cpu().numpy(), FT.vectors_host_text(sets[0][0][r // N_OCR: r // N_OCR + 1, r % N_OCR: r % N_OCR + 1].cpu(),
                                                                            sets[0][1][r // N_OCR: r // N_OCR + 1, r % N_OCR: r % N_OCR + 1].cpu(), small)[0, 0]) for r in rows)
    return us, n_valid[0], sum(n_ids), same, index["matrix"].numel() * 4 + sum(index[k].numel() * 4 for k in ("cp", "len", "slots"))


def _pieces(cps):
    out, cur = [], []
    for c in cps:
        if c == 0x20:
            out.append(cur)
            cur = []
        else:
            cur.append(c)
    return out + [cur]


class _RowsOnDemand:
    """matrix[i] for the few rows the twin reads, fetched from the device once"""

    def __init__(self, matrix, ids):
        import torch
        self.rows = dict(zip(ids, matrix[torch.tensor(ids, device=matrix.device)].cpu().numpy())) if ids else {}

    def __getitem__(self, i):
        return self.rows[int(i)]


def main():
    ap = measure.arg_parser()
    ap.add_argument("--nwords", type=int, default=2500000)
    ap.add_argument("--bucket", type=int, default=2000000)
    args = ap.parse_args()
    sys.path.insert(0, ROOT)
    measure.require_gpu("bench_fasttext.py")
    (m, a, z), valid, ids, same, resident = time_kernel(args.nwords, args.bucket)
    gathered = ids * DIM * 4
    lines = ["FastText from text, B = %d, %d OCR slots, Lw = %d; synthetic table nwords = %d, bucket = %d, dim = %d, minn = %d, maxn = %d" % (
                 B, N_OCR, LW, args.nwords, args.bucket, DIM, MINN, MAXN),
             "resident on the device: %.2f GB (matrix and word index)" % (resident / 1e9),
             "kernel output equals the host twin on the sampled rows: %s" % same,
             "launch, bf16, normalised, columns 0..299 of [3200, 3008]: us per launch, median (min .. max) of %d replays of %d launches over %d token sets" % (REPS, ROUNDS, COPIES),
             "  %8.2f us (%.2f .. %.2f)" % (m, a, z),
             "first token set: %d valid rows of %d slots, %d ids gathered (%.1f per valid row)" % (valid, B * N_OCR, ids, ids / max(valid, 1)),
             "  bytes gathered %d; divided by the median time: %.1f GB/s (reported only: no target is set for this access pattern;\n  the %d token sets' rows fit the Infinity Cache and stay there between replays, so this is not an HBM figure)" % (gathered, gathered / (m * 1e-6) / 1e9, COPIES)]
    lines += ["bytes per batch (B * 50 slots; a ragged batch ships its valid rows only, %d of %d in the first token set):" % (valid, B * N_OCR),
              "  text: int32 code points + lengths, every slot (shared with PHOC)  %9d" % (B * N_OCR * (LW + 1) * 4),
              "  padded fp32 FastText, as the reference ships it                   %9d" % (B * N_OCR * DIM * 4),
              "  fp16 FastText rows of a ragged batch, valid rows only             %9d" % (valid * DIM * 2)]
    measure.finish(lines, args.out, same, "the kernel and the host twin disagree")


if __name__ == "__main__":
    main()

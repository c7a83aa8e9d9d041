"""Integer operands for the exact-arithmetic tests (tests/test_exact_integer_cpu.py, tests/test_exact_integer_gpu.py).

When every operand of a GEMM or of an fp32 reduction is a small integer, every product and every partial sum -- in ANY order -- is an integer far below
2^24: fp32 accumulation is exact, so the fp32 result does not depend on the tile, the split, the pair slice or the kernel that produced it, and a bf16
result is the single round-to-nearest-even of that integer.  The expected output is computed exactly (float64 matmul) and compared with torch.equal.

    ints               seeded integer-valued tensors (bf16 / fp32), optionally with a share of the entries zeroed
    exact_mm           the reference product in float64 (exact at these magnitudes; runs where its operands live)
    assert_exact_budget   max sum_k |a||b| (+ what the epilogue adds) < 2^17: seven binary orders under fp32's 2^24
    rne_bf16           float64 -> fp32 (asserted exact) -> bf16, torch's round-to-nearest-even
    tie_share / assert_ties   the share of reference elements that lie exactly halfway between two bf16 values (integers above 256): at least 1 %
                       in every bf16 reference, or the round-to-nearest-even claim would go untested
    gemm_case, wgrad_case, grouped_case   the case tables of the GPU file, with their expected outputs; each generator asserts its own budget and tie share
"""
import functools

import torch

BF16 = torch.bfloat16
BUDGET = 2.0 ** 17
MIN_TIE_SHARE = 0.01

TILES4 = (64, 128, 160, 192, 256)                              # 4-wave kernels (gemm.hip)
TILES8 = (1128, 1192, 3192, 1256, 1448, 12192, 12448)          # 8-wave (gemm8.hip) and 12-wave loader-wave (gemm12.hip) kernels


def ints(shape, seed, lo=-3, hi=3, dtype=BF16, zero_frac=0.0):
    """integers drawn uniformly from [lo, hi] by a seeded generator (on the host), as `dtype`; zero_frac: that share of the entries is zeroed"""
    g = torch.Generator().manual_seed(seed)
    x = torch.randint(lo, hi + 1, tuple(shape), generator=g)
    if zero_frac:
        x = x * (torch.rand(tuple(shape), generator=g) >= zero_frac)
    y = x.to(dtype)
    assert torch.equal(y.to(torch.int64), x), "not representable in %s: [%d, %d]" % (dtype, lo, hi)
    return y


def half_zero_ints(shape, seed, lo=-3, hi=3, dtype=BF16):
    """ints with about half of the entries zero (what a dropout mask or a ReLU leaves of a gradient)"""
    return ints(shape, seed, lo, hi, dtype, zero_frac=0.5)


def exact_mm(a, b):
    """a [M, K] . b [K, N] in float64: exact for integer operands inside the budget, and BLAS-fast (an int64 matmul of 11648 x 768 x 768 is not)"""
    return a.double() @ b.double()


def _amax(t):
    return float(t.double().abs().max()) if torch.is_tensor(t) else abs(float(t))


def assert_exact_budget(a, b, *extras, gain=1.0, name=""):
    """max over the output of  gain * sum_k |a||b|  +  sum of max|extra|  must stay below 2^17.  a [M, K], b [K, N] as contracted; `extras` are the terms
    an epilogue adds, already scaled as the kernel scales them; `gain` what it multiplies the product by.  Returns the bound it found."""
    k = a.shape[1]
    assert b.shape[0] == k, (a.shape, b.shape)
    prod = k * _amax(a) * _amax(b)                                    # cheap upper bound first: the deep problems never need the |a| @ |b| product
    add = sum(_amax(e) for e in extras)
    if gain * prod + add >= BUDGET:
        prod = float((a.double().abs() @ b.double().abs()).max())
    worst = gain * prod + add
    assert worst < BUDGET, "%s: |result| can reach %.0f, the exact-arithmetic budget is 2^17 = %.0f" % (name, worst, BUDGET)
    return worst


def rne_bf16(x_f64):
    """the expected bf16 result of an exact value: float64 -> fp32 is exact here (asserted), fp32 -> bf16 is torch's round-to-nearest-even"""
    f = x_f64.to(torch.float32)
    assert torch.equal(f.double(), x_f64.double()), "reference is not exact in fp32"
    return f.to(BF16)


def is_tie(x_f64):
    """elements that lie exactly halfway between two neighbouring bf16 values and are above 256 in magnitude (below it every integer is a bf16 value)"""
    f = x_f64.to(torch.float32)
    return ((f.view(torch.int32) & 0xFFFF) == 0x8000) & (f.abs() > 256)


def tie_share(x_f64):
    return float(is_tie(x_f64).double().mean())


def assert_ties(x_f64, name=""):
    s = tie_share(x_f64)
    assert s >= MIN_TIE_SHARE, "%s: only %.3f %% of the reference elements are bf16 ties (need %.0f %%): round-to-nearest-even would go untested" % (name, 100 * s, 100 * MIN_TIE_SHARE)
    return s


def describe_mismatch(got, want, name=""):
    """None when got == want element for element; otherwise one line: how many differ, the first index, got / want there and the exact difference
    (an integer, or one bf16 step at a tie: it names the dropped or doubled term)"""
    if got.shape != want.shape:
        return "%s: shape %s, want %s" % (name, tuple(got.shape), tuple(want.shape))
    if got.dtype != want.dtype:
        return "%s: dtype %s, want %s" % (name, got.dtype, want.dtype)
    want = want.to(got.device)
    if torch.equal(got, want):
        return None
    bad = (got != want) | (got != got)
    flat = int(torch.nonzero(bad.reshape(-1))[0])
    idx = []
    for n in reversed(got.shape):
        idx.append(flat % n)
        flat //= n
    idx = tuple(reversed(idx))
    g, w = float(got[idx]), float(want[idx])
    return "%s: %d of %d elements differ; first at %s: got %r, want %r, difference %r" % (name, int(bad.sum()), got.numel(), idx, g, w, g - w)


# ------------------------------------------------------------------------------------------------ forward / dgrad
# name -> (M, N, K, r): operands uniform in [-r, r].  r grows as K shrinks so that the products' standard deviation sqrt(K) r (r + 1) / 3 stays near 300:
# a fifth of the results then lie in [256, 1024), where every second (fourth) integer is a bf16 tie.
GEMM_CASES = {
    "ragged712": (600, 520, 712, 5),        # ragged in M, N and K (K % 64 != 0): the 4-wave tiles
    "k64": (600, 520, 64, 10),              # one k-tile: the 8- and 12-wave tiles
    "k704": (256, 256, 704, 5),             # eleven k-tiles
    "persistent": (3500, 3080, 128, 8),     # 323 tiles of 192 x 192 on 256 CUs: blocks cross tile boundaries with the next tile's operands in flight
    "split3": (100, 72, 1600, 4),           # forced and automatic split-K, the epilogue folded into the reduction
    "split8": (64, 8, 4096, 3),
}
BIAS_R, RES_R, AUX_R = 300, 100, 3
BIAS_HI = (3000, 3600)        # the dropout case's bias: above every |product| (asserted), so acc + bias is never zero and the kept value always differs from the dropped one


def _seed(name):
    return 1000 * (1 + sorted(GEMM_CASES).index(name))


@functools.lru_cache(maxsize=None)
def gemm_case(name, device="cpu"):
    """operands and expected outputs of one forward / dgrad case, on `device`:
        x [M, K], w [N, K] (forward: x w^T), wt [K, N] (dgrad layout: x wt), bias / bias_hi fp32 [N], res / aux bf16 [M, N]
        want[...]: fwd_none, fwd_none_f32, fwd_bias, fwd_bias_f32, fwd_res (bias + residual, p_drop = 0), dgrad_none, dgrad_aux, dgrad_res;
        fwd_drop / dgrad_drop: (dropped, kept) = (rne(res), rne(res + 2 (acc + bias_hi))): p_drop = 0.5 makes 1 / keep exactly 2
    Asserts the budget of every epilogue, at least 1 % ties in every bf16 reference, and that dropped != kept everywhere."""
    M, N, K, r = GEMM_CASES[name]
    s = _seed(name)
    c = dict(M=M, N=N, K=K)
    c["x"], c["w"], c["wt"] = ints((M, K), s + 1, -r, r).to(device), ints((N, K), s + 2, -r, r).to(device), ints((K, N), s + 3, -r, r).to(device)
    c["bias"] = ints((N,), s + 4, -BIAS_R, BIAS_R, torch.float32).to(device)
    c["bias_hi"] = ints((N,), s + 5, BIAS_HI[0], BIAS_HI[1], torch.float32).to(device)
    c["res"], c["aux"] = ints((M, N), s + 6, -RES_R, RES_R).to(device), ints((M, N), s + 7, -AUX_R, AUX_R).to(device)
    fwd, dg = exact_mm(c["x"], c["w"].t()), exact_mm(c["x"], c["wt"])
    bias, bias_hi, res, aux = c["bias"].double(), c["bias_hi"].double(), c["res"].double(), c["aux"].double()
    for b, what in ((c["w"].t(), "forward"), (c["wt"], "dgrad")):
        assert_exact_budget(c["x"], b, bias, res, name="%s %s bias + residual" % (name, what))
        assert_exact_budget(c["x"], b, 2 * bias_hi, res, gain=2.0, name="%s %s dropout" % (name, what))
    assert_exact_budget(c["x"], c["wt"], gain=float(AUX_R), name="%s dgrad * aux" % name)
    exact = dict(fwd_none=fwd, fwd_bias=fwd + bias, fwd_res=fwd + bias + res, dgrad_none=dg, dgrad_aux=dg * aux, dgrad_res=dg + bias + res)
    want = {k: rne_bf16(v) for k, v in exact.items()}
    want["fwd_none_f32"], want["fwd_bias_f32"] = fwd.float(), (fwd + bias).float()
    assert torch.equal(want["fwd_bias_f32"].double(), fwd + bias)
    for k, acc in (("fwd_drop", fwd), ("dgrad_drop", dg)):
        assert float(acc.abs().max()) < BIAS_HI[0], "%s: |acc| reaches the dropout case's bias" % name
        exact[k] = res + 2.0 * (acc + bias_hi)
        want[k] = (rne_bf16(res), rne_bf16(exact[k]))
        assert bool((want[k][0] != want[k][1]).all()), "%s %s: dropped and kept values coincide somewhere: the mask could not be read" % (name, k)
    c["ties"] = {k: assert_ties(v, "%s %s" % (name, k)) for k, v in exact.items()}
    c["want"] = want
    return c


# ------------------------------------------------------------------------------------------------ weight gradient (fp32 outputs: no ties to ask for)
WGRAD_CASES = [(1000, 520, 264), (182, 768, 3072), (5000, 768, 8), (11648, 768, 768)]      # (R, M, N): dW [M, N] = dy [R, M]^T x [R, N]
C_R = 500         # the gradient already in C / in the bias gradient: integers up to 500 -- above 256 not all bf16 values, so a C carried at bf16 precision shows


@functools.lru_cache(maxsize=None)
def wgrad_case(R, M, N, device="cpu", want_ref=True):
    """dy [R, M] (about half zeros), x [R, N], c0 fp32 [M, N] and b0 fp32 [M] in [-500, 500]; prod = dy^T x and colsum = sum_r dy in float64"""
    s = 7 * R + M + N
    c = dict(dy=half_zero_ints((R, M), s + 1).to(device), x=ints((R, N), s + 2).to(device),
             c0=ints((M, N), s + 3, -C_R, C_R, torch.float32).to(device), b0=ints((M,), s + 4, -C_R, C_R, torch.float32).to(device))
    assert_exact_budget(c["dy"].t(), c["x"], c["c0"], name="wgrad %s" % ((R, M, N),))
    assert_exact_budget(c["dy"].t(), torch.ones(R, 1, device=device), c["b0"], name="bias grad %s" % ((R, M, N),))
    if want_ref:
        c["prod"], c["colsum"] = exact_mm(c["dy"].t(), c["x"]), c["dy"].double().sum(0)
    return c


LAYER = [(768, 3072), (3072, 768), (768, 768), (2304, 768)]        # an encoder layer's four weight gradients (M, N)
# name -> list of (R, M, N, has_bias): one sam_gemm_bf16_grouped launch
GROUPED_CASES = {
    "pair1024": [(1024, m, n, j in (1, 3)) for j, (m, n) in enumerate(LAYER)],                       # 108 tiles of 256 x 256: every tile's K range split over a pair of blocks
    "ragged512": [(512, 200, 328, True), (512, 520, 264, False)],                                    # tile edges
    "unsplit512": [(512, 3072, 3072, True)],                                                         # too many tiles for pairs: one block per tile
    "mixed": [(1024, m, n, j in (0, 1, 3, 5, 6)) for j, (m, n) in enumerate(LAYER * 2)] +             # a layer pair (deep: 288 tiles of 192 x 256, 32 of them in 8 k-slices)
             [(512, m, n, j in (1, 2)) for j, (m, n) in enumerate(LAYER)],                           # with shallow tiles behind it
}
GROUPED_TILES = {"pair1024": (128, 1256, 0), "ragged512": (128, 1256, 0), "unsplit512": (128, 1256, 0), "mixed": (128, 1256, 12448, 0)}


@functools.lru_cache(maxsize=None)
def grouped_case(name, device="cpu", want_ref=True):
    """list of dicts like wgrad_case's (b0 None for a problem without bias rider)"""
    out = []
    for j, (R, M, N, has_bias) in enumerate(GROUPED_CASES[name]):
        s = 100000 + 97 * j + R + M + N
        c = dict(dy=half_zero_ints((R, M), s + 1).to(device), x=ints((R, N), s + 2).to(device),
                 c0=ints((M, N), s + 3, -C_R, C_R, torch.float32).to(device), b0=ints((M,), s + 4, -C_R, C_R, torch.float32).to(device) if has_bias else None)
        assert_exact_budget(c["dy"].t(), c["x"], c["c0"], name="grouped %s %d" % (name, j))
        assert_exact_budget(c["dy"].t(), torch.ones(R, 1, device=device), C_R, name="grouped bias %s %d" % (name, j))
        if want_ref:
            c["prod"], c["colsum"] = exact_mm(c["dy"].t(), c["x"]), c["dy"].double().sum(0)
        out.append(c)
    return out


# ------------------------------------------------------------------------------------------------ fp32 reductions
COLSUM_SHAPES = [(1000, 2304)] + [(m, n) for m in (1, 63, 64, 65) for n in (4, 60, 64, 68)]
SUMSQ_N = (1, 3, 4, 1023, 1000003)


def colsum_case(M, N):
    x = half_zero_ints((M, N), 31 * M + N) if M > 1 else ints((M, N), 31 * M + N)
    assert_exact_budget(torch.ones(1, M), x, C_R, name="colsum %s" % ((M, N),))
    return x


def sumsq_case(n):
    """values in [-2, 2]; the long vector keeps one entry in fifty non-zero, so that its sum of squares (at most 4 n / 50) stays inside the budget"""
    g = ints((n,), 77 + n, -2, 2, torch.float32, zero_frac=0.98 if n > 30000 else 0.0)
    assert float((g.double() ** 2).sum()) < BUDGET, n
    return g


def scatter_case(T, D, rows, seed, padding_idx=0):
    """dy bf16 [T, D] in [-3, 3], ids int64 [T] with repeats (one row a third of the list) and padding entries, base fp32 [rows, D] in [-500, 500]"""
    g = torch.Generator().manual_seed(seed)
    ids = torch.randint(0, rows, (T,), generator=g)
    ids[torch.randperm(T, generator=g)[: T // 3]] = min(7, rows - 1)
    ids[: max(1, T // 10)] = padding_idx
    dy = ints((T, D), seed + 1)
    base = ints((rows, D), seed + 2, -C_R, C_R, torch.float32)
    assert 3 * T + C_R < BUDGET
    return dy, ids, base


PTR_SHAPES = [(12, 50, 768), (5, 7, 64)]      # (S, No, D): the matrix-core kernel and the dot-product kernel
PTR_SCALE = 2.0 ** -5


def ptr_case(S, No, D, B=3):
    """q [B, S, D], k [B, No, D] in [-3, 3]; mask [B, No] with sample 1 fully padded; ds fp32 [B, S, No] in [-3, 3].  With scale = 2^-5 every score and every
    gradient is an integer multiple of 2^-5 below 2^17: 22 significant bits at most, exact in fp32 in any order"""
    s = S + No + D
    q, k = ints((B, S, D), s + 1), ints((B, No, D), s + 2)
    mask = torch.ones(B, No, dtype=torch.uint8)
    mask[0, No - No // 5:] = 0
    mask[1] = 0
    mask[2, No // 3:] = 0
    ds = ints((B, S, No), s + 3, dtype=torch.float32)
    assert_exact_budget(q[0], k[0].t(), 10000.0, name="ptr scores")
    assert 9.0 * max(S, No) < BUDGET
    return q, k, mask, ds

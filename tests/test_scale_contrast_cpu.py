"""Scale contrast, the host half: the sliced comparison helper's blind-spot demonstration, the inputs the GPU tests (tests/test_scale_contrast_gpu.py)
share, the check that the per-row 1e-3 GEMM bound is fair for a plain fp32 matmul of those inputs, and the host emulation of the one-pass attention
backward's fp16 second stage that fixes the row-contrast range and bound (no GPU: everything here is torch on the CPU)."""
import math

import numpy as np
import pytest
import torch

from oracle import sa_m4c_oracle as O
from tests.golden import common as C
from tests.test_attention_gpu import make_problem, oracle_attention
from tests.util import assert_close_bf16, assert_close_bf16_sliced

BF16 = torch.bfloat16


# ------------------------------------------------------------------------------------------------ the helper itself
def test_sliced_helper_sees_what_the_global_bound_cannot():
    """one row at 2^-20 of the others carries a 10 % error: 1e-7 of the tensor's maximum, so assert_close_bf16 passes it; judged against its own
    scale it is a hundred times over the bound.  The message names the slice, its scale and its error; all-zero reference slices must be exact."""
    g = torch.Generator().manual_seed(0)
    ref = torch.randn(6, 40, generator=g, dtype=torch.float64)
    ref[3] *= 2.0 ** -20
    got = ref.clone()
    got[3] *= 1.1
    assert_close_bf16(got, ref, name="global")                              # blind
    with pytest.raises(AssertionError) as ei:
        assert_close_bf16_sliced(got, ref, (1,), name="rows")
    msg = str(ei.value)
    assert "slice (3, 0)" in msg and "%.4g" % ref[3].abs().max().item() in msg and "%.4g" % (got[3] - ref[3]).abs().max().item() in msg, msg
    assert_close_bf16_sliced(ref.clone(), ref, (1,), ulps=0, name="exact")
    assert_close_bf16_sliced(got, ref, (0, 1), name="one slice = the global bound")
    # the other axis: a column slice (reduce over dim 0) that is fine row-wise fails column-wise only where it is wrong
    got2 = ref.clone()
    got2[:, 7] = 0.0
    with pytest.raises(AssertionError, match=r"slice \(0, 7\)"):
        assert_close_bf16_sliced(got2, ref, (0,), name="columns")
    # an all-zero reference slice: exactly zero or a failure, whatever the rest of the tensor holds
    ref0 = ref.clone()
    ref0[2] = 0.0
    ok = ref0.clone()
    assert_close_bf16_sliced(ok, ref0, (1,), name="zero row kept")
    ok[2, 5] = 1e-30
    with pytest.raises(AssertionError, match=r"slice \(2, 0\)"):
        assert_close_bf16_sliced(ok, ref0, (1,), name="zero row touched")
    assert_close_bf16(ok, ref0, name="global")                              # blind again
    with pytest.raises(AssertionError):
        assert_close_bf16_sliced(torch.full_like(ref, float("nan")), ref, (1,))


# ------------------------------------------------------------------------------------------------ GEMM inputs
ROW_EXPONENTS = (-24, -12, 0, 12, 24)
GEMM_MNK = (600, 520, 192)            # ragged in M and N for every tile, three k-tiles of 64
GEMM_K_4WAVE = 712                    # the 4-wave kernels also take K % 64 != 0
WGRAD_RMN = (1000, 520, 264)


def rnd(shape, seed, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(*shape, generator=g) * scale).to(BF16)


def row_exponents(n, seed):
    """one exponent of ROW_EXPONENTS per row; every value occurs, neighbours differ more often than not"""
    g = torch.Generator().manual_seed(seed)
    k = torch.tensor(ROW_EXPONENTS)[torch.randint(0, len(ROW_EXPONENTS), (n,), generator=g)]
    k[:len(ROW_EXPONENTS)] = torch.tensor(ROW_EXPONENTS)
    return k


def pow2(k, device="cpu"):
    """2^k as exact fp64 factors, built on the host (a device pow / ldexp need not be exact) -- multiplying by them in fp64 is"""
    k = k.detach().cpu()
    return torch.ldexp(torch.ones(k.shape, dtype=torch.float64), k.double()).to(device)


def scale_rows(x, k):
    """x[i, :] * 2^k[i], exact in bf16 (|k| <= 24 on O(1) data stays far inside the exponent range)"""
    exact = x.double() * pow2(k, x.device)[:, None]
    y = exact.to(x.dtype)
    assert torch.equal(y.double(), exact)
    return y


def gemm_operands(K):
    """forward / dgrad operands of the contrast tests: x [M, K], W [N, K] (forward), Wt [K, N] (dgrad), aux [M, N], per-row exponents [M]"""
    M, N, _ = GEMM_MNK
    return dict(x=rnd((M, K), 81), w=rnd((N, K), 82, 0.05), wt=rnd((K, N), 83, 0.05), aux=rnd((M, N), 84), k=row_exponents(M, 85))


def wgrad_operands(R=WGRAD_RMN[0], M=WGRAD_RMN[1], N=WGRAD_RMN[2], seed=0):
    """dy [R, M], x [R, N] and one exponent per COLUMN m of dy (= row m of dW, element m of the bias gradient)"""
    return dict(dy=rnd((R, M), seed + 86), x=rnd((R, N), seed + 87), k=row_exponents(M, seed + 88))


@pytest.mark.parametrize("K", [GEMM_MNK[2], GEMM_K_4WAVE])
def test_plain_fp32_matmul_meets_the_per_row_gemm_bound(K):
    """the per-row bound of the GPU tests (1e-3 * max|row| for fp32 outputs, + one bf16 ulp for bf16 outputs) is no measurement of the kernels: a plain
    fp32 product of the same contrast operands meets it against fp64 with the contraction in either order.  Why: the fp32 sum of K products is off by at
    most K * 2^-24 * sum|a b| <= 6e-5 * sum|a b| at K <= 1000, and for Gaussian rows sum|a b| ~ 0.64 K sigma_a sigma_b while max|row| ~ 3 sqrt(K) sigma_a
    sigma_b: the worst case is 6e-5 * 0.2 sqrt(K) <= 4e-4 of the row's maximum, the typical (random-sign) error a thousand times less."""
    ops = gemm_operands(K)
    xs = scale_rows(ops["x"], ops["k"])
    for nm, a, b in (("forward", xs, ops["w"].t()), ("dgrad", xs, ops["wt"])):
        ref = a.double() @ b.double()
        assert ref.abs().amax(1).min() > 0
        e1 = assert_close_bf16_sliced(a.float() @ b.float(), ref, (1,), ulps=0, name=nm + " fp32")
        rev = torch.arange(K - 1, -1, -1)
        e2 = assert_close_bf16_sliced(a.float()[:, rev] @ b.float()[rev], ref, (1,), ulps=0, name=nm + " fp32, K reversed")
        assert_close_bf16_sliced((a.float() @ b.float()).to(BF16), ref, (1,), ulps=1, name=nm + " bf16 of fp32")
        assert max(e1, e2) < 1e-4, (e1, e2)                                   # two orders inside the bound that the kernels get
    # the exact-scaling premise: the contrast product is the plain product with its rows shifted
    plain = ops["x"].double() @ ops["w"].double().t()
    assert torch.equal(xs.double() @ ops["w"].double().t(), plain * pow2(ops["k"])[:, None])


def test_plain_fp32_matmul_meets_the_per_row_wgrad_bound():
    w = wgrad_operands()
    dys = scale_rows(w["dy"].t().contiguous(), w["k"]).t().contiguous()
    ref = dys.double().t() @ w["x"].double()
    R = dys.shape[0]
    rev = torch.arange(R - 1, -1, -1)
    assert_close_bf16_sliced(dys.float().t() @ w["x"].float(), ref, (1,), ulps=0, name="wgrad fp32")
    assert_close_bf16_sliced(dys.float()[rev].t() @ w["x"].float()[rev], ref, (1,), ulps=0, name="wgrad fp32, R reversed")
    # the bias gradient: every element is its own slice, the bound is 1e-3 of the element
    rb = dys.double().sum(0)
    assert_close_bf16_sliced(dys.float().sum(0)[:, None], rb[:, None], (1,), ulps=0, name="bias grad fp32")
    assert_close_bf16_sliced(dys.float()[rev].sum(0)[:, None], rb[:, None], (1,), ulps=0, name="bias grad fp32, reversed")


# ------------------------------------------------------------------------------------------------ attention inputs
H, HD = 12, 64
P_DROP = 0.1
INV_KEEP = 1.0 / (1.0 - round(P_DROP * 65536) / 65536.0)
ATTN_CASES = ("spatial57", "pad200")
HEAD_EXPONENT = 20


def attn_case(case):
    """(problem dict with `allow` [B, H, N, N] bool and `spatial`, qkv bf16 [B*N, 3*H*64], dO bf16 [B*N, H*64])"""
    if case == "spatial57":
        pr = make_problem(2, 5, 30, 20, 7, seed=2)
        pr["allow"] = O.allow_mask(pr["key_valid"], pr["T"], pr["n_oo"], pr["n_dec"], pr["adj"], (1, 2), H)
        pr["spatial"] = True
    else:                                  # key padding only, 200 tokens: the chunked 193..384 path, 8-word mask rows
        T = 200
        kvm = torch.from_numpy(C.pad_mask([T, 77], T))
        pr = dict(B=2, T=T, n_oo=0, n_dec=0, N=T, H=H, key_valid=kvm, adj=None, spatial=False)
        pr["allow"] = O.allow_mask(kvm, T, 0, 0, None, (), H)
    g = torch.Generator().manual_seed(5)
    qkv = (torch.randn(pr["B"] * pr["N"], 3 * H * HD, generator=g) * 1.5).to(BF16)
    dout = torch.randn(pr["B"] * pr["N"], H * HD, generator=g).to(BF16)
    return pr, qkv, dout


def head_exponents(B):
    """(kq, kv, kd) [B, H] in {-20, 0, 20}: q * 2^kq and k * 2^-kq (scores unchanged), v * 2^kv, dO * 2^kd; neighbouring heads and the two samples differ in each"""
    b, h = torch.meshgrid(torch.arange(B), torch.arange(H), indexing="ij")
    e = HEAD_EXPONENT
    return ((b + h) % 3 - 1) * e, ((2 * h + b + 1) % 3 - 1) * e, ((h + 2 * b + 2) % 3 - 1) * e


def _shift(x, k):
    y = x.double() * pow2(k, x.device)
    out = y.to(x.dtype)
    assert torch.equal(out.double(), y), "the shift must be exact in %s" % x.dtype
    return out


def apply_head_exponents(qkv, dout, B):
    N = qkv.shape[0] // B
    kq, kv, kd = head_exponents(B)
    x = qkv.view(B, N, 3, H, HD)
    ks = torch.stack([kq, -kq, kv], 1)[:, None, :, :, None]                # [B, 1, 3, H, 1]
    return _shift(x, ks).reshape(qkv.shape), _shift(dout.view(B, N, H, HD), kd[:, None, :, None]).reshape(dout.shape)


def head_shift_of_out(B):
    """exponent by which `out` [B, N, H, 64] moves under head_exponents: kv"""
    return head_exponents(B)[1][:, None, :, None]


def head_shift_of_dqkv(B):
    """exponents by which dqkv [B, N, 3, H, 64] moves: dQ kd + kv - kq, dK kd + kv + kq, dV kd"""
    kq, kv, kd = head_exponents(B)
    return torch.stack([kd + kv - kq, kd + kv + kq, kd], 1)[:, None, :, :, None]


# rows of dO: exponent -k per TOKEN (all heads of the token), in a fixed cycle.  ROW_K_CHECKED are bounded per row with ROW_FRAC, ROW_K_NONZERO only has to come
# out non-zero where the emulation keeps it non-zero, None = a dO row of exact zeros (dQ row exactly zero).  The k = 0 rows keep the head's dO maximum where it was.
ROW_K_MAX = 10
ROW_K_CHECKED = (0, 4, ROW_K_MAX)
ROW_K_NONZERO = 16
ROW_CYCLE = (0, ROW_K_MAX, None, 4, 0, ROW_K_NONZERO, ROW_K_MAX, 4)
# ROW_E: the emulation's largest per-row error of dQ on the UNSCALED inputs of each case (in the helper's terms: the smallest `frac` its bf16 result passes with, over
# the rows with at least two allowed keys), measured by test_emulation_fixes_the_row_contrast_range_and_bound.  It is a conditioning figure as much as a rounding one:
# dS = P (dP - delta) cancels where the softmax is nearly one-hot, so the spatial case (rows with two or three allowed keys) sits at 3.9e-2 and the 200-token case
# (77+ keys per row) at 5.9e-4.  ROW_FRAC, the GPU tests' per-row bound: twice that, for the accumulation order and the exp2 / rcp approximations not modelled.
ROW_E = {"spatial57": 3.86e-2, "pad200": 5.91e-4}
ROW_FRAC = {c: 2 * e for c, e in ROW_E.items()}


def rows_with_a_gradient(allow):
    """[B, N, H] bool: query rows with at least two allowed keys.  With one key the softmax is the constant 1 and dQ is zero by cancellation (dP - delta), which no
    finite-precision delta reproduces exactly: such rows are judged with their head, not on their own."""
    return (allow.sum(-1) >= 2).permute(0, 2, 1)


def row_exponents_of_tokens(N, k_small=None):
    """(k [N] int, zero [N] bool, checked [N] bool); k_small: every non-zero exponent of the cycle replaced by this one (the k = 0 rows keep setting the head's maximum)"""
    cyc = [ROW_CYCLE[(i * 5 + i // 8) % len(ROW_CYCLE)] for i in range(N)]
    if k_small is not None:
        cyc = [c if not c else k_small for c in cyc]
    zero = torch.tensor([c is None for c in cyc])
    k = torch.tensor([0 if c is None else c for c in cyc])
    checked = torch.tensor([c is not None and c in ROW_K_CHECKED for c in cyc])
    return k, zero, checked


def apply_row_exponents(dout, B, k_small=None):
    N = dout.shape[0] // B
    kk, zero, _ = row_exponents_of_tokens(N, k_small)
    d = _shift(dout.view(B, N, -1), -kk[None, :, None])
    d = torch.where(zero[None, :, None], torch.zeros_like(d), d)
    return d.reshape(dout.shape)


# ------------------------------------------------------------------------------------------------ the emulation
def _f16(x):
    return x.to(torch.float32).to(torch.float16).to(torch.float64)        # RNE with subnormals, as v_cvt_pk_f16_f32


def _bf(x):
    return x.to(torch.float32).to(BF16).to(torch.float64)


def _block_fp16(x):
    """csrc/attn_common.h bf2h_pk per (batch, head): x [B, H, n, 64] (bf16 values) -> (its fp16 image as real numbers, e) with image = x * 2^e exactly,
    e = 112 - c, c = max(E_max - 29, 0) from the biased exponent of the head's largest magnitude; an element whose exponent field is <= c loses its implicit
    one (exponent field c: the mantissa bits alone, as an fp16 subnormal) or flushes to zero (below c)"""
    ax = x.abs()
    mx = ax.amax(dim=(-1, -2), keepdim=True)
    e8 = torch.where(ax > 0, torch.floor(torch.log2(ax.clamp_min(2.0 ** -126))) + 127, torch.zeros_like(ax))
    emax = torch.where(mx > 0, torch.floor(torch.log2(mx.clamp_min(2.0 ** -126))) + 127, torch.zeros_like(mx))
    c = (emax - 29).clamp_min(0)
    e = 112 - c
    img = torch.ldexp(x, e.expand_as(x))
    frac_only = torch.sign(x) * (ax * torch.exp2(127 - e8) - 1.0) * 2.0 ** -14          # m7 / 128 * 2^-14
    img = torch.where(e8 > c, img, torch.where(e8 == c, frac_only, torch.zeros_like(x)))
    assert img.abs().max() < 2.0 ** 15
    return img, e


def emulate_fused_pair(qkv, dout, allow, keep, B, scale=0.125, p_drop=P_DROP):
    """sam_attn_fwd_train + sam_attn_bwd_fused with every fp16 / bf16 rounding the kernels' comments describe and everything else in fp64:
    forward -- P * 2^14 rounded to fp16 ahead of the PV MFMA (the row sum is taken before rounding and before dropout), V as block-scaled fp16 (exact), out = bf16,
    out_lo = bf16(out_exact - out);  backward -- Q, K, dO, V as block-scaled fp16 with the flush below 2^-29 of the head's maximum, delta = rowsum(dO * (out +
    out_lo)), P * 2^14 = exp2(s - lse2 + 14), dS * 2^eS rounded to fp16 with eS = eD + eV - 22 - sh and kappa = inv_keep * scale = m * 2^sh (subnormal below 2^-14,
    zero below 2^-25), P~ rounded to fp16, dQ = dS16 . K16, dK = dS16^T . Q16, dV = P~16^T . dO16, each scaled back and rounded to bf16.
    -> (out [B*N, H*64], dqkv [B*N, 3*H*64]) as fp64 tensors holding bf16 values."""
    rows = qkv.shape[0]
    N = rows // B
    x = qkv.double().view(B, N, 3, H, HD).permute(2, 0, 3, 1, 4)
    q, k, v = x[0], x[1], x[2]
    do = dout.double().view(B, N, H, HD).permute(0, 2, 1, 3)
    inv_keep = INV_KEEP if p_drop > 0 else 1.0
    keepf = keep.double() if keep is not None else torch.ones_like(allow, dtype=torch.float64)
    s2 = (q @ k.transpose(-1, -2)) * (scale * math.log2(math.e))
    s2 = s2.masked_fill(~allow, float("-inf"))
    alive = allow.any(-1, keepdim=True)
    mx = torch.where(alive, s2.amax(-1, keepdim=True), torch.zeros_like(s2[..., :1]))
    p14 = torch.exp2(s2 - mx + 14)
    ssum = p14.sum(-1, keepdim=True)
    v16, ev = _block_fp16(v)
    o = torch.where(alive, (_f16(p14) * keepf) @ v16 * torch.exp2(-ev) * inv_keep / ssum.clamp_min(2.0 ** -40), torch.zeros_like(q))
    o_hi = _bf(o)
    o_lo = _bf(o - o_hi)
    lse2 = torch.where(alive, mx + torch.log2(ssum.clamp_min(2.0 ** -40)) - 14, torch.full_like(mx, float("inf")))
    # backward
    q16, eq = _block_fp16(q)
    k16, ek = _block_fp16(k)
    d16, ed = _block_fp16(do)
    kappa = inv_keep * scale
    _, sh = math.frexp(kappa)
    es = ed + ev - 22 - sh
    delta = (do * (o_hi + o_lo)).sum(-1, keepdim=True)
    pn14 = torch.exp2(s2 - lse2 + 14)                                      # dead rows: exp2(-inf) = 0
    pn14 = torch.where(alive, pn14, torch.zeros_like(pn14))
    acc_dp = (d16 @ v16.transpose(-1, -2)) * keepf
    ds = pn14 * (acc_dp * kappa * torch.exp2(-36.0 - sh + torch.zeros_like(es)) + (-scale * delta) * torch.exp2(ed + ev - 36 - sh))
    ds16 = _f16(ds)
    assert ds16.abs().max() < 2.0 ** 15
    pt16 = _f16(pn14) * keepf
    dq = _bf((ds16 @ k16) * torch.exp2(-es - ek))
    dk = _bf((ds16.transpose(-1, -2) @ q16) * torch.exp2(-es - eq))
    dv = _bf((pt16.transpose(-1, -2) @ d16) * torch.exp2(-14 - ed) * inv_keep)
    dqkv = torch.stack([dq, dk, dv], 0).permute(1, 3, 0, 2, 4).reshape(rows, 3 * H * HD)
    return o_hi.permute(0, 2, 1, 3).reshape(rows, H * HD), dqkv


def oracle_pair(qkv, dout, allow, keep, B, scale=0.125, p_drop=P_DROP):
    """fp64 oracle (tests/test_attention_gpu.py: oracle_attention) forward and backward -> (out, dqkv)"""
    x = qkv.double().requires_grad_(True)
    out, _ = oracle_attention(x, allow, B, H, scale, keep, INV_KEEP if (p_drop > 0 and keep is not None) else 1.0)
    (out * dout.double()).sum().backward()
    return out.detach(), x.grad


def needed_frac(got, ref, slice_dims, ulps=1):
    """per slice: the smallest `frac` with which assert_close_bf16_sliced passes (0 where the slice is exact; inf where a zero slice is touched)"""
    got, ref = got.double(), ref.double()
    scale = ref.abs().amax(dim=slice_dims, keepdim=True)
    over = ((got - ref).abs() - ulps * 2.0 ** -8 * ref.abs()).amax(dim=slice_dims, keepdim=True).clamp_min(0)
    return torch.where(scale > 0, over / scale.clamp_min(1e-300), torch.where(over > 0, torch.full_like(over, float("inf")), torch.zeros_like(over)))


def host_keep(allow, seed=17):
    g = torch.Generator().manual_seed(seed)
    return torch.rand(allow.shape, generator=g) >= P_DROP


def dq_rows(dqkv, B):
    """dqkv [B*N, 3*H*64] -> its dQ part as [B, N, H, 64]: one slice per (token, head) under slice_dims = (3,)"""
    return dqkv.view(B, dqkv.shape[0] // B, 3, H, HD)[:, :, 0]


_EMU = {}


def emulated_row_errors(case):
    """{k: (largest needed per-row frac of dQ over the rows at 2^-k, every such row that the oracle has non-zero is non-zero)} of the emulation with a host-drawn keep mask;
    k = 0: unscaled inputs, all rows; else every non-zero exponent of the cycle replaced by k (the k = 0 rows stay and set the head's maximum)"""
    if case not in _EMU:
        pr, qkv, dout = attn_case(case)
        B = pr["B"]
        keep = host_keep(pr["allow"])
        ok = rows_with_a_gradient(pr["allow"])
        res = {}
        for k in (0, 4, ROW_K_MAX, ROW_K_MAX + 1, ROW_K_NONZERO):
            d = apply_row_exponents(dout, B, k_small=k) if k else dout
            _, ref = oracle_pair(qkv, d, pr["allow"], keep, B)
            _, emu = emulate_fused_pair(qkv, d, pr["allow"], keep, B)
            kk, zero, _ = row_exponents_of_tokens(pr["N"], k)
            sel = ok & (((kk == k) & ~zero)[None, :, None] if k else torch.ones_like(ok))
            nf = needed_frac(dq_rows(emu, B), dq_rows(ref, B), (3,))[..., 0]
            live = sel & (dq_rows(ref, B).abs().amax(-1) > 0)
            res[k] = (nf[sel].max().item(), bool((dq_rows(emu, B).abs().amax(-1)[live] > 0).all()))
        _EMU[case] = res
    return _EMU[case]


@pytest.mark.parametrize("case", ATTN_CASES)
def test_emulation_fixes_the_row_contrast_range_and_bound(case):
    """where ROW_E, ROW_FRAC and ROW_K_MAX come from (nothing here has seen a kernel's output).  Measured with the host-drawn keep mask:
        case        E (unscaled)  bound 2E   rows at 2^-4   2^-10     2^-11     2^-16
        spatial57   3.86e-2       7.7e-2     1.0e-2         6.8e-3    6.8e-3    5.9e-2
        pad200      5.90e-4       1.18e-3    4.7e-4         7.3e-4    2.2e-3    3.4e-2
    The fp16 image of dS keeps 11 bits down to 2^-14 and the typical dS16 of these inputs is 2^-2 .. 2^-4: a dO row 2^-10 below the head's largest still has
    full-precision dS, at 2^-11 the first entries are subnormal and the well-conditioned case leaves its bound, so ROW_K_MAX = 10.  At 2^-16 every row is still non-zero."""
    res = emulated_row_errors(case)
    e0 = res[0][0]
    assert 0.95 * ROW_E[case] <= e0 <= ROW_E[case], (e0, ROW_E[case])
    for k in (4, ROW_K_MAX):
        assert res[k][0] <= ROW_FRAC[case], (k, res[k], ROW_FRAC[case])
    if case == "pad200":
        assert res[ROW_K_MAX + 1][0] > ROW_FRAC[case], "ROW_K_MAX is the largest exponent the emulation keeps inside the bound"
    assert all(v[1] for v in res.values()), res
    # the mixed rows of the GPU test itself, and the head-level figures it bounds with 1e-3
    pr, qkv, dout = attn_case(case)
    B, N = pr["B"], pr["N"]
    keep = host_keep(pr["allow"])
    d = apply_row_exponents(dout, B)
    out_ref, ref = oracle_pair(qkv, d, pr["allow"], keep, B)
    out_emu, emu = emulate_fused_pair(qkv, d, pr["allow"], keep, B)
    _, zero, checked = row_exponents_of_tokens(N)
    sel = rows_with_a_gradient(pr["allow"]) & checked[None, :, None]
    nf = needed_frac(dq_rows(emu, B), dq_rows(ref, B), (3,))[..., 0]
    assert nf[sel].max().item() <= ROW_FRAC[case]
    assert (dq_rows(emu, B)[:, zero] == 0).all() and (dq_rows(ref, B)[:, zero] == 0).all()
    assert_close_bf16_sliced(emu.view(B, N, 3, H, HD), ref.view(B, N, 3, H, HD), (1, 4), name="emulated dqkv per (part, sample, head)")
    assert_close_bf16_sliced(out_emu.view(B, N, H, HD), out_ref.view(B, N, H, HD), (1, 3), name="emulated out per (sample, head)")


def test_emulation_is_scale_free_per_head():
    """the premise of the bitwise companion test: with power-of-two head scales the emulated pipeline's outputs are the uniform run's, shifted"""
    pr, qkv, dout = attn_case("spatial57")
    B, N = pr["B"], pr["N"]
    keep = host_keep(pr["allow"])
    o0, g0 = emulate_fused_pair(qkv, dout, pr["allow"], keep, B)
    q1, d1 = apply_head_exponents(qkv, dout, B)
    o1, g1 = emulate_fused_pair(q1, d1, pr["allow"], keep, B)
    assert torch.equal(o1.view(B, N, H, HD), o0.view(B, N, H, HD) * pow2(head_shift_of_out(B)))
    assert torch.equal(g1.view(B, N, 3, H, HD), g0.view(B, N, 3, H, HD) * pow2(head_shift_of_dqkv(B)))

"""Exact arithmetic on integer operands, the host half (no GPU: everything here is torch on the CPU).

(1) The premise: fp32 sums of integer products below 2^17 do not depend on the order -- sequential, shuffled, split into 2 / 3 / 7 slices, pairwise -- and
    equal the float64 reference bit for bit (with Gaussian operands the same orders disagree: that is why the parity tests carry a tolerance).
(2) The gap: each fault below is applied to an exact reference of tests/exact_cases.py.  The bound the GPU tests use today (tests/util.py:assert_close_bf16
    with the arguments of tests/test_gemm_gpu.py) passes it; the exact comparison of tests/test_exact_integer_gpu.py fails it.
        * the result rounded twice: bf16 before the residual is added, bf16 again on store (passes the cross-variant bound everywhere; the bound against
          the reference catches it among the tensor's largest elements only)
        * C carried in bf16 across an accumulate
        * round-half-away-from-zero instead of round-to-nearest-even in the bf16 store
        * the bias applied after the dropout scale instead of before it
    Truncation instead of round-to-nearest-even is NOT in the list: at these magnitudes the old bound catches it (shown below), so it is no gap.
(3) Budget (< 2^17) and tie share (>= 1 % of every bf16 reference) of every case table the GPU file uses."""
import pytest
import torch

from tests import exact_cases as E
from tests.util import assert_close_bf16

BF16 = torch.bfloat16


# ------------------------------------------------------------------------------------------------ (1) the premise
def _sum_sequential(p, order):
    acc = torch.zeros_like(p[:, 0])
    for k in order:
        acc = acc + p[:, k]
    return acc


def _sum_blocked(p, slices):
    K = p.shape[1]
    per = (K + slices - 1) // slices
    parts = [_sum_sequential(p, range(s * per, min(K, (s + 1) * per))) for s in range(slices)]
    acc = parts[0]
    for q in parts[1:]:
        acc = acc + q
    return acc


def _sum_pairwise(p):
    while p.shape[1] > 1:
        if p.shape[1] % 2:
            p = torch.cat([p, torch.zeros_like(p[:, :1])], 1)
        p = p[:, 0::2] + p[:, 1::2]
    return p[:, 0]


def _orders(p):
    K = p.shape[1]
    g = torch.Generator().manual_seed(5)
    yield "sequential", _sum_sequential(p, range(K))
    yield "reversed", _sum_sequential(p, range(K - 1, -1, -1))
    for j in range(3):
        yield "shuffled %d" % j, _sum_sequential(p, torch.randperm(K, generator=g).tolist())
    for s in (2, 3, 7):
        yield "%d slices" % s, _sum_blocked(p, s)
    yield "pairwise", _sum_pairwise(p)
    yield "torch.sum", p.sum(1)


def test_fp32_sums_of_integer_products_do_not_depend_on_the_order():
    M, K, N, r = 24, 712, 40, 5
    a, b = E.ints((M, K), 1, -r, r), E.ints((K, N), 2, -r, r)
    E.assert_exact_budget(a, b)
    p = a.float()[:, :, None] * b.float()[None]                     # [M, K, N] fp32 products: exact
    ref = E.exact_mm(a, b)
    for name, s in _orders(p):
        assert s.dtype == torch.float32 and torch.equal(s.double(), ref), name
    # the same orders on Gaussian operands disagree with one another: what the parity tests' tolerance is for
    g = torch.Generator().manual_seed(3)
    pg = torch.randn(M, K, 1, generator=g) * torch.randn(1, K, N, generator=g)
    sums = [s for _, s in _orders(pg)]
    assert any(not torch.equal(sums[0], s) for s in sums[1:])


# ------------------------------------------------------------------------------------------------ (2) faults the old bound passes
def _old_bound_passes(got, ref, **kw):
    assert_close_bf16(got, ref, **kw)
    return True


def _exact_fails(got, want):
    msg = E.describe_mismatch(got, want, "fault")
    assert msg is not None and "differ" in msg and "difference" in msg, msg
    return msg


def _round_half_away(x_f64):
    """fp32 -> bf16 by adding half a step to the magnitude and truncating: right everywhere except at exact ties with an even lower neighbour"""
    bits = x_f64.to(torch.float32).view(torch.int32)
    return ((bits + 0x8000) & ~0xFFFF).view(torch.float32).to(BF16)


def _truncate(x_f64):
    return (x_f64.to(torch.float32).view(torch.int32) & ~0xFFFF).view(torch.float32).to(BF16)


@pytest.fixture(scope="module")
def case():
    return E.gemm_case("ragged712")


def test_fault_double_rounding_before_the_residual(case):
    """half a gap: the cross-variant bound (ulps=2: `split dropout+res vs unsplit`, `fwd dropout+res vs 4-wave kernel`) passes every element; the bound against
    the fp32 reference (ulps=1) catches it, but only among the tensor's largest elements where both roundings go the same way -- about one element in a
    thousand here, which Gaussian data need not hit.  The exact comparison sees every element that is rounded differently: one in nine."""
    c = case
    acc = E.exact_mm(c["x"], c["w"].t()) + c["bias"].double()
    exact = acc + c["res"].double()
    want = c["want"]["fwd_res"]
    got = E.rne_bf16(E.rne_bf16(acc).double() + c["res"].double())                  # bf16 before the residual, bf16 again on store
    assert _old_bound_passes(got, want.float(), ulps=2, name="vs another variant")
    over = (got.double() - exact).abs() > 1e-3 * exact.abs().max() + 2.0 ** -8 * exact.abs()      # assert_close_bf16's default bound, element by element
    assert 0 < float(over.double().mean()) < 5e-3 and float(exact.abs()[over].min()) > 0.25 * float(exact.abs().max())
    _exact_fails(got, want)
    assert float((got != want).double().mean()) > 0.05                                # ... the exact check sees many times as many


def test_fault_c_carried_in_bf16_across_an_accumulate():
    R, M, N = E.WGRAD_CASES[-1]                                                        # the deep one: sums of thousands, against which an error of 1 is 1e-3 of nothing
    c = E.wgrad_case(R, M, N)
    want = (c["c0"].double() + c["prod"]).float()
    got = (c["c0"].to(BF16).double() + c["prod"]).float()
    assert not torch.equal(c["c0"].to(BF16).float(), c["c0"])                         # integers up to 500 are not all bf16 values
    assert _old_bound_passes(got, c["c0"].double() + c["prod"], ulps=0, name="split-k wgrad")      # test_wgrad_split_k_and_fused_bias_grad
    _exact_fails(got, want)
    wantb = (c["b0"].double() + c["colsum"]).float()
    gotb = (c["b0"].to(BF16).double() + c["colsum"]).float()
    assert _old_bound_passes(gotb, c["b0"].double() + c["colsum"], ulps=0, frac=2e-3, name="bias grad")
    _exact_fails(gotb, wantb)


def test_fault_round_half_away_instead_of_nearest_even(case):
    c = case
    for key, exact in (("fwd_none", E.exact_mm(c["x"], c["w"].t())), ("dgrad_aux", E.exact_mm(c["x"], c["wt"]) * c["aux"].double())):
        got = _round_half_away(exact)
        assert _old_bound_passes(got, exact, name=key)
        assert _old_bound_passes(got, c["want"][key].float(), ulps=2, name=key)
        _exact_fails(got, c["want"][key])
        differ = got != c["want"][key]
        assert bool((differ <= E.is_tie(exact)).all()) and float(differ.double().mean()) > 0.3 * c["ties"][key]      # wrong at ties only, and at about half of them


def test_truncation_is_caught_by_the_old_bound_too_so_it_is_no_gap(case):
    c = case
    exact = E.exact_mm(c["x"], c["w"].t())
    got = _truncate(exact)
    with pytest.raises(AssertionError):
        assert_close_bf16(got, exact, name="fwd")
    _exact_fails(got, c["want"]["fwd_none"])


def test_fault_bias_applied_after_the_dropout_scale(case):
    """p_drop = 0.5: kept = res + 2 (acc + bias); the fault computes res + 2 acc + bias.  With a bias that is small against the tensor's maximum (the
    existing tests draw it from N(0, 1) or N(0, 0.01) against sums of hundreds) the kept-value bound of test_forward_gelu_and_dropout_residual passes it."""
    c = case
    acc = E.exact_mm(c["x"], c["w"].t())
    bias = E.ints((c["N"],), 9, -1, 1, torch.float32).double()
    assert float(bias.abs().max()) == 1.0
    kept = c["res"].double() + 2.0 * (acc + bias)
    want, got = E.rne_bf16(kept), E.rne_bf16(c["res"].double() + 2.0 * acc + bias)
    assert _old_bound_passes(got, kept, name="kept values")
    assert _old_bound_passes(got, want.float(), ulps=2, name="vs another variant")
    _exact_fails(got, want)


def test_mismatch_report_names_count_index_values_and_difference():
    want = torch.arange(12, dtype=torch.float32).reshape(3, 4)
    got = want.clone()
    got[1, 2] += 5
    got[2, 3] -= 1
    msg = E.describe_mismatch(got, want, "demo")
    assert msg == "demo: 2 of 12 elements differ; first at (1, 2): got 11.0, want 6.0, difference 5.0", msg
    assert E.describe_mismatch(want.clone(), want) is None
    assert "dtype" in E.describe_mismatch(want.to(BF16), want)


# ------------------------------------------------------------------------------------------------ (3) the case tables
def test_generators_are_integer_valued_seeded_and_half_zero():
    a, b = E.ints((50, 60), 4), E.ints((50, 60), 4)
    assert torch.equal(a, b) and a.dtype == BF16 and float(a.min()) == -3 and float(a.max()) == 3 and torch.equal(a.float(), a.float().round())
    z = E.half_zero_ints((200, 200), 5, dtype=torch.float32)
    assert z.dtype == torch.float32 and 0.5 < float((z == 0).float().mean()) < 0.64          # half zeroed, a seventh of the rest zero anyway
    with pytest.raises(AssertionError):
        E.ints((4, 4), 1, -300, 300)                                   # 257 is not a bf16 value


def test_budget_and_tie_assertions_bite():
    a, b = E.ints((8, 4096), 1, -16, 16), E.ints((4096, 8), 2, -16, 16)
    with pytest.raises(AssertionError, match="budget"):
        E.assert_exact_budget(a, b)                                     # 4096 products of about 8.5 x 8.5 in magnitude: past 2^17
    assert E.assert_exact_budget(E.ints((8, 64), 1), E.ints((64, 8), 2), 100.0, gain=2.0) <= 2 * 64 * 9 + 100
    with pytest.raises(AssertionError, match="budget"):
        E.assert_exact_budget(E.ints((8, 64), 1), E.ints((64, 8), 2), 2.0 ** 17)
    small = E.exact_mm(E.ints((64, 64), 1), E.ints((64, 64), 2))        # |sums| of 64 products in [-9, 9] never reach 256: no ties
    with pytest.raises(AssertionError, match="ties"):
        E.assert_ties(small)
    t = torch.tensor([257.0, 258.0, 259.0, 514.0, 516.0, 255.5, 3.0, -261.0], dtype=torch.float64)
    assert E.is_tie(t).tolist() == [True, False, True, True, False, False, False, True]
    assert E.rne_bf16(t).tolist() == [256.0, 258.0, 260.0, 512.0, 516.0, 256.0, 3.0, -260.0]
    with pytest.raises(AssertionError):
        E.rne_bf16(torch.tensor([2.0 ** 30 + 1], dtype=torch.float64))


@pytest.mark.parametrize("name", sorted(E.GEMM_CASES))
def test_gemm_case_tables_meet_budget_and_tie_share(name):
    c = E.gemm_case(name)                                               # asserts budget, ties and dropped != kept itself
    assert set(c["ties"]) == {"fwd_none", "fwd_bias", "fwd_res", "dgrad_none", "dgrad_aux", "dgrad_res", "fwd_drop", "dgrad_drop"}
    assert min(c["ties"].values()) >= E.MIN_TIE_SHARE
    for k in ("fwd_drop", "dgrad_drop"):
        dropped, kept = c["want"][k]
        assert bool((dropped != kept).all())


def test_weight_gradient_and_reduction_tables_meet_the_budget():
    for R, M, N in E.WGRAD_CASES:
        E.wgrad_case(R, M, N, want_ref=False)
    for name in E.GROUPED_CASES:
        assert len(E.grouped_case(name, want_ref=False)) == len(E.GROUPED_CASES[name]) <= 12
    for M, N in E.COLSUM_SHAPES:
        E.colsum_case(M, N)
    for n in E.SUMSQ_N:
        g = E.sumsq_case(n)
        assert g.numel() == n and float(g.abs().max()) <= 2
    assert float((E.sumsq_case(1000003) != 0).sum()) > 10000
    for S, No, D in E.PTR_SHAPES:
        q, k, mask, ds = E.ptr_case(S, No, D)
        assert int(mask[1].sum()) == 0 and int(mask[0].sum()) > 0
        sc = torch.einsum("bsd,bod->bso", q.double(), k.double()) * E.PTR_SCALE - 10000.0 * (1 - mask.double())[:, None, :]
        assert torch.equal(sc.float().double(), sc)                     # scores with the literal -10000 added: exact in fp32
    dy, ids, base = E.scatter_case(777, 768, 97, 5)
    assert int((ids == 0).sum()) >= 77 and int((ids == 7).sum()) >= 200

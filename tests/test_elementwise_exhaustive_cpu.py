"""The judging side of the exhaustive element-wise tests (tests/test_elementwise_exhaustive_gpu.py), and the proof that it is neither
vacuous nor unsatisfiable.  No GPU.

The suite's tensor-wide bound (tests/util.py: 1e-3 * max|ref| + 1 ulp) at random Gaussian points lets two kinds of defect through:

  * the GELU family of csrc/common.h (gelu_erf, gelu_erf_and_grad, gelu_erf_grad: Abramowitz-Stegun 7.1.26 with hardware rcp / exp2).  A wrong digit
    in a coefficient, a wrong exponent constant or a sign slip in the negative tail gives errors of 1e-4 .. 1e-3: under 1e-3 * max|ref|.
  * fp32 -> bf16 store rounding (pack_bf16x2, documented RNE).  Random data never holds a tie (low half exactly 0x8000).

Here: every bf16 value as an input (all_finite_bf16), a PER-ELEMENT bound (gelu_bound), fp64 references through erfc, a numpy float32 emulation of the
kernels' arithmetic that must meet the bound everywhere (satisfiable), the same emulation with one defect at a time that must miss it while passing the
old bound on the Gaussian inputs of tests/test_gemm_gpu.py::test_forward_gelu_and_dropout_residual (not vacuous; the gap is real), and the fp32 tie
patterns (tie_patterns) with an integer-arithmetic RNE of their own.

What the bound sees best: 2^-8 * |ref| is a whole bf16 ulp of the result, so a defect whose error is a small fraction of the result shows where the
reference is small next to the error -- GELU's negative side, and above all GELU', which crosses zero at x = -0.7518 with a CDF defect at full size next
to a reference of ~0.  The mutant tests judge both planes that gelu_erf_and_grad produces, print both verdicts, and assert on GELU'."""
import functools
import math

import numpy as np
import torch

F32 = np.float32
TIE_LOW_HALVES = (0x0000, 0x0001, 0x7FFF, 0x8000, 0x8001, 0xFFFF)
GELU_FLOOR = 4e-7


# ----------------------------------------------------------------------------- inputs
def all_bf16_bits():
    """uint32 [256, 256]: element [m, n] = the bf16 bit pattern m * 256 + n in the high half of an fp32 word"""
    return (np.arange(65536, dtype=np.uint32) << 16).reshape(256, 256)


def all_finite_bf16():
    """fp32 [256, 256]: element [m, n] is the bf16 bit pattern m * 256 + n widened to fp32; the inf / NaN patterns are replaced by 0 (inf * 0 in an
    identity GEMM would poison their rows)"""
    v = all_bf16_bits().view(np.float32).copy()
    v[~np.isfinite(v)] = 0.0
    return v


def tie_patterns():
    """fp32 [393216]: every high half 0x0000 .. 0xFFFF with the low halves {0x0000, 0x0001, 0x7FFF, 0x8000, 0x8001, 0xFFFF}: exact values, exact ties (0x8000)
    under both parities of the kept bit, one fp32 step to either side of a tie, carries into the exponent, finite values that round to +-inf, infs, NaNs"""
    hi = np.arange(65536, dtype=np.uint32)[:, None] << 16
    lo = np.array(TIE_LOW_HALVES, dtype=np.uint32)[None, :]
    return (hi | lo).reshape(-1).view(np.float32).copy()


def rne_bf16_bits(x32):
    """uint16 bf16 bits of fp32 `x32`, round-to-nearest-even in integer arithmetic (independent of torch); NaN -> the quiet NaN 0x7FC0 | sign"""
    u = np.ascontiguousarray(x32, dtype=np.float32).view(np.uint32).astype(np.uint64)
    r = ((u + 0x7FFF + ((u >> 16) & 1)) >> 16).astype(np.uint32)
    nan = np.isnan(x32)
    r = np.where(nan, ((u >> 16) & 0x8000).astype(np.uint32) | 0x7FC0, r)
    return r.astype(np.uint16)


def half_up_bf16_bits(x32):
    """defect (d): round half UP in magnitude (add 0x8000, truncate) instead of to even"""
    u = np.ascontiguousarray(x32, dtype=np.float32).view(np.uint32).astype(np.uint64)
    return ((u + 0x8000) >> 16).astype(np.uint16)


def torch_bf16_bits(x32):
    """uint16 bits of torch.Tensor.to(bfloat16) on the CPU: the reference the GPU tests compare with"""
    t = torch.from_numpy(np.ascontiguousarray(x32, dtype=np.float32)).to(torch.bfloat16)
    return t.view(torch.int16).numpy().view(np.uint16)


def bf16_bits_to_f64(b16):
    return (b16.astype(np.uint32) << 16).view(np.float32).astype(np.float64)


# ----------------------------------------------------------------------------- references and the bound
def gelu_ref(x):
    """fp64 GELU through erfc (1 + erf loses the negative tail): 0.5 * x * erfc(-x / sqrt 2)"""
    xt = torch.from_numpy(np.ascontiguousarray(x, dtype=np.float64))
    return (0.5 * xt * torch.special.erfc(-xt / math.sqrt(2.0))).numpy()


def dgelu_ref(x):
    """fp64 GELU': 0.5 * erfc(-x / sqrt 2) + x * exp(-x^2 / 2) / sqrt(2 pi)"""
    xt = torch.from_numpy(np.ascontiguousarray(x, dtype=np.float64))
    return (0.5 * torch.special.erfc(-xt / math.sqrt(2.0)) + xt * torch.exp(-0.5 * xt * xt) / math.sqrt(2.0 * math.pi)).numpy()


def gelu_bound(x, ref, floor=GELU_FLOOR):
    """per element: 2^-8 * |ref| (the quantum of storing the result in bf16, as in tests/util.py) + floor * max(1, |x|) (A&S 7.1.26's 1.5e-7 on erf, times
    |x|, plus fp32 rounding and the 1-ulp hardware rcp / exp2).  No max|ref| term."""
    x = np.asarray(x, dtype=np.float64)
    return 2.0 ** -8 * np.abs(np.asarray(ref, dtype=np.float64)) + floor * np.maximum(1.0, np.abs(x))


def judge(got, x, ref, floor=GELU_FLOOR):
    """-> (number of elements over gelu_bound, worst err / bound, x at the worst)"""
    got, x, ref = (np.asarray(a, dtype=np.float64).reshape(-1) for a in (got, x, ref))
    with np.errstate(divide="ignore", invalid="ignore"):          # (floor = 0 and ref = 0: a zero bound; err 0 there counts as met)
        ratio = np.where(np.abs(got - ref) == 0, 0.0, np.abs(got - ref) / gelu_bound(x, ref, floor))
    ratio = np.where(np.isfinite(got), ratio, np.inf)
    k = int(np.argmax(ratio))
    return int((ratio > 1.0).sum()), float(ratio[k]), float(x[k])


def old_bound_ok(got, ref):
    """tests/util.py:assert_close_bf16 with its defaults, as a predicate: |got - ref| <= 1e-3 * max|ref| + 2^-8 * |ref| everywhere"""
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    return bool(np.isfinite(got).all() and (np.abs(got - ref) <= 1e-3 * np.abs(ref).max() + 2.0 ** -8 * np.abs(ref)).all())


# ----------------------------------------------------------------------------- the kernels' arithmetic in numpy float32
def _fma(a, b, c):
    """fmaf: the fp32 product is exact in fp64, so one fp64 add and one rounding to fp32 follow (a double rounding only in cases of measure ~2^-29)"""
    return (np.asarray(a, dtype=np.float64) * np.asarray(b, dtype=np.float64) + np.float64(c)).astype(F32)


def _step(a, n):
    """a moved by n fp32 ulps (n in -1, 0, 1)"""
    return a if n == 0 else np.nextafter(a, F32(np.inf if n > 0 else -np.inf), dtype=F32)


def emulate(x, c3=1.421413741, kexp=0.72134752044448170, flip_tail_below=None, rcp_ulp=0, exp_ulp=0):
    """csrc/common.h gelu_phi_and_cdf / gelu_erf_and_grad, operation for operation in float32 -> (gelu fp32, gelu' fp32).
    Defects: c3 (the polynomial's third coefficient), kexp (log2(e) / 2 of the exponential), flip_tail_below (GELU' with the Gaussian term's sign
    flipped for x below that value); rcp_ulp / exp_ulp move the two hardware functions' results by that many fp32 ulps."""
    x = np.ascontiguousarray(x, dtype=F32)
    with np.errstate(over="ignore", under="ignore", invalid="ignore"):
        z = np.abs(x) * F32(0.70710678118654752)
        t = _step(F32(1.0) / _fma(z, F32(0.3275911), F32(1.0)), rcp_ulp)
        e = _step(np.exp2(((F32(-kexp) * x) * x).astype(np.float64)).astype(F32), exp_ulp)
        poly = _fma(t, F32(1.061405429), F32(-1.453152027))
        poly = _fma(poly, t, F32(c3))
        poly = _fma(poly, t, F32(-0.284496736))
        poly = _fma(poly, t, F32(0.254829592))
        erf_abs = F32(1.0) - (poly * t) * e
        cdf = F32(0.5) + F32(0.5) * np.copysign(erf_abs, x)
        gauss = (x * F32(0.39894228040143268)) * e
        if flip_tail_below is not None:
            gauss = np.where(x < F32(flip_tail_below), -gauss, gauss)
        return (x * cdf).astype(F32), (cdf + gauss).astype(F32)


def to_bf16_f64(a32):
    """fp32 -> bf16 (RNE) -> fp64: what a kernel's bf16 store leaves"""
    return bf16_bits_to_f64(rne_bf16_bits(a32))


@functools.lru_cache(maxsize=None)
def finite_inputs():
    """every finite bf16 value once (65280 of them), fp32"""
    v = all_bf16_bits().view(np.float32).reshape(-1)
    return v[np.isfinite(v)].copy()


@functools.lru_cache(maxsize=None)
def finite_refs():
    x = finite_inputs().astype(np.float64)
    return gelu_ref(x), dgelu_ref(x)


@functools.lru_cache(maxsize=None)
def gaussian_case():
    """the pre-activation of tests/test_gemm_gpu.py::test_forward_gelu_and_dropout_residual (same seeds, same shapes) and its fp64 GELU / GELU'"""
    from tests.test_gemm_gpu import rnd
    M, N, K = 728, 3072, 768
    x, w = rnd((M, K), 4), rnd((N, K), 5, 0.05)
    b = torch.randn(N, generator=torch.Generator().manual_seed(6)) * 0.1
    pre = (x.float() @ w.float().t() + b).numpy().reshape(-1)
    p64 = pre.astype(np.float64)
    return pre, gelu_ref(p64), dgelu_ref(p64)


def _planes(**defect):
    """(err-judgement of the GELU plane, of the GELU' plane) of the emulation on every finite bf16 input"""
    x = finite_inputs()
    rg, rd = finite_refs()
    g, d = emulate(x, **defect)
    return judge(to_bf16_f64(g), x, rg), judge(to_bf16_f64(d), x, rd)


def _passes_old_bound_on_gaussian(**defect):
    pre, rg, rd = gaussian_case()
    g, d = emulate(pre, **defect)
    return old_bound_ok(to_bf16_f64(g), rg), old_bound_ok(to_bf16_f64(d), rd)


# ----------------------------------------------------------------------------- tests
def test_input_sets_are_what_they_say():
    v = all_finite_bf16()
    bits = all_bf16_bits()
    assert v.shape == (256, 256) and v.dtype == np.float32 and np.isfinite(v).all()
    assert v[0x3F, 0x80] == 1.0 and v[0xC0, 0x00] == -2.0 and v[0x41, 0x80] == 16.0       # [m, n] = pattern m * 256 + n
    nonfinite = ((bits >> 23) & 0xFF) == 0xFF
    assert int(nonfinite.sum()) == 256 and (v[nonfinite] == 0).all()                      # 2 infs + 254 NaNs
    assert (v.view(np.uint32)[~nonfinite] == bits[~nonfinite]).all()                      # everything else bit for bit, -0 and subnormals included
    assert (v.view(np.uint32) & 0xFFFF == 0).all()                                        # exactly representable in bf16
    t = tie_patterns()
    u = t.view(np.uint32)
    assert t.shape == (393216,) and len(np.unique(u)) == 393216
    assert set(np.unique(u & 0xFFFF).tolist()) == set(TIE_LOW_HALVES) and (np.bincount(u >> 16, minlength=65536) == 6).all()
    # ties under both parities of the kept bit, a carry into the exponent, and a finite value that rounds to inf are all present
    for word in (0x3F808000, 0x3F818000, 0x3FFF8000, 0x7F7F8000, 0xFF7F8000, 0x00008000, 0x007F8000):
        assert word in u
    assert np.isfinite(np.array([0x7F7F8000], dtype=np.uint32).view(np.float32))[0]


def test_integer_rne_agrees_with_torch_on_every_tie_pattern():
    """the GPU tests compare with torch.Tensor.to(bfloat16) on the CPU: that reference is itself checked here against round-to-nearest-even written in
    integer arithmetic, on all 393216 patterns (NaNs: both must give a NaN)"""
    t = tie_patterns()
    mine, ref = rne_bf16_bits(t), torch_bf16_bits(t)
    nan = np.isnan(t)
    assert (mine[~nan] == ref[~nan]).all()
    for b in (mine[nan], ref[nan]):
        assert ((b & 0x7F80) == 0x7F80).all() and ((b & 0x007F) != 0).all()
    # spot values: tie to even down, tie to even up, carry into the exponent, finite -> inf, one step under a tie, one over
    words = np.array([0x3F808000, 0x3F818000, 0x3FFF8000, 0x7F7F8000, 0x3F807FFF, 0x3F808001], dtype=np.uint32)
    assert rne_bf16_bits(words.view(np.float32)).tolist() == [0x3F80, 0x3F82, 0x4000, 0x7F80, 0x3F80, 0x3F81]


def test_fp64_references_keep_the_negative_tail():
    x = np.array([-30.0, -10.0, -5.0, 0.0, 5.0])
    g, d = gelu_ref(x), dgelu_ref(x)
    assert g[0] < 0 and abs(g[0] / (-30.0 * 4.906713927148187e-198) - 1) < 1e-9          # -30 * Phi(-30); 1 + erf gives 0 here
    assert abs(g[1] / (-10.0 * 7.61985302416053e-24) - 1) < 1e-9
    assert abs(g[2] / (-5.0 * 2.866515718791939e-07) - 1) < 1e-9 and g[3] == 0 and d[3] == 0.5
    assert abs(d[2] - (2.866515718791939e-07 - 5.0 * 1.4867195147342979e-06)) < 1e-18
    assert abs(g[4] - 5.0 * (1 - 2.866515718791939e-07)) < 1e-12


def test_emulated_kernel_arithmetic_meets_the_bound_on_every_finite_bf16():
    """Satisfiable: the float32 emulation of common.h's GELU family, rounded to bf16, meets gelu_bound on all 65280 finite inputs with zero exceptions, in both
    planes, and the smallest floor that still passes is printed.  Measured before the bf16 store: GELU 4.4e-7 absolute at x = 3.27 (1.4e-7 per max(1, |x|));
    GELU' 2.4e-7 near x = 0, where 1 - poly * t * e cancels to erf ~ 0.  After the store the tightest element is x = 0.00244: GELU' = 0.50097 sits at the
    bottom of a binade, where half the bf16 spacing (2^-9) is all of 2^-8 * |ref| and only the floor is left for the arithmetic (err / bound 0.993).
    The same with the two hardware functions moved by +-1 fp32 ulp (rcp, exp2: the documented accuracy of v_rcp_f32 / v_exp_f32), all nine combinations:
    still zero exceptions; the largest fp32 err / max(1, |x|) is 3.72e-7 (GELU', rcp and exp2 both one ulp low, x = 0.0247), inside the 4e-7 floor.  Should
    the hardware alone ever push a correct implementation past the floor, that figure doubled (7.4e-7) is the floor the issue allows."""
    x = finite_inputs()
    rg, rd = finite_refs()
    g, d = emulate(x)
    for name, got, ref in (("gelu", g, rg), ("gelu'", d, rd)):
        assert np.isfinite(got).all()
        n_bad, worst, at = judge(to_bf16_f64(got), x, ref)
        floors = [f for f in (0.0, 2.5e-8, 5e-8, 1e-7, 2e-7, 4e-7) if judge(to_bf16_f64(got), x, ref, floor=f)[0] == 0]
        e32 = np.abs(got.astype(np.float64) - ref)
        k = int(e32.argmax())
        print("PARITY emulation %-5s: %d of %d over gelu_bound; worst err/bound %.3f at x=%.6g; smallest passing floor %.3g; fp32 max abs err %.3g at x=%.4g, max err/max(1,|x|) %.3g"
              % (name, n_bad, x.size, worst, at, min(floors), e32[k], x[k], (e32 / np.maximum(1.0, np.abs(x))).max()))
        assert n_bad == 0, (name, n_bad, worst, at)
    worst_scaled = 0.0
    for rcp_ulp in (-1, 0, 1):
        for exp_ulp in (-1, 0, 1):
            gp, dp = emulate(x, rcp_ulp=rcp_ulp, exp_ulp=exp_ulp)
            for got, ref in ((gp, rg), (dp, rd)):
                worst_scaled = max(worst_scaled, float((np.abs(got.astype(np.float64) - ref) / np.maximum(1.0, np.abs(x))).max()))
                assert judge(to_bf16_f64(got), x, ref)[0] == 0, (rcp_ulp, exp_ulp)
    print("PARITY emulation with rcp / exp2 moved by +-1 ulp: largest fp32 err/max(1,|x|) %.3g (floor %.3g)" % (worst_scaled, GELU_FLOOR))
    assert worst_scaled <= GELU_FLOOR


def test_emulation_meets_the_old_bound_on_the_gaussian_inputs_too():
    assert _passes_old_bound_on_gaussian() == (True, True)


def _mutant(name, expect_plane, **defect):
    (jg, jd) = _planes(**defect)
    old = _passes_old_bound_on_gaussian(**defect)
    print("PARITY mutant %-28s: gelu %d over (worst err/bound %.3g at x=%.5g), gelu' %d over (worst %.3g at x=%.5g); old bound on the Gaussian inputs passes: gelu %s gelu' %s"
          % (name, jg[0], jg[1], jg[2], jd[0], jd[1], jd[2], old[0], old[1]))
    assert old == (True, True), "the old bound already catches this defect: it demonstrates no gap"
    failing = {"gelu": jg, "gelu'": jd}[expect_plane]
    assert failing[0] > 0 and failing[1] > 1.0, "gelu_bound does not catch the defect"
    return jg, jd


def test_mutant_wrong_polynomial_coefficient_is_caught_only_by_the_new_bound():
    """(a) 1.421413741 -> 1.422413741: erf off by 1e-3 * t^3 * exp(-x^2/2), up to 2.4e-4 in the CDF.  Where GELU is large that is a fraction of its bf16 ulp, so
    the GELU plane stays inside the bound; GELU' crosses zero at x = -0.7518 with the error at full size."""
    _mutant("(a) coefficient 1.4214->1.4224", "gelu'", c3=1.422413741)


def test_mutant_wrong_exponent_constant_is_caught_only_by_the_new_bound():
    """(b) 0.72134752 -> 0.72034752 in exp2: exp(-x^2/2) off by 6.9e-4 * x^2 relative, in the erf complement and in GELU's Gaussian term (the two partly
    cancel in GELU' below zero, which is why this defect clears the bound by the smallest factor of the three)"""
    _mutant("(b) exponent 0.7213->0.7203", "gelu'", kexp=0.72034752044448170)


def test_mutant_sign_slip_in_the_negative_tail_is_caught_only_by_the_new_bound():
    """(c) GELU' with the Gaussian term's sign flipped in the negative tail, x < -4.5: an error of 2|x| phi(x) <= 1.4e-4 next to a reference of -7e-5.
    (Flipped for ALL x < 0 the error is 0.48 at x = -1, which the old bound catches as well: that form demonstrates no gap and was replaced by this one.)"""
    pre, _, _ = gaussian_case()
    assert (pre < -4.5).sum() >= 100          # the Gaussian inputs do exercise the defect; the old bound still passes
    wide = _passes_old_bound_on_gaussian(flip_tail_below=0.0)
    assert wide[1] is False
    jg, jd = _mutant("(c) gauss sign flipped x<-4.5", "gelu'", flip_tail_below=-4.5)
    assert jg[0] == 0          # the GELU plane does not use the Gaussian term


def test_mutant_round_half_up_differs_only_on_ties():
    """(d) bf16 store rounding half-up instead of to nearest even.  On 1e6 random normals it differs from torch.Tensor.to(bfloat16) ONLY where the draw happens to be
    an exact tie -- an fp32 normal's low half is 0x8000 with probability 2^-16, so a handful of the million are (13 here, 9 of them with an even kept bit); it
    is identical on every other element, and all million pass the suite's old bound (the difference is one bf16 ulp).  On the tie set it differs on
    exactly the ties whose kept bit is even: 32640 non-NaN patterns."""
    rnd = torch.randn(1000000, generator=torch.Generator().manual_seed(0)).numpy()
    ur = rnd.view(np.uint32)
    d_rnd = half_up_bf16_bits(rnd) != torch_bf16_bits(rnd)
    assert ((ur[d_rnd] & 0xFFFF) == 0x8000).all() and int(d_rnd.sum()) <= 40          # (40: > 6 sigma above the expected 2^-17 * 1e6 = 7.6)
    assert old_bound_ok(bf16_bits_to_f64(half_up_bf16_bits(rnd)), rnd.astype(np.float64))
    t = tie_patterns()
    ok = ~np.isnan(t)
    u = t.view(np.uint32)
    differs = half_up_bf16_bits(t) != torch_bf16_bits(t)
    expect = ok & ((u & 0xFFFF) == 0x8000) & (((u >> 16) & 1) == 0)
    assert (differs[ok] == expect[ok]).all() and int(differs[ok].sum()) == int(expect.sum()) == 32640
    print("PARITY mutant (d) round half up             : differs from RNE on %d of 1000000 random normals (all exact ties; old bound passes), on %d of %d tie patterns"
          % (int(d_rnd.sum()), int(differs[ok].sum()), int(ok.sum())))

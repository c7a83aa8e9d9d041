"""Exhaustive element-wise parity on the GPU: the GELU family on EVERY bf16 input through every GEMM epilogue that calls it, and round-to-nearest-even at
exact ties through every kind of bf16 store.  The judging function, the fp64 references and the input sets live in tests/test_elementwise_exhaustive_cpu.py,
which also shows that the bound can be met and that it catches what the suite's tensor-wide bound lets through.

A 256 x 256 x 256 GEMM of V (element [m, n] = bf16 pattern m * 256 + n; inf / NaN -> 0) against an identity weight reproduces every finite bf16 value exactly as a
pre-activation -- except that -0 arrives as +0 (the accumulator starts at +0 and (+0) + (-0 * 1) = +0 under round-to-nearest).  In the dgrad layout an
accumulator of exactly 1.0 everywhere (dy all ones, W's first row ones) multiplies the auxiliary plane, so DGELU returns GELU'(aux) and MUL_AUX returns
the plane itself bit for bit: a lo / hi or column mix-up in an epilogue's read of the packed plane moves values between neighbouring columns, which differ.

Families (each owns an epilogue): the 4-wave kernels (gemm.hip, 4-wide epilogue of gemm_common.h) at 64 x 64 and 128 x 128 tiles; the 8-wave kernels (gemm8.hip, 8-wide
epilogue) at 192 x 192 (ragged here: 256 = 192 + 64) and 256 x 256; the 8-wave 192 x 192 kernel with the deferred, LDS-staged epilogue of its own (force_tile 3192);
the 12-wave loader kernels (gemm12.hip); and the split-K reduction's epilogue (splitk_epilogue_kernel).  The 8- and 12-wave kernels have no EPI_BIAS_GELU and no
EPI_DGELU instance (gemm8.hip / gemm12.hip: "inference, old callers -> 4-wave kernels") and whole k-tiles only: there the test asserts that the library declines
those two epilogues, checks the pre-activation through EPI_BIAS, and runs the dgrad products with K = 64 instead of 8."""
import numpy as np
import pytest
import torch

from tests.test_elementwise_exhaustive_cpu import (all_finite_bf16, dgelu_ref, gelu_ref, judge, rne_bf16_bits, tie_patterns, torch_bf16_bits)

pytestmark = pytest.mark.gpu

BF16 = torch.bfloat16
# name, ops.gemm selector, has EPI_BIAS_GELU / EPI_DGELU instances, K of the dgrad products (the smallest the family accepts: K % 8 for the 4-wave kernels, whole
# 64-wide k-tiles for the 8- and 12-wave kernels, two k-tiles for a split in two)
FAMILIES = [
    ("4-wave 64x64", dict(force_tile=64), True, 8),
    ("4-wave 128x128", dict(force_tile=128), True, 8),
    ("8-wave 192x192", dict(force_tile=1192), False, 64),
    ("8-wave 256x256", dict(force_tile=1256), False, 64),
    ("8-wave 192x192 deferred epilogue", dict(force_tile=3192), False, 64),
    ("12-wave 192x192", dict(force_tile=12192), False, 64),
    ("split-K epilogue", dict(split_k=2), True, 128),
]
IDS = [f[0].replace(" ", "_") for f in FAMILIES]


def _mods():
    from sam_textvqa_amd import _capi, ops
    return ops, _capi


def _bf16_from_bits(bits16):
    return torch.from_numpy(np.ascontiguousarray(bits16, dtype=np.uint16).view(np.int16)).view(BF16)


def _bits(t):
    """uint16 numpy bits of a bf16 tensor (any device)"""
    return t.detach().cpu().contiguous().view(torch.int16).numpy().view(np.uint16)


def _gemm(sel, *a, **kw):
    """ops.gemm on one kernel family, failing loudly when the family was not the one that ran.  force_tile >= 1000 is an error inside the library when the 8- / 12-wave
    kernels have no instance (gemm.hip: launch()); force_tile 64 / 128 select the 4-wave tile directly; a split that the library declined (split_k_used != 2) would
    silently run the plain 4-wave kernel, so the descriptor is read back."""
    ops, capi = _mods()
    seen, real = [], capi.call

    def spy(name, *args, **k2):
        if name == "sam_gemm_bf16":
            seen.append(args[0])
        return real(name, *args, **k2)
    capi.call = spy
    try:
        out = ops.gemm(*a, **sel, **kw)
    finally:
        capi.call = real
    if sel.get("split_k"):
        assert seen and seen[0].split_k_used == sel["split_k"], "the split-K epilogue kernel was not reached: split_k_used = %s" % (seen[0].split_k_used if seen else None)
    return out


class _Case:
    """inputs and fp64 references, built once for the module and never written to"""

    def __init__(self):
        v32 = all_finite_bf16()
        self.v_bits = (v32.view(np.uint32) >> 16).astype(np.uint16)                       # [256, 256], -0 and subnormals included
        self.v = _bf16_from_bits(self.v_bits).cuda()
        self.eye = torch.eye(256, dtype=BF16, device="cuda")
        self.zero_bias = torch.zeros(256, device="cuda")
        self.pre_bits = np.where(self.v_bits == 0x8000, 0, self.v_bits).astype(np.uint16)    # what the identity GEMM leaves: -0 -> +0
        self.x_pre = (self.pre_bits.astype(np.uint32) << 16).view(np.float32).astype(np.float64)
        self.x_aux = v32.astype(np.float64)
        self.gelu_pre, self.dgelu_pre = gelu_ref(self.x_pre), dgelu_ref(self.x_pre)
        self.dgelu_aux = dgelu_ref(self.x_aux)
        self.dplane_bits = rne_bf16_bits(self.dgelu_aux.astype(np.float32))               # a stored bf16 GELU' plane (MUL_AUX's operand)
        self.dplane = _bf16_from_bits(self.dplane_bits).cuda()
        assert np.isfinite(self.gelu_pre).all() and np.isfinite(self.dgelu_pre).all() and np.isfinite(self.dgelu_aux).all()


_CASE = []


def _case():
    if not _CASE:
        _CASE.append(_Case())
    return _CASE[0]


def _dgrad_operands(k):
    """dy [256, k] all ones, W [k, 256] with its first row ones and the rest zero: every accumulator is exactly 1.0, in any order of summation"""
    dy = torch.ones(256, k, dtype=BF16, device="cuda")
    w = torch.zeros(k, 256, dtype=BF16, device="cuda")
    w[0] = 1
    return dy, w


def _check_plane(tag, got, x, ref, is_grad):
    """gelu_bound on every element, nothing non-finite, and the exact limits: |x| >= 16 gives x (GELU) / 1 (GELU') above and (+-)0 below; GELU(+0) is +0"""
    g = got.float().cpu().numpy().astype(np.float64)
    gb = _bits(got)
    assert np.isfinite(g).all(), "%s: %d non-finite outputs, first at x=%r" % (tag, int((~np.isfinite(g)).sum()), x[~np.isfinite(g)][:4])
    n_bad, worst, at = judge(g, x, ref)
    print("PARITY %-58s: %5d of %d over gelu_bound; worst err/bound %.3f at x=%.6g" % (tag, n_bad, g.size, worst, at))
    assert n_bad == 0, "%s: %d elements over gelu_bound, worst err/bound %.3f at x=%.6g" % (tag, n_bad, worst, at)
    hi, lo = x >= 16.0, x <= -16.0
    assert hi.sum() > 14000 and lo.sum() > 14000
    if is_grad:
        assert (g[hi] == 1.0).all(), "%s: GELU' must be exactly 1 for x >= 16" % tag
        assert (g[lo] == 0.0).all(), "%s: GELU' must be exactly 0 for x <= -16" % tag
    else:
        assert (g[hi] == x[hi]).all(), "%s: GELU(x) must be exactly x for x >= 16" % tag
        assert (g[lo] == 0.0).all(), "%s: GELU(x) must be (+-)0 for x <= -16" % tag
        pz = (x == 0) & ~np.signbit(x)
        assert pz.sum() >= 1 and (gb[pz] == 0).all(), "%s: GELU(+0) must be +0" % tag


@pytest.mark.parametrize("name,sel,has_plain,kd", FAMILIES, ids=IDS)
def test_gelu_family_on_every_finite_bf16(name, sel, has_plain, kd):
    ops, capi = _mods()
    c = _case()
    # the pre-activation is V, bit for bit (-0 -> +0): through EPI_BIAS_GELU's aux_out where the family has that epilogue, through EPI_BIAS where it has not
    if has_plain:
        pre = torch.empty(256, 256, dtype=BF16, device="cuda")
        h = _gemm(sel, c.v, c.eye, epilogue=capi.EPI_BIAS_GELU, bias=c.zero_bias, aux_out=pre)
    else:
        with pytest.raises(capi.SamHipError):
            _gemm(sel, c.v, c.eye, epilogue=capi.EPI_BIAS_GELU, bias=c.zero_bias, aux_out=torch.empty(256, 256, dtype=BF16, device="cuda"))
        pre, h = _gemm(sel, c.v, c.eye, epilogue=capi.EPI_BIAS, bias=c.zero_bias), None
    diff = _bits(pre) != c.pre_bits
    assert not diff.any(), "%s: pre-activation differs from V at %d patterns, first 0x%04x -> 0x%04x" % (name, int(diff.sum()), int(c.v_bits[diff][0]), int(_bits(pre)[diff][0]))
    if h is not None:
        _check_plane("%s BIAS_GELU out" % name, h, c.x_pre, c.gelu_pre, False)
    # training form: activation and derivative from one exponential
    dact = torch.empty(256, 256, dtype=BF16, device="cuda")
    h2 = _gemm(sel, c.v, c.eye, epilogue=capi.EPI_BIAS_GELU_GRAD, bias=c.zero_bias, aux_out=dact)
    _check_plane("%s BIAS_GELU_GRAD out" % name, h2, c.x_pre, c.gelu_pre, False)
    _check_plane("%s BIAS_GELU_GRAD aux_out" % name, dact, c.x_pre, c.dgelu_pre, True)
    # dgrad layout, accumulator exactly 1.0
    dy, w = _dgrad_operands(kd)
    one = _gemm(sel, dy, w, b_kcontig=False)
    assert (_bits(one) == 0x3F80).all(), "%s: the all-ones dgrad product is not exactly 1.0" % name
    if has_plain:
        dg = _gemm(sel, dy, w, b_kcontig=False, epilogue=capi.EPI_DGELU, aux_in=c.v)
        _check_plane("%s DGELU (1.0 * gelu'(V))" % name, dg, c.x_aux, c.dgelu_aux, True)
    else:
        with pytest.raises(capi.SamHipError):
            _gemm(sel, dy, w, b_kcontig=False, epilogue=capi.EPI_DGELU, aux_in=c.v)
    # MUL_AUX: 1.0 * a is exact, so the stored GELU' plane comes back bit for bit -- and so does V itself (every element distinct, -0 and subnormals included)
    for what, plane, bits in (("gelu' plane", c.dplane, c.dplane_bits), ("V", c.v, c.v_bits)):
        got = _bits(_gemm(sel, dy, w, b_kcontig=False, epilogue=capi.EPI_MUL_AUX, aux_in=plane))
        bad = got != bits
        print("PARITY %-58s: %5d of %d differ from the plane" % ("%s MUL_AUX (1.0 * %s)" % (name, what), int(bad.sum()), bad.size))
        assert not bad.any(), "%s: MUL_AUX of %s differs at %d elements, first [%d, %d]: 0x%04x -> 0x%04x" % (
            (name, what, int(bad.sum())) + tuple(int(i) for i in np.argwhere(bad)[0]) + (int(bits[bad][0]), int(got[bad][0])))


# ----------------------------------------------------------------------------- round to nearest even at ties
def _assert_rne(tag, got_bits, x32):
    """bit-identical to torch.Tensor.to(bfloat16) on the CPU for every non-NaN input, NaN wherever the input is NaN"""
    x32 = np.ascontiguousarray(x32, dtype=np.float32).reshape(-1)
    got_bits = got_bits.reshape(-1)
    ref, nan = torch_bf16_bits(x32), np.isnan(x32)
    bad = (got_bits != ref) & ~nan
    got_nan = ((got_bits & 0x7F80) == 0x7F80) & ((got_bits & 0x007F) != 0)
    ties = int((((x32.view(np.uint32) & 0xFFFF) == 0x8000) & ~nan).sum())
    print("PARITY %-58s: %5d of %d differ from RNE (%d exact ties among them); %d of %d NaN inputs not NaN" % (tag, int(bad.sum()), int((~nan).sum()), ties, int((nan & ~got_nan).sum()), int(nan.sum())))
    assert not bad.any(), "%s: %d results differ from RNE, first 0x%08x -> 0x%04x (RNE 0x%04x)" % (tag, int(bad.sum()), int(x32.view(np.uint32)[bad][0]), int(got_bits[bad][0]), int(ref[bad][0]))
    assert (got_nan == nan).all(), "%s: NaN in, NaN out (and only then)" % tag


def test_cast_bf16_rounds_to_nearest_even_on_every_tie_pattern():
    """sam_cast_f32_to_bf16 (the bf16 shadow of the flat parameter buffer): all 393216 tie patterns; the same patterns repeated past the 4096-block grid cap with a
    length that is a multiple of neither the block nor the grid stride, so some threads take a second trip; a length of 4; nothing written past n; and
    n % 4 != 0 is rejected by the library (cast_bf16_kernel takes n / 4)."""
    ops, capi = _mods()
    t = tie_patterns()
    assert t.size % 4 == 0
    y = torch.empty(t.size, dtype=BF16, device="cuda")
    ops.cast_bf16(torch.from_numpy(t).cuda(), y)
    _assert_rne("cast_bf16 tie patterns", _bits(y), t)
    long = np.concatenate([t] * 11 + [t[32768 * 6 + 3:32768 * 6 + 7]])          # 4325380 elements = 1081345 float4: > 4096 * 256, odd
    assert long.size // 4 > 4096 * 256 and (long.size // 4) % 256 != 0
    guard = torch.full((long.size + 16,), 7.0, dtype=BF16, device="cuda")
    ops.cast_bf16(torch.from_numpy(long).cuda(), guard[:long.size])
    _assert_rne("cast_bf16 grid-stride length %d" % long.size, _bits(guard[:long.size]), long)
    assert (_bits(guard[long.size:]) == 0x40E0).all(), "cast_bf16 wrote past n"
    four = np.array([0x3F808000, 0x3F818000, 0x7F7F8000, 0xBFFF8000], dtype=np.uint32).view(np.float32)
    guard = torch.full((20,), 7.0, dtype=BF16, device="cuda")
    ops.cast_bf16(torch.from_numpy(four).cuda(), guard[:4])
    assert _bits(guard[:4]).tolist() == [0x3F80, 0x3F82, 0x7F80, 0xC000] and (_bits(guard[4:]) == 0x40E0).all()
    for n in (5, 6, 7, 1):
        with pytest.raises(capi.SamHipError):
            ops.cast_bf16(torch.zeros(n, device="cuda"), torch.empty(8, dtype=BF16, device="cuda"))


def test_adam_shadow_rounds_to_nearest_even_and_a_zero_step_leaves_the_parameters():
    """sam_adam_step with both learning rates 0 on every finite tie pattern, a random finite gradient, m = v = 0: the parameters come back bit for bit and the bf16
    shadow is RNE(p).  One pattern is an exception by IEEE arithmetic, not by the kernel: p = -0 with a negative gradient.  The update is p - (0 / bc1) * (m / denom)
    = (-0) - (-0) = +0, as it is in torch.optim.Adam (addcdiv_ with a zero step).  The reference is therefore p - copysign(0, g), computed on the CPU; the test
    asserts that it equals p everywhere else."""
    ops, capi = _mods()
    t = tie_patterns()
    p0 = t[np.isfinite(t)]
    n = p0.size
    assert n == 391680 and n % 4 == 0
    g0 = torch.randn(n, generator=torch.Generator().manual_seed(7))
    assert torch.isfinite(g0).all() and (g0 != 0).all()
    p_ref = (torch.from_numpy(p0) - torch.copysign(torch.zeros(n), g0)).numpy()
    moved = p_ref.view(np.uint32) != p0.view(np.uint32)
    assert int(moved.sum()) <= 1 and (p0.view(np.uint32)[moved] == 0x80000000).all()
    p, g = torch.from_numpy(p0).cuda(), g0.cuda()
    m, v = torch.zeros(n, device="cuda"), torch.zeros(n, device="cuda")
    pb = torch.full((n,), 7.0, dtype=BF16, device="cuda")
    n1 = (n // 3) // 4 * 4
    ops.adam_step(p, g, m, v, pb, [n1, n], [0.0, 0.0], 1)
    got = p.cpu().numpy()
    bad = got.view(np.uint32) != p_ref.view(np.uint32)
    print("PARITY %-58s: %5d of %d parameters changed by a zero step" % ("adam_step lr=0 p", int(bad.sum()), n))
    assert not bad.any(), "adam_step with lr = 0 changed %d parameters, first 0x%08x -> 0x%08x" % (int(bad.sum()), int(p_ref.view(np.uint32)[bad][0]), int(got.view(np.uint32)[bad][0]))
    _assert_rne("adam_step bf16 shadow", _bits(pb), p_ref)
    same = ~moved
    assert (_bits(pb)[same] == torch_bf16_bits(p0)[same]).all()
    assert torch.isfinite(m).all() and torch.isfinite(v).all()


def _tie_rows():
    """per row m: h (a bf16 value: mantissa m & 127 -- both parities of the kept bit, 0x7F carries into the exponent -- at biased exponent 127 or 254, where the
    carry reaches inf), half an ulp of it, and one fp32 ulp of it -- three bf16 values"""
    m = np.arange(256)
    e = np.where(m < 128, 127, 254)
    h = ((e << 7) | (m & 127)).astype(np.uint16)
    half = ((e - 8) << 7).astype(np.uint16)
    step = ((e - 23) << 7).astype(np.uint16)
    return e, h, half, step


def _tie_gemm_operands(k):
    """A [256, k], W [256, k] (forward layout): out[m, n] = s_n * (h_m + half_m + c_n * step_m), s in {+1, -1}, c in {0, +1, -1}: an exact tie and one fp32 step to
    either side of it, 24 significant bits at the most, every partial sum exactly representable in fp32"""
    _, h, half, step = _tie_rows()
    a = np.zeros((256, k), dtype=np.uint16)
    a[:, 0], a[:, 1], a[:, 2] = h, half, step
    n = np.arange(256)
    s, c = np.where(n % 2 == 0, 1.0, -1.0), np.array([0.0, 1.0, -1.0])[(n // 2) % 3]
    w = torch.zeros(256, k)
    w[:, 0] = w[:, 1] = torch.from_numpy(s).float()
    w[:, 2] = torch.from_numpy(s * c).float()
    return _bf16_from_bits(a), w.to(BF16)


@pytest.mark.parametrize("name,sel,k", [("4-wave 128x128", dict(force_tile=128), 8), ("8-wave 256x256", dict(force_tile=1256), 64)], ids=["4-wave", "8-wave"])
def test_gemm_store_rounds_to_nearest_even_at_ties(name, sel, k):
    """K = 8 operands (zero-padded to one whole k-tile of 64 for the 8-wave kernel, which takes nothing less) whose sum is exact in fp32 and is a tie, or one fp32 step
    beside one.  fp32 sums in both orders and the fp64 sum agree on the CPU, so the order of accumulation cannot matter; the bf16 output must be RNE(sum)."""
    a, w = _tie_gemm_operands(k)
    a64, w64 = a.double(), w.double()
    s64 = a64 @ w64.t()
    fwd, rev = torch.zeros(256, 256), torch.zeros(256, 256)
    for j in range(k):
        fwd = fwd + a[:, j].float()[:, None] * w[:, j].float()[None, :]
        rev = rev + a[:, k - 1 - j].float()[:, None] * w[:, k - 1 - j].float()[None, :]
    s32 = a.float() @ w.float().t()
    assert torch.equal(fwd.double(), s64) and torch.equal(rev.double(), s64) and torch.equal(s32.double(), s64) and torch.isfinite(s32).all()
    low = s32.numpy().view(np.uint32) & 0xFFFF
    assert set(np.unique(low).tolist()) == {0x7FFF, 0x8000, 0x8001} and int((low == 0x8000).sum()) > 20000
    out = _gemm(sel, a.cuda(), w.cuda())
    _assert_rne("gemm store %s (K=%d)" % (name, k), _bits(out), s32.numpy())
    assert int((_bits(out) & 0x7FFF == 0x7F80).sum()) > 0          # the finite sums past the last tie did reach +-inf


def test_add_dropout_sum_rounds_to_nearest_even_at_ties():
    """sam_add_dropout_bf16 with p = 0: a = +-h, b = +-(half an ulp of h, or its bf16 neighbour above or below): a + b is exact in fp32 and is a tie or beside one"""
    ops, capi = _mods()
    e, h, half, _ = _tie_rows()
    n = np.arange(256)
    sign = np.where(n % 2 == 0, 0, 0x8000).astype(np.uint16)
    kind = (n // 2) % 3
    a_bits = h[:, None] | sign[None, :]
    b_mag = np.where(kind[None, :] == 0, half[:, None], np.where(kind[None, :] == 1, half[:, None] | 1, (((e - 9) << 7) | 0x7F).astype(np.uint16)[:, None]))
    b_bits = (b_mag | sign[None, :]).astype(np.uint16)
    a, b = _bf16_from_bits(a_bits), _bf16_from_bits(b_bits)
    s32 = a.float() + b.float()
    assert torch.equal(s32.double(), a.double() + b.double()) and torch.isfinite(s32).all()
    low = s32.numpy().view(np.uint32) & 0xFFFF
    assert set(np.unique(low).tolist()) == {0x7F80, 0x8000, 0x8100}
    out = ops.add_dropout(a.cuda(), b.cuda(), 0.0)
    _assert_rne("add_dropout p=0 (a + b)", _bits(out), s32.numpy())

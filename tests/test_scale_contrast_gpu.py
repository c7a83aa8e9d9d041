"""GPU parity under scale contrast: rows, heads and samples of ONE problem at magnitudes 2^-24 .. 2^24 apart, every slice judged against its own scale
(tests/util.py: assert_close_bf16_sliced) and, where the scales are powers of two, bit for bit against the uniform run.  The GEMM family and the attention
kernels; inputs, the fairness of the bounds and the fp16 emulation behind the row-contrast bound are in tests/test_scale_contrast_cpu.py."""
import pytest
import torch

from tests import test_scale_contrast_cpu as S
from tests.util import assert_close_bf16_sliced, unpack_bits

pytestmark = pytest.mark.gpu

H, HD = S.H, S.HD


def _mods():
    from sam_textvqa_amd import _capi, ops
    return ops, _capi


def _shifted(c, k, dim=0):
    """c * 2^k along `dim`, exactly (fp64 holds every bf16 / fp32 value and the shift)"""
    shape = [1] * c.dim()
    shape[dim] = -1
    return c.double() * S.pow2(k, c.device).view(shape)


def _assert_shifted(con, plain, k, name):
    """con == plain * 2^k[row], bit for bit; the message says how many elements differ, where, by how much, and how many of them hold the UNSHIFTED plain value"""
    want = _shifted(plain, k)
    bad = con.double() != want
    if bad.any():
        r, c = bad.nonzero(as_tuple=True)
        rel = ((con.double() - want).abs() / want.abs().clamp_min(1e-300))[bad]
        stale = (con.double() == plain.double())[bad].float().mean().item()
        raise AssertionError("%s: %d of %d elements are not the plain run's times 2^k: rows %d..%d (%d distinct), columns %d..%d (%d distinct), relative difference %.3g .. %.3g, "
                             "%.0f %% of them equal to the plain run's unshifted value; exponents of the rows involved: %s"
                             % (name, int(bad.sum()), bad.numel(), int(r.min()), int(r.max()), r.unique().numel(), int(c.min()), int(c.max()), c.unique().numel(),
                                rel.min().item(), rel.max().item(), 100 * stale, sorted(set(k.to(r.device)[r.unique()].tolist()))))


# ------------------------------------------------------------------------------------------------ GEMM family
_GEMM = {}


def _gemm_case(K):
    """operands on the device, contrast copies, fp64 references of the contrast products (computed once per K)"""
    if K not in _GEMM:
        o = {k: v.cuda() for k, v in S.gemm_operands(K).items()}
        o["xs"] = S.scale_rows(o["x"], o["k"])
        o["ref_fwd"] = o["xs"].double() @ o["w"].double().t()
        o["ref_dgrad"] = o["xs"].double() @ o["wt"].double()
        _GEMM[K] = o
    return _GEMM[K]


FOUR_WAVE = (64, 128, 160, 192, 256)
EIGHT_WAVE = (1192, 1256, 1448, 1128, 3192, 12192, 12448)


@pytest.mark.parametrize("tile,split", [(t, 0) for t in FOUR_WAVE + EIGHT_WAVE] + [(0, 3)])
def test_gemm_rows_at_contrasting_scales(tile, split):
    """forward and dgrad layouts, (M, N, K) = (600, 520, 192) -- K = 712 on the 4-wave kernels, which take partial k-tiles -- with row i of A times 2^k_i,
    k_i in {-24, -12, 0, 12, 24}: (a) row i of C is the plain run's row i times 2^k_i, bit for bit (nothing in a tile may depend on a neighbour row's magnitude);
    (b) every row of C within 1e-3 of ITS OWN maximum (+ one bf16 ulp for bf16 outputs) of the fp64 product.  Every kernel of the family through force_tile;
    split = 3: the 64 x 64 split-K kernel with the epilogue in the reduction pass."""
    ops, capi = _mods()
    o = _gemm_case(S.GEMM_K_4WAVE if tile in FOUR_WAVE else S.GEMM_MNK[2])
    kw = dict(force_tile=tile, split_k=split)
    runs = [("fwd none", dict(b="w"), "ref_fwd", 1),
            ("fwd none f32", dict(b="w", out_dtype=torch.float32), "ref_fwd", 0),
            ("fwd dropout(0)+res(none)", dict(b="w", epilogue=capi.EPI_BIAS_DROPOUT_RES), "ref_fwd", 1),
            ("dgrad none", dict(b="wt", b_kcontig=False), "ref_dgrad", 1),
            ("dgrad * aux", dict(b="wt", b_kcontig=False, epilogue=capi.EPI_MUL_AUX, aux_in=o["aux"]), None, 1)]
    if tile in EIGHT_WAVE:
        runs.pop(1)                         # the 8-wave and loader-wave kernels store bf16 only
    for name, args, ref, ulps in runs:
        args = dict(args)
        b = o[args.pop("b")]
        plain = ops.gemm(o["x"], b, **args, **kw)
        con = ops.gemm(o["xs"], b, **args, **kw)
        _assert_shifted(con, plain, o["k"], "%s tile %d split %d" % (name, tile, split))
        r = o[ref] if ref else o["ref_dgrad"] * o["aux"].double()
        assert_close_bf16_sliced(con, r, (1,), ulps=ulps, name="%s tile %d split %d" % (name, tile, split))


@pytest.mark.parametrize("tile", FOUR_WAVE)
@pytest.mark.parametrize("form", ["unsplit", "split accumulate", "split store"])
def test_wgrad_columns_at_contrasting_scales(tile, form):
    """wgrad layout, R = 1000, M = 520, N = 264: column m of dy times 2^k_m -> row m of dW and bias_grad[m] are the plain run's times 2^k_m bit for bit (the
    contraction over R is untouched) and within 1e-3 of their own scale of the fp64 product; un-split, split-K accumulated into C by the reduction launch (with the
    fused bias gradient) and split-K in the store form"""
    ops, capi = _mods()
    w = {k: v.cuda() for k, v in S.wgrad_operands().items()}
    dys = S.scale_rows(w["dy"].t().contiguous(), w["k"]).t().contiguous()
    M, N = S.WGRAD_RMN[1:]
    outs = []
    for dy in (w["dy"], dys):
        dw, db = torch.zeros(M, N, device="cuda"), torch.zeros(M, device="cuda")
        if form == "unsplit":
            ops.gemm(dy, w["x"], a_kcontig=False, b_kcontig=False, out=dw, accumulate=True, force_tile=tile)
            db = None
        elif form == "split accumulate":
            ops.gemm(dy, w["x"], a_kcontig=False, b_kcontig=False, out=dw, accumulate=True, split_k=4, bias_grad=db, force_tile=tile)
        else:
            dw.fill_(7.5)
            ops.gemm(dy, w["x"], a_kcontig=False, b_kcontig=False, out=dw, accumulate=False, split_k=4, force_tile=tile)
            db = None
        outs.append((dw, db))
    (pw, pb), (cw, cb) = outs
    _assert_shifted(cw, pw, w["k"], "wgrad %s tile %d" % (form, tile))
    assert_close_bf16_sliced(cw, dys.double().t() @ w["x"].double(), (1,), ulps=0, name="wgrad %s tile %d" % (form, tile))
    if cb is not None:
        _assert_shifted(cb[:, None], pb[:, None], w["k"], "bias grad %s tile %d" % (form, tile))
        assert_close_bf16_sliced(cb[:, None], dys.double().sum(0)[:, None], (1,), ulps=0, name="bias grad %s tile %d" % (form, tile))


LAYER_PAIR = [(768, 3072), (3072, 768), (768, 768), (2304, 768)] * 2


@pytest.mark.parametrize("force,R,shapes,bias", [(128, 512, [(200, 328), (520, 264)], (0,)), (1256, 512, [(200, 328), (520, 264)], (0,)), (12448, 1024, LAYER_PAIR, (0, 1, 3, 5, 6))])
def test_grouped_wgrad_columns_at_contrasting_scales(force, R, shapes, bias):
    """the grouped weight gradient in its three forms: the 4-wave kernel, the 8-wave kernel with the pair exchange through the workspace (the smallest ragged
    set of test_grouped_wgrad_eight_wave_ragged_and_unsplit) and the loader-wave kernel -- which declines sets with fewer deep tiles than CUs, so its set is the
    smallest it takes: a layer pair at R = 1024 (256 whole tiles + 32 tiles summed from 8 slices inside the launch).  Same two assertions as the single wgrad."""
    ops, capi = _mods()
    jobs = {"plain": [], "contrast": []}
    meta = []
    for j, (m, n) in enumerate(shapes):
        w = {k: v.cuda() for k, v in S.wgrad_operands(R, m, n, seed=10 * j).items()}
        dys = S.scale_rows(w["dy"].t().contiguous(), w["k"]).t().contiguous()
        for nm, dy in (("plain", w["dy"]), ("contrast", dys)):
            jobs[nm].append((dy, w["x"], torch.zeros(m, n, device="cuda"), torch.zeros(m, device="cuda") if j in bias else None))
        meta.append((w["k"], dys, w["x"]))
    ops.wgrad_grouped(jobs["plain"], force_tile=force)
    if force == 12448:
        # the kernels share one workspace per stream: an 8-wave launch of a small set in between leaves its accumulator halves where the loader-wave kernel keeps
        # its slice counters (it clears them itself since this test found it summing stale partials after such a launch)
        small = {k: v.cuda() for k, v in S.wgrad_operands(512, 200, 328).items()}
        ops.wgrad_grouped([(small["dy"], small["x"], torch.zeros(200, 328, device="cuda"), None)], force_tile=1256)
    ops.wgrad_grouped(jobs["contrast"], force_tile=force)
    if force != 128:
        ops.grouped_ws_check()
    for j, ((_, _, pw, pb), (_, _, cw, cb), (k, dys, x)) in enumerate(zip(jobs["plain"], jobs["contrast"], meta)):
        _assert_shifted(cw, pw, k, "grouped wgrad %d problem %d (%d x %d)" % (force, j, cw.shape[0], cw.shape[1]))
        assert_close_bf16_sliced(cw, dys.double().t() @ x.double(), (1,), ulps=0, name="grouped wgrad %d problem %d" % (force, j))
        if cb is not None:
            _assert_shifted(cb[:, None], pb[:, None], k, "grouped bias grad %d problem %d" % (force, j))
            assert_close_bf16_sliced(cb[:, None], dys.double().sum(0)[:, None], (1,), ulps=0, name="grouped bias grad %d problem %d" % (force, j))


# ------------------------------------------------------------------------------------------------ attention
_ATTN = {}


def _attn_case(case):
    if case not in _ATTN:
        ops, _ = _mods()
        pr, qkv, dout = S.attn_case(case)
        base = ops.mask_bits_prefix_lm(pr["key_valid"].to(torch.uint8).cuda(), pr["n_dec"])
        pr["bits"] = ops.mask_bits_spatial(base, pr["adj"].cuda(), pr["T"], H, (1, 2)) if pr["spatial"] else base
        _ATTN[case] = (pr, qkv, dout)
    return _ATTN[case]


def _run_pair(pr, qkv, dout, fused):
    """forward (dropout 0.1, fixed seed: the keep bits do not depend on the data) and backward on the device -> out, dqkv, keep [B, H, N, N] bool (host)"""
    ops, _ = _mods()
    B = pr["B"]
    q, d = qkv.cuda(), dout.cuda()
    if fused:
        out, lse2, keep_bits, out_lo = ops.attn_fwd(q, pr["bits"], B, H, 0.125, S.P_DROP, seed=1234, offset=7, want_residual=True)
        dqkv = ops.attn_bwd(d, q, lse2, pr["bits"], keep_bits, B, H, 0.125, S.P_DROP, out=out, out_lo=out_lo)
    else:
        out, lse2, keep_bits = ops.attn_fwd(q, pr["bits"], B, H, 0.125, S.P_DROP, seed=1234, offset=7)
        dqkv = ops.attn_bwd(d, q, lse2, pr["bits"], keep_bits, B, H, 0.125, S.P_DROP)
    return out, dqkv, unpack_bits(keep_bits, pr["N"])


@pytest.mark.parametrize("fused", [False, True], ids=["fwd+bwd", "fwd_train+bwd_fused"])
@pytest.mark.parametrize("case", S.ATTN_CASES)
def test_attention_heads_and_samples_at_contrasting_scales(case, fused):
    """q, k, v and dO of every (sample, head) at its own power of two (q * 2^k with k * 2^-k: the scores stay; v and dO freely; exponents -20, 0, 20, neighbouring
    heads and the two samples apart in each).  `out` per (sample, head) and dqkv per (part, sample, head) within 1e-3 of the slice's own maximum of the fp64
    oracle -- a block scale leaked from a neighbouring head would flush the 2^-20 heads to zero and pass the global bound -- and both bit-identical to the
    uniform run shifted per slice: every block scale is a per-(batch, head) power of two, every other factor is applied in fp32."""
    pr, qkv, dout = _attn_case(case)
    B, N = pr["B"], pr["N"]
    out0, g0, keep = _run_pair(pr, qkv, dout, fused)
    q1, d1 = S.apply_head_exponents(qkv, dout, B)
    out1, g1, keep1 = _run_pair(pr, q1, d1, fused)
    assert torch.equal(keep, keep1)
    ref_out, ref_g = S.oracle_pair(q1, d1, pr["allow"], keep, B)
    assert_close_bf16_sliced(out1.view(B, N, H, HD), ref_out.view(B, N, H, HD), (1, 3), name="out per (sample, head)")
    assert_close_bf16_sliced(g1.view(B, N, 3, H, HD), ref_g.view(B, N, 3, H, HD), (1, 4), name="dqkv per (part, sample, head)")
    assert torch.equal(out1.double().view(B, N, H, HD), out0.double().view(B, N, H, HD) * S.pow2(S.head_shift_of_out(B), "cuda"))
    assert torch.equal(g1.double().view(B, N, 3, H, HD), g0.double().view(B, N, 3, H, HD) * S.pow2(S.head_shift_of_dqkv(B), "cuda"))


@pytest.mark.parametrize("fused", [False, True], ids=["fwd+bwd", "fwd_train+bwd_fused"])
@pytest.mark.parametrize("case", S.ATTN_CASES)
def test_attention_rows_of_one_head_at_contrasting_scales(case, fused):
    """dO rows (tokens) at 2^0, 2^-4, 2^-10, 2^-16 of the head's largest and rows of exact zeros, interleaved.  dQ row i scales with dO row i, dK / dV are carried
    by the large rows.  Per (token, head) row of dQ with at least two allowed keys: within ROW_FRAC of the row's own maximum for the rows down to 2^-10 --
    ROW_FRAC = 2 x the host emulation's largest per-row error on these inputs (spatial57: E = 3.86e-2, bound 7.7e-2, a conditioning figure of its two- and
    three-key rows; pad200: E = 5.91e-4, bound 1.18e-3), 2^-10 the smallest row the emulation keeps inside it (at 2^-11 the fp16 image of dS goes subnormal:
    2.2e-3); rows at 2^-16 that the emulation (run here with the kernel's own keep bits) keeps non-zero are non-zero; zero dO rows give exactly zero dQ rows.
    dK, dV and the whole of dQ per (part, sample, head) at 1e-3, `out` (which never sees dO) bit-identical to the plain run's."""
    pr, qkv, dout = _attn_case(case)
    B, N = pr["B"], pr["N"]
    d1 = S.apply_row_exponents(dout, B)
    out1, g1, keep = _run_pair(pr, qkv, d1, fused)
    out0, _, _ = _run_pair(pr, qkv, dout, fused)
    assert torch.equal(out0, out1)
    ref_out, ref_g = S.oracle_pair(qkv, d1, pr["allow"], keep, B)
    k, zero, checked = S.row_exponents_of_tokens(N)
    got_q, ref_q = S.dq_rows(g1, B), S.dq_rows(ref_g, B)
    assert (got_q[:, zero] == 0).all(), "a zero dO row must give an exactly zero dQ row"
    sel = (S.rows_with_a_gradient(pr["allow"]) & checked[None, :, None]).cuda()
    masked_got = torch.where(sel[..., None], got_q.double(), torch.zeros_like(got_q, dtype=torch.float64))
    masked_ref = torch.where(sel[..., None].cpu(), ref_q, torch.zeros_like(ref_q))
    assert_close_bf16_sliced(masked_got, masked_ref, (3,), frac=S.ROW_FRAC[case], name="dQ per (token, head)")
    e = S.needed_frac(masked_got.cpu(), masked_ref, (3,)).max().item()
    _, emu_g = S.emulate_fused_pair(qkv, d1, pr["allow"], keep, B)
    small = (S.rows_with_a_gradient(pr["allow"]) & (k == S.ROW_K_NONZERO)[None, :, None] & ~zero[None, :, None]) & (S.dq_rows(emu_g, B).abs().amax(-1) > 0)
    assert small.any() and (got_q.abs().amax(-1)[small.cuda()] > 0).all(), "a row the emulation keeps non-zero came out zero"
    assert_close_bf16_sliced(g1.view(B, N, 3, H, HD), ref_g.view(B, N, 3, H, HD), (1, 4), name="dqkv per (part, sample, head)")
    assert_close_bf16_sliced(out1.view(B, N, H, HD), ref_out.view(B, N, H, HD), (1, 3), name="out per (sample, head)")
    print("PARITY dQ rows at 2^0 .. 2^-%d of the head's dO maximum, %s, %s: %.2e of the row's own maximum beyond the bf16 ulp (bound %.2e)"
          % (S.ROW_K_MAX, case, "fused" if fused else "two-kernel", e, S.ROW_FRAC[case]))

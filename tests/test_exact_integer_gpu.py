"""Exact arithmetic on the GPU: with small-integer operands (tests/exact_cases.py) every product and every partial sum of the GEMM family and of the fp32
reductions around it is an integer far below 2^24, so the result does not depend on the tile, the split, the pair slice or the kernel, and a bf16 output
is the single round-to-nearest-even of an integer.  Every comparison here is torch.equal against a float64 reference -- no tolerance, no measured number --
and every variant of one operation is compared with every other bit for bit.  A failure prints the number of differing elements, the first index,
got / want there and the exact difference (an integer, or one bf16 step at a tie): it names the dropped or doubled term.

The one premise that only the hardware can confirm -- the bf16 MFMA adds integer products below 2^17 exactly -- is the first test of the file
(test_single_tile_mfma_premise).  The GELU epilogues, attention, LayerNorm, BCE and Adam are not order-free on any input and stay out."""
import pytest
import torch

from tests import exact_cases as E

pytestmark = pytest.mark.gpu
DEV = "cuda"
BF16 = torch.bfloat16
F32 = torch.float32


def _mods():
    from sam_textvqa_amd import _capi, ops
    return ops, _capi


@pytest.fixture(scope="module", autouse=True)
def _drop_cached_cases():
    yield
    for f in (E.gemm_case, E.wgrad_case, E.grouped_case):
        f.cache_clear()


class Checks:
    """collects every mismatch of a test (so that one message shows which variants disagree and by how much), fails at the end"""

    def __init__(self):
        self.fails, self.n = [], 0

    def eq(self, got, want, name):
        self.n += 1
        msg = E.describe_mismatch(got, want, name)
        if msg:
            print(msg)
            self.fails.append(msg)
        return msg is None

    def done(self):
        assert not self.fails, "%d of %d comparisons are not bit-exact:\n%s" % (len(self.fails), self.n, "\n".join(self.fails[:40]))


# ------------------------------------------------------------------------------------------------ the premise
def test_single_tile_mfma_premise():
    """one 64 x 64 x 64 tile, no epilogue: fp32 and bf16 outputs of the 4-wave kernel equal the float64 product"""
    ops, capi = _mods()
    x, w = E.ints((64, 64), 1, -10, 10).to(DEV), E.ints((64, 64), 2, -10, 10).to(DEV)
    E.assert_exact_budget(x, w.t())
    ref = E.exact_mm(x, w.t())
    ck = Checks()
    ck.eq(ops.gemm(x, w, out_dtype=F32, force_tile=64), ref.float(), "single tile fp32")
    ck.eq(ops.gemm(x, w, force_tile=64), E.rne_bf16(ref), "single tile bf16")
    ck.done()


# ------------------------------------------------------------------------------------------------ forward and dgrad
def _tiles(ts):
    return [dict(force_tile=t) for t in ts]


GEMM_VARIANTS = {
    "ragged712": _tiles(E.TILES4) + [dict()],
    "k64": _tiles(E.TILES8) + [dict(force_tile=128), dict()],
    "k704": _tiles(E.TILES8) + [dict(force_tile=128), dict()],
    "persistent": _tiles(E.TILES8) + [dict(force_tile=128), dict()],
    "split3": [dict(split_k=3), dict(split_k=-1), dict(force_tile=64), dict()],          # dict(): ops.gemm lets the library split a skinny long-K problem
    "split8": [dict(split_k=8), dict(split_k=-1), dict(force_tile=64), dict()],
}
SEED, OFFSET = 11, 3


def _run_variant(ops, capi, c, kw):
    x, w, wt, bias, res = c["x"], c["w"], c["wt"], c["bias"], c["res"]
    M, N = c["M"], c["N"]
    drop = dict(epilogue=capi.EPI_BIAS_DROPOUT_RES, bias=c["bias_hi"], residual=res, p_drop=0.5, seed=SEED, offset=OFFSET)
    o = {}
    o["fwd_none"] = ops.gemm(x, w, **kw)
    o["fwd_bias"] = ops.gemm(x, w, epilogue=capi.EPI_BIAS, bias=bias, **kw)
    o["fwd_res"] = ops.gemm(x, w, epilogue=capi.EPI_BIAS_DROPOUT_RES, bias=bias, residual=res, **kw)
    o["fwd_drop"] = ops.gemm(x, w, **drop, **kw)
    o["dgrad_none"] = ops.gemm(x, wt, b_kcontig=False, **kw)
    o["dgrad_aux"] = ops.gemm(x, wt, b_kcontig=False, epilogue=capi.EPI_MUL_AUX, aux_in=c["aux"], **kw)
    o["dgrad_res"] = ops.gemm(x, wt, b_kcontig=False, epilogue=capi.EPI_BIAS_DROPOUT_RES, bias=bias, residual=res, **kw)
    o["dgrad_drop"] = ops.gemm(x, wt, b_kcontig=False, **drop, **kw)
    if kw.get("force_tile", 0) < 1000:                      # fp32 outputs: the 4-wave kernels and the split-K reduction (the 8- and 12-wave kernels store bf16 only)
        o["fwd_none_f32"] = ops.gemm(x, w, out_dtype=F32, **kw)
        o["fwd_bias_f32"] = ops.gemm(x, w, out_dtype=F32, epilogue=capi.EPI_BIAS, bias=bias, **kw)
    # strided views: lda larger than K; out a column slice of a wider buffer, whose other columns must stay as they were
    o["fwd_none@lda"] = ops.gemm(c["x_wide"][:, 64:], w, **kw)
    wide = torch.full((M, N + 64), 7.0, dtype=BF16, device=DEV)
    ops.gemm(x, w, epilogue=capi.EPI_BIAS, bias=bias, out=wide[:, 32:32 + N], **kw)
    o["fwd_bias@ldc"] = wide
    return o


@pytest.mark.parametrize("name", list(GEMM_VARIANTS))
def test_forward_and_dgrad_every_variant_is_bit_exact(name):
    """every forced tile, the default picker and (split cases) forced and automatic split-K: each epilogue's output equals the exact reference and the first
    variant's output; under p_drop = 0.5 every element is exactly rne(res) or rne(res + 2 (acc + bias)) and the kept set is the same in every variant"""
    ops, capi = _mods()
    c = dict(E.gemm_case(name, DEV))
    M, N, K = c["M"], c["N"], c["K"]
    c["x_wide"] = torch.cat([E.ints((M, 64), 99, -9, 9).to(DEV), c["x"]], 1)
    want = dict(c["want"])
    want["fwd_none@lda"] = want["fwd_none"]
    want["fwd_bias@ldc"] = torch.full((M, N + 64), 7.0, dtype=BF16, device=DEV)
    want["fwd_bias@ldc"][:, 32:32 + N] = want["fwd_bias"]
    ck = Checks()
    first, first_tag, kept_sets = None, None, {}
    for kw in GEMM_VARIANTS[name]:
        tag = "%s %s" % (name, kw or "default")
        o = _run_variant(ops, capi, c, kw)
        for key, got in o.items():
            if key.endswith("_drop"):
                dropped, kept = want[key]
                is_kept = got == kept
                ck.eq(got, torch.where(is_kept, kept, dropped), "%s %s: neither rne(res) nor rne(res + 2 (acc + bias))" % (tag, key))
                share = float(is_kept.double().mean())
                assert abs(share - 0.5) <= 2.5 / (M * N) ** 0.5, (tag, key, share)          # five binomial standard deviations
                if key in kept_sets:
                    ck.eq(is_kept, kept_sets[key], "%s %s: kept set differs from %s's" % (tag, key, first_tag))
                else:
                    kept_sets[key] = is_kept
            else:
                ck.eq(got, want[key], "%s %s vs float64" % (tag, key))
            if first is not None and key in first:
                ck.eq(got, first[key], "%s %s vs %s" % (tag, key, first_tag))
        if first is None:
            first, first_tag = o, tag
    ck.done()


# ------------------------------------------------------------------------------------------------ weight gradient and its riders
def _wg(ops, c, out, **kw):
    return ops.gemm(c["dy"], c["x"], a_kcontig=False, b_kcontig=False, out=out, **kw)


@pytest.mark.parametrize("R,M,N", E.WGRAD_CASES)
def test_weight_gradient_every_form_is_bit_exact(R, M, N):
    """dW = dy^T x, fp32: unsplit, split_k -1 / 4 / 7, accumulated into a non-zero integer C, the split-K store form, the fused bias gradient accumulated into
    a non-zero integer vector or overwritten -- all equal to the float64 reference (hence to one another)"""
    ops, capi = _mods()
    c = E.wgrad_case(R, M, N, DEV)
    plain, acc = c["prod"].float(), (c["c0"].double() + c["prod"]).float()
    b_plain, b_acc = c["colsum"].float(), (c["b0"].double() + c["colsum"]).float()
    junk = lambda t: torch.full_like(t, 7.5)
    ck = Checks()
    ck.eq(_wg(ops, c, None, out_dtype=F32, split_k=1), plain, "unsplit")
    dw, db = junk(c["c0"]), junk(c["b0"])
    _wg(ops, c, dw, split_k=1, bias_grad=db)
    ck.eq(dw, plain, "unsplit, overwrite"); ck.eq(db, b_plain, "unsplit, bias gradient overwritten")
    dw, db = c["c0"].clone(), c["b0"].clone()
    _wg(ops, c, dw, accumulate=True, split_k=1, bias_grad=db)
    ck.eq(dw, acc, "unsplit, accumulate"); ck.eq(db, b_acc, "unsplit, bias gradient accumulated")
    tiles = E.TILES4 if (R, M, N) == E.WGRAD_CASES[0] else ()
    for kw in [dict(split_k=s) for s in (-1, 4, 7)] + [dict(split_k=-1, force_tile=t) for t in tiles]:
        dw, db = c["c0"].clone(), c["b0"].clone()
        _wg(ops, c, dw, accumulate=True, bias_grad=db, **kw)
        ck.eq(dw, acc, "accumulate %s" % kw); ck.eq(db, b_acc, "bias gradient %s" % kw)
        dw = c["c0"].clone()
        _wg(ops, c, dw, accumulate=True, **kw)
        ck.eq(dw, acc, "accumulate, no rider %s" % kw)
    for s in (4, 7):
        dw = junk(c["c0"])
        _wg(ops, c, dw, accumulate=False, split_k=s)
        ck.eq(dw, plain, "split-K store, split_k=%d" % s)
    ck.done()


def test_splitk_reduce_on_an_integer_workspace():
    """sam_gemm_splitk_reduce by itself: C (a column view) += the sum of S partial tiles, the bias gradient += the sum of S partial rows"""
    ops, capi = _mods()
    S, M, N = 5, 24, 36
    ws = E.ints((S * M * N + S * M,), 41, -1000, 1000, F32).to(DEV)
    wide = E.ints((M, N + 12), 42, -E.C_R, E.C_R, F32).to(DEV)
    b0 = E.ints((M,), 43, -E.C_R, E.C_R, F32).to(DEV)
    want_c = wide.double().clone()
    want_c[:, 4:4 + N] += ws[:S * M * N].double().view(S, M, N).sum(0)
    want_b = b0.double() + ws[S * M * N:].double().view(S, M).sum(0)
    assert float(want_c.abs().max()) < E.BUDGET
    cv, b = wide[:, 4:4 + N], b0.clone()
    capi.call("sam_gemm_splitk_reduce", ws.data_ptr(), S, M, N, cv.data_ptr(), cv.stride(0), b.data_ptr(), capi.stream_handle())
    ck = Checks()
    ck.eq(wide, want_c.float(), "splitk_reduce C"); ck.eq(b, want_b.float(), "splitk_reduce bias gradient")
    ck.done()


@pytest.mark.parametrize("name", list(E.GROUPED_CASES))
def test_grouped_weight_gradient_every_kernel_is_bit_exact(name):
    """sam_gemm_bf16_grouped on the 4-wave kernel (128), the 8-wave pair-exchange kernel (1256), the loader-wave kernel (12448, the mixed-depth set) and the
    default choice: accumulate into non-zero integer gradients and overwrite, with bias riders -- all equal to the float64 reference (hence to one another)"""
    ops, capi = _mods()
    cs = E.grouped_case(name, DEV)
    ck = Checks()
    for tile in E.GROUPED_TILES[name]:
        for accumulate in (True, False):
            start = (lambda t: t.clone()) if accumulate else (lambda t: torch.full_like(t, -3.5))
            jobs = [(c["dy"], c["x"], start(c["c0"]), None if c["b0"] is None else start(c["b0"])) for c in cs]
            ops.wgrad_grouped(jobs, force_tile=tile, accumulate=accumulate)
            ops.grouped_ws_check()
            for j, (c, job) in enumerate(zip(cs, jobs)):
                tag = "%s force_tile=%d %s problem %d" % (name, tile, "accumulate" if accumulate else "overwrite", j)
                ck.eq(job[2], ((c["c0"].double() if accumulate else 0.0) + c["prod"]).float(), tag + " dW")
                if job[3] is not None:
                    ck.eq(job[3], ((c["b0"].double() if accumulate else 0.0) + c["colsum"]).float(), tag + " bias gradient")
    ck.done()


# ------------------------------------------------------------------------------------------------ fp32 reductions that are order-free on integers
@pytest.mark.parametrize("M,N", E.COLSUM_SHAPES)
def test_colsum_is_exact(M, N):
    ops, capi = _mods()
    x = E.colsum_case(M, N).to(DEV)
    base = E.ints((N,), 3 * M + N, -E.C_R, E.C_R, F32).to(DEV)
    ref = x.double().sum(0)
    ck = Checks()
    out = torch.full((N,), 7.5, device=DEV)
    ops.colsum(x, out, accumulate=False)
    ck.eq(out, ref.float(), "colsum")
    out = base.clone()
    ops.colsum(x, out, accumulate=True)
    ck.eq(out, (base.double() + ref).float(), "colsum accumulated")
    if N >= 16:                                              # a column view of x into a slice of the output: the rest of the output stays
        n0, n1 = N // 4 // 4 * 4, N // 4 // 4 * 4 + N // 2 // 4 * 4
        out = base.clone()
        ops.colsum(x[:, n0:n1], out[n0:n1], accumulate=True)
        want = base.double().clone()
        want[n0:n1] += ref[n0:n1]
        ck.eq(out, want.float(), "colsum of a column view")
    ck.done()


@pytest.mark.parametrize("n", E.SUMSQ_N)
def test_sumsq_is_the_integer_sum_of_squares(n):
    ops, capi = _mods()
    g = E.sumsq_case(n).to(DEV)
    out = torch.full((1,), -1.0, device=DEV)
    ops.sumsq(g, out)
    ck = Checks()
    ck.eq(out, (g.double() ** 2).sum().float().reshape(1), "sumsq n=%d" % n)
    ck.done()


def test_sumsq_row_sparse_route_skips_untouched_rows():
    """sam_sparse_rows: rows of the region whose flag is 0 are skipped whatever they hold; the flagged rows and the dense rest (with an n & 3 tail) are summed"""
    ops, capi = _mods()
    rows, d, head, tail = 37, 64, 4096, 1003
    lo, hi = head, head + rows * d
    g = E.ints((hi + tail,), 5, -2, 2, F32).to(DEV)
    touched = (torch.arange(rows) % 3 != 1).to(torch.uint8).to(DEV)
    out = torch.full((1,), -1.0, device=DEV)
    ops.sumsq(g, out, sparse=(lo, hi, d, touched))
    sq = g.double() ** 2
    want = sq[:lo].sum() + sq[hi:].sum() + (sq[lo:hi].view(rows, d).sum(1) * touched.double()).sum()
    assert float(sq.sum()) < E.BUDGET and float(want) < float(sq.sum())
    ck = Checks()
    ck.eq(out, want.float().reshape(1), "row-sparse sumsq")
    ck.done()


def _index_add(base, ids, dy, rows, padding_idx):
    keep = (ids != padding_idx) & (ids >= 0) & (ids < rows)
    return base.double().index_add_(0, ids[keep], dy.double()[keep]).float()


@pytest.mark.parametrize("T,D,rows", [(777, 768, 97), (5, 256, 11), (1280, 768, 3000)])
def test_embedding_backward_routes_equal_index_add(T, D, rows):
    """sam_embedding_bwd on its no-atomics route (aligned table) and on its atomic route (a table 4 bytes off a 16-byte boundary), sam_embedding_bwd_sorted:
    integer dy, repeated indices (one row a third of the list), padding entries -- all equal index_add_ in float64; on integers the atomics have no order excuse"""
    ops, capi = _mods()
    dy, ids, base = E.scatter_case(T, D, rows, 1000 + T)
    want = _index_add(base.to(DEV), ids.to(DEV), dy.to(DEV), rows, 0)
    ck = Checks()
    tab = base.clone().to(DEV)
    ops.embedding_bwd(dy.to(DEV), ids.to(DEV), tab, padding_idx=0)
    ck.eq(tab, want, "embedding_bwd, no atomics")
    buf = torch.zeros(rows * D + 4, device=DEV)
    off = buf[1:1 + rows * D].view(rows, D)
    assert off.data_ptr() % 16 == 4
    off.copy_(base)
    ops.embedding_bwd(dy.to(DEV), ids.to(DEV), off, padding_idx=0)
    ck.eq(off, want, "embedding_bwd, atomics")
    order = torch.sort(ids, stable=True)
    tab = base.clone().to(DEV)
    ops.embedding_bwd_sorted(dy[order.indices].contiguous().to(DEV), order.values.to(DEV), tab, padding_idx=0)
    ck.eq(tab, want, "embedding_bwd_sorted")
    ck.done()


@pytest.mark.parametrize("with_types", [False, True])
def test_embed_sum_backward_equals_index_add(with_types):
    ops, capi = _mods()
    b, s, d, n_types = 7, 12, 96, 3
    de = E.ints((b * s, d), 61).to(DEV)
    types = torch.randint(0, n_types, (b * s,), generator=torch.Generator().manual_seed(62)).to(torch.uint8).to(DEV) if with_types else None
    pos0, tt0 = E.ints((20, d), 63, -E.C_R, E.C_R, F32).to(DEV), E.ints((n_types, d), 64, -E.C_R, E.C_R, F32).to(DEV)
    d_pos, d_tt = pos0.clone(), tt0.clone()
    ops.embed_sum_bwd(de, s, d_pos, d_tt, types, n_types=n_types if with_types else 1)
    want_pos = pos0.double().clone()
    want_pos[:s] += de.double().view(b, s, d).sum(0)
    t_ids = types.long() if with_types else torch.zeros(b * s, dtype=torch.long, device=DEV)
    want_tt = tt0.double().index_add_(0, t_ids, de.double())
    ck = Checks()
    ck.eq(d_pos, want_pos.float(), "embed_sum_bwd d_pos"); ck.eq(d_tt, want_tt.float(), "embed_sum_bwd d_tt")
    ck.done()


def test_gather2_add_backward_equals_index_add():
    ops, capi = _mods()
    b, s, d, v, n_ocr = 6, 12, 768, 300, 50
    inds = torch.randint(0, v + n_ocr, (b, s), generator=torch.Generator().manual_seed(4))
    inds[:, 0] = 1
    inds[0, 5:] = 0                                   # the padding index, repeated
    inds[3, 2:9] = v + 7                              # one OCR row repeated
    inds = inds.to(DEV)
    dy = E.ints((b * s, d), 65).to(DEV)
    d_ans, d_ocr, d_emb = ops.gather2_add_bwd(dy, inds, v, n_ocr, p_drop=0.0)
    flat = inds.reshape(-1)
    is_ocr = flat >= v
    want_ans = torch.zeros(v, d, dtype=torch.float64, device=DEV).index_add_(0, flat[~is_ocr], dy.double()[~is_ocr])
    rows = (torch.arange(b, device=DEV).repeat_interleave(s) * n_ocr + flat - v)[is_ocr]
    want_ocr = torch.zeros(b * n_ocr, d, dtype=torch.float64, device=DEV).index_add_(0, rows, dy.double()[is_ocr])
    ck = Checks()
    ck.eq(d_ans, want_ans.float(), "gather2_add_bwd d_ans"); ck.eq(d_ocr, want_ocr.float(), "gather2_add_bwd d_ocr"); ck.eq(d_emb, dy, "gather2_add_bwd d_emb")
    ck.done()


@pytest.mark.parametrize("S,No,D", E.PTR_SHAPES)
def test_pointer_scores_are_exact(S, No, D):
    """scale = 2^-5: the forward equals q . k * 2^-5 - 10000 (1 - mask) exactly (one sample fully padded), dq / dk equal rne_bf16 of the exact products"""
    ops, capi = _mods()
    q, k, mask, ds = (t.to(DEV) for t in E.ptr_case(S, No, D))
    want = torch.einsum("bsd,bod->bso", q.double(), k.double()) * E.PTR_SCALE - 10000.0 * (1.0 - mask.double())[:, None, :]
    ck = Checks()
    out = ops.ptr_scores_fwd(q, k, mask, E.PTR_SCALE)
    ck.eq(out, want.float(), "ptr scores")
    assert bool((out[1] <= -10000.0 + 9.0 * D * E.PTR_SCALE).all())
    dq, dk = ops.ptr_scores_bwd(ds, q, k, E.PTR_SCALE)
    ck.eq(dq, E.rne_bf16(torch.einsum("bso,bod->bsd", ds.double(), k.double()) * E.PTR_SCALE), "ptr dq")
    ck.eq(dk, E.rne_bf16(torch.einsum("bso,bsd->bod", ds.double(), q.double()) * E.PTR_SCALE), "ptr dk")
    ck.done()

"""GPU parity of the attention entry points that serve inference and `output_attentions` (include/sam_hip.h): sam_attn_probs, sam_attn_fwd_rows,
sam_attn_fwd_dec, sam_attn_fwd_dec_shared and sam_attn_dec_row, each called directly.  Every reference is fp64 on the host from the same bf16-rounded
q | k | v values; where the header promises bit-identity with the full kernel, the full kernel (sam_attn_fwd, pinned by tests/test_attention_gpu.py) is
the reference.  B = 2 samples, H = 3 heads of 64 throughout: no path below depends on the head count.

tests/test_attention_gpu.py's make_problem / oracle_attention are not used here: the first builds relation masks from boxes at H = 12 (these tests take
per-head masks from mask_bits_from_int8_bhnn, as the issue of this file asks), the second returns the fp32 context, not the probabilities.
tests/test_attention_infer_cpu.py holds the CPU half: that plain fp32 arithmetic meets the per-row bound used for sam_attn_probs on these inputs."""
import functools
import math

import pytest
import torch

from tests.util import assert_close_bf16, assert_close_bf16_sliced, unpack_bits

pytestmark = pytest.mark.gpu

B, H, HD = 2, 3, 64
SCALE = 1.0 / math.sqrt(HD)
# every key-tile class of pick_nkt (2, 4, 8, 12, 16, 24 tiles of 16 keys) from both sides of each boundary, plus the workload's 182
LENS = [1, 17, 32, 33, 64, 65, 128, 129, 182, 192, 193, 256, 257, 384]
P_DROP = 0.1
INV_KEEP = 1.0 / (1.0 - round(P_DROP * 65536) / 65536.0)


def _ops():
    from sam_textvqa_amd import ops
    return ops


def _err():
    from sam_textvqa_amd._capi import SamHipError
    return SamHipError


# ------------------------------------------------------------------------------------------------ problems and fp64 references (host only)
def default_n_dec(n):
    return min(12, n // 3)


@functools.lru_cache(maxsize=None)
def make_inputs(n, per_head, n_dec=None, batch=B, seed=0):
    """q | k | v bf16 [batch*n, 3*H*64] and a prefix-LM allow mask (encoder keys visible to every row unless padded, decoder keys causally to decoder rows)
    with up to three padded encoder keys in sample 0; per_head: ANDed with a random relation tensor int8 [batch, H, n, n] in which (last sample, last
    head, row n // 2) sees no key at all.  Built on the host: `allow` bool [batch, H or 1, n, n] is what the references use, the device bits are checked
    against it before any kernel runs (device_bits).  Cached: treat the result as read-only."""
    n_dec = default_n_dec(n) if n_dec is None else n_dec
    n_enc = n - n_dec
    g = torch.Generator().manual_seed(1000 * seed + 7 * n + int(per_head))
    qkv = (torch.randn(batch * n, 3 * H * HD, generator=g) * 1.5).to(torch.bfloat16)
    key_valid = torch.ones(batch, n_enc, dtype=torch.uint8)
    n_pad = min(3, n_enc - 1)
    if n_pad > 0:
        key_valid[0, n_enc - n_pad:] = 0
    allow = torch.zeros(batch, 1, n, n, dtype=torch.bool)
    allow[:, :, :, :n_enc] = key_valid.bool()[:, None, None, :]
    if n_dec:
        allow[:, :, n_enc:, n_enc:] = torch.tril(torch.ones(n_dec, n_dec, dtype=torch.bool))
    rel, dead = None, None
    if per_head:
        rel = (torch.rand(batch, H, n, n, generator=g) > 0.4).to(torch.int8)
        dead = (batch - 1, H - 1, n // 2)
        rel[dead] = 0
        allow = allow & rel.bool()
    return dict(n=n, n_dec=n_dec, n_enc=n_enc, batch=batch, qkv=qkv, key_valid=key_valid, allow=allow, rel=rel, dead=dead)


def device_bits(pr):
    """the allow words the kernels read, and proof that they say what the host mask says"""
    ops = _ops()
    bits = ops.mask_bits_prefix_lm(pr["key_valid"].cuda(), pr["n_dec"])
    if pr["rel"] is not None:
        bits = ops.mask_bits_from_int8_bhnn(pr["rel"].cuda(), bits)
    assert torch.equal(unpack_bits(bits, pr["n"]), pr["allow"])
    return bits


def heads(qkv, batch, dtype=torch.float64):
    """[batch*n, 3*H*64] -> q, k, v as [batch, H, n, 64]"""
    n = qkv.shape[0] // batch
    x = qkv.to(dtype).view(batch, n, 3, H, HD).permute(2, 0, 3, 1, 4)
    return x[0], x[1], x[2]


def softmax_probs(qkv, allow, batch, dtype=torch.float64):
    """softmax(scale * q k^T) over the allowed keys, exact zeros at masked keys and in rows with no allowed key (sa_m4c.py:563-586), in `dtype`"""
    q, k, _ = heads(qkv, batch, dtype)
    s = (q @ k.transpose(-1, -2)) * SCALE
    s = s.masked_fill(~allow, float("-inf"))
    alive = allow.any(-1, keepdim=True).expand_as(s)
    p = torch.softmax(s.masked_fill(~alive, 0.0), dim=-1)
    return torch.where(alive & allow, p, torch.zeros_like(p))


@functools.lru_cache(maxsize=None)
def reference_probs(n, per_head):
    pr = make_inputs(n, per_head)
    return softmax_probs(pr["qkv"], pr["allow"], pr["batch"])


def context_of(p, qkv, batch):
    """fp64 P @ V on the device, merged back to [batch*n, H*64]"""
    v = heads(qkv, batch)[2].to(p.device)
    return (p.double() @ v).permute(0, 2, 1, 3).reshape(qkv.shape[0], H * HD)


def over_bound(got, ref, frac=1e-3, ulps=1):
    """largest err / bound of assert_close_bf16's bound (frac * max|ref| + ulps * 2^-8 * |ref|): the figure the PARITY lines report"""
    ref = ref.detach().to(device=got.device, dtype=torch.float64)
    return ((got.detach().double() - ref).abs() / (frac * ref.abs().max() + ulps * 2.0 ** -8 * ref.abs())).max().item()


def bits_of(t):
    return t.view(torch.int16 if t.dtype == torch.bfloat16 else torch.int32)


# ------------------------------------------------------------------------------------------------ 1. sam_attn_probs
@pytest.mark.parametrize("per_head", [False, True], ids=["shared", "per_head"])
@pytest.mark.parametrize("n", LENS)
def test_attn_probs_against_fp64_softmax(n, per_head):
    """sam_attn_probs: "P = allow ? exp2(scale * log2(e) * <q, k> - lse2) : 0 ... times head_scale[h] ... Fully masked rows are exact zeros".
    One wave per query row walks the keys 64 at a time, so LENS puts the key loop at 1..6 trips with full and ragged last trips, and the mask row at every
    word count (1, 2, 4, 6, 8, 12); lse2 comes from sam_attn_fwd at each of its key-tile classes.  shared: allow_stride_h = 0; per_head: one mask per
    head, with one (sample, head, row) that sees nothing.
    Values: per query row, |P - fp64 softmax| <= 1e-3 * max of the row (tests/test_attention_infer_cpu.py: plain fp32 meets this bound on these inputs,
    so it is the arithmetic's bound, not a measurement of the kernel).  Masked keys and the dead row are exactly 0.0, the dead row's lse2 is +inf.  Live rows
    sum to 1 within 1e-3: at most 384 fp32 terms, each within 2^-23 relative of its value plus the shared rounding of lse2 (|lse2| < 64, so 2^-18 in the
    exponent, 4e-6 relative), two orders inside the bound.  Closure: fp64 P @ V reproduces the forward's `out` at the forward's own bound (1e-3 of max
    + 1 bf16 ulp), which ties the rebuilt probabilities to what the fused kernel used.  head_scale [1, 0, 1.25]: bit-identical to an fp32 multiply of
    the unscaled result, the 0.0 head all zeros."""
    ops = _ops()
    pr = make_inputs(n, per_head)
    ref = reference_probs(n, per_head)
    allow = pr["allow"].expand(B, H, n, n)
    qkv, bits = pr["qkv"].cuda(), device_bits(pr)
    out, lse2, keep = ops.attn_fwd(qkv, bits, B, H, SCALE, 0.0)
    assert keep is None
    p = ops.attn_probs(qkv, bits, lse2, None, B, H, SCALE)
    assert p.shape == (B, H, n, n) and p.dtype == torch.float32
    e_val = assert_close_bf16_sliced(p, ref, slice_dims=(-1,), ulps=0, name="attn_probs N=%d" % n)
    assert (p.cpu()[~allow] == 0).all(), "masked keys must be exact zeros"
    alive = allow.any(-1)
    if per_head:
        assert not alive[pr["dead"]]
    assert (p.cpu()[~alive] == 0).all()
    l2 = lse2.cpu()
    assert torch.isinf(l2[~alive]).all() and (l2[~alive] > 0).all() and torch.isfinite(l2[alive]).all()
    e_sum = (p.double().sum(-1).cpu()[alive] - 1.0).abs().max().item()
    assert e_sum <= 1e-3, e_sum
    ctx = context_of(p, pr["qkv"], B)
    assert_close_bf16(out, ctx, name="P @ V vs attn_fwd out N=%d" % n)
    hs = torch.tensor([1.0, 0.0, 1.25], device="cuda")
    ph = ops.attn_probs(qkv, bits, lse2, None, B, H, SCALE, head_scale=hs)
    assert torch.equal(ph, p * hs.view(1, H, 1, 1)) and (ph[:, 1] == 0).all()
    print("PARITY attn_probs N=%d %s: values %.4f of bound, row sums %.4f of bound, P@V vs out %.3f of bound"
          % (n, "per-head" if per_head else "shared", e_val / 1e-3, e_sum / 1e-3, over_bound(out, ctx)))


@pytest.mark.parametrize("per_head", [False, True], ids=["shared", "per_head"])
@pytest.mark.parametrize("n", [17, 182, 257])
def test_attn_probs_with_the_forward_dropout(n, per_head):
    """sam_attn_probs: "times keep / (1 - p_drop) where the forward dropped (keep: its bit planes, NULL = no dropout)".  Lengths with 1, 6 and 12 keep
    words per row (the last one ragged).  P is exactly 0 where the forward's keep bit or the allow bit is clear; elsewhere it equals the undropped
    probabilities on the same lse2 times inv_keep = 1 / (1 - round(p * 65536) / 65536) within one fp32 ulp: the library's fp32 inv_keep is 0.42 * 2^-24
    relative from the exact quotient (under half an ulp of any product) and the fp32 multiply adds half an ulp (the ulp is that of the larger of the two values, which
    covers a product rounded up across a power of two; no live probability here is anywhere near the subnormals).  fp64 P_drop @ V reproduces the dropout forward's `out` at the forward's bound."""
    ops = _ops()
    pr = make_inputs(n, per_head)
    allow = pr["allow"].expand(B, H, n, n)
    qkv, bits = pr["qkv"].cuda(), device_bits(pr)
    out, lse2, keep_bits = ops.attn_fwd(qkv, bits, B, H, SCALE, P_DROP, seed=4321, offset=11)
    keep = unpack_bits(keep_bits, n)
    live = keep & allow
    assert 0 < int((allow & ~keep).sum()) < int(allow.sum())
    p_drop = ops.attn_probs(qkv, bits, lse2, keep_bits, B, H, SCALE, P_DROP)
    p_plain = ops.attn_probs(qkv, bits, lse2, None, B, H, SCALE)
    assert (p_drop.cpu()[~live] == 0).all()
    got, want = p_drop.double().cpu(), p_plain.double().cpu() * INV_KEEP
    ulp = torch.ldexp(torch.ones_like(want), torch.floor(torch.log2(torch.maximum(got, want).clamp_min(2.0 ** -126))).to(torch.int32) - 23)
    err = ((got - want).abs() / ulp)[live].max().item()
    assert err <= 1.0, err
    ctx = context_of(p_drop, pr["qkv"], B)
    assert_close_bf16(out, ctx, name="P_drop @ V vs dropout forward N=%d" % n)
    print("PARITY attn_probs dropout N=%d %s: %.3f fp32 ulp from P * inv_keep (bound 1), P_drop@V vs out %.3f of bound" % (n, "per-head" if per_head else "shared", err, over_bound(out, ctx)))


def test_attn_probs_error_paths():
    """sam_attn_probs rejects on the host: dropout without the forward's keep bits ("dropout needs the forward's keep bits"), 385 keys (past the fused kernels'
    single-pass limit) and head_dim != 64"""
    ops = _ops()
    pr = make_inputs(17, False)
    qkv, bits = pr["qkv"].cuda(), device_bits(pr)
    lse2 = ops.attn_fwd(qkv, bits, B, H, SCALE, 0.0)[1]
    with pytest.raises(_err()):
        ops.attn_probs(qkv, bits, lse2, None, B, H, SCALE, P_DROP)
    big = torch.zeros(B * 385, 3 * H * HD, dtype=torch.bfloat16, device="cuda")
    with pytest.raises(_err()):
        ops.attn_probs(big, torch.zeros(B, 1, 385, 13, dtype=torch.int32, device="cuda"), torch.zeros(B, H, 385, device="cuda"), None, B, H, SCALE)
    hd32 = torch.zeros(B * 17, 3 * H * 32, dtype=torch.bfloat16, device="cuda")
    with pytest.raises(_err()):
        ops.attn_probs(hd32, bits, lse2, None, B, H, SCALE)


# ------------------------------------------------------------------------------------------------ 2. sam_attn_fwd_rows
@pytest.mark.parametrize("n", [40, 100, 182, 230, 350])
def test_attn_fwd_rows_computes_its_rows_and_leaves_the_others(n):
    """sam_attn_fwd_rows: "only query rows >= q_begin (rounded down to a multiple of 16) are computed, against the keys/values of ALL rows of qkv; other
    rows of out / lse2 are left untouched".  N = 40 / 100 / 182 / 230 / 350 run the 4-, 8-, 12-, 16- and 24-tile kernels (4 or 8 waves striding the 16-row
    strips); q_begin = 0, 1, 15 start at strip 0, 16 and 17 at strip 1, N - 12 is the decoding loop's call, N - 1 the last strip alone.  `out` and `lse2`
    are pre-filled with finite sentinels (bf16 7.0, fp32 -123.0): rows from the strip boundary on are bit-identical to a full sam_attn_fwd pass, rows
    below it still hold the sentinel bits, for every sample and head, with a shared and with a per-head mask (whose dead row has lse2 = +inf)."""
    ops = _ops()
    for per_head in (False, True):
        pr = make_inputs(n, per_head)
        qkv, bits = pr["qkv"].cuda(), device_bits(pr)
        full, full_lse, _ = ops.attn_fwd(qkv, bits, B, H, SCALE, 0.0)
        full, full_lse = bits_of(full).view(B, n, -1), bits_of(full_lse)
        for q_begin in (0, 1, 15, 16, 17, n - 12, n - 1):
            out = torch.full((B * n, H * HD), 7.0, dtype=torch.bfloat16, device="cuda")
            lse2 = torch.full((B, H, n), -123.0, dtype=torch.float32, device="cuda")
            sent_out, sent_lse = bits_of(out).view(B, n, -1).clone(), bits_of(lse2).clone()
            ops.attn_fwd_rows(qkv, bits, B, H, SCALE, q_begin, out, lse2)
            lo = q_begin // 16 * 16
            got, got_lse = bits_of(out).view(B, n, -1), bits_of(lse2)
            assert torch.equal(got[:, lo:], full[:, lo:]) and torch.equal(got_lse[:, :, lo:], full_lse[:, :, lo:]), (n, per_head, q_begin)
            assert torch.equal(got[:, :lo], sent_out[:, :lo]) and torch.equal(got_lse[:, :, :lo], sent_lse[:, :, :lo]), (n, per_head, q_begin)


def test_attn_fwd_rows_error_paths():
    """sam_attn_fwd_rows: q_begin outside [0, N) is rejected on the host"""
    ops = _ops()
    n = 40
    pr = make_inputs(n, False)
    qkv, bits = pr["qkv"].cuda(), device_bits(pr)
    out = torch.zeros(B * n, H * HD, dtype=torch.bfloat16, device="cuda")
    lse2 = torch.zeros(B, H, n, device="cuda")
    for q_begin in (n, -1):
        with pytest.raises(_err()):
            ops.attn_fwd_rows(qkv, bits, B, H, SCALE, q_begin, out, lse2)


# ------------------------------------------------------------------------------------------------ 3. sam_attn_fwd_dec / sam_attn_fwd_dec_shared
DEC_PAIRS = [(20, 4), (32, 1), (33, 16), (100, 17), (128, 12), (129, 12), (200, 30), (256, 12), (257, 12), (384, 30)]


def beam_problem(pr, group, seed):
    """`group` beams per sample of a cached problem: distinct decoder rows per beam [b0*group*n_dec, 3*H*64], and the expanded batch a full pass would run
    (encoder rows repeated per beam, each beam's decoder rows written into its copy)"""
    b0, n, n_dec, n_enc = pr["batch"], pr["n"], pr["n_dec"], pr["n_enc"]
    g = torch.Generator().manual_seed(seed)
    dec = (torch.randn(b0 * group * n_dec, 3 * H * HD, generator=g) * 1.5).to(torch.bfloat16)
    expanded = pr["qkv"].view(b0, n, -1).repeat_interleave(group, 0).clone()
    expanded[:, n_enc:] = dec.view(b0 * group, n_dec, -1)
    return dec, expanded.view(b0 * group * n, -1)


@pytest.mark.parametrize("n,n_dec", DEC_PAIRS)
def test_attn_fwd_dec_and_dec_shared_equal_the_full_kernel(n, n_dec):
    """sam_attn_fwd_dec: "Same arithmetic per row as sam_attn_fwd (the results are bit-identical to a full pass over the same values)"; sam_attn_fwd_dec_shared:
    "the `group` beams of a sample have the SAME text / object / OCR rows ... kept ONCE per sample and decoder sample b reads those of sample b / group".
    The pairs reach every DEC instantiation of the dispatcher -- 2 key tiles (20, 32), 4 (33), 8 (100, 128), 12 (129), 16 (200, 256), 24 (257, 384) --
    with n_dec = 1, 4, 12, 16, 17 and 30: decoder rows inside one 16-row strip, exactly one strip, and over two and three strips whose first also holds
    encoder rows.  group = 1 is sam_attn_fwd_dec; 3, 5, 8 share one cached copy and one set of allow words among the beams.  The reference is the full
    kernel on the expanded batch (encoder rows and allow words repeated per beam); shared and per-head masks; the cache's own decoder rows hold 7.0 and
    are never read."""
    ops = _ops()
    b0, n_enc = B, n - n_dec
    for per_head in (False, True):
        pr = make_inputs(n, per_head, n_dec=n_dec)
        bits = device_bits(pr)
        cache = pr["qkv"].clone()
        cache.view(b0, n, -1)[:, n_enc:] = 7.0
        cache = cache.cuda()
        for group in (1, 3, 5, 8):
            b = b0 * group
            dec, expanded = beam_problem(pr, group, seed=31 * n + group)
            full, _, _ = ops.attn_fwd(expanded.cuda(), bits.repeat_interleave(group, 0).contiguous(), b, H, SCALE, 0.0)
            got = ops.attn_fwd_dec(cache, dec.cuda(), bits, b, n, n_dec, H, SCALE, kv_group=group)
            assert torch.equal(bits_of(got).view(b, n_dec, -1), bits_of(full).view(b, n, -1)[:, n_enc:]), (n, n_dec, per_head, group)


# ------------------------------------------------------------------------------------------------ 4. sam_attn_dec_row
def dec_row_reference(pr, dec, group, t):
    """fp64 softmax(scale * q k^T over the allowed keys) v of decoder row t of every beam against its sample's encoder rows and its own decoder rows
    (the reference loop of tests/test_decode_gpu.py's single-row test); a row with no allowed key gives zeros.  -> [b0*group, H, 64]"""
    b0, n, n_dec, n_enc = pr["batch"], pr["n"], pr["n_dec"], pr["n_enc"]
    b = b0 * group
    e3, d3 = pr["qkv"].double().view(b0, n, 3, H, HD), dec.double().view(b, n_dec, 3, H, HD)
    ok_all = pr["allow"].expand(b0, H, n, n)[:, :, n_enc + t]                          # [b0, H, n]
    want = torch.zeros(b, H, HD, dtype=torch.float64)
    for bb in range(b):
        s0 = bb // group
        kk = torch.cat([e3[s0, :n_enc, 1], d3[bb, :, 1]], 0)                           # [n, H, 64]
        vv = torch.cat([e3[s0, :n_enc, 2], d3[bb, :, 2]], 0)
        for hh in range(H):
            ok = ok_all[s0, hh]
            if not ok.any():
                continue
            sc = (kk[:, hh] @ d3[bb, t, 0, hh]) * SCALE
            want[bb, hh] = torch.softmax(sc.masked_fill(~ok, float("-inf")), 0) @ vv[:, hh]
    return want


@pytest.mark.parametrize("b0,group,n,n_dec,steps", [(1, 9, 100, 9, (0, 4, 8)), (2, 2, 65, 2, (0, 1)), (2, 3, 130, 3, (0, 1, 2)), (1, 5, 384, 30, (0, 29)), (2, 1, 33, 1, (0,))])
def test_attn_dec_row_at_its_edges(b0, group, n, n_dec, steps):
    """sam_attn_dec_row: "the attention output of decoder row t of decoder sample b against its sample's first N - n_dec cached rows and its own decoder
    rows 0..t ... fp32 arithmetic on the bf16 cache values; a row with no allowed key gives zeros".
    (1, 9, 100, 9): nine beams on the block's four waves, three trips of the beam loop with one beam in the last.  (2, 2, 65, 2) at t = 0, 1 and
    (2, 3, 130, 3) at t = 0, 1, 2: nkeys = n_enc + t + 1 = 64, 65 and 128, 129, 130, on and past the 64-lane boundaries of the kernel's `64 * m >= nkeys`
    skips.  (1, 5, 384, 30) at t = 0, 29: 354 staged rows (the largest footprint a 30-step decoder leaves) and nkeys = 384, all six 64-key trips.
    (2, 1, 33, 1): n_dec = 1.  Bound as in tests/test_decode_gpu.py: 1e-3 of max + 1 bf16 ulp against fp64 on the same bf16 values.  Decoder rows after
    t and the cache's own decoder rows are NaN: never read.  In the per-head mask (sample 0, head 1) sees no key at the case's last step: exact zeros."""
    ops = _ops()
    b, n_enc = b0 * group, n - n_dec
    worst = 0.0
    for per_head in (False, True):
        pr = make_inputs(n, per_head, n_dec=n_dec, batch=b0, seed=4)
        if per_head:
            rel = pr["rel"].clone()
            rel[0, 1, n_enc + steps[-1]] = 0
            pr = dict(pr, rel=rel, allow=pr["allow"] & rel.bool())
        bits = device_bits(pr)
        dec, _ = beam_problem(pr, group, seed=17 * n + group)
        cache = pr["qkv"].clone()
        cache.view(b0, n, -1)[:, n_enc:] = float("nan")
        cache = cache.cuda()
        for t in steps:
            poisoned = dec.clone()
            poisoned.view(b, n_dec, -1)[:, t + 1:] = float("nan")
            got = ops.attn_dec_row(cache, poisoned.cuda(), bits, b, n, n_dec, t, H, SCALE, kv_group=group).view(b, H, HD)
            want = dec_row_reference(pr, dec, group, t)
            assert_close_bf16(got, want, name="attn_dec_row N=%d group=%d t=%d" % (n, group, t))
            worst = max(worst, over_bound(got, want))
            if per_head and t == steps[-1]:
                assert (got[:group, 1] == 0).all() and (want[:group, 1] == 0).all()
    print("PARITY attn_dec_row b0=%d group=%d N=%d n_dec=%d: %.3f of bound" % (b0, group, n, n_dec, worst))

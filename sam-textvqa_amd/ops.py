"""Thin torch-facing wrappers over the C-ABI (raw ops; autograd lives in autograd.py).

Every function takes/returns CUDA(ROCm) tensors, allocates outputs with torch, passes raw device
pointers + the current HIP stream to libsam_hip.so and never synchronises."""
import ctypes as C
import os

import torch

from . import _capi as capi
from . import torchops
from .layouts import ANSWER_TABLE, ANSWER_TABLE_OUT, EVAL_BEAMS, EVAL_BOARD, EVAL_MERGED, EVAL_ROWS, SCORE_TABLE, SCORE_TABLE_OUT, WITNESS

BF16 = torch.bfloat16


class _TorchOpsProxy:
    """torch.ops.sam_hip with the package's error type: TORCH_CHECK failures (plain RuntimeError) surface as SamHipError, like the ctypes route's"""
    _cache = {}

    def __getattr__(self, name):
        fn = self._cache.get(name)
        if fn is None:
            op = getattr(torchops.ns(), name)

            def fn(*a, _op=op, **kw):
                try:
                    return _op(*a, **kw)
                except capi.SamHipError:
                    raise
                except RuntimeError as e:
                    raise capi.SamHipError(str(e).split("\n")[0]) from None
            self._cache[name] = fn
        return fn


_PROXY = _TorchOpsProxy()


def _tops():
    """torch.ops.sam_hip when the custom-op route is on (default) and bench.py's per-call event profiler is not recording (it brackets ctypes calls)"""
    return _PROXY if (torchops.enabled() and capi.profiler is None) else None


def _chk(t, dtype, name):
    if not t.is_cuda:
        raise capi.SamHipError("%s must live on the GPU (no CPU path in this package)" % name)
    if t.dtype != dtype:
        raise capi.SamHipError("%s: expected dtype %s, got %s" % (name, dtype, t.dtype))
    if not t.is_contiguous():
        raise capi.SamHipError("%s must be contiguous" % name)
    return t


_GPU = (_chk, capi.SamHipError)          # what the layouts' checks of a dict of GPU tensors apply to each tensor, and what they raise


def words_per_row(n):
    nw = capi.call("sam_attn_words_per_row", int(n))
    if nw <= 0:
        raise capi.SamHipError("sequence length %d exceeds the fused-attention limit (384 keys)" % n)
    return nw


# ----------------------------------------------------------------------------- masks
def pack_masks(question_mask, obj_mask, ocr_mask):
    """the batch's three padding masks -> (key_valid uint8 [B, T+No+Nc], question uint8 [B,T], ocr uint8 [B,Nc]) in one launch"""
    ms = []
    for m in (question_mask, obj_mask, ocr_mask):
        if not m.is_cuda:
            raise capi.SamHipError("pack_masks: masks must live on the GPU")
        ms.append(m.contiguous() if m.dtype == torch.int64 else m.ne(0).to(torch.int64).contiguous())
    q, o, c = ms
    t_ = _tops()
    if t_ is not None:
        return t_.pack_masks(q, o, c)
    b, t, no, nc = q.shape[0], q.shape[1], o.shape[1], c.shape[1]
    kv = torch.empty((b, t + no + nc), dtype=torch.uint8, device=q.device)
    q8 = torch.empty((b, t), dtype=torch.uint8, device=q.device)
    c8 = torch.empty((b, nc), dtype=torch.uint8, device=q.device)
    capi.call("sam_pack_masks_u8", capi.ptr(q), t, capi.ptr(o), no, capi.ptr(c), nc, b, capi.ptr(kv), capi.ptr(q8), capi.ptr(c8), capi.stream_handle())
    return kv, q8, c8


def mask_bits_prefix_lm(key_valid, n_dec):
    """key_valid: uint8 [B, n_enc] -> uint32 [B, 1, N, NW] (MMT prefix-LM/causal mask, sa_m4c.py:805-844)."""
    _chk(key_valid, torch.uint8, "key_valid")
    t_ = _tops()
    if t_ is not None:
        return t_.mask_bits_prefix_lm(key_valid, int(n_dec))
    b, n_enc = key_valid.shape
    n = n_enc + n_dec
    nw = words_per_row(n)
    out = torch.empty((b, 1, n, nw), dtype=torch.int32, device=key_valid.device)
    capi.call("sam_mask_bits_prefix_lm", capi.ptr(key_valid), b, n_enc, n_dec, nw, capi.ptr(out), capi.stream_handle())
    return out


def mask_bits_from_additive(mask):
    """mask: float32 [B,1,N,N] additive (0 / -10000) -> uint32 [B,1,N,NW]."""
    _chk(mask, torch.float32, "attention_mask")
    b, one, n, n2 = mask.shape
    if one != 1 or n != n2:
        raise capi.SamHipError("attention_mask must be [B,1,N,N], got %s" % (tuple(mask.shape),))
    t_ = _tops()
    if t_ is not None:
        return t_.mask_bits_from_additive(mask)
    nw = words_per_row(n)
    out = torch.empty((b, 1, n, nw), dtype=torch.int32, device=mask.device)
    capi.call("sam_mask_bits_from_additive", capi.ptr(mask), b, n, nw, capi.ptr(out), capi.stream_handle())
    return out


def _quadrant_bits(quadrants):
    qbits = 0
    for quad in quadrants:
        if quad not in (1, 2, 4, 7, 8, 9):
            raise ValueError("illegal attention_mask_quadrants entry %r" % (quad,))  # sa_m4c.py:548-549
        qbits |= 1 << quad
    return qbits


def mask_bits_spatial(base_bits, adj, n_txt, n_heads, quadrants):
    """base_bits [B,1,N,NW] & relation tensor int8 [B,Noo,Noo,R] -> uint32 [B,H,N,NW] (sa_m4c.py:470-552,568)."""
    _chk(base_bits, torch.int32, "base_bits")
    _chk(adj, torch.int8, "spatial_adj_matrix")
    b, _, n, nw = base_bits.shape
    n_oo, r = adj.shape[1], adj.shape[3]
    qbits = _quadrant_bits(quadrants)
    t_ = _tops()
    if t_ is not None:
        return t_.pack_relations(base_bits, adj, int(n_txt), int(n_heads), qbits)
    out = torch.empty((b, n_heads, n, nw), dtype=torch.int32, device=adj.device)
    capi.call("sam_mask_bits_spatial", capi.ptr(base_bits), capi.ptr(adj), b, n, nw, n_txt, n_oo, r, n_heads, qbits,
              capi.ptr(out), capi.stream_handle())
    return out


def _box_rows(boxes, name):
    """[B, n, >= 4] fp32 or float64 boxes on the GPU with unit column stride and samples back to back -> (tensor, row stride in elements)"""
    if not boxes.is_cuda:
        raise capi.SamHipError("%s must live on the GPU (no CPU path in this package)" % name)
    if boxes.dim() != 3 or boxes.shape[2] < 4 or boxes.dtype not in (torch.float32, torch.float64):
        raise capi.SamHipError("%s: expected fp32 or float64 [B, n, >= 4], got %s %s" % (name, boxes.dtype, tuple(boxes.shape)))
    if boxes.shape[1] and (boxes.stride(2) != 1 or boxes.stride(1) < 4 or boxes.stride(0) != boxes.shape[1] * boxes.stride(1)):
        boxes = boxes.contiguous()
    return boxes, boxes.stride(1)


def mask_bits_from_boxes(base_bits, obj_boxes, ocr_boxes, n_txt, n_heads, quadrants, context, distance_threshold=0.5, out=None):
    """base_bits [B,1,N,NW] & the batch's boxes -> uint32 [B,H,N,NW] in ONE launch (include/sam_hip_pipeline.h: sam_mask_bits_from_boxes): the bits
    mask_bits_spatial(base_bits, spatial_relation_tensor(float64(cat(obj[..., :4], ocr[..., :4])), context, distance_threshold), ...) gives, with no
    [B,n,n,12] tensor in between.  obj_boxes / ocr_boxes: fp32 (pad_obj_bboxes / pad_ocr_bboxes, [B, n, 5]) or float64 [B, n, >= 4], xyxy in columns
    0..3, all-zero rows = padding; ocr_boxes may be None.  `out`: write into this [B,H,N,NW] int32 buffer."""
    _chk(base_bits, torch.int32, "base_bits")
    b, _, n, nw = base_bits.shape
    obj_boxes, ld_obj = _box_rows(obj_boxes, "obj_boxes")
    n_obj, n_ocr, ld_ocr = obj_boxes.shape[1], 0, 0
    if ocr_boxes is not None and ocr_boxes.shape[1] > 0:
        ocr_boxes, ld_ocr = _box_rows(ocr_boxes, "ocr_boxes")
        n_ocr = ocr_boxes.shape[1]
        if ocr_boxes.dtype != obj_boxes.dtype or ocr_boxes.shape[0] != obj_boxes.shape[0]:
            raise capi.SamHipError("mask_bits_from_boxes: obj_boxes and ocr_boxes must share dtype and batch size")
    else:
        ocr_boxes = None
    if obj_boxes.shape[0] != b:
        raise capi.SamHipError("mask_bits_from_boxes: boxes of %d samples, base_bits of %d" % (obj_boxes.shape[0], b))
    qbits = _quadrant_bits(quadrants)
    if out is None:
        out = torch.empty((b, n_heads, n, nw), dtype=torch.int32, device=base_bits.device)
    else:
        _chk(out, torch.int32, "out")
        if tuple(out.shape) != (b, n_heads, n, nw):
            raise capi.SamHipError("mask_bits_from_boxes: out must be [%d, %d, %d, %d], got %s" % (b, n_heads, n, nw, tuple(out.shape)))
    capi.call("sam_mask_bits_from_boxes", capi.ptr(base_bits), capi.ptr(obj_boxes), ld_obj, n_obj, capi.ptr(ocr_boxes), ld_ocr, n_ocr,
              int(obj_boxes.dtype == torch.float64), b, n, nw, int(n_txt), int(n_heads), int(context), float(distance_threshold), qbits,
              capi.ptr(out), capi.stream_handle(), meta=dict(kernel="mask_bits_from_boxes", bytes=4.0 * out.numel()))
    return out


# ----------------------------------------------------------------------------- attention
def attn_fwd(qkv, allow, batch, n_heads, scale, p_drop=0.0, seed=0, offset=0, want_residual=False):
    """qkv bf16 [B*N, 3*H*64]; allow uint32 [B, H or 1, N, NW] -> (out bf16 [B*N, H*64], lse2 f32 [B,H,N], keep or None);
    want_residual=True (training: sam_attn_fwd_train) appends out_lo, the bf16 rounding residual of `out` the one-pass backward takes delta from."""
    _chk(qkv, BF16, "qkv"); _chk(allow, torch.int32, "allow")
    rows, three_d = qkv.shape
    n = rows // batch
    d_model = three_d // 3
    out = torch.empty((rows, d_model), dtype=BF16, device=qkv.device)
    out_lo = torch.empty_like(out) if want_residual else None
    lse2 = torch.empty((batch, n_heads, n), dtype=torch.float32, device=qkv.device)
    keep = torch.empty((batch, n_heads, n, allow.shape[-1]), dtype=torch.int32, device=qkv.device) if p_drop > 0 else None
    sh = 0 if allow.shape[1] == 1 else allow.stride(1)
    nw = allow.shape[-1]
    alg_bytes = batch * ((5 if want_residual else 4) * n * d_model * 2 + n_heads * n * nw * 4 * (2 if p_drop > 0 else 1) + n_heads * n * 4)
    meta = dict(kernel="attn_fwd", bytes=alg_bytes, flops=4.0 * batch * n * n * d_model, shape=(batch, n, n_heads))
    if want_residual:
        capi.call("sam_attn_fwd_train", capi.ptr(qkv), capi.ptr(allow), allow.stride(0), sh, batch, n, n_heads, d_model // n_heads,
                  float(scale), float(p_drop), int(seed), int(offset), capi.ptr(out), capi.ptr(out_lo), capi.ptr(lse2), capi.ptr(keep), capi.stream_handle(), meta=meta)
        return out, lse2, keep, out_lo
    capi.call("sam_attn_fwd", capi.ptr(qkv), capi.ptr(allow), allow.stride(0), sh, batch, n, n_heads, d_model // n_heads,
              float(scale), float(p_drop), int(seed), int(offset), capi.ptr(out), capi.ptr(lse2), capi.ptr(keep), capi.stream_handle(), meta=meta)
    return out, lse2, keep


def attn_probs(qkv, allow, lse2, keep, batch, n_heads, scale, p_drop=0.0, head_scale=None):
    """the attention probabilities the fused forward did not materialise: fp32 [B, H, N, N] from its q | k rows, allow bits, log2-sum-exps and keep bits
    (include/sam_hip.h: sam_attn_probs; sa_m4c.py:600-609 `output_attentions`)"""
    _chk(qkv, BF16, "qkv"); _chk(allow, torch.int32, "allow"); _chk(lse2, torch.float32, "lse2")
    rows, three_d = qkv.shape
    n, d_model = rows // batch, three_d // 3
    sh = 0 if allow.shape[1] == 1 else allow.stride(1)
    if head_scale is not None:
        _chk(head_scale, torch.float32, "head_scale")
    out = torch.empty((batch, n_heads, n, n), dtype=torch.float32, device=qkv.device)
    capi.call("sam_attn_probs", capi.ptr(qkv), capi.ptr(allow), allow.stride(0), sh, capi.ptr(lse2), capi.ptr(keep if p_drop > 0 else None), capi.ptr(head_scale),
              batch, n, n_heads, d_model // n_heads, float(scale), float(p_drop), capi.ptr(out), capi.stream_handle(),      # (dropout without keep bits: the library's error)
              meta=dict(kernel="attn_probs", bytes=4.0 * out.numel()))
    return out


def attn_fwd_rows(qkv, allow, batch, n_heads, scale, q_begin, out, lse2):
    """inference: recompute only query rows >= q_begin of `out` (bf16 [B*N, H*64], updated in place) against all keys of qkv"""
    _chk(qkv, BF16, "qkv"); _chk(allow, torch.int32, "allow"); _chk(out, BF16, "out")
    rows, three_d = qkv.shape
    n = rows // batch
    d_model = three_d // 3
    sh = 0 if allow.shape[1] == 1 else allow.stride(1)
    capi.call("sam_attn_fwd_rows", capi.ptr(qkv), capi.ptr(allow), allow.stride(0), sh, batch, n, n_heads, d_model // n_heads, float(scale), int(q_begin),
              capi.ptr(out), capi.ptr(lse2), capi.stream_handle())
    return out


def attn_fwd_dec(qkv_enc, qkv_dec, allow, batch, n, n_dec, n_heads, scale, out_dec=None, kv_group=1):
    """decoding step: decoder rows' q|k|v in their own compact buffer qkv_dec [B*n_dec, 3*H*64], encoder rows read from the full-pass cache
    qkv_enc [B*N, 3*H*64] -> attention output of the decoder rows [B*n_dec, H*64] (sam_attn_fwd_dec).  kv_group > 1 (beam search): qkv_enc and
    allow hold B / kv_group samples, each shared by kv_group consecutive decoder blocks (sam_attn_fwd_dec_shared)."""
    _chk(qkv_enc, BF16, "qkv_enc"); _chk(qkv_dec, BF16, "qkv_dec"); _chk(allow, torch.int32, "allow")
    d_model = qkv_enc.shape[1] // 3
    if out_dec is None:
        out_dec = torch.empty((batch * n_dec, d_model), dtype=BF16, device=qkv_enc.device)
    sh = 0 if allow.shape[1] == 1 else allow.stride(1)
    if kv_group > 1:
        capi.call("sam_attn_fwd_dec_shared", capi.ptr(qkv_enc), capi.ptr(qkv_dec), capi.ptr(allow), allow.stride(0), sh, batch, int(kv_group), n, n_dec, n_heads,
                  d_model // n_heads, float(scale), capi.ptr(out_dec), capi.stream_handle())
        return out_dec
    capi.call("sam_attn_fwd_dec", capi.ptr(qkv_enc), capi.ptr(qkv_dec), capi.ptr(allow), allow.stride(0), sh, batch, n, n_dec, n_heads, d_model // n_heads,
              float(scale), capi.ptr(out_dec), capi.stream_handle())
    return out_dec


def greedy_pick(fixed, ocr, prev_inds):
    """prev_inds[r, s + 1] = argmax over [fixed | ocr] of row (r, s), s < S - 1, in place (sa_m4c.py:299-302); fixed f32 [R*S, V], ocr f32 [R*S, No]"""
    _chk(prev_inds, torch.int64, "prev_inds")
    r, s = prev_inds.shape
    capi.call("sam_greedy_pick", capi.ptr(fixed), fixed.stride(0), capi.ptr(ocr), ocr.stride(0), r, s, fixed.shape[1], ocr.shape[1], capi.ptr(prev_inds), capi.stream_handle())
    return prev_inds


def attn_dec_row(qkv_enc, qkv_dec, allow, batch, n, n_dec, t, n_heads, scale, kv_group=1):
    """attention output of decoder row t only, bf16 [B, H*64] (sam_attn_dec_row): qkv_enc [B/kv_group * N, 3*H*64] cached by the full pass, qkv_dec
    [B*n_dec, 3*H*64] with rows 0..t of every decoder sample valid"""
    _chk(qkv_enc, BF16, "qkv_enc"); _chk(qkv_dec, BF16, "qkv_dec"); _chk(allow, torch.int32, "allow")
    d_model = qkv_enc.shape[1] // 3
    out = torch.empty((batch, d_model), dtype=BF16, device=qkv_enc.device)
    sh = 0 if allow.shape[1] == 1 else allow.stride(1)
    capi.call("sam_attn_dec_row", capi.ptr(qkv_enc), capi.ptr(qkv_dec), capi.ptr(allow), allow.stride(0), sh, batch, int(kv_group), n, n_dec, int(t), n_heads,
              d_model // n_heads, float(scale), capi.ptr(out), out.stride(0), capi.stream_handle())
    return out


def beam_step(fixed, ocr, n_samples, beam, seqs, cum, done, eos, t=0, ctl=None, prev_pos=None):
    """one BeamSearch.decode step (sam_beam_step), state (seqs int64 [B*K, S], cum f32 [B*K], done u8 [B*K]) updated in place"""
    _chk(seqs, torch.int64, "seqs"); _chk(cum, torch.float32, "cum"); _chk(done, torch.uint8, "done")
    s = seqs.shape[1]
    if beam > 1 and os.environ.get("SAM_BEAM_STEP_SPLIT", "1") != "0":
        # scan over one block per (sample, beam) + merge (sam_beam_step_split): the same result in a quarter of the time at beam 5
        ws = _workspace(int(capi.call("sam_beam_step_ws_bytes", int(n_samples), int(beam))), fixed.device, "beam_step")
        capi.call("sam_beam_step_split", capi.ptr(fixed), fixed.stride(0), capi.ptr(ocr), ocr.stride(0), int(n_samples), int(beam), s, fixed.shape[1], ocr.shape[1], int(eos),
                  int(t), capi.ptr(ctl), capi.ptr(cum), capi.ptr(done), capi.ptr(seqs), capi.ptr(prev_pos), capi.ptr(ws), capi.stream_handle())
        return
    capi.call("sam_beam_step", capi.ptr(fixed), fixed.stride(0), capi.ptr(ocr), ocr.stride(0), int(n_samples), int(beam), s, fixed.shape[1], ocr.shape[1], int(eos), int(t),
              capi.ptr(ctl), capi.ptr(cum), capi.ptr(done), capi.ptr(seqs), capi.ptr(prev_pos), capi.stream_handle())


_FUSED_MAX_N = None


def attn_bwd_fused_max_n():
    global _FUSED_MAX_N
    if _FUSED_MAX_N is None:
        _FUSED_MAX_N = int(capi.call("sam_attn_bwd_fused_max_n"))
    return _FUSED_MAX_N


def attn_bwd(dout, qkv, lse2, allow, keep, batch, n_heads, scale, p_drop=0.0, out=None, out_lo=None):
    """-> dqkv bf16 [B*N, 3*H*64].  With the forward's output and residual (attn_fwd(..., want_residual=True)) and N <= attn_bwd_fused_max_n() (384: 193..384 keys run
    as 2 x 2 sub-problems of 192) this is the one-pass kernel (sam_attn_bwd_fused); otherwise the two-kernel form (sam_attn_bwd: a dQ pass that also produces delta, then dK / dV)."""
    _chk(dout, BF16, "dout"); _chk(qkv, BF16, "qkv")
    rows, three_d = qkv.shape
    n = rows // batch
    d_model = three_d // 3
    dqkv = torch.empty_like(qkv)
    sh = 0 if allow.shape[1] == 1 else allow.stride(1)
    bits_bytes = n_heads * n * (allow.shape[-1] * 4 * (2 if keep is not None else 1) + 8)
    if out is not None and out_lo is not None and n <= attn_bwd_fused_max_n() and os.environ.get("SAM_ATTN_BWD_FUSED", "1") != "0":
        _chk(out, BF16, "out"); _chk(out_lo, BF16, "out_lo")
        capi.call("sam_attn_bwd_fused", capi.ptr(dout), capi.ptr(qkv), capi.ptr(out), capi.ptr(out_lo), capi.ptr(lse2), capi.ptr(allow), allow.stride(0), sh,
                  capi.ptr(keep), batch, n, n_heads, d_model // n_heads, float(scale), float(p_drop), capi.ptr(dqkv), capi.stream_handle(),
                  meta=dict(kernel="attn_bwd(fused)", flops=10.0 * batch * n * n * d_model, shape=(batch, n, n_heads),
                            bytes=batch * (10 * n * d_model * 2 + bits_bytes)))        # reads q,k,v,dO,O,O_lo; writes dq,dk,dv
        return dqkv
    delta = torch.empty((batch, n_heads, n), dtype=torch.float32, device=qkv.device)
    capi.call("sam_attn_bwd", capi.ptr(dout), capi.ptr(qkv), capi.ptr(lse2), capi.ptr(allow), allow.stride(0), sh,
              capi.ptr(keep), batch, n, n_heads, d_model // n_heads, float(scale), float(p_drop), capi.ptr(dqkv), capi.ptr(delta),
              capi.stream_handle(),
              meta=dict(kernel="attn_bwd(dq+dkdv)", flops=10.0 * batch * n * n * d_model, shape=(batch, n, n_heads),
                        bytes=batch * (8 * n * d_model * 2 + bits_bytes)))
    return dqkv


# ----------------------------------------------------------------------------- GEMM
def _dp(t):
    return None if t is None else t.data_ptr()


def gemm(a, b, *, a_kcontig=True, b_kcontig=True, m=None, n=None, k=None, out=None, out_dtype=BF16, epilogue=capi.EPI_NONE,
         bias=None, residual=None, aux_out=None, aux_in=None, accumulate=False, p_drop=0.0, seed=0, offset=0, split_k=0, bias_grad=None, force_tile=0, ln=None):
    """C[M,N] = epilogue(sum_k A(m,k) B(k,n)); see include/sam_hip.h `sam_gemm_bf16` for layouts and epilogues.
    a, b: 2-D bf16 tensors whose LAST dim is contiguous (row stride = leading dimension)."""
    for t, nm in ((a, "A"), (b, "B")):
        if not t.is_cuda or t.dtype != BF16 or t.dim() != 2 or t.stride(1) != 1:
            raise capi.SamHipError("gemm %s: need a 2-D bf16 GPU tensor with contiguous last dim" % nm)
    M = m if m is not None else (a.shape[0] if a_kcontig else a.shape[1])
    K = k if k is not None else (a.shape[1] if a_kcontig else a.shape[0])
    N = n if n is not None else (b.shape[0] if b_kcontig else b.shape[1])
    if out is None:
        out = torch.empty((M, N), dtype=out_dtype, device=a.device)
    d = capi.GemmDesc()
    d.M, d.N, d.K = M, N, K
    d.a_kcontig, d.b_kcontig = int(a_kcontig), int(b_kcontig)
    d.c_is_f32, d.accumulate, d.epilogue = int(out.dtype == torch.float32), int(accumulate), int(epilogue)
    d.A, d.lda, d.B, d.ldb, d.C, d.ldc = a.data_ptr(), a.stride(0), b.data_ptr(), b.stride(0), out.data_ptr(), out.stride(0)
    d.bias = _dp(bias)
    d.residual, d.ldr = _dp(residual), (residual.stride(0) if residual is not None else 0)
    d.aux_out, d.aux_in = _dp(aux_out), _dp(aux_in)
    aux = aux_out if aux_out is not None else aux_in
    d.ld_aux = aux.stride(0) if aux is not None else 0
    d.p_drop, d.seed, d.offset = float(p_drop), int(seed), int(offset)
    wgrad_split = bool(accumulate) and out.dtype == torch.float32 and epilogue == capi.EPI_NONE      # partials reduced INTO C by sam_gemm_splitk_reduce
    if split_k == 0 and not accumulate and bias_grad is None and force_tile == 0 and M <= 4096 and K >= 1536 and M * N <= (4 << 20):
        split_k = -1       # skinny problem with a long K (TextBert's 20 tokens/sample, classifier dgrad): let the library split K and fold
                           # the epilogue into the partial-sum reduction (it declines when the grid already fills the chip)
    d.split_k, d.bias_grad, d.force_tile = int(split_k), _dp(bias_grad), int(force_tile)
    if ln is not None:          # capi.LnFuse, filled by gemm_ln: the library normalises the rows itself when it runs this GEMM split over K
        d.ln = C.pointer(ln)
    if split_k not in (0, 1):
        want = split_k if split_k > 0 else (32 if wgrad_split else 8)
        ws = _workspace(min(want * (M * N + M) * 4, 96 << 20), a.device, "splitk")
        d.ws, d.ws_bytes, d.defer_reduce = ws.data_ptr(), ws.numel() * 4, 1
    capi.call("sam_gemm_bf16", d, capi.stream_handle(),
              meta=dict(kernel="gemm<a_kc=%d,b_kc=%d,epi=%d,f32=%d>" % (d.a_kcontig, d.b_kcontig, d.epilogue, d.c_is_f32), flops=2.0 * M * N * K, shape=(M, N, K)))
    if d.split_k_used > 1 and wgrad_split:   # the fixed-order reduction of the split-K partials is its own launch (and its own profile row)
        capi.call("sam_gemm_splitk_reduce", d.ws, d.split_k_used, M, N, out.data_ptr(), out.stride(0), d.bias_grad, capi.stream_handle(),
                  meta=dict(kernel="splitk_reduce", bytes=4.0 * M * N * (d.split_k_used + 2)))
    return out


def gemm_ln(a, b, gamma, beta, eps, **kw):
    """LayerNorm(gemm(a, b, epilogue=EPI_BIAS_DROPOUT_RES, ...)) -> (z, y, mean, rstd): z = the pre-LayerNorm sums (bf16, what the backward reads), y / mean /
    rstd as layernorm_fwd(z).  One launch less when the GEMM runs split over K (sam_ln_fuse: the reduction pass normalises the rows it owns); the
    separate sam_layernorm_fwd otherwise -- the same bits either way."""
    m = a.shape[0] if kw.get("a_kcontig", True) else a.shape[1]
    n = b.shape[0] if kw.get("b_kcontig", True) else b.shape[1]
    if capi.profiler is not None or n % 4 or n > 2048 or gamma.dtype != torch.float32 or beta.dtype != torch.float32:
        z = gemm(a, b, **kw)
        return (z,) + tuple(layernorm_fwd(z, gamma, beta, eps))
    y = torch.empty((m, n), dtype=BF16, device=a.device)
    mean = torch.empty((m,), dtype=torch.float32, device=a.device)
    rstd = torch.empty((m,), dtype=torch.float32, device=a.device)
    ln = capi.LnFuse()
    ln.gamma, ln.beta, ln.eps, ln.y, ln.ldy, ln.mean, ln.rstd, ln.done = gamma.data_ptr(), beta.data_ptr(), float(eps), y.data_ptr(), y.stride(0), mean.data_ptr(), rstd.data_ptr(), 0
    if m >= 2048:          # MMT-size products: the exchange workspace of the LayerNorm inside the launch (zero-filled once per device and stream; sam_ln_fuse.xws)
        xws = _ln_xws(a.device, int(capi.call("sam_gemm_ln_ws_bytes", m, n)))
        ln.xws, ln.xws_bytes = xws.data_ptr(), xws.numel() * 4
    z = gemm(a, b, ln=ln, **kw)
    if ln.done:
        return z, y, mean, rstd
    return (z,) + tuple(layernorm_fwd(z, gamma, beta, eps))


# ----------------------------------------------------------------------------- scratch
_WS = {}
_LN_XWS = {}


def _ln_xws(device, nbytes):
    """per-(device, stream) exchange workspace of the in-launch LayerNorm: zero-filled when (re)allocated, left with zero counters by every launch"""
    key = (device, capi.stream_handle().value)
    buf = _LN_XWS.get(key)
    if buf is None or buf.numel() * 4 < nbytes:
        buf = torch.zeros((nbytes + 3) // 4, dtype=torch.float32, device=device)
        _LN_XWS[key] = buf
    return buf


def capi_ln_words():
    """words in front of the (mean, M2) pairs of an in-launch LayerNorm workspace: error word + counters (csrc/gemm_common.h: LN_WS_PART0)"""
    return 64 + 4 * 1024


def ln_xws_check():
    """raise if a launch's bounded wait for a row's statistics ran out (word 0 of a workspace); synchronises"""
    for buf in _LN_XWS.values():
        if int(buf[:1].view(torch.int32).item()) != 0:
            buf[:1].zero_()
            raise capi.SamHipError("LayerNorm inside the GEMM launch: a block waited in vain for the other parts of its rows (another kernel held the CUs its partners needed)")


def _workspace(nbytes, device, tag):
    """per-(device, stream, tag) scratch that only grows; the kernels that use one buffer are ordered by its stream (TextBert runs on a
    side stream next to the object / OCR encoders: each stream gets its own scratch)"""
    key = (device, capi.stream_handle().value, tag)
    buf = _WS.get(key)
    if buf is None or buf.numel() * 4 < nbytes:
        buf = torch.empty((nbytes + 3) // 4, dtype=torch.float32, device=device)
        _WS[key] = buf
    return buf


# ----------------------------------------------------------------------------- layernorm / reductions
def layernorm_fwd(x, gamma, beta, eps):
    """x [M,D] bf16 or fp32 (last dim contiguous) -> (y bf16 [M,D], mean f32 [M], rstd f32 [M])"""
    if x.dim() != 2 or x.stride(1) != 1 or x.dtype not in (BF16, torch.float32) or not x.is_cuda:
        raise capi.SamHipError("layernorm_fwd: need a 2-D bf16/fp32 GPU tensor with contiguous rows")
    m, d = x.shape
    y = torch.empty((m, d), dtype=BF16, device=x.device)
    mean = torch.empty(m, dtype=torch.float32, device=x.device)
    rstd = torch.empty(m, dtype=torch.float32, device=x.device)
    capi.call("sam_layernorm_fwd", capi.ptr(x), int(x.dtype == torch.float32), x.stride(0), capi.ptr(gamma), capi.ptr(beta), float(eps), m, d,
              capi.ptr(y), y.stride(0), capi.ptr(mean), capi.ptr(rstd), capi.stream_handle())
    return y, mean, rstd


class LnFinalizeQueue:
    """deferred LayerNorm-backward finalizes of the per-kernel (ctypes) route: see sam_layernorm_bwd_finalize_batch in include/sam_hip.h.  The Trainer
    switches deferral on for the span of a backward pass and flushes before the gradient norm; the C++ custom ops keep their own queue
    (torch.ops.sam_hip.set_ln_defer / ln_finalize_flush)."""
    defer = False
    items = []      # (ws tensor, rows, accumulate, dgamma, dbeta, dbias, D)

    @classmethod
    def flush(cls):
        if not cls.items:
            return
        by_d = {}
        for it in cls.items:
            by_d.setdefault(it[6], []).append(it)
        for d, its in by_d.items():
            arr = (capi.LnFinalizeItem * len(its))()
            for a, (ws, rows, acc, dg, db, dbias, _) in zip(arr, its):
                a.ws, a.rows, a.accumulate, a.dgamma, a.dbeta, a.dbias = ws.data_ptr(), rows, acc, dg.data_ptr(), db.data_ptr(), _dp(dbias)
            capi.call("sam_layernorm_bwd_finalize_batch", arr, len(its), d, capi.stream_handle())
        cls.items = []

    @classmethod
    def clear(cls):
        """drop queued finalizes without running them (a backward pass that raised: their workspaces may be gone)"""
        cls.items = []
        cls.defer = False


def layernorm_bwd(dy, x, mean, rstd, gamma, dgamma, dbeta, dbias=None, want_dropped=False, p_drop=0.0, seed=0, offset=0, accumulate=True, may_defer=False):
    """-> (dx bf16, dx_dropped bf16 or None); dgamma/dbeta/dbias (fp32 [D]) are accumulated in place (overwritten with accumulate=False).
    may_defer: the parameter-gradient reduction may be left to LnFinalizeQueue.flush() when deferral is on"""
    _chk(dy, BF16, "dy")
    m, d = x.shape
    dx = torch.empty((m, d), dtype=BF16, device=x.device)
    dxd = torch.empty((m, d), dtype=BF16, device=x.device) if (want_dropped and p_drop > 0) else None
    defer = may_defer and LnFinalizeQueue.defer
    nbytes = capi.call("sam_layernorm_bwd_ws_bytes", d)
    ws = torch.empty(((nbytes + 3) // 4,), dtype=torch.float32, device=x.device) if defer else _workspace(nbytes, x.device, "ln")
    capi.call("sam_layernorm_bwd", capi.ptr(dy), dy.stride(0), capi.ptr(x), int(x.dtype == torch.float32), x.stride(0), capi.ptr(mean), capi.ptr(rstd),
              capi.ptr(gamma), m, d, capi.ptr(dx), capi.ptr(dxd), dx.stride(0), float(p_drop), int(seed), int(offset), capi.ptr(dgamma), capi.ptr(dbeta),
              capi.ptr(dbias), int(bool(accumulate)) | (4 if defer else 0), capi.ptr(ws), capi.stream_handle())
    if defer:
        LnFinalizeQueue.items.append((ws, int(capi.call("sam_layernorm_bwd_partial_rows", m)), int(bool(accumulate)), dgamma, dbeta, dbias, d))
    return dx, (dxd if dxd is not None else (dx if want_dropped else None))


def add_dropout(a, b, p_drop, seed=0, offset=0):
    """dropout(a + b) -> bf16 [M, D] (b may be None: plain dropout, which is also its own backward on dy); hidden-state dropout stream"""
    for name, t in (("a", a), ("b", b)):
        if t is not None and (not t.is_cuda or t.dtype != BF16 or t.dim() != 2 or t.stride(1) != 1):
            raise capi.SamHipError("add_dropout: %s must be a bf16 [M, D] GPU tensor with unit column stride" % name)
    m, d = a.shape
    out = torch.empty((m, d), dtype=BF16, device=a.device)
    capi.call("sam_add_dropout_bf16", capi.ptr(a), a.stride(0), capi.ptr(b), 0 if b is None else b.stride(0), capi.ptr(out), out.stride(0), m, d,
              float(p_drop), int(seed), int(offset), capi.stream_handle())
    return out


def input_encoder_fwd(za, bbox, wb, bias_b, ln_a, ln_b, p_drop=0.0, seed=0, offset=0):
    """dropout(LN_a(za) + LN_b(bbox W_b^T + b_b)) -> (out bf16 [R, D], stats f32 [R, 4]); za bf16 [R, D], bbox fp32 [R, >= 4] (row stride free),
    wb bf16 [D, ldw] (sam_input_encoder_fwd)"""
    _chk(za, BF16, "za")
    if not bbox.is_cuda or bbox.dtype != torch.float32 or bbox.dim() != 2 or bbox.stride(1) != 1 or bbox.shape[1] < 4:
        raise capi.SamHipError("input_encoder_fwd: bbox must be a 2-D fp32 GPU tensor with >= 4 contiguous columns")
    r, d = za.shape
    out = torch.empty((r, d), dtype=BF16, device=za.device)
    stats = torch.empty((r, 4), dtype=torch.float32, device=za.device)
    capi.call("sam_input_encoder_fwd", capi.ptr(za), za.stride(0), capi.ptr(bbox), bbox.stride(0), capi.ptr(wb), wb.stride(0), capi.ptr(bias_b), capi.ptr(ln_a.weight),
              capi.ptr(ln_a.bias), capi.ptr(ln_b.weight), capi.ptr(ln_b.bias), float(ln_a.variance_epsilon), r, d, float(p_drop), int(seed), int(offset), capi.ptr(out),
              out.stride(0), capi.ptr(stats), capi.stream_handle())
    return out, stats


def input_encoder_bwd(dy, za, bbox, wb, bias_b, ln_a, ln_b, stats, dwb, dbias_b, p_drop=0.0, seed=0, offset=0, accumulate=True):
    """-> d za bf16 [R, D]; d gamma / d beta of both LayerNorms, d bias_b and d wb (fp32 [D, ldgw] view, columns 0..3) are accumulated in place"""
    _chk(dy, BF16, "dy")
    r, d = za.shape
    dza = torch.empty((r, d), dtype=BF16, device=za.device)
    ws = _workspace(capi.call("sam_input_encoder_bwd_ws_bytes", r, d), za.device, "enc_in")
    capi.call("sam_input_encoder_bwd", capi.ptr(dy), dy.stride(0), capi.ptr(za), za.stride(0), capi.ptr(bbox), bbox.stride(0), capi.ptr(wb), wb.stride(0), capi.ptr(bias_b),
              capi.ptr(ln_a.weight), capi.ptr(ln_b.weight), capi.ptr(stats), r, d, float(p_drop), int(seed), int(offset), capi.ptr(dza), dza.stride(0),
              capi.ptr(ln_a.weight.grad), capi.ptr(ln_a.bias.grad), capi.ptr(ln_b.weight.grad), capi.ptr(ln_b.bias.grad), capi.ptr(dbias_b), capi.ptr(dwb), dwb.stride(0),
              int(bool(accumulate)), capi.ptr(ws), capi.stream_handle())
    return dza


def colsum(x, out, accumulate=True):
    """out[n] (+)= sum_m x[m,n]  (x bf16 [M,N], out fp32 [N])"""
    m, n = x.shape
    ws = _workspace(capi.call("sam_colsum_ws_bytes", n), x.device, "colsum")
    capi.call("sam_colsum_bf16", capi.ptr(x), x.stride(0), m, n, capi.ptr(out), int(accumulate), capi.ptr(ws), capi.stream_handle())
    return out


# ----------------------------------------------------------------------------- front end (csrc/embed.hip)
def l2norm_pack(x, out, col0=0, normalize=True, zero_upto=0, eps=1e-12):
    """out[:, col0:col0+D] = bf16(F.normalize(x, dim=-1)) (normalize=False: plain cast); x fp32 [M, D]; out bf16 [M, ldo];
    columns [col0+D, zero_upto) of out are zeroed"""
    _chk(out, BF16, "out")
    if not x.is_cuda or x.dtype != torch.float32 or x.dim() != 2:
        raise capi.SamHipError("l2norm_pack: x must be a 2-D fp32 GPU tensor")
    m, d = x.shape
    if x.stride(1) != 1 or out.stride(1) != 1 or out.shape[0] != m:
        raise capi.SamHipError("l2norm_pack: x / out must be row-major with the same number of rows")
    capi.call("sam_l2norm_pack_bf16", capi.ptr(x), x.stride(0), m, d, int(bool(normalize)), float(eps), capi.ptr(out), out.stride(0), int(col0), int(zero_upto),
              capi.stream_handle())
    return out


def embed_sum_fwd(pos, tt, rows, seq, table=None, ids=None, type_ids=None):
    """fp32 [rows, D] = table[ids] (bf16, optional) + pos[r % seq] + tt[type_ids[r]] (type 0 when type_ids is None)"""
    d = pos.shape[1]
    out = torch.empty((rows, d), dtype=torch.float32, device=pos.device)
    capi.call("sam_embed_sum_fwd", capi.ptr(table), table.stride(0) if table is not None else 0, capi.ptr(ids), table.shape[0] if table is not None else 0,
              capi.ptr(pos), pos.stride(0), int(seq), capi.ptr(tt), tt.stride(0), capi.ptr(type_ids), tt.shape[0], rows, d, capi.ptr(out), out.stride(0),
              capi.stream_handle())
    return out


def embed_sum_bwd(d_e, seq, d_pos, d_tt, type_ids=None, n_types=1):
    """d_pos[s] += sum_b d_e[b*seq+s];  d_tt[t] += sum_{type==t} d_e  (d_e bf16 [R, D]; d_pos / d_tt fp32 gradient rows, accumulated)"""
    _chk(d_e, BF16, "d_e")
    r, d = d_e.shape
    ws = _workspace(capi.call("sam_embed_sum_bwd_ws_bytes", int(seq), int(n_types), d), d_e.device, "embed")
    capi.call("sam_embed_sum_bwd", capi.ptr(d_e), d_e.stride(0), r, d, int(seq), capi.ptr(type_ids), int(n_types), capi.ptr(d_pos), d_pos.stride(0),
              capi.ptr(d_tt), d_tt.stride(0), capi.ptr(ws), capi.stream_handle())


def gather2_add_fwd(ans, ocr, inds, n_ocr, emb=None, p_drop=0.0, seed=0, offset=0):
    """bf16 [B*S, D] = (ind < V ? ans[ind] : ocr[b*n_ocr + ind - V]) + dropout(emb);  ans bf16 [V,D], ocr bf16 [B*n_ocr,D], inds int64 [B,S]"""
    _chk(ans, BF16, "ans"); _chk(ocr, BF16, "ocr"); _chk(inds, torch.int64, "inds")
    b, s = inds.shape
    v, d = ans.shape
    out = torch.empty((b * s, d), dtype=BF16, device=ans.device)
    capi.call("sam_gather2_add_fwd", capi.ptr(ans), ans.stride(0), v, capi.ptr(ocr), ocr.stride(0), int(n_ocr), capi.ptr(inds), b, s, d, capi.ptr(emb),
              emb.stride(0) if emb is not None else 0, float(p_drop), int(seed), int(offset), capi.ptr(out), out.stride(0), capi.stream_handle())
    return out


def gather2_add_bwd(dy, inds, v, n_ocr, want_emb=True, p_drop=0.0, seed=0, offset=0):
    """-> (d_ans fp32 [V,D], d_ocr fp32 [B*n_ocr,D], d_emb bf16 [B*S,D] | None)"""
    _chk(dy, BF16, "dy")
    b, s = inds.shape
    d = dy.shape[1]
    d_ans = torch.empty((v, d), dtype=torch.float32, device=dy.device)
    d_ocr = torch.empty((b * n_ocr, d), dtype=torch.float32, device=dy.device)
    copy_blocks([(None, d_ans.view(1, 1, -1)), (None, d_ocr.view(1, 1, -1))])       # both atomics buffers cleared by one launch
    d_emb = torch.empty((b * s, d), dtype=BF16, device=dy.device) if want_emb else None
    capi.call("sam_gather2_add_bwd", capi.ptr(dy), dy.stride(0), int(v), int(n_ocr), capi.ptr(inds), b, s, d, capi.ptr(d_ans), d_ans.stride(0), capi.ptr(d_ocr),
              d_ocr.stride(0), float(p_drop), int(seed), int(offset), capi.ptr(d_emb), d_emb.stride(0) if want_emb else 0, capi.stream_handle())
    return d_ans, d_ocr, d_emb


# ----------------------------------------------------------------------------- loss / pointer net / optimizer
def bce_loss(fixed, ocr, targets, loss_mask, grad_scale=1.0, global_count=None):
    """fixed f32 [R,V], ocr f32 [R,No], targets f32 [R,V+No], loss_mask f32 [R] -> (loss f32 [1], d_fixed bf16 [R,V], d_ocr f32 [R,No]);
    global_count (device f32 scalar): the all-reduced number of unmasked steps of the global batch, used as the normaliser instead of this rank's"""
    r, v = fixed.shape
    no = ocr.shape[1]
    t_ = _tops()
    if t_ is not None and loss_mask.is_contiguous():
        return t_.bce_loss(fixed, ocr, targets, loss_mask, float(grad_scale), global_count)
    loss = torch.empty(1, dtype=torch.float32, device=fixed.device)
    d_fixed = torch.empty((r, v), dtype=BF16, device=fixed.device)
    d_ocr = torch.empty((r, no), dtype=torch.float32, device=fixed.device)
    capi.call("sam_bce_loss", capi.ptr(fixed), fixed.stride(0), capi.ptr(ocr), ocr.stride(0), capi.ptr(targets), targets.stride(0), capi.ptr(loss_mask),
              r, v, no, float(grad_scale), capi.ptr(global_count), capi.ptr(loss), capi.ptr(d_fixed), d_fixed.stride(0), capi.ptr(d_ocr), d_ocr.stride(0), capi.stream_handle())
    return loss, d_fixed, d_ocr


def ptr_scores_fwd(q, k, ocr_mask_u8, scale):
    """q bf16 [B,S,D], k bf16 [B,No,D], mask u8 [B,No] -> f32 [B,S,No]"""
    b, s, d = q.shape
    no = k.shape[1]
    t_ = _tops()
    if t_ is not None:
        return t_.ptr_scores(q, k, ocr_mask_u8, float(scale))
    out = torch.empty((b, s, no), dtype=torch.float32, device=q.device)
    capi.call("sam_ptr_scores_fwd", capi.ptr(q), capi.ptr(k), capi.ptr(ocr_mask_u8), b, s, no, d, float(scale), capi.ptr(out), out.stride(0), out.stride(1),
              capi.stream_handle())
    return out


def ptr_scores_bwd(dscores, q, k, scale):
    b, s, d = q.shape
    no = k.shape[1]
    t_ = _tops()
    if t_ is not None:
        return t_.ptr_scores_bwd(dscores, q, k, float(scale))
    dq, dk = torch.empty_like(q), torch.empty_like(k)
    capi.call("sam_ptr_scores_bwd", capi.ptr(dscores), dscores.stride(0), dscores.stride(1), capi.ptr(q), capi.ptr(k), b, s, no, d, float(scale),
              capi.ptr(dq), capi.ptr(dk), capi.stream_handle())
    return dq, dk


def _sparse_struct(sparse):
    """sparse = (lo, hi, row_len, touched uint8 tensor) or None -> capi.SparseRows or None (NULL); the caller holds it for the duration of the call"""
    if sparse is None:
        return None
    s = capi.SparseRows()
    s.lo, s.hi, s.row_len, s.touched = int(sparse[0]), int(sparse[1]), int(sparse[2]), sparse[3].data_ptr()
    return s


def sumsq(g, out, sparse=None):
    """out[0] = sum g^2; sparse = (lo, hi, row_len, touched): rows of that region whose flag is 0 are skipped (sam_sparse_rows)"""
    t_ = _tops()
    if t_ is not None:
        t_.sumsq(g, out, list(sparse[:3]) if sparse else [], sparse[3] if sparse else None)
        return out
    ws = _workspace(capi.call("sam_sumsq_ws_bytes"), g.device, "sumsq")
    sp = _sparse_struct(sparse)
    capi.call("sam_sumsq_f32", capi.ptr(g), g.numel(), sp, capi.ptr(out), capi.ptr(ws), capi.stream_handle())
    return out


def adam_step(p, g, m, v, p_bf16, seg_end, seg_lr, step, gnorm_sq=None, max_norm=0.0, betas=(0.9, 0.999), eps=1e-8, sparse=None):
    t_ = _tops()
    if t_ is not None:
        t_.adam_step(p, g, m, v, p_bf16, [int(e) for e in seg_end], [float(l) for l in seg_lr], int(step), float(betas[0]), float(betas[1]), float(eps), gnorm_sq,
                     float(max_norm), None, list(sparse[:3]) if sparse else [], sparse[3] if sparse else None)
        return
    n = len(seg_end)
    ends = (C.c_int64 * n)(*[int(e) for e in seg_end])
    lrs = (C.c_float * n)(*[float(l) for l in seg_lr])
    sp = _sparse_struct(sparse)
    capi.call("sam_adam_step", capi.ptr(p), capi.ptr(g), capi.ptr(m), capi.ptr(v), capi.ptr(p_bf16), p.numel(), ends, lrs, n, float(betas[0]), float(betas[1]),
              float(eps), int(step), capi.ptr(gnorm_sq), float(max_norm), sp, capi.stream_handle())


def adam_step_dev(p, g, m, v, p_bf16, seg_end, dev_sched, gnorm_sq=None, max_norm=0.0, betas=(0.9, 0.999), eps=1e-8, sparse=None):
    """adam_step with the schedule [lr per segment, 1 - beta1^t, 1 - beta2^t] read from the device tensor `dev_sched` (graph-captured steps)"""
    t_ = _tops()
    if t_ is not None:
        t_.adam_step(p, g, m, v, p_bf16, [int(e) for e in seg_end], [], 0, float(betas[0]), float(betas[1]), float(eps), gnorm_sq, float(max_norm), dev_sched,
                     list(sparse[:3]) if sparse else [], sparse[3] if sparse else None)
        return
    n = len(seg_end)
    ends = (C.c_int64 * n)(*[int(e) for e in seg_end])
    sp = _sparse_struct(sparse)
    capi.call("sam_adam_step_dev", capi.ptr(p), capi.ptr(g), capi.ptr(m), capi.ptr(v), capi.ptr(p_bf16), p.numel(), ends, n, float(betas[0]), float(betas[1]),
              float(eps), capi.ptr(dev_sched), capi.ptr(gnorm_sq), float(max_norm), sp, capi.stream_handle())


def adam_step_range(p, g, m, v, p_bf16, seg_end, dev_sched, lo, hi, gnorm_sq=None, max_norm=0.0, betas=(0.9, 0.999), eps=1e-8, sparse=None, zero_grad=True, gate=None,
                    max_blocks=0):
    """adam_step_dev over the elements [lo, hi) only (sam_adam_step_range): the update in pieces, each on the stream that needs it; `zero_grad`: the piece's
    gradient is cleared after use; `gate`: int32 device scalar, 0 = the launch does nothing"""
    n = len(seg_end)
    ends = (C.c_int64 * n)(*[int(e) for e in seg_end])
    sp = _sparse_struct(sparse)          # (the row-sparse region is walked by the piece that contains it)
    capi.call("sam_adam_step_range", capi.ptr(p), capi.ptr(g), capi.ptr(m), capi.ptr(v), capi.ptr(p_bf16), p.numel(), ends, n, float(betas[0]), float(betas[1]),
              float(eps), capi.ptr(dev_sched), capi.ptr(gnorm_sq), float(max_norm), sp, int(lo), int(hi), int(bool(zero_grad)), capi.ptr(gate), int(max_blocks), capi.stream_handle())


def copy_blocks(blocks):
    """up to 8 strided copies / casts / accumulations / zero-fills in one launch (sam_copy_blocks).  Each block: (src | None, dst, accumulate=False) with
    src / dst 3-D views [batches, rows, cols] (any batch / row stride, unit column stride, bf16 or fp32); src None fills dst with zeros."""
    for i in range(0, len(blocks), 8):
        part = blocks[i: i + 8]
        arr = (capi.CopyDesc * len(part))()
        for e, blk in zip(arr, part):
            src, dst = blk[0], blk[1]
            acc = bool(blk[2]) if len(blk) > 2 else False
            if dst.dim() != 3 or dst.stride(2) != 1 or dst.dtype not in (BF16, torch.float32) or not dst.is_cuda:
                raise capi.SamHipError("copy_blocks: dst must be a 3-D bf16 / fp32 GPU view with unit column stride")
            if src is not None and (src.shape != dst.shape or src.stride(2) != 1 or src.dtype not in (BF16, torch.float32) or not src.is_cuda):
                raise capi.SamHipError("copy_blocks: src must match dst's shape, bf16 / fp32, unit column stride")
            e.src, e.dst = (src.data_ptr() if src is not None else None), dst.data_ptr()
            e.batches, e.rows, e.cols = dst.shape
            e.src_batch_stride, e.src_row_stride = (src.stride(0), src.stride(1)) if src is not None else (0, 0)
            e.dst_batch_stride, e.dst_row_stride = dst.stride(0), dst.stride(1)
            e.src_f32, e.dst_f32, e.accumulate = int(src is not None and src.dtype == torch.float32), int(dst.dtype == torch.float32), int(acc)
        capi.call("sam_copy_blocks", arr, len(part), capi.stream_handle())


def rowvec(mode, a, b=None, vec=None):
    """bf16 rows: "mul" a * b | "add_vec" a + vec[cols] | "mul_vec" a * vec[cols] (vec fp32) -> bf16 [rows, cols] (include/sam_hip.h: sam_rowvec_bf16)"""
    m = {"mul": 0, "add_vec": 1, "mul_vec": 2}[mode]
    _chk(a, BF16, "a")
    if a.dim() != 2 or a.stride(1) != 1:
        raise capi.SamHipError("rowvec: a must be 2-D with contiguous rows")
    if m == 0:
        if b is None:
            raise capi.SamHipError("rowvec mul: the second operand is missing")
        _chk(b, BF16, "b")
        if b.shape != a.shape or b.stride(1) != 1:
            raise capi.SamHipError("rowvec mul: b must have a's shape and contiguous rows")
    else:
        if vec is None:
            raise capi.SamHipError("rowvec %s: the fp32 vector is missing" % mode)
        _chk(vec, torch.float32, "vec")
        if vec.numel() != a.shape[1] or not vec.is_contiguous():
            raise capi.SamHipError("rowvec: vec must be a contiguous fp32 vector of a's width")
    out = torch.empty(a.shape, dtype=BF16, device=a.device)
    capi.call("sam_rowvec_bf16", m, capi.ptr(a), a.stride(0), capi.ptr(b), b.stride(0) if b is not None else 0, capi.ptr(vec), capi.ptr(out), out.stride(0),
              a.shape[0], a.shape[1], capi.stream_handle(), meta=dict(kernel="rowvec", bytes=2.0 * a.numel() * (3 if m == 0 else 2)))
    return out


def ge_u8(x, threshold):
    """uint8 [n] = x >= threshold for an int64 tensor (token types of the previous predictions, sa_m4c.py:936)"""
    _chk(x, torch.int64, "x")
    out = torch.empty(x.numel(), dtype=torch.uint8, device=x.device)
    capi.call("sam_ge_u8", capi.ptr(x), x.numel(), int(threshold), capi.ptr(out), capi.stream_handle())
    return out


def greedy_decode_ws(batch, steps, n_layers, device):
    """zero-filled workspace of sam_greedy_decode_steps for `batch` rows (int32 word 256 = its sticky error flag)"""
    nbytes = capi.call("sam_greedy_decode_ws_bytes", int(batch), int(steps), int(n_layers))
    return torch.zeros((nbytes + 3) // 4, dtype=torch.int32, device=device)


def tile_weight(w):
    """bf16 [N, K] (any row stride) -> the fragment-tiled copy [ceil(N / 16), K / 8, 16, 8] sam_greedy_decode_steps reads (rows zero-padded to 16)"""
    n, k = w.shape
    if k % 8:
        raise capi.SamHipError("tile_weight: K must be a multiple of 8")
    npad = (n + 15) // 16 * 16
    if npad != n:
        w = torch.cat([w, w.new_zeros((npad - n, k))], dim=0)
    return w.reshape(npad // 16, 16, k // 8, 8).permute(0, 2, 1, 3).contiguous()


def greedy_decode_steps(layers, d, ws, t_begin, t_end):
    """greedy decoding steps t_begin .. t_end-1 in one persistent launch (sam_greedy_decode_steps, include/sam_hip.h).
    layers: per encoder layer a dict of tensors {wqkv, wo, w1, w2 (bf16, fragment-tiled: tile_weight), bqkv, bo, b1, b2, ln1_g, ln1_b, ln2_g, ln2_b (fp32), qkv (bf16 [B*N, 3D] cache),
    allow (int32 bits [B, Hm, N, NW])}; d: dict with the scalar fields and tensors of sam_decode_desc.  Raises SamHipError(UNSUPPORTED) for shapes the
    kernel is not built for."""
    arr = (capi.DecodeLayer * len(layers))()
    for e, l in zip(arr, layers):
        for k in ("wqkv", "wo", "w1", "w2"):
            _chk(l[k], BF16, k)
            if l[k].dim() != 4 or l[k].shape[2:] != (16, 8):
                raise capi.SamHipError("greedy_decode_steps: %s must be fragment-tiled (ops.tile_weight)" % k)
        _chk(l["qkv"], BF16, "qkv")
        for k in ("wqkv", "wo", "w1", "w2", "bqkv", "bo", "b1", "b2", "ln1_g", "ln1_b", "ln2_g", "ln2_b", "qkv", "allow"):
            setattr(e, k, l[k].data_ptr())
        al = l["allow"]
        e.allow_stride_b, e.allow_stride_h = al.stride(0), (0 if al.shape[1] == 1 else al.stride(1))
    desc = capi.DecodeDesc()
    for k in ("n_layers", "B", "N", "n_enc", "S", "H", "D", "F", "V", "No"):
        setattr(desc, k, int(d[k]))
    desc.t_begin, desc.t_end = int(t_begin), int(t_end)
    for k in ("scale", "ln_eps", "emb_ln_eps", "ptr_scale"):
        setattr(desc, k, float(d[k]))
    desc.layers = arr
    for k in ("pos_emb", "type_emb", "emb_ln_g", "emb_ln_b", "bc", "bq", "fixed_scores", "ocr_scores"):
        _chk(d[k], torch.float32, k)
    for k in ("ans_ln", "ocr_ln", "wc", "wq", "ptr_k"):
        _chk(d[k], BF16, k)
    _chk(d["prev_inds"], torch.int64, "prev_inds"); _chk(d["ocr_mask"], torch.uint8, "ocr_mask")
    for k in ("pos_emb", "type_emb", "emb_ln_g", "emb_ln_b", "ans_ln", "ocr_ln", "wc", "bc", "wq", "bq", "ptr_k", "ocr_mask", "prev_inds", "fixed_scores", "ocr_scores"):
        setattr(desc, k, d[k].data_ptr())
    desc.seq_out = d["seq_out"].data_ptr() if d.get("seq_out") is not None else None
    for k in ("wc", "wq"):
        if d[k].dim() != 4 or d[k].shape[2:] != (16, 8):
            raise capi.SamHipError("greedy_decode_steps: %s must be fragment-tiled (ops.tile_weight)" % k)
    desc.ld_pos, desc.ld_type, desc.ld_fixed = d["pos_emb"].stride(0), d["type_emb"].stride(0), int(d["ld_fixed"])
    capi.call("sam_greedy_decode_steps", desc, capi.ptr(ws), ws.numel() * ws.element_size(), capi.stream_handle())


def step_advance(rng_state, offset_stride, step_counter, base_lrs, dev_sched, betas=(0.9, 0.999), warmup_iters=1000, warmup_factor=0.2,
                 lr_decay_iters=(14000, 19000), lr_decay=0.1):
    """head node of a captured training step (sam_step_advance): rng_state[1] += offset_stride; t = ++step_counter[0];
    dev_sched = [base_lr * lambda(t - 1) per segment, 1 - beta1^t, 1 - beta2^t], all in device memory"""
    t_ = _tops()
    if t_ is not None:
        t_.step_advance(rng_state, int(offset_stride), step_counter, [float(l) for l in base_lrs], int(warmup_iters), float(warmup_factor),
                        [int(i) for i in lr_decay_iters], float(lr_decay), float(betas[0]), float(betas[1]), dev_sched)
        return
    sc = capi.LrSchedule()
    sc.nseg = len(base_lrs)
    for i, l in enumerate(base_lrs):
        sc.base_lr[i] = float(l)
    sc.warmup_iters, sc.warmup_factor, sc.n_decay, sc.lr_decay = int(warmup_iters), float(warmup_factor), len(lr_decay_iters), float(lr_decay)
    for i, it in enumerate(lr_decay_iters):
        sc.decay_iters[i] = int(it)
    sc.beta1, sc.beta2 = float(betas[0]), float(betas[1])
    capi.call("sam_step_advance", capi.ptr(rng_state), int(offset_stride), capi.ptr(step_counter), sc, capi.ptr(dev_sched),
              capi.stream_handle())


def set_cu_reserve(n):
    """CUs withheld from every persistent grid of the training step (include/sam_hip.h: sam_set_cu_reserve); returns the value in force (a multiple of 8).
    Grids already captured into a hipGraph keep what they were captured with: set it BEFORE the Trainer's first captured step."""
    capi.call("sam_set_cu_reserve", int(n))
    return cu_reserve()


def cu_reserve():
    return int(capi.call("sam_get_cu_reserve"))


def debug_cu_hog(blocks, microseconds, stream=None):
    """measurement aid: `blocks` workgroups each holding one CU (64 KB of LDS) for `microseconds` on `stream` (default: the current one)"""
    st = capi.stream_handle() if stream is None else C.c_void_p(stream.cuda_stream)
    capi.call("sam_debug_cu_hog", int(blocks), float(microseconds), st)


def set_rng_state(state):
    """state: uint64-as-int64 [2] device tensor {seed, offset base} (or None): see sam_set_rng_state in include/sam_hip.h"""
    capi.call("sam_set_rng_state", capi.ptr(state))


def cast_bf16(x, y):
    capi.call("sam_cast_f32_to_bf16", capi.ptr(x), capi.ptr(y), x.numel(), capi.stream_handle())
    return y


def embedding_bwd(dy, idx, grad_table, padding_idx=-1):
    """grad_table[idx[t], :] += dy[t, :]  (dy bf16 [T,D], idx int64 [T], grad_table fp32 [rows, D]); padding_idx rows are skipped.
    grad_table._sam_touched (uint8 [rows], set by the Trainer): the rows that receive a gradient are flagged (row-sparse optimizer)"""
    t, d = dy.shape
    capi.call("sam_embedding_bwd", capi.ptr(dy), dy.stride(0), capi.ptr(idx), t, d, grad_table.shape[0], int(padding_idx), capi.ptr(grad_table), grad_table.stride(0),
              capi.ptr(getattr(grad_table, "_sam_touched", None)), capi.stream_handle())


def embedding_bwd_sorted(dy, idx_sorted, grad_table, padding_idx=-1):
    """embedding_bwd for an index list sorted ascending: fixed summation order, one writer per table row (no atomics)"""
    t, d = dy.shape
    capi.call("sam_embedding_bwd_sorted", capi.ptr(dy), dy.stride(0), capi.ptr(idx_sorted), t, d, grad_table.shape[0], int(padding_idx), capi.ptr(grad_table),
              grad_table.stride(0), capi.ptr(getattr(grad_table, "_sam_touched", None)), capi.stream_handle())


def mask_bits_from_int8_bhnn(rel, base_bits=None):
    """rel int8 [B,H,N,N] (non-zero = visible), optional base bits [B,1,N,NW] -> uint32 [B,H,N,NW]"""
    _chk(rel, torch.int8, "rel")
    b, h, n, n2 = rel.shape
    t_ = _tops()
    if t_ is not None:
        return t_.pack_relations_bhnn(rel, base_bits)
    nw = words_per_row(n)
    out = torch.empty((b, h, n, nw), dtype=torch.int32, device=rel.device)
    capi.call("sam_mask_bits_from_int8_bhnn", capi.ptr(rel), capi.ptr(base_bits), b, h, n, nw, capi.ptr(out), capi.stream_handle())
    return out


def spatial_relation_tensor(boxes, context=3, distance_threshold=0.5):
    """boxes f64 [B,N,4] on the GPU -> int8 [B,N,N,12] (HIP kernel; same semantics as spatial_graph.relation_tensor)"""
    _chk(boxes, torch.float64, "boxes")
    b, n, _ = boxes.shape
    out = torch.empty((b, n, n, 12), dtype=torch.int8, device=boxes.device)
    capi.call("sam_spatial_relation_tensor", capi.ptr(boxes), b, n, int(context), float(distance_threshold), capi.ptr(out), capi.stream_handle())
    return out


_GROUPED_WS = {}


def _grouped_ws(device, nbytes):
    """exchange workspace of sam_gemm_bf16_grouped: one zero-filled buffer per (device, stream), grown on demand.  The kernel leaves its flag
    words zero, so the buffer is filled once; launches on one stream are ordered, so they can share it."""
    key = (device.index, torch.cuda.current_stream(device).cuda_stream)
    buf = _GROUPED_WS.get(key)
    if buf is None or buf.numel() * 4 < nbytes:
        buf = torch.zeros(((nbytes + 3) // 4,), dtype=torch.float32, device=device)
        _GROUPED_WS[key] = buf
    return buf


def grouped_ws_check():
    """raise if any pair exchange of sam_gemm_bf16_grouped gave up waiting for its partner block (error word of the workspace; synchronises)"""
    for key, buf in _GROUPED_WS.items():
        if int(buf[:1].view(torch.int32).item()) != 0:
            buf[:1].zero_()
            raise capi.SamHipError("sam_gemm_bf16_grouped: a workgroup pair never became co-resident (device %s); the step's weight gradients are invalid" % (key[0],))


def reset_workspaces():
    """forget every cached scratch buffer (after a failed step: a grouped-wgrad workspace may hold stale pair flags, an LN scratch stale partials);
    the next call allocates fresh, zero-filled ones"""
    _GROUPED_WS.clear()
    _WS.clear()
    _LN_XWS.clear()
    LnFinalizeQueue.clear()


def wgrad_grouped(jobs, force_tile=0, accumulate=True):
    """jobs: list of (dy [R,M] bf16, x [R,N] bf16, dW fp32 [M,N] view, dbias fp32 [M] or None).  dW += dy^T x (and dbias += colsum(dy))
    for all jobs in ONE launch (sam_gemm_bf16_grouped); accumulate=False: both are overwritten instead (no read of the old gradient)."""
    n = len(jobs)
    arr = (capi.GemmDesc * n)()
    flops = 0.0
    for d, job in zip(arr, jobs):
        dy, x, dw, db = job[:4]
        acc_j = job[4] if len(job) > 4 else accumulate          # (a job may carry its own flag: problems that accumulate next to problems that overwrite)
        d.M, d.N, d.K = dy.shape[1], x.shape[1], dy.shape[0]
        d.a_kcontig = d.b_kcontig = 0
        d.c_is_f32, d.accumulate, d.epilogue = 1, int(bool(acc_j)), capi.EPI_NONE
        d.A, d.lda, d.B, d.ldb, d.C, d.ldc = dy.data_ptr(), dy.stride(0), x.data_ptr(), x.stride(0), dw.data_ptr(), dw.stride(0)
        d.bias_grad = _dp(db)
        flops += 2.0 * d.M * d.N * d.K
    if force_tile != 128:
        ws = _grouped_ws(jobs[0][0].device, capi.call("sam_gemm_grouped_ws_bytes", arr, n))
        arr[0].ws, arr[0].ws_bytes = ws.data_ptr(), ws.numel() * 4
    arr[0].force_tile = force_tile
    capi.call("sam_gemm_bf16_grouped", arr, n, capi.stream_handle(), meta=dict(kernel="gemm_grouped_wgrad", flops=flops, shape=(n, int(arr[0].K))))


# ----------------------------------------------------------------------------- spatial auxiliary heads (csrc/aux_heads.hip)
AUX_FUSIONS = {"mul": capi.AUX_MUL, "add": capi.AUX_ADD}


def _aux_fusion(fusion):
    code = AUX_FUSIONS.get(fusion) if isinstance(fusion, str) else fusion
    if code not in (capi.AUX_MUL, capi.AUX_ADD):
        raise ValueError("aux_spatial_fusion must be 'mul' or 'add', got %r" % (fusion,))
    return code


def _aux_operands(o, d, w):
    _chk(o, torch.float32, "O")
    _chk(d, torch.float32, "D")
    _chk(w, torch.float32, "W")
    if o.dim() != 3 or o.shape != d.shape or o.shape[2] != 32 or tuple(w.shape) != (12, 32):
        raise capi.SamHipError("aux pair head: O, D must be fp32 [B, n, 32] of one shape and W [12, 32] (got %s, %s, %s)"
                               % (tuple(o.shape), tuple(d.shape), tuple(w.shape)))
    if o.shape[0] == 0 or o.shape[1] == 0:
        raise capi.SamHipError("aux pair head: empty operands %s" % (tuple(o.shape),))
    return o.shape[0], o.shape[1]


def aux_pair_fwd(o, d, w, bias, fusion="mul"):
    """spatial_classifier(f(O_i, D_j)) for every pair (sa_m4c.py:316-347): O, D fp32 [B, n, 32], W fp32 [12, 32], bias fp32 [12] -> fp32 [B, n, n, 12]"""
    code = _aux_fusion(fusion)
    b, n = _aux_operands(o, d, w)
    _chk(bias, torch.float32, "bias")
    out = torch.empty((b, n, n, 12), dtype=torch.float32, device=o.device)
    capi.call("sam_aux_pair_fwd", capi.ptr(o), capi.ptr(d), capi.ptr(w), capi.ptr(bias), b, n, code, capi.ptr(out), capi.stream_handle())
    return out


def aux_pair_bwd(g, o, d, w, dw, dbias, fusion="mul", accumulate=True):
    """-> (dO, dD) fp32 [B, n, 32]; dW [12, 32] / dbias [12] fp32 are accumulated in place (overwritten with accumulate=False)"""
    code = _aux_fusion(fusion)
    b, n = _aux_operands(o, d, w)
    _chk(g, torch.float32, "G")
    if tuple(g.shape) != (b, n, n, 12):
        raise capi.SamHipError("aux pair head: G must be fp32 [%d, %d, %d, 12], got %s" % (b, n, n, tuple(g.shape)))
    for t, name in ((dw, "dW"), (dbias, "dbias")):
        if not t.is_cuda or t.dtype != torch.float32 or not t.is_contiguous():
            raise capi.SamHipError("aux pair head: %s must be a contiguous fp32 GPU tensor" % name)
    d_o, d_d = torch.empty_like(o), torch.empty_like(d)
    nbytes = capi.call("sam_aux_pair_bwd_ws_bytes", b, n)
    ws = _workspace(nbytes, o.device, "aux")
    capi.call("sam_aux_pair_bwd", capi.ptr(g), capi.ptr(o), capi.ptr(d), capi.ptr(w), b, n, code, capi.ptr(d_o), capi.ptr(d_d), capi.ptr(dw), capi.ptr(dbias),
              int(bool(accumulate)), capi.ptr(ws), ws.numel() * 4, capi.stream_handle())
    return d_o, d_d


# ----------------------------------------------------------------------------- the aux heads' loss from relation codes (csrc/aux_loss.hip)
def codes_from_relation_tensor(adj, check=True):
    """spatial_adj_matrices["1"] ([..., 12], the one-hot torch_broadcast_adj_matrix makes of the base relation code) -> uint8 [...] codes: channel r set ->
    r + 1, an all-zero row -> 0.  Plain torch on whatever device `adj` lives on; the result cannot exceed 12 for a one-hot.  check (two reads of a device
    flag on the host: not for the training step): a row with more than one channel set is not a context-1 tensor -> ValueError."""
    if adj.dim() < 1 or adj.shape[-1] != 12:
        raise ValueError("relation tensor must end in 12 channels, got %s" % (tuple(adj.shape),))
    a = adj.to(torch.int16)
    if check and (bool(((a != 0) & (a != 1)).any()) or bool((a.sum(-1) > 1).any())):
        raise ValueError("relation tensor is not a 12-channel one-hot (spatial context 1): rows must hold at most one 1")
    return (a * torch.arange(1, 13, dtype=torch.int16, device=adj.device)).sum(-1).to(torch.uint8)


def relation_tensor_from_codes(codes):
    """uint8 [...] codes -> int8 [..., 12] one-hot (0 -> an all-zero row); a code above 12 raises ValueError"""
    check_relation_codes(codes)
    return (codes.unsqueeze(-1).to(torch.int16) == torch.arange(1, 13, dtype=torch.int16, device=codes.device)).to(torch.int8)


def check_relation_codes(codes):
    if codes.dtype != torch.uint8:
        raise ValueError("relation codes must be uint8, got %s" % codes.dtype)
    if codes.numel() and int(codes.max()) > 12:
        raise ValueError("relation code %d: codes are 0 (no relation) or 1..12" % int(codes.max()))
    return codes


def relation_codes_from_boxes(obj_boxes, ocr_boxes=None, distance_threshold=0.5):
    """the batch's boxes -> uint8 [B, n, n] relation codes, n = n_obj + n_ocr, in ONE launch (sam_relation_codes_from_boxes): the code whose channel
    spatial_relation_tensor(float64(cat(obj[..., :4], ocr[..., :4])), context=1, distance_threshold) sets, 0 where it sets none.  Boxes as
    mask_bits_from_boxes takes them."""
    obj_boxes, ld_obj = _box_rows(obj_boxes, "obj_boxes")
    b, n_obj, n_ocr, ld_ocr = obj_boxes.shape[0], obj_boxes.shape[1], 0, 0
    if ocr_boxes is not None and ocr_boxes.shape[1] > 0:
        ocr_boxes, ld_ocr = _box_rows(ocr_boxes, "ocr_boxes")
        n_ocr = ocr_boxes.shape[1]
        if ocr_boxes.dtype != obj_boxes.dtype or ocr_boxes.shape[0] != b:
            raise capi.SamHipError("relation_codes_from_boxes: obj_boxes and ocr_boxes must share dtype and batch size")
    else:
        ocr_boxes = None
    if b == 0 or n_obj == 0:
        raise capi.SamHipError("relation_codes_from_boxes: need at least one sample and one object row, got %s" % (tuple(obj_boxes.shape),))
    n = n_obj + n_ocr
    codes = torch.empty((b, n, n), dtype=torch.uint8, device=obj_boxes.device)
    capi.call("sam_relation_codes_from_boxes", capi.ptr(obj_boxes), ld_obj, n_obj, capi.ptr(ocr_boxes), ld_ocr, n_ocr, int(obj_boxes.dtype == torch.float64),
              b, float(distance_threshold), capi.ptr(codes), capi.stream_handle())
    return codes


# ----------------------------------------------------------------------------- the loss's codes and valid flags in one launch (csrc/aux_targets.hip)
AUX_MASK_DTYPES = (torch.bool, torch.uint8, torch.int8, torch.int32, torch.int64)


def aux_targets_fusable(rel, obj_mask, ocr_mask):
    """whether aux_targets takes these operands as they are (GPU tensors, int8 relation tensor or None, two masks of ONE accepted dtype): what
    SAM4C.spatial_aux_loss asks before it chooses between the launch and the torch composition"""
    return (obj_mask.is_cuda and ocr_mask.is_cuda and obj_mask.device == ocr_mask.device and obj_mask.dtype == ocr_mask.dtype and obj_mask.dtype in AUX_MASK_DTYPES
            and obj_mask.dim() == 2 and ocr_mask.dim() == 2 and (rel is None or (rel.is_cuda and rel.device == obj_mask.device and rel.dtype == torch.int8 and rel.dim() == 4)))


def _aux_mask_rows(t, name):
    """-> (tensor with unit column stride, row stride in elements)"""
    if not t.is_cuda or t.dim() != 2 or t.dtype not in AUX_MASK_DTYPES:
        raise capi.SamHipError("aux_targets: %s must be a 2-D GPU tensor of bool, uint8, int8, int32 or int64 (got %s, %s)" % (name, tuple(t.shape), t.dtype))
    if (t.shape[1] > 0 and t.stride(1) != 1) or (t.shape[0] > 1 and t.stride(0) < t.shape[1]):
        t = t.contiguous()
    return t, (t.stride(0) if t.shape[0] > 1 else t.shape[1])


def aux_targets(rel, obj_mask, ocr_mask):
    """spatial_adj_matrices["1"] (int8 [B, n, n, 12], contiguous, or None) and the two padding masks ([B, n_obj], [B, n_ocr]: bool or an integer dtype, one
    dtype, rows may be strided) -> (codes uint8 [B, n, n] or None, valid uint8 [B, n]) in ONE launch (sam_aux_targets) on the current stream, nothing
    read back: valid = cat(masks) != 0; codes = codes_from_relation_tensor(rel, check=False) on the pairs of two valid rows and 0 elsewhere (pairs the
    loss never reads).  rel=None: only valid (a batch whose codes come from relation_codes_from_boxes)."""
    obj_mask, ld_obj = _aux_mask_rows(obj_mask, "obj_mask")
    ocr_mask, ld_ocr = _aux_mask_rows(ocr_mask, "ocr_mask")
    if obj_mask.dtype != ocr_mask.dtype or obj_mask.shape[0] != ocr_mask.shape[0] or obj_mask.device != ocr_mask.device:
        raise capi.SamHipError("aux_targets: obj_mask and ocr_mask must share dtype, device and batch size")
    b, n_obj, n_ocr = obj_mask.shape[0], obj_mask.shape[1], ocr_mask.shape[1]
    n = n_obj + n_ocr
    codes = None
    if rel is not None:
        _chk(rel, torch.int8, "rel")
        if tuple(rel.shape) != (b, n, n, 12) or not rel.is_contiguous() or rel.device != obj_mask.device:
            raise capi.SamHipError("aux_targets: rel must be a contiguous int8 [%d, %d, %d, 12] beside the masks, got %s" % (b, n, n, tuple(rel.shape)))
        codes = torch.empty((b, n, n), dtype=torch.uint8, device=rel.device)
    valid = torch.empty((b, n), dtype=torch.uint8, device=obj_mask.device)
    capi.call("sam_aux_targets", capi.ptr(rel), capi.ptr(obj_mask) if n_obj else None, ld_obj, n_obj, capi.ptr(ocr_mask) if n_ocr else None, ld_ocr, n_ocr,
              obj_mask.element_size(), b, n, capi.ptr(codes), capi.ptr(valid), capi.stream_handle())
    return codes, valid


def aux_targets_host(rel, obj_mask, ocr_mask):
    """the twin of aux_targets in plain torch, on whatever device the tensors live on (CPU included): the same bytes, the zeroed codes of the pairs
    with a row that is not valid included"""
    valid = torch.cat([obj_mask, ocr_mask], dim=-1).ne(0).to(torch.uint8)
    if rel is None:
        return None, valid
    pair = (valid.unsqueeze(2) & valid.unsqueeze(1)).to(rel.device)
    return codes_from_relation_tensor(rel, check=False) * pair, valid


def _aux_loss_operands(o, d, w, bias, codes, valid):
    b, n = _aux_operands(o, d, w)
    _chk(bias, torch.float32, "bias")
    _chk(codes, torch.uint8, "codes")
    _chk(valid, torch.uint8, "valid")
    if tuple(bias.shape) != (12,) or tuple(codes.shape) != (b, n, n) or tuple(valid.shape) != (b, n):
        raise capi.SamHipError("aux pair loss: bias [12], codes uint8 [%d, %d, %d] and valid uint8 [%d, %d] expected, got %s, %s, %s"
                               % (b, n, n, b, n, tuple(bias.shape), tuple(codes.shape), tuple(valid.shape)))
    return b, n


def aux_pair_loss(o, d, w, bias, codes, valid, fusion="mul"):
    """masked BCE-with-logits of spatial_classifier(f(O_i, D_j)) against the one-hot of codes, over the pairs with valid[i] & valid[j], divided by their
    number (include/sam_hip_aux_loss.h) -> (loss fp32 [1], count fp32 [1]); no [B, n, n, 12] tensor is written.  O, D fp32 [B, n, 32], W [12, 32],
    bias [12], codes uint8 [B, n, n] (0..12; the caller checks the range: check_relation_codes), valid uint8 [B, n]."""
    code = _aux_fusion(fusion)
    b, n = _aux_loss_operands(o, d, w, bias, codes, valid)
    out = torch.empty(2, dtype=torch.float32, device=o.device)
    nbytes = capi.call("sam_aux_pair_loss_fwd_ws_bytes", b, n)
    ws = _workspace(nbytes, o.device, "aux_loss")
    capi.call("sam_aux_pair_loss_fwd", capi.ptr(o), capi.ptr(d), capi.ptr(w), capi.ptr(bias), capi.ptr(codes), capi.ptr(valid), b, n, code,
              capi.ptr(out), C.c_void_p(out.data_ptr() + 4), capi.ptr(ws), ws.numel() * 4, capi.stream_handle())
    return out[:1], out[1:]


def aux_pair_loss_bwd(grad_out, count, o, d, w, bias, codes, valid, dw, dbias, fusion="mul", accumulate=True):
    """-> (dO, dD) fp32 [B, n, 32] of grad_out * loss; dW [12, 32] / dbias [12] fp32 are accumulated in place (overwritten with accumulate=False).
    grad_out (fp32 [1] on the GPU, or None = 1) and count (the forward's) are read by the kernel on the device."""
    code = _aux_fusion(fusion)
    b, n = _aux_loss_operands(o, d, w, bias, codes, valid)
    for t, name, numel in ((grad_out, "grad_out", 1), (count, "count", 1), (dw, "dW", 384), (dbias, "dbias", 12)):
        if t is None and name == "grad_out":
            continue
        if not t.is_cuda or t.dtype != torch.float32 or not t.is_contiguous() or t.numel() != numel:
            raise capi.SamHipError("aux pair loss: %s must be a contiguous fp32 GPU tensor of %d element(s)" % (name, numel))
    d_o, d_d = torch.empty_like(o), torch.empty_like(d)
    nbytes = capi.call("sam_aux_pair_loss_bwd_ws_bytes", b, n)
    ws = _workspace(nbytes, o.device, "aux")
    capi.call("sam_aux_pair_loss_bwd", capi.ptr(grad_out), capi.ptr(count), capi.ptr(o), capi.ptr(d), capi.ptr(w), capi.ptr(bias), capi.ptr(codes),
              capi.ptr(valid), b, n, code, capi.ptr(d_o), capi.ptr(d_d), capi.ptr(dw), capi.ptr(dbias), int(bool(accumulate)), capi.ptr(ws), ws.numel() * 4,
              capi.stream_handle())
    return d_o, d_d


def _aux_scores_host(o, d, w, bias, valid, fusion):
    """-> (S float64 [B, n, n, 12] on the host with exact f(0) W + bias at pairs that are not valid, M bool [B, n, n]): the scores both host twins read"""
    _aux_fusion(fusion)
    o, d, w, bias = (t.double().cpu() if not t.requires_grad else t for t in (o, d, w, bias))
    valid = valid.cpu() != 0
    pair = o.unsqueeze(2) * d.unsqueeze(1) if fusion in ("mul", capi.AUX_MUL) else o.unsqueeze(2) + d.unsqueeze(1)
    m = valid.unsqueeze(2) & valid.unsqueeze(1)
    pair = torch.where(m.unsqueeze(-1), pair, torch.zeros_like(pair))                     # rows that are not valid are never used
    return pair @ w.t() + bias, m


def aux_loss_host(o, d, w, bias, codes, valid, fusion="mul"):
    """the loss in float64 torch on the host: the twin the kernels are tested against.  -> (loss, count) as 0-d float64 tensors, differentiable w.r.t. o, d, w, bias"""
    s, m = _aux_scores_host(o, d, w, bias, valid, fusion)
    codes = check_relation_codes(codes.cpu())
    y = relation_tensor_from_codes(codes).double()
    bce = torch.clamp(s, min=0) - s * y + torch.log1p(torch.exp(-s.abs()))
    count = m.sum().double()
    return (bce.sum(-1) * m).sum() / count.clamp(min=1.0), count


# ----------------------------------------------------------------------------- the aux heads' confusion counts (csrc/aux_stats.hip)
AUX_CLASSES = 13          # 0 no relation, 1..12 the relation whose channel is code - 1


def new_aux_stats(device="cuda"):
    """resident totals for aux_pair_stats(into=...): (confusion int64 [13, 13], fired int64 [13, 12]), zeros"""
    return (torch.zeros(AUX_CLASSES, AUX_CLASSES, dtype=torch.int64, device=device), torch.zeros(AUX_CLASSES, 12, dtype=torch.int64, device=device))


def _aux_stats_into(into, device):
    confusion, fired = into
    for t, name, shape in ((confusion, "confusion", (AUX_CLASSES, AUX_CLASSES)), (fired, "fired", (AUX_CLASSES, 12))):
        if not t.is_cuda or t.device != device or t.dtype != torch.int64 or not t.is_contiguous() or tuple(t.shape) != shape:
            raise capi.SamHipError("aux pair stats: %s must be a contiguous int64 %s tensor beside the operands" % (name, list(shape)))
    return confusion, fired


def aux_pair_stats(o, d, w, bias, codes, valid, fusion="mul", into=None):
    """the relation confusion counts of spatial_classifier(f(O_i, D_j)) over the pairs with valid[i] & valid[j] (include/sam_hip_aux_stats.h; DESIGN.md
    section 3.24) -> (confusion int64 [13, 13]: [true class, argmax-rule class], fired int64 [13, 12]: [true class, channel with S > 0]); no [B, n, n, 12]
    tensor is written and nothing is read back.  Operands as aux_pair_loss, except that codes above 12 are allowed (class 0).  into=(confusion, fired):
    resident int64 tensors the counts are ADDED to (and returned)."""
    code = _aux_fusion(fusion)
    b, n = _aux_loss_operands(o, d, w, bias, codes, valid)
    confusion, fired = _aux_stats_into(into, o.device) if into is not None else (torch.empty(AUX_CLASSES, AUX_CLASSES, dtype=torch.int64, device=o.device),
                                                                                 torch.empty(AUX_CLASSES, 12, dtype=torch.int64, device=o.device))
    nbytes = C.c_int64(0)
    capi.call("sam_aux_pair_stats_ws_bytes", b, n, C.byref(nbytes))
    ws = _workspace(nbytes.value, o.device, "aux_stats")
    capi.call("sam_aux_pair_stats", capi.ptr(o), capi.ptr(d), capi.ptr(w), capi.ptr(bias), capi.ptr(codes), capi.ptr(valid), b, n, code, capi.ptr(confusion),
              capi.ptr(fired), int(into is not None), capi.ptr(ws), ws.numel() * 4, capi.stream_handle())
    return confusion, fired


def aux_stats_from_logits(logits, codes, valid):
    """the twin of aux_pair_stats in plain torch over dense scores [B, n, n, 12] (any float dtype, CPU or GPU): the definition of DESIGN.md section 3.24
    taken literally -- the running `S[r] > best` scan from best = 0, so a tie keeps the first maximum and a NaN neither fires nor wins; pairs with a row
    that is not valid are never looked at.  -> (confusion int64 [13, 13], fired int64 [13, 12]) on the logits' device"""
    if logits.dim() != 4 or logits.shape[-1] != 12 or not logits.is_floating_point() or logits.shape[1] != logits.shape[2]:
        raise ValueError("aux_stats_from_logits: logits must be a float [B, n, n, 12] tensor, got %s %s" % (tuple(logits.shape), logits.dtype))
    b, n = logits.shape[0], logits.shape[1]
    if tuple(codes.shape) != (b, n, n) or tuple(valid.shape) != (b, n) or codes.dtype != torch.uint8:
        raise ValueError("aux_stats_from_logits: codes uint8 [%d, %d, %d] and valid [%d, %d] expected, got %s, %s" % (b, n, n, b, n, tuple(codes.shape), tuple(valid.shape)))
    dev = logits.device
    v = valid.to(dev) != 0
    m = v.unsqueeze(2) & v.unsqueeze(1)
    s = logits[m]                                               # [pairs, 12]: only the valid pairs
    c = codes.to(dev)[m].long()
    c = torch.where((c >= 1) & (c <= 12), c, torch.zeros_like(c))
    best = torch.zeros(s.shape[0], dtype=s.dtype, device=dev)
    p = torch.zeros(s.shape[0], dtype=torch.int64, device=dev)
    for r in range(12):
        win = s[:, r] > best
        best = torch.where(win, s[:, r], best)
        p = torch.where(win, torch.full_like(p, r + 1), p)
    confusion = torch.bincount(c * AUX_CLASSES + p, minlength=AUX_CLASSES * AUX_CLASSES).reshape(AUX_CLASSES, AUX_CLASSES)
    fired = torch.zeros(AUX_CLASSES, 12, dtype=torch.int64, device=dev).index_add_(0, c, (s > 0).to(torch.int64))
    return confusion, fired


def aux_stats_host(o, d, w, bias, codes, valid, fusion="mul"):
    """the counts from float64 scores on the host (the scores aux_loss_host forms), through aux_stats_from_logits: what the kernel is tested against"""
    s, _ = _aux_scores_host(o.detach(), d.detach(), w.detach(), bias.detach(), valid, fusion)
    return aux_stats_from_logits(s, codes.cpu(), valid.cpu())


# ----------------------------------------------------------------------------- Faster R-CNN fc7 fine-tuning (csrc/fc7.hip)
def _bf16_rows(t, name):
    if not t.is_cuda or t.dtype != BF16 or t.dim() != 2 or t.stride(1) != 1:
        raise capi.SamHipError("%s: need a 2-D bf16 GPU tensor with contiguous rows" % name)


def l2norm_pack_bf16(x, out, col0=0, normalize=True, zero_upto=0, eps=1e-12):
    """out[:, col0:col0+D] = bf16(F.normalize(x, dim=-1)) (normalize=False: plain copy); x bf16 [M, D] (any row stride); out bf16 [M, ldo];
    columns [col0+D, zero_upto) of out are zeroed -- l2norm_pack for bf16 rows (the fc7 GEMM's output)"""
    _bf16_rows(x, "l2norm_pack_bf16 x")
    _bf16_rows(out, "l2norm_pack_bf16 out")
    m, d = x.shape
    if out.shape[0] != m:
        raise capi.SamHipError("l2norm_pack_bf16: x / out must have the same number of rows")
    capi.call("sam_l2norm_pack_from_bf16", capi.ptr(x), x.stride(0), m, d, int(bool(normalize)), float(eps), capi.ptr(out), out.stride(0), int(col0),
              int(zero_upto), capi.stream_handle(), meta=dict(kernel="l2norm_pack_from_bf16", bytes=4.0 * m * d))
    return out


def fc7_bwd_rows(g, y, normalize=True, eps=1e-12, out=None):
    """dz = [y > 0] * d F.normalize(y) / dy applied to g (normalize=False: [y > 0] * g); g, y bf16 [M, D] -> dz bf16 [M, D]"""
    _bf16_rows(g, "fc7_bwd_rows g")
    _bf16_rows(y, "fc7_bwd_rows y")
    if g.shape != y.shape:
        raise capi.SamHipError("fc7_bwd_rows: g %s and y %s differ in shape" % (tuple(g.shape), tuple(y.shape)))
    m, d = y.shape
    if out is None:
        out = torch.empty((m, d), dtype=BF16, device=y.device)
    capi.call("sam_fc7_bwd_rows", capi.ptr(g), g.stride(0), capi.ptr(y), y.stride(0), m, d, int(bool(normalize)), float(eps), capi.ptr(out), out.stride(0),
              capi.stream_handle(), meta=dict(kernel="fc7_bwd_rows", bytes=6.0 * m * d))
    return out


# ----------------------------------------------------------------------------- M4C answer targets (csrc/answers.hip)
ANSWER_TABLE_KEYS = ANSWER_TABLE.keys


def answer_outputs(B, L, W, device, ld=None, dense=True):
    """the sampler's output buffers: targets fp32 [B, L, W] (a view with row stride ld >= W), train_prev_inds int64 [B, L], the two masks fp32 [B, L],
    answer_choice int32 [B].  dense=False: no "targets" entry and no [B, L, W] allocation -- answer_sample then draws without writing them, for a loss that
    reads the tables itself (bce_loss_table)"""
    out = {"train_prev_inds": torch.empty((B, L), dtype=torch.int64, device=device),
           "train_loss_mask": torch.empty((B, L), dtype=torch.float32, device=device), "train_acc_mask": torch.empty((B, L), dtype=torch.float32, device=device),
           "answer_choice": torch.empty((B,), dtype=torch.int32, device=device)}
    if not dense:
        return out
    ld = W if ld is None else int(ld)
    if ld < W:
        raise capi.SamHipError("answer targets: row stride %d < width %d" % (ld, W))
    buf = torch.empty((B, L, ld), dtype=torch.float32, device=device)
    return dict({"targets": buf[:, :, :W]}, **out)


def _check_answer_table(table):
    """dtype / shape checks of a collated answer table on the GPU -> (B, S, L, G, E)"""
    ANSWER_TABLE.require(table, _GPU)
    if table["seq_grp"].dim() != 3:
        raise capi.SamHipError("answer table: seq_grp must be [B, S, L]")
    B, S, L = table["seq_grp"].shape
    G, E = table["grp_idx"].shape[-1], table["grp_extra"].shape[-1]
    ANSWER_TABLE.check(table, _GPU, B=B, S=S, L=L, G=G, E=E)
    return B, S, L, G, E


def answer_sample(table, width, bos, key, step=0, step_dev=None, force_choice=None, out=None):
    """sam_answer_sample: draw one decoding sequence per sample from the collated answer table (answers.collate_answer_tables, moved to the GPU) and write
    the dense M4C targets.  The draw reads its step as step_dev[0] + step (step_dev: int64 [1] device counter, or None); force_choice int32 [B] pins it.
    out: buffers from answer_outputs (allocated here when None); buffers without a "targets" entry (answer_outputs(dense=False)): the dense targets are
    not written.  Returns out."""
    B, S, L, G, E = _check_answer_table(table)
    if out is None:
        out = answer_outputs(B, L, int(width), table["meta"].device)
    tg = out.get("targets")
    if tg is not None:
        if not tg.is_cuda or tg.dtype != torch.float32:
            raise capi.SamHipError("answer targets must be an fp32 GPU tensor")
        if tuple(tg.shape) != (B, L, int(width)):
            raise capi.SamHipError("answer targets: expected [%d, %d, %d], got %s" % (B, L, int(width), tuple(tg.shape)))
    if step_dev is not None:
        _chk(step_dev, torch.int64, "step_dev")
    if force_choice is not None:
        _chk(force_choice, torch.int32, "force_choice")
    key = int(key) & 0xFFFFFFFFFFFFFFFF
    t_ = _tops()
    if t_ is not None:
        skey = key - (1 << 64) if key >= 1 << 63 else key
        if tg is None:
            t_.answer_sample_notargets(*[table[k] for k in ANSWER_TABLE_KEYS], int(width), int(bos), skey, step_dev, int(step), force_choice,
                                       out["train_prev_inds"], out["train_loss_mask"], out["train_acc_mask"], out["answer_choice"])
        else:
            t_.answer_sample(*[table[k] for k in ANSWER_TABLE_KEYS], int(bos), skey, step_dev, int(step), force_choice, tg,
                             out["train_prev_inds"], out["train_loss_mask"], out["train_acc_mask"], out["answer_choice"])
        return out
    if tg is not None and (tg.stride(2) != 1 or tg.stride(0) != L * tg.stride(1)):
        raise capi.SamHipError("answer targets must be [B, L, W] with unit column stride over a [B, L, ld] buffer")
    for k, dt, nel in (("train_prev_inds", torch.int64, B * L), ("train_loss_mask", torch.float32, B * L), ("train_acc_mask", torch.float32, B * L),
                       ("answer_choice", torch.int32, B)):
        _chk(out[k], dt, k)
        if out[k].numel() != nel:
            raise capi.SamHipError("%s: %d elements, expected %d" % (k, out[k].numel(), nel))
    if force_choice is not None and force_choice.numel() != B:
        raise capi.SamHipError("force_choice: %d elements, expected %d" % (force_choice.numel(), B))
    capi.call("sam_answer_sample", *[capi.ptr(table[k]) for k in ANSWER_TABLE_KEYS], B, S, L, G, E, int(width), int(bos), key, capi.ptr(step_dev), int(step),
              capi.ptr(force_choice), capi.ptr(tg), tg.stride(1) if tg is not None else 0, capi.ptr(out["train_prev_inds"]), capi.ptr(out["train_loss_mask"]),
              capi.ptr(out["train_acc_mask"]), capi.ptr(out["answer_choice"]), capi.stream_handle(),
              meta=dict(kernel="answer_sample", bytes=B * L * int(width) * 4 if tg is not None else B * L * 20, shape=(B, L, int(width))))
    return out


def bce_loss_table(fixed, ocr, table, choice, loss_mask, grad_scale=1.0, global_count=None, want_grads=True, pred=None):
    """sam_bce_loss_table: bce_loss on the targets answer_sample would write for `choice` (int32 [B], the sampler's answer_choice), read from the collated
    answer table itself -- no dense targets.  fixed f32 [R,V], ocr f32 [R,No], R = B * L, loss_mask f32 [R] -> (loss f32 [1], d_fixed bf16 [R,V],
    d_ocr f32 [R,No], pred); the gradients are bit-identical to bce_loss's.  want_grads=False: loss (and pred) only, the gradients are None.
    pred: None (no predictions), True (a fresh int64 [R]) or an int64 [R] buffer to fill -- the argmax of every row of concat(fixed, ocr), masked rows
    included, first maximum wins."""
    r, v = fixed.shape
    no = ocr.shape[1]
    for t, name in ((fixed, "fixed_scores"), (ocr, "ocr_scores")):
        if not t.is_cuda or t.dtype != torch.float32 or t.dim() != 2:
            raise capi.SamHipError("%s must be a 2-D fp32 GPU tensor" % name)
    if fixed.stride(1) != 1 or (no and ocr.stride(1) != 1) or ocr.shape[0] != r:
        raise capi.SamHipError("bce_loss_table: 2-D score blocks of equal row count with unit last stride")
    B, S, L, G, E = _check_answer_table(table)
    _chk(choice, torch.int32, "choice")
    _chk(loss_mask, torch.float32, "loss_mask")
    if B * L != r or loss_mask.numel() != r or choice.numel() != B:
        raise capi.SamHipError("bce_loss_table: %d score rows / %d mask entries / %d choices for a table of %d x %d decoding steps" % (r, loss_mask.numel(), choice.numel(), B, L))
    if pred is True:
        pred = torch.empty((r,), dtype=torch.int64, device=fixed.device)
    elif pred is False:
        pred = None
    if pred is not None:
        _chk(pred, torch.int64, "pred")
        if pred.numel() != r:
            raise capi.SamHipError("bce_loss_table: pred has %d elements, expected %d" % (pred.numel(), r))
    if global_count is not None:
        _chk(global_count, torch.float32, "global_count")
    t_ = _tops()
    if t_ is not None:
        loss, d_fixed, d_ocr = t_.bce_loss_table(fixed, ocr, [table[k] for k in ANSWER_TABLE_KEYS], choice, loss_mask, float(grad_scale), global_count,
                                                 bool(want_grads), pred)
        return (loss, d_fixed, d_ocr, pred) if want_grads else (loss, None, None, pred)
    loss = torch.empty(1, dtype=torch.float32, device=fixed.device)
    d_fixed = torch.empty((r, v), dtype=BF16, device=fixed.device) if want_grads else None
    d_ocr = torch.empty((r, no), dtype=torch.float32, device=fixed.device) if want_grads else None
    capi.call("sam_bce_loss_table", capi.ptr(fixed), fixed.stride(0), capi.ptr(ocr), ocr.stride(0), *[capi.ptr(table[k]) for k in ANSWER_TABLE_KEYS], B, S, L, G, E,
              capi.ptr(choice), capi.ptr(loss_mask), r, v, no, float(grad_scale), capi.ptr(global_count), capi.ptr(loss), capi.ptr(d_fixed),
              d_fixed.stride(0) if want_grads else 0, capi.ptr(d_ocr), d_ocr.stride(0) if want_grads else 0, capi.ptr(pred), capi.stream_handle(),
              meta=dict(kernel="bce_loss_table", shape=(r, v + no)))
    return loss, d_fixed, d_ocr, pred


# ----------------------------------------------------------------------------- TextVQA / ST-VQA metrics (csrc/score.hip)
SCORE_TABLE_KEYS = SCORE_TABLE.keys


def score_answers(pred, table, vocab_cp, vocab_len, eos, totals=None, out=None):
    """sam_score_answers: pred int64 [B, L] prediction ids, table the collated score table (metrics.collate_score_tables, on the GPU), vocab_cp int32 [V, Lw] /
    vocab_len int32 [V] (metrics.vocab_text) -> (scores fp32 [B, 3] = VQA soft accuracy, ST-VQA accuracy, ANLS; flags int32 [B]: bit 0 an out-of-range id
    ended the walk, bit 1 an empty prediction met an empty ground truth).  totals float64 [4]: the three batch sums and B are added to it, in a fixed order.
    out: (scores, flags) buffers to fill (allocated here when None)."""
    _chk(pred, torch.int64, "pred")
    _chk(vocab_cp, torch.int32, "vocab_cp")
    _chk(vocab_len, torch.int32, "vocab_len")
    SCORE_TABLE.require(table, _GPU)
    if pred.dim() != 2 or table["gt_norm"].dim() != 3 or table["ocr"].dim() != 3 or vocab_cp.dim() != 2:
        raise capi.SamHipError("score_answers: pred [B, L], gt_norm [B, A, Lg], ocr [B, No, Lw], vocab_cp [V, Lw]")
    B, L = pred.shape
    _, A, Lg = table["gt_norm"].shape
    _, No, Lw = table["ocr"].shape
    V = vocab_cp.shape[0]
    SCORE_TABLE.check(table, _GPU, B=B, A=A, Lg=Lg, No=No, Lw=Lw)
    if vocab_cp.shape[1] != Lw or vocab_len.numel() != V:
        raise capi.SamHipError("score_answers: vocab_cp %s / vocab_len %d for words of Lw = %d code points" % (tuple(vocab_cp.shape), vocab_len.numel(), Lw))
    if out is None:
        out = (torch.empty((B, 3), dtype=torch.float32, device=pred.device), torch.empty((B,), dtype=torch.int32, device=pred.device))
    scores, flags = out
    _chk(scores, torch.float32, "scores")
    _chk(flags, torch.int32, "flags")
    if scores.numel() != 3 * B or flags.numel() != B:
        raise capi.SamHipError("score_answers: scores [%d, 3] and flags [%d] expected" % (B, B))
    if totals is not None:
        _chk(totals, torch.float64, "totals")
        if totals.numel() != 4:
            raise capi.SamHipError("score_answers: totals must be float64 [4]")
    t_ = _tops()
    if t_ is not None:
        t_.score_answers(pred, [table[k] for k in SCORE_TABLE_KEYS], vocab_cp, vocab_len, int(eos), scores, flags, totals)
        return scores, flags
    capi.call("sam_score_answers", capi.ptr(pred), *[capi.ptr(table[k]) for k in SCORE_TABLE_KEYS], capi.ptr(vocab_cp), capi.ptr(vocab_len), B, L, A, Lg, No, Lw, V,
              int(eos), capi.ptr(scores), capi.ptr(flags), capi.ptr(totals), capi.stream_handle(), meta=dict(kernel="score_answers", shape=(B, L)))
    return scores, flags


# ----------------------------------------------------------------------------- ragged region features (csrc/ragged.hip)
_RAGGED_SRC = (torch.float32, torch.float16)
_RAGGED_DST = (BF16, torch.float32)


def ragged_expand(counts, n_max, parts, mask=None, eps=1e-12, batch=None):
    """sam_ragged_expand, one launch: counts int32 [B] on the GPU (valid rows per sample, clamped to [0, n_max] by the kernel); parts a list of up to six
    (src, dst, col0, normalize, zero_upto): src [cap_rows, width] fp32 / fp16 holding the samples' valid rows back to back (all parts share cap_rows),
    dst [B * n_max, ld] bf16 / fp32 receiving row (b, i) at column col0 -- normalised like l2norm_pack when `normalize`, zeros for i >= count, columns
    [col0 + width, zero_upto) zeroed.  mask int64 [B, n_max] (optional) receives the padding mask.  Nothing is read by the host: capturable.
    batch: B when counts is None (only to let the library report the missing pointer)."""
    if counts is not None:
        _chk(counts, torch.int32, "counts")
    B = int(batch) if batch is not None else (counts.numel() if counts is not None else 0)
    n_max = int(n_max)
    cap = None
    norm = []
    for k, part in enumerate(parts):
        src, dst, col0, normalize, zero_upto = part
        for t, kinds, name in ((src, _RAGGED_SRC, "src"), (dst, _RAGGED_DST, "dst")):
            if not torch.is_tensor(t) or not t.is_cuda or t.dtype not in kinds or t.dim() != 2 or t.stride(1) != 1:
                raise capi.SamHipError("ragged_expand: part %d: %s must be a row-major 2-D GPU tensor of %s" % (k, name, " / ".join(str(d) for d in kinds)))
        if cap is None:
            cap = src.shape[0]
        if src.shape[0] != cap or dst.shape[0] != B * n_max:
            raise capi.SamHipError("ragged_expand: part %d: src has %d rows (others %d), dst %d rows (B * n_max = %d)" % (k, src.shape[0], cap, dst.shape[0], B * n_max))
        norm.append((src, dst, int(col0), int(bool(normalize)), int(zero_upto)))
    if mask is not None:
        _chk(mask, torch.int64, "mask")
        if mask.numel() != B * n_max:
            raise capi.SamHipError("ragged_expand: mask must be int64 [B, n_max] = [%d, %d]" % (B, n_max))
    if cap is None:
        cap = 1                                             # mask only: no source is read
    t_ = _tops()
    if t_ is not None and counts is not None and len(norm) <= capi.RAGGED_MAX_PARTS:
        t_.ragged_expand(counts, n_max, [p[0] for p in norm], [p[1] for p in norm], [p[2] for p in norm], [p[3] for p in norm], [p[4] for p in norm], mask, float(eps))
        return
    arr = (capi.RaggedPart * max(len(norm), 1))()
    for k, (src, dst, col0, normalize, zero_upto) in enumerate(norm):
        arr[k] = capi.RaggedPart(src.data_ptr(), src.stride(0), int(src.dtype == torch.float16), src.shape[1], dst.data_ptr(), dst.stride(0),
                                 int(dst.dtype == torch.float32), col0, normalize, zero_upto)
    capi.call("sam_ragged_expand", capi.ptr(counts), B, n_max, int(cap), arr, len(norm), float(eps), capi.ptr(mask), capi.stream_handle(),
              meta=dict(kernel="ragged_expand", shape=(B, n_max, len(norm))))


# ----------------------------------------------------------------------------- batches gathered from the resident store (csrc/store.hip)
STORE_BAD_INDEX, STORE_BAD_RANGE = 1, 2                  # the status bits of include/sam_hip_store.h


def _store_rows(t, rows, who, name):
    """a row table for the store's gathers: a GPU tensor whose rows (everything behind dim 0) are contiguous; -> (row stride, row width) in bytes"""
    if not torch.is_tensor(t) or not t.is_cuda or t.dim() < 1 or t.shape[0] != rows or t[:1].numel() == 0:
        raise capi.SamHipError("%s: %s must be a GPU tensor of %d non-empty rows" % (who, name, rows))
    if t.dim() > 1 and not t[0].is_contiguous():
        raise capi.SamHipError("%s: the rows of %s must be contiguous" % (who, name))
    esz = t.element_size()
    width = esz * t[0].numel()
    ld = t.stride(0) * esz if rows > 1 else max(t.stride(0) * esz, width)
    if ld < width:
        raise capi.SamHipError("%s: the rows of %s overlap" % (who, name))
    return ld, width


def _store_parts(parts, src_rows, dst_rows, who, keyed):
    words = 6 if keyed else 5
    arr = (C.c_int64 * (words * max(len(parts), 1)))()
    for k, part in enumerate(parts):
        src, dst = part[0], part[1]
        key = int(part[2]) if keyed else 0
        if keyed and key not in (0, 1):
            raise capi.SamHipError("%s: part %d: key %r (0: by question, 1: by image)" % (who, k, part[2]))
        ld_s, w_s = _store_rows(src, src_rows[key], who, "part %d: src" % k)
        ld_d, w_d = _store_rows(dst, dst_rows, who, "part %d: dst" % k)
        if src.dtype != dst.dtype or w_s != w_d or src.device != dst.device:
            raise capi.SamHipError("%s: part %d: src rows are %d bytes of %s, dst rows %d bytes of %s (nothing is converted)" % (who, k, w_s, src.dtype, w_d, dst.dtype))
        arr[k * words: k * words + 5] = [src.data_ptr(), ld_s, dst.data_ptr(), ld_d, w_s]
        if keyed:
            arr[k * words + 5] = key
    return arr


def _store_index(sample_idx, image_of, status, n_images, who):
    _chk(sample_idx, torch.int32, "sample_idx")
    _chk(status, torch.int32, "status")
    B = sample_idx.numel()
    if status.numel() != B:
        raise capi.SamHipError("%s: status must be int32 [B] = [%d]" % (who, B))
    if image_of is not None:
        _chk(image_of, torch.int32, "image_of")
    return B, (image_of.numel() if image_of is not None else int(n_images))


def store_gather_ragged(sample_idx, image_of, row_off, n_max, parts, counts_out, status):
    """sam_store_gather_ragged, one launch (include/sam_hip_store.h): sample_idx int32 [B]; image_of int32 [n_questions] or None (the samples are image
    indices); row_off int64 [n_images + 1]; parts a list of up to eight (src [total_rows, ...], dst [cap_rows, ...]) of one dtype and row width each,
    rows contiguous, any row stride; counts_out, status int32 [B] (status is OR-ed into).  Sample b's first min(rows, n_max) rows land back to back
    behind those of the samples in front; destination rows past the total are not written.  Nothing is read by the host."""
    who = "store_gather_ragged"
    _chk(row_off, torch.int64, "row_off")
    n_images = row_off.numel() - 1
    B, n_q = _store_index(sample_idx, image_of, status, n_images, who)
    _chk(counts_out, torch.int32, "counts_out")
    if counts_out.numel() != B or not parts:
        raise capi.SamHipError("%s: counts_out must be int32 [B] = [%d] and parts must not be empty" % (who, B))
    total, cap = parts[0][0].shape[0], parts[0][1].shape[0]
    arr = _store_parts(parts, (total, total), cap, who, keyed=False)
    capi.call("sam_store_gather_ragged", capi.ptr(sample_idx), B, capi.ptr(image_of), n_q, capi.ptr(row_off), n_images, int(total), int(n_max), arr, len(parts),
              capi.ptr(counts_out), capi.ptr(status), int(cap), capi.stream_handle(), meta=dict(kernel="store_gather_ragged", shape=(B, int(n_max), len(parts))))


def store_gather_fixed(sample_idx, image_of, n_images, parts, status):
    """sam_store_gather_fixed, one launch: parts a list of up to eight (src, dst, key): key 0 copies row sample_idx[b] of src [n_questions, ...], key 1
    row image_of[sample_idx[b]] of src [n_images, ...], to row b of dst [B, ...]; an out-of-range index gives a zero row and status bit 1."""
    who = "store_gather_fixed"
    B, n_q = _store_index(sample_idx, image_of, status, n_images, who)
    if not parts:
        raise capi.SamHipError("%s: parts must not be empty" % who)
    arr = _store_parts(parts, (n_q, int(n_images)), B, who, keyed=True)
    capi.call("sam_store_gather_fixed", capi.ptr(sample_idx), B, capi.ptr(image_of), n_q, int(n_images), arr, len(parts), capi.ptr(status), capi.stream_handle(),
              meta=dict(kernel="store_gather_fixed", shape=(B, len(parts))))


def sample_batch(state, n, rank, world, flags, sample_idx, valid, status):
    """sam_sample_batch, one launch (include/sam_hip_sampler.h): state int64 [4] {seed, epoch, step_in_epoch, batches_drawn} is read on the device and
    advanced there (flags & 8: left as it is); sample_idx, valid int32 [B] receive this rank's batch; status int32 [1] is OR-ed into (bit 1: a state
    out of range, nothing drawn).  flags: 1 shuffle, 2 drop_last, 4 drop_last_batch, 8 peek.  Nothing is read by the host."""
    who = "sample_batch"
    _chk(state, torch.int64, "state")
    _chk(sample_idx, torch.int32, "sample_idx")
    _chk(valid, torch.int32, "valid")
    _chk(status, torch.int32, "status")
    B = sample_idx.numel()
    if state.numel() != 4 or valid.numel() != B or status.numel() != 1:
        raise capi.SamHipError("%s: state must be int64 [4], valid int32 [B] = [%d] and status int32 [1]" % (who, B))
    capi.call("sam_sample_batch", capi.ptr(state), int(n), B, int(rank), int(world), int(flags), capi.ptr(sample_idx), capi.ptr(valid), capi.ptr(status),
              capi.stream_handle(), meta=dict(kernel="sample_batch", shape=(B, int(world))))


# ----------------------------------------------------------------------------- evaluation results by question index (csrc/evalboard.hip)
EVALBOARD_KEYS = EVAL_BOARD.keys                         # a board's eight tensors, in the ABI's order
EVALBOARD_ROW_KEYS = EVAL_ROWS.keys                      # the eval_beams outputs a board row holds
EVALBOARD_BAD_INDEX = 1                                  # the status bit of include/sam_hip_evalboard.h


def _board_shape(board, who, name="board"):
    """the eight tensors of a board on the GPU -> (n, P)"""
    EVAL_BOARD.require(board, _GPU, "%s: %s" % (who, name))
    if board["answer"].dim() != 2:
        raise capi.SamHipError("%s: %s['answer'] must be int32 [n, P]" % (who, name))
    n, P = board["answer"].shape
    EVAL_BOARD.check(board, _GPU, "%s: %s" % (who, name), n=n, P=P)
    return n, P


def evalboard_collect(board, res, sample_idx, valid=None):
    """sam_evalboard_collect, one launch (include/sam_hip_evalboard.h): board a dict of the EVALBOARD_KEYS tensors for n questions of answer width P; res
    eval_beams' result dict for B samples (its best_scores, oracle, best_flags, best, answer [B, P], answer_len are read); sample_idx int32 [B]; valid
    int32 [B] or None (every slot valid).  A live slot's row goes to board row sample_idx[b] when that row is empty (first write wins); seen counts the
    live slots; a valid slot out of range sets status bit 0.  Nothing is allocated and nothing is read by the host."""
    who = "evalboard_collect"
    n, P = _board_shape(board, who)
    _chk(sample_idx, torch.int32, "sample_idx")
    B = sample_idx.numel()
    if valid is not None:
        _chk(valid, torch.int32, "valid")
        if valid.numel() != B:
            raise capi.SamHipError("%s: valid must be int32 [B] = [%d]" % (who, B))
    EVAL_ROWS.require(res, _GPU, who + ": res")
    EVAL_ROWS.check(res, _GPU, who + ": res", B=B, P=P)
    capi.call("sam_evalboard_collect", capi.ptr(sample_idx), capi.ptr(valid), B, *[capi.ptr(res[k]) for k in EVALBOARD_ROW_KEYS], n, P,
              *[capi.ptr(board[k]) for k in EVALBOARD_KEYS], capi.stream_handle(), meta=dict(kernel="evalboard_collect", shape=(B, n, P)))


def evalboard_reduce(board, out=None):
    """sam_evalboard_reduce, one launch: -> float64 [8] on the device (allocated here when out is None; overwritten): the three score sums over the rows
    with seen > 0, the number of such rows, the three oracle sums over the same rows, the sum of their seen -- in score_answers' fixed order over the
    board's rows, so the sums depend on the board alone"""
    who = "evalboard_reduce"
    n, _ = _board_shape(board, who)
    if out is None:
        out = torch.empty(8, dtype=torch.float64, device=board["seen"].device)
    _chk(out, torch.float64, "out")
    if out.numel() != 8:
        raise capi.SamHipError("%s: out must be float64 [8]" % who)
    capi.call("sam_evalboard_reduce", capi.ptr(board["scores"]), capi.ptr(board["oracle"]), capi.ptr(board["seen"]), n, capi.ptr(out), capi.stream_handle(),
              meta=dict(kernel="evalboard_reduce", shape=(n,)))
    return out


def evalboard_merge(dst, src):
    """sam_evalboard_merge, one launch: every row src has seen goes into dst where dst's row is empty, dst.seen += src.seen, dst.status |= src.status.
    Two boards of one shape that share no memory."""
    who = "evalboard_merge"
    n, P = _board_shape(dst, who, "dst")
    if _board_shape(src, who, "src") != (n, P):
        raise capi.SamHipError("%s: dst is a board of n=%d P=%d, src of n=%d P=%d" % ((who, n, P) + _board_shape(src, who, "src")))
    capi.call("sam_evalboard_merge", *[capi.ptr(dst[k]) for k in EVALBOARD_KEYS], *[capi.ptr(src[k]) for k in EVALBOARD_KEYS], n, P, capi.stream_handle(),
              meta=dict(kernel="evalboard_merge", shape=(n, P)))


# ----------------------------------------------------------------------------- answer-space upper bounds: witness sequences (csrc/coverage.hip)
WITNESS_KEYS = WITNESS.keys                              # sam_answer_witness' five outputs, in the ABI's order


def answer_witness(answer_text, answer_text_len, ocr_text, ocr_text_len, index, L, out=None):
    """sam_answer_witness, one launch, one workgroup per sample (include/sam_hip_coverage.h): answer_text int32 [B, A <= 64, La <= 128] / answer_text_len
    int32 [B, A], ocr_text int32 [B, No <= 64, Lw <= 64] / ocr_text_len int32 [B, No], index: answers.vocab_index with its tensors on the GPU, L <= 64 the
    decoding length.  -> dict of the WITNESS_KEYS tensors (allocated here when out is None; every element is written): words int32 [B, A], reach int32
    [3, B, A], any int32 [3, B], seqs int64 [3, B * A, L], counts int32 [B, 4]; the leading 3 is the source (vocabulary, OCR tokens, both).  Nothing is
    read by the host."""
    who = "answer_witness"
    for t, name in ((answer_text, "answer_text"), (answer_text_len, "answer_text_len"), (ocr_text, "ocr_text"), (ocr_text_len, "ocr_text_len"),
                    (index["cp"], "index['cp']"), (index["len"], "index['len']"), (index["slots"], "index['slots']")):
        if not torch.is_tensor(t):
            raise capi.SamHipError("%s: %s must be a tensor" % (who, name))
        _chk(t, torch.int32, name)
    if answer_text.dim() != 3 or ocr_text.dim() != 3 or index["cp"].dim() != 2:
        raise capi.SamHipError("%s: answer_text [B, A, La], ocr_text [B, No, Lw] and index['cp'] [V, Lv] expected" % who)
    B, A, La = answer_text.shape
    No, Lw = ocr_text.shape[1:]
    V, Lv = index["cp"].shape
    if ocr_text.shape[0] != B or answer_text_len.numel() != B * A or ocr_text_len.numel() != B * No or index["len"].numel() != V or int(index["V"]) != V:
        raise capi.SamHipError("%s: answer_text_len [B, A], ocr_text [B, No, Lw] with ocr_text_len [B, No], index['len'] [V] expected (B=%d A=%d No=%d V=%d)"
                               % (who, B, A, No, V))
    L = int(L)
    if out is None:
        out = WITNESS.empty(answer_text.device, B=B, A=A, L=max(L, 0))
    WITNESS.require(out, _GPU, who + ": out")
    WITNESS.check(out, _GPU, who + ": out", B=B, A=A, L=max(L, 0))
    capi.call("sam_answer_witness", capi.ptr(answer_text), La, capi.ptr(answer_text_len), capi.ptr(ocr_text), Lw, capi.ptr(ocr_text_len), capi.ptr(index["cp"]), Lv,
              capi.ptr(index["len"]), capi.ptr(index["slots"]), B, A, La, No, Lw, V, Lv, index["slots"].numel(), int(index["EOS"]), L,
              *[capi.ptr(out[k]) for k in WITNESS_KEYS], capi.stream_handle(), meta=dict(kernel="answer_witness", shape=(B, A, No, L)))
    return out


# ----------------------------------------------------------------------------- PHOC from the OCR tokens' text (csrc/phoc.hip)
PHOC_DIM = 604


def _slot_text(who, text, text_len, counts, dst, n_max):
    """the operands phoc_from_text and fasttext_from_text share: text [B, n_max, Lw] (or 2-D with n_max), text_len, counts, the dst rows -> (B, n_max, Lw)"""
    _chk(text_len, torch.int32, "text_len")
    if not torch.is_tensor(text) or not text.is_cuda or text.dtype != torch.int32 or text.dim() not in (2, 3) or not text.is_contiguous():
        raise capi.SamHipError("%s: text must be a contiguous int32 GPU tensor [B, n_max, Lw] (or [B * n_max, Lw] with n_max)" % who)
    if text.dim() == 3:
        B, n_max, Lw = text.shape
    else:
        if not n_max or text.shape[0] % int(n_max):
            raise capi.SamHipError("%s: 2-D text needs n_max dividing its %d rows" % (who, text.shape[0]))
        n_max, Lw = int(n_max), text.shape[1]
        B = text.shape[0] // n_max
    if text_len.numel() != B * n_max:
        raise capi.SamHipError("%s: text_len must hold B * n_max = %d lengths, got %s" % (who, B * n_max, tuple(text_len.shape)))
    if counts is not None:
        _chk(counts, torch.int32, "counts")
        if counts.numel() != B:
            raise capi.SamHipError("%s: counts must be int32 [B] = [%d]" % (who, B))
    if not torch.is_tensor(dst) or not dst.is_cuda or dst.dtype not in _RAGGED_DST or dst.dim() != 2 or dst.stride(1) != 1 or dst.shape[0] != B * n_max:
        raise capi.SamHipError("%s: dst must be a row-major 2-D GPU tensor of bf16 / fp32 with B * n_max = %d rows" % (who, B * n_max))
    return B, n_max, Lw


def phoc_from_text(text, text_len, counts, dst, col0=0, normalize=False, eps=1e-12, n_max=None):
    """sam_phoc_from_text, one launch: text int32 [B, n_max, Lw] code points (Lw <= 64; the layout of score_table["ocr"]), text_len int32 [B, n_max] (clamped
    to [0, Lw] by the kernel), counts int32 [B] or None (valid slots per sample, clamped to [0, n_max]; slots at or past it give all-zero rows); dst
    [B * n_max, ld] fp32 / bf16 receives the 604 PHOC columns of slot (b, i) at column col0 -- the 0/1 row, or with `normalize` the row scaled exactly as
    ragged_expand / l2norm_pack scale the same 0/1 source row.  Columns outside [col0, col0 + 604) are not touched.  Nothing is read by the host: capturable.
    text may also be 2-D [B * n_max, Lw] with n_max given."""
    B, n_max, Lw = _slot_text("phoc_from_text", text, text_len, counts, dst, n_max)
    t_ = _tops()
    if t_ is not None:
        t_.phoc_from_text(text, text_len, counts, B, n_max, dst, int(col0), bool(normalize), float(eps))
        return dst
    capi.call("sam_phoc_from_text", capi.ptr(text), Lw, capi.ptr(text_len), capi.ptr(counts), B, n_max, Lw, capi.ptr(dst), dst.stride(0), int(col0),
              int(dst.dtype == torch.float32), int(bool(normalize)), float(eps), capi.stream_handle(), meta=dict(kernel="phoc_from_text", shape=(B, n_max, Lw)))
    return dst


# ----------------------------------------------------------------------------- answer tables from the answers' text (csrc/answer_text.hip)
def answer_table_from_text(answer_text, answer_text_len, ocr_text, ocr_text_len, index, out, max_match_num=20):
    """sam_answer_table_from_text, one launch, one workgroup per sample: answer_text int32 [B, A, La <= 128] / answer_text_len int32 [B, A] (the cleaned
    answers' exact code points), ocr_text int32 [B, No <= 64, Lw <= 64] / ocr_text_len int32 [B, No] (phoc.pack_ocr_text), index: answers.vocab_index with
    its tensors on the GPU; out: the eight ANSWER_TABLE_KEYS tensors at their capacities plus "status" int32 [B] (answers.table_outputs) -- every element
    is written: bit for bit answers.collate_answer_tables of answers.build_answer_table per sample, an all-zero row and one status bit where those raise.
    Nothing is read by the host."""
    for t, name in ((answer_text, "answer_text"), (answer_text_len, "answer_text_len"), (ocr_text, "ocr_text"), (ocr_text_len, "ocr_text_len"),
                    (index["cp"], "index['cp']"), (index["len"], "index['len']"), (index["slots"], "index['slots']")):
        if not torch.is_tensor(t):
            raise capi.SamHipError("answer_table_from_text: %s must be a tensor" % name)
        _chk(t, torch.int32, name)
    if answer_text.dim() != 3 or ocr_text.dim() != 3 or index["cp"].dim() != 2:
        raise capi.SamHipError("answer_table_from_text: answer_text [B, A, La], ocr_text [B, No, Lw] and index['cp'] [V, Lv] expected")
    B, A, La = answer_text.shape
    No, Lw = ocr_text.shape[1:]
    V, Lv = index["cp"].shape
    if ocr_text.shape[0] != B or answer_text_len.numel() != B * A or ocr_text_len.numel() != B * No or index["len"].numel() != V or int(index["V"]) != V:
        raise capi.SamHipError("answer_table_from_text: answer_text_len [B, A], ocr_text [B, No, Lw] with ocr_text_len [B, No], index['len'] [V] expected "
                               "(B=%d A=%d No=%d V=%d)" % (B, A, No, V))
    if out["seq_grp"].dim() != 3 or out["grp_idx"].dim() != 2 or out["grp_extra"].dim() != 2:
        raise capi.SamHipError("answer_table_from_text: out['seq_grp'] [B, S, L], out['grp_idx'] [B, G], out['grp_extra'] [B, E] expected")
    S, L = out["seq_grp"].shape[1:]
    G, E = out["grp_idx"].shape[1], out["grp_extra"].shape[1]
    ANSWER_TABLE_OUT.check(out, _GPU, "answer_table_from_text: out", B=B, S=S, L=L, G=G, E=E)
    t_ = _tops()
    if t_ is not None:
        t_.answer_table_from_text(answer_text, answer_text_len, ocr_text, ocr_text_len, index["cp"], index["len"], index["slots"], int(index["UNK"]), int(index["EOS"]),
                                  int(max_match_num), [out[k] for k in ANSWER_TABLE_KEYS] + [out["status"]])
        return out
    capi.call("sam_answer_table_from_text", capi.ptr(answer_text), La, capi.ptr(answer_text_len), capi.ptr(ocr_text), Lw, capi.ptr(ocr_text_len), capi.ptr(index["cp"]),
              Lv, capi.ptr(index["len"]), capi.ptr(index["slots"]), B, A, La, No, Lw, V, Lv, index["slots"].numel(), int(index["UNK"]), int(index["EOS"]), S, L, G, E,
              int(max_match_num), *[capi.ptr(out[k]) for k in ANSWER_TABLE_KEYS], capi.ptr(out["status"]), capi.stream_handle(),
              meta=dict(kernel="answer_table_from_text", shape=(B, A, No)))
    return out


# ----------------------------------------------------------------------------- the metrics' score tables from text (csrc/score_text.hip)
def score_table_from_text(answer_text, answer_text_len, ocr_text, ocr_text_len, ocr_count, out):
    """sam_score_table_from_text, one launch, one workgroup per sample: answer_text int32 [B, A <= 64, La <= 128] / answer_text_len int32 [B, A] (the cleaned
    answers' exact code points), ocr_text int32 [B, No, Lw <= 64] / ocr_text_len int32 [B, No] (phoc.pack_ocr_text), ocr_count int32 [B] (the sample's OCR
    tokens; the slots behind them become "<pad>"); out: the eight SCORE_TABLE_KEYS tensors at the capacities (A, Lw, Lg) plus "status" int32 [B]
    (metrics.score_table_outputs) -- every element is written: bit for bit metrics.collate_score_tables of metrics.build_score_table per sample for text
    that metrics.device_lowerable accepts, an all-zero row and one status bit where those raise.  Nothing is read by the host."""
    for t, name in ((answer_text, "answer_text"), (answer_text_len, "answer_text_len"), (ocr_text, "ocr_text"), (ocr_text_len, "ocr_text_len"),
                    (ocr_count, "ocr_count")):
        if not torch.is_tensor(t):
            raise capi.SamHipError("score_table_from_text: %s must be a tensor" % name)
        _chk(t, torch.int32, name)
    if answer_text.dim() != 3 or ocr_text.dim() != 3:
        raise capi.SamHipError("score_table_from_text: answer_text [B, A, La] and ocr_text [B, No, Lw] expected")
    B, A, La = answer_text.shape
    No, Lw = ocr_text.shape[1:]
    if ocr_text.shape[0] != B or answer_text_len.numel() != B * A or ocr_text_len.numel() != B * No or ocr_count.numel() != B:
        raise capi.SamHipError("score_table_from_text: answer_text_len [B, A], ocr_text [B, No, Lw] with ocr_text_len [B, No] and ocr_count [B] expected "
                               "(B=%d A=%d No=%d)" % (B, A, No))
    if out["gt_norm"].dim() != 3 or out["gt_norm"].shape[1] != A:
        raise capi.SamHipError("score_table_from_text: out['gt_norm'] [B, A, Lg] expected")
    Lg = out["gt_norm"].shape[2]
    SCORE_TABLE_OUT.check(out, _GPU, "score_table_from_text: out", B=B, A=A, Lg=Lg, No=max(No, 1), Lw=Lw)
    t_ = _tops()
    if t_ is not None:
        t_.score_table_from_text(answer_text, answer_text_len, ocr_text, ocr_text_len, ocr_count, [out[k] for k in SCORE_TABLE_KEYS] + [out["status"]])
        return out
    capi.call("sam_score_table_from_text", capi.ptr(answer_text), La, capi.ptr(answer_text_len), capi.ptr(ocr_text), Lw, capi.ptr(ocr_text_len), capi.ptr(ocr_count),
              B, A, La, No, Lw, Lg, *[capi.ptr(out[k]) for k in SCORE_TABLE_KEYS], capi.ptr(out["status"]), capi.stream_handle(),
              meta=dict(kernel="score_table_from_text", shape=(B, A, No)))
    return out


# ----------------------------------------------------------------------------- beam-search output to per-question results (csrc/eval_beams.hip)
EVAL_BEAMS_KEYS = EVAL_BEAMS.keys


def _eval_beams_operands(who, layout, seqs, cum, table, vocab_cp, vocab_len, beam, skip, totals, out):
    """the checks eval_beams and eval_beams_merged share, in one order and with one wording -> ((B, K, S, skip, A, Lg, No, Lw, V), out): out is allocated
    from `layout` when None"""
    _chk(seqs, torch.int64, "seqs")
    _chk(cum, torch.float32, "cum")
    _chk(vocab_cp, torch.int32, "vocab_cp")
    _chk(vocab_len, torch.int32, "vocab_len")
    SCORE_TABLE.require(table, _GPU)
    if seqs.dim() != 2 or table["gt_norm"].dim() != 3 or table["ocr"].dim() != 3 or vocab_cp.dim() != 2:
        raise capi.SamHipError(who + ": seqs [B * K, S], gt_norm [B, A, Lg], ocr [B, No, Lw], vocab_cp [V, Lw]")
    K, skip = int(beam), int(skip)
    R, S = seqs.shape
    B, A, Lg = table["gt_norm"].shape
    _, No, Lw = table["ocr"].shape
    V = vocab_cp.shape[0]
    if K < 1 or R != B * K or cum.numel() != R:
        raise capi.SamHipError(who + ": seqs has %d rows and cum %d elements for B = %d samples of K = %d beams" % (R, cum.numel(), B, K))
    SCORE_TABLE.check(table, _GPU, B=B, A=A, Lg=Lg, No=No, Lw=Lw)
    if vocab_cp.shape[1] != Lw or vocab_len.numel() != V:
        raise capi.SamHipError(who + ": vocab_cp %s / vocab_len %d for words of Lw = %d code points" % (tuple(vocab_cp.shape), vocab_len.numel(), Lw))
    L = max(S - skip, 0)
    if out is None:
        out = layout.empty(seqs.device, B=B, K=K, L=L, Lw=Lw)
    layout.check(out, _GPU, who + ": out", B=B, K=K, L=L, Lw=Lw)
    if totals is not None:
        _chk(totals, torch.float64, "totals")
        if totals.numel() != 4:
            raise capi.SamHipError(who + ": totals must be float64 [4]")
    return (B, K, S, skip, A, Lg, No, Lw, V), out


def eval_beams_outputs(B, K, L, Lw, device):
    """fresh output buffers of eval_beams: the nine EVAL_BEAMS_KEYS tensors for B samples of K beams, L scored steps and words of Lw code points"""
    return EVAL_BEAMS.empty(device, B=B, K=K, L=L, Lw=Lw)


def eval_beams(seqs, cum, table, vocab_cp, vocab_len, eos, beam, skip=1, totals=None, out=None):
    """sam_eval_beams, two launches (three with totals): seqs int64 [B * K, S] (complete_seqs; rows b * K .. b * K + K - 1 are sample b's beams), cum fp32
    [B * K] (topkscores), table the collated score table of the B samples on the GPU (not repeated per beam), vocab_cp int32 [V, Lw] / vocab_len int32 [V]
    (metrics.vocab_text), beam = K <= 64; the first `skip` columns of seqs are not scored (L = S - skip <= 64).  -> dict of the EVAL_BEAMS_KEYS tensors:
    beam_scores fp32 [B * K, 3] / beam_flags int32 [B * K] (bit for bit score_answers of seqs[:, skip:] on the table repeated K times), best int32 [B]
    (numpy.argmax of the sample's K cumulative scores), best_ids int64 [B, L] / best_scores fp32 [B, 3] / best_flags int32 [B] (the chosen beam's rows),
    oracle fp32 [B, 3] (the per-metric maximum over the beams), answer int32 [B, L * (Lw + 1)] / answer_len int32 [B] (the chosen beam's stripped string as
    code points, zeros behind it).  totals float64 [4]: best_scores' column sums and B are added to it, in a fixed order.  out: buffers from
    eval_beams_outputs (allocated here when None; every element is written).  Nothing is read by the host."""
    (B, K, S, skip, A, Lg, No, Lw, V), out = _eval_beams_operands("eval_beams", EVAL_BEAMS, seqs, cum, table, vocab_cp, vocab_len, beam, skip, totals, out)
    t_ = _tops()
    if t_ is not None:
        t_.eval_beams(seqs, cum, [table[k] for k in SCORE_TABLE_KEYS], vocab_cp, vocab_len, int(eos), K, skip, [out[k] for k in EVAL_BEAMS_KEYS], totals)
        return out
    capi.call("sam_eval_beams", capi.ptr(seqs), capi.ptr(cum), *[capi.ptr(table[k]) for k in SCORE_TABLE_KEYS], capi.ptr(vocab_cp), capi.ptr(vocab_len), B, K, S, skip,
              A, Lg, No, Lw, V, int(eos), *[capi.ptr(out[k]) for k in EVAL_BEAMS_KEYS], capi.ptr(totals), capi.stream_handle(),
              meta=dict(kernel="eval_beams", shape=(B, K, S)))
    return out


# ----------------------------------------------------------------------------- ... chosen by answer string: equal strings merged (csrc/beam_merge.hip)
EVAL_MERGED_KEYS = EVAL_MERGED.keys                      # EVAL_BEAMS_KEYS, then the seven outputs sam_eval_beams_merged adds, in the ABI's order


def eval_beams_merged_outputs(B, K, L, Lw, device):
    """fresh output buffers of eval_beams_merged: the sixteen EVAL_MERGED_KEYS tensors for B samples of K beams, L scored steps and words of Lw code points"""
    return EVAL_MERGED.empty(device, B=B, K=K, L=L, Lw=Lw)


def eval_beams_merged(seqs, cum, table, vocab_cp, vocab_len, eos, beam, skip=1, totals=None, out=None):
    """sam_eval_beams_merged (include/sam_hip_beam_merge.h), two launches (three with totals): eval_beams' operands, checked as it checks
    them.  -> dict of the EVAL_MERGED_KEYS tensors.  beam_scores, beam_flags and oracle are eval_beams' bit for bit; beam_answer int32 [B * K, L * (Lw + 1)]
    / beam_answer_len int32 [B * K] hold every beam's stripped string (the n-best list); group int32 [B * K] the lowest beam of the sample that spells the
    same string (a beam with an out-of-range id stays alone), n_groups int32 [B] how many distinct groups; mass fp32 [B * K] the log of the group's summed
    probabilities (a single member's own cum); best int32 [B] the member with the largest cum of the group with the largest mass, best_ids / best_scores /
    best_flags / answer / answer_len its rows, best_mass fp32 [B] that group's mass; plain_best int32 [B] what eval_beams returns as best.  totals float64
    [4]: the new best_scores' column sums and B are added to it.  out: buffers from eval_beams_merged_outputs (allocated here when None; every element is
    written).  Nothing is read by the host."""
    (B, K, S, skip, A, Lg, No, Lw, V), out = _eval_beams_operands("eval_beams_merged", EVAL_MERGED, seqs, cum, table, vocab_cp, vocab_len, beam, skip, totals,
                                                                  out)
    capi.call("sam_eval_beams_merged", capi.ptr(seqs), capi.ptr(cum), *[capi.ptr(table[k]) for k in SCORE_TABLE_KEYS], capi.ptr(vocab_cp), capi.ptr(vocab_len), B, K, S,
              skip, A, Lg, No, Lw, V, int(eos), *[capi.ptr(out[k]) for k in EVAL_MERGED_KEYS], capi.ptr(totals), capi.stream_handle(),
              meta=dict(kernel="eval_beams_merged", shape=(B, K, S)))
    return out


# ----------------------------------------------------------------------------- raw UTF-8 strings to cleaned code points (csrc/textprep.hip)
TEXT_FROM_UTF8_KEYS = ("text", "text_len", "status")
UNICODE_KEYS = ("block", "rec", "pool")                     # unicode_table.KEYS
QUESTION_FROM_UTF8_KEYS = ("question_text", "question_text_len", "status")


def _chk_unicode(table, who):
    """a table of unicode_table.build() with its tensors on the GPU"""
    if not isinstance(table, dict) or any(k not in table for k in UNICODE_KEYS):
        raise capi.SamHipError("%s: unicode must be a table of unicode_table.build() moved with unicode_table.to()" % who)
    for k in UNICODE_KEYS:
        _chk(table[k], torch.int32, "unicode[%r]" % k)
    if table["block"].numel() != 0x110000 >> 7 or table["rec"].numel() < 256 or table["rec"].numel() % 256 or table["pool"].numel() < 1:
        raise capi.SamHipError("%s: the table is block int32 [8704], rec int32 [n_blocks, 128, 2] and pool int32 [n_pool >= 1]" % who)


def _unicode_args(table):
    return (capi.ptr(table["block"]), table["block"].numel(), capi.ptr(table["rec"]), table["rec"].numel() // 256, capi.ptr(table["pool"]), table["pool"].numel())


def _utf8_io(who, raw, raw_off, keys, width, what, out):
    """raw uint8 [nbytes] / raw_off int32 [n + 1] and the three int32 outputs `keys` = (text [n, width], length [n], status [n]), allocated here when `out`
    is None; what: the names of n and width in the messages -> (n, out)"""
    _chk(raw, torch.uint8, "raw")
    _chk(raw_off, torch.int32, "raw_off")
    if raw.dim() != 1 or raw_off.dim() != 1 or raw_off.numel() < 2:
        raise capi.SamHipError("%s: raw uint8 [nbytes] and raw_off int32 [%s + 1] with %s >= 1" % (who, what[0], what[0]))
    n = raw_off.numel() - 1
    if out is None:
        out = {k: torch.empty(shape, dtype=torch.int32, device=raw.device) for k, shape in zip(keys, ((n, width), (n,), (n,)))}
    for k, nel in zip(keys, (n * width, n, n)):
        _chk(out[k], torch.int32, "out[%r]" % k)
        if out[k].numel() != nel:
            raise capi.SamHipError("%s: out[%r] has %d elements, expected %d (%s=%d %s=%d)" % (who, k, out[k].numel(), nel, what[0], n, what[1], width))
    return n, out


def text_from_utf8(raw, raw_off, L, mode, out=None, unicode=None):
    """sam_text_from_utf8, one launch, one wave per slot: raw uint8 [nbytes] (the slots' UTF-8 back to back), raw_off int32 [S + 1], L <= 128 code points per
    slot, mode: the bit set 1 lower ASCII | 2 delete , and ? | 4 "'s" -> " 's" | 8 strip (15 word_cleaner, 9 word_cleaner_lower, 0 verbatim).  -> dict:
    text int32 [S, L] (zeros behind the length), text_len int32 [S], status int32 [S] (1 not strict UTF-8, 2 over L code points, 4 bad offsets; a flagged
    slot has an all-zero row and length 0).  out: such a dict to write into (allocated here when None; every element is written).  Nothing is read by the
    host.  unicode: a table of unicode_table.build() on the GPU -- the launch is sam_text_from_utf8_unicode then, and bit 1 of mode is str.lower() of the
    whole slot (U+0130 and the final sigma included)."""
    L, mode = int(L), int(mode)
    if not 1 <= L <= 128 or not 0 <= mode <= 15:
        raise capi.SamHipError("text_from_utf8: L = %d must be in [1, 128] and mode = %d a set of the bits 1, 2, 4, 8" % (L, mode))
    S, out = _utf8_io("text_from_utf8", raw, raw_off, TEXT_FROM_UTF8_KEYS, L, ("S", "L"), out)
    if unicode is not None:
        _chk_unicode(unicode, "text_from_utf8")
    t_ = _tops()
    if unicode is not None:
        if t_ is not None:
            t_.text_from_utf8_unicode(raw, raw_off, L, mode, *[unicode[k] for k in UNICODE_KEYS], out["text"], out["text_len"], out["status"])
            return out
        capi.call("sam_text_from_utf8_unicode", capi.ptr(raw), raw.numel(), capi.ptr(raw_off), S, L, mode, *_unicode_args(unicode), capi.ptr(out["text"]),
                  capi.ptr(out["text_len"]), capi.ptr(out["status"]), capi.stream_handle(), meta=dict(kernel="text_from_utf8_unicode", shape=(S, L, raw.numel())))
        return out
    if t_ is not None:
        t_.text_from_utf8(raw, raw_off, L, mode, out["text"], out["text_len"], out["status"])
        return out
    capi.call("sam_text_from_utf8", capi.ptr(raw), raw.numel(), capi.ptr(raw_off), S, L, mode, capi.ptr(out["text"]), capi.ptr(out["text_len"]), capi.ptr(out["status"]),
              capi.stream_handle(), meta=dict(kernel="text_from_utf8", shape=(S, L, raw.numel())))
    return out


def question_from_utf8(raw, raw_off, Lq, unicode, out=None):
    """sam_question_from_utf8, one launch, one wave per question: raw uint8 [nbytes] (the questions' UTF-8 back to back), raw_off int32 [B + 1], Lq <= 1024,
    unicode: a table of unicode_table.build() on the GPU.  -> dict: question_text int32 [B, Lq] and question_text_len int32 [B] as
    wordpiece.pack_question_text writes them (an ASCII question verbatim, any other one normalised, PUNCT_FLAG on), status int32 [B] (1 not strict UTF-8,
    2 over Lq code points, 4 bad offsets, 8 a special-token string, 16 a code point only the host can normalise; a flagged question has an all-zero row and
    length 0).  out: such a dict to write into (allocated here when None; every element is written).  Nothing is read by the host."""
    Lq = int(Lq)
    if not 1 <= Lq <= 1024:
        raise capi.SamHipError("question_from_utf8: Lq = %d must be in [1, 1024]" % Lq)
    B, out = _utf8_io("question_from_utf8", raw, raw_off, QUESTION_FROM_UTF8_KEYS, Lq, ("B", "Lq"), out)
    _chk_unicode(unicode, "question_from_utf8")
    t_ = _tops()
    if t_ is not None:
        t_.question_from_utf8(raw, raw_off, Lq, *[unicode[k] for k in UNICODE_KEYS], *[out[k] for k in QUESTION_FROM_UTF8_KEYS])
        return out
    capi.call("sam_question_from_utf8", capi.ptr(raw), raw.numel(), capi.ptr(raw_off), B, Lq, *_unicode_args(unicode), *[capi.ptr(out[k]) for k in QUESTION_FROM_UTF8_KEYS],
              capi.stream_handle(), meta=dict(kernel="question_from_utf8", shape=(B, Lq, raw.numel())))
    return out


# ----------------------------------------------------------------------------- the build's sticky status record (csrc/answer_status.hip)
def answer_status_fold(status, state, step=0, step_dev=None):
    """sam_answer_status_fold, one launch of one wave: folds status int32 [B] (answer_table_from_text's out["status"]) into state int64 [4] = (OR of the
    status bits seen, number of flagged samples saturating at 2^62, step of the first flagged sample, its batch index -- the lowest of that step; the last
    two -1 while nothing was flagged).  The step is step_dev[0] + step (step_dev: int64 [1] device counter, or None), as answer_sample reads it.  Nothing
    is read by the host.  Returns state."""
    _chk(status, torch.int32, "status")
    _chk(state, torch.int64, "state")
    if status.numel() < 1 or state.numel() != 4:
        raise capi.SamHipError("answer_status_fold: status int32 [B >= 1] and state int64 [4] expected, got %d and %d elements" % (status.numel(), state.numel()))
    if step_dev is not None:
        _chk(step_dev, torch.int64, "step_dev")
    t_ = _tops()
    if t_ is not None:
        t_.answer_status_fold(status, step_dev, int(step), state)
        return state
    capi.call("sam_answer_status_fold", capi.ptr(status), status.numel(), capi.ptr(step_dev), int(step), capi.ptr(state), capi.stream_handle(),
              meta=dict(kernel="answer_status_fold", shape=(status.numel(),)))
    return state


# ----------------------------------------------------------------------------- the questions' WordPiece ids from their text (csrc/wordpiece.hip)
def wordpiece_from_text(text, text_len, index, indices, mask, count):
    """sam_wordpiece_from_text, one launch, one wave per sample: text int32 [B, Lq <= 1024] / text_len int32 [B] (wordpiece.pack_question_text; the length
    is clamped to [0, Lq] by the kernel), index: wordpiece.vocab_index with its tensors on the GPU; indices / mask int64 [B, T <= 64] (row-major; T columns of
    a wider row are allowed) and count int32 [B] receive [CLS] ids [SEP] cut to T with [PAD] = 0 behind, the 0/1 mask and the number of entries -- every
    element is written: element for element wordpiece.encode_host.  Nothing is read by the host."""
    for t, name in ((text, "question_text"), (text_len, "question_text_len"), (index["cp"], "index['cp']"), (index["len"], "index['len']"),
                    (index["slots"], "index['slots']"), (count, "count")):
        if not torch.is_tensor(t):
            raise capi.SamHipError("wordpiece_from_text: %s must be a tensor" % name)
        _chk(t, torch.int32, name)
    if text.dim() != 2 or index["cp"].dim() != 2:
        raise capi.SamHipError("wordpiece_from_text: question_text [B, Lq] and index['cp'] [V, Lv] expected")
    B, Lq = text.shape
    V, Lv = index["cp"].shape
    if text_len.numel() != B or count.numel() != B or index["len"].numel() != V or int(index["V"]) != V:
        raise capi.SamHipError("wordpiece_from_text: question_text_len [B], count [B], index['len'] [V] expected (B=%d V=%d)" % (B, V))
    for t, name in ((indices, "indices"), (mask, "mask")):
        if not torch.is_tensor(t) or not t.is_cuda or t.dtype != torch.int64 or t.dim() != 2 or t.shape[0] != B or t.stride(1) != 1 or (B > 1 and t.stride(0) < t.shape[1]):
            raise capi.SamHipError("wordpiece_from_text: %s must be a row-major int64 GPU tensor [B, T] = [%d, T] (row stride >= T)" % (name, B))
    T = indices.shape[1]
    if mask.shape[1] != T:
        raise capi.SamHipError("wordpiece_from_text: indices is [B, %d] and mask [B, %d]" % (T, mask.shape[1]))
    unk, cls, sep = int(index["UNK"]), int(index["CLS"]), int(index["SEP"])
    t_ = _tops()
    if t_ is not None:
        t_.wordpiece_from_text(text, text_len, index["cp"], index["len"], index["slots"], unk, cls, sep, indices, mask, count)
        return indices, mask, count
    capi.call("sam_wordpiece_from_text", capi.ptr(text), Lq, capi.ptr(text_len), capi.ptr(index["cp"]), Lv, capi.ptr(index["len"]), capi.ptr(index["slots"]), B, Lq, V, Lv,
              index["slots"].numel(), unk, cls, sep, T, capi.ptr(indices), indices.stride(0) if B > 1 else T, capi.ptr(mask), mask.stride(0) if B > 1 else T,
              capi.ptr(count), capi.stream_handle(), meta=dict(kernel="wordpiece_from_text", shape=(B, Lq, T)))
    return indices, mask, count


# ----------------------------------------------------------------------------- the OCR tokens' FastText vectors from their text (csrc/fasttext.hip)
def fasttext_from_text(text, text_len, counts, index, dst, col0=0, normalize=False, eps=1e-12, n_max=None):
    """sam_fasttext_from_text, one launch, one wave per slot: text int32 [B, n_max, Lw] code points (Lw <= 64; phoc.pack_ocr_text), text_len int32 [B, n_max]
    (clamped to [0, Lw] by the kernel), counts int32 [B] or None (valid slots per sample, clamped to [0, n_max]; slots at or past it give all-zero rows);
    index: fasttext.model_index with its tensors on the GPU (fasttext.index_to).  dst [B * n_max, ld] fp32 / bf16 receives the dim columns of slot (b, i) at
    column col0 (col0 and ld multiples of 4): the fp32 vector of fasttext.vectors_host_text bit for bit (bf16: rounded once), or with `normalize` what
    l2norm_pack writes from that fp32 row.  Columns outside [col0, col0 + dim) are not touched.  Nothing is read by the host: capturable.
    text may also be 2-D [B * n_max, Lw] with n_max given."""
    B, n_max, Lw = _slot_text("fasttext_from_text", text, text_len, counts, dst, n_max)
    matrix, cp, ln, slots = index["matrix"], index["cp"], index["len"], index["slots"]
    for t, name in ((cp, "index['cp']"), (ln, "index['len']"), (slots, "index['slots']")):
        if not torch.is_tensor(t):
            raise capi.SamHipError("fasttext_from_text: %s must be a tensor" % name)
        _chk(t, torch.int32, name)
    _chk(matrix, torch.float32, "index['matrix']")
    nwords, bucket, dim = int(index["nwords"]), int(index["bucket"]), int(index["dim"])
    if matrix.dim() != 2 or tuple(matrix.shape) != (nwords + bucket, dim) or cp.dim() != 2 or cp.shape[0] != nwords or ln.numel() != nwords:
        raise capi.SamHipError("fasttext_from_text: index['matrix'] must be [nwords + bucket, dim] = [%d, %d], index['cp'] [nwords, Lv], index['len'] [nwords]; got %s %s %s" % (
            nwords + bucket, dim, tuple(matrix.shape), tuple(cp.shape), tuple(ln.shape)))
    minn, maxn, eos = int(index["minn"]), int(index["maxn"]), int(index["eos"])
    t_ = _tops()
    if t_ is not None:
        t_.fasttext_from_text(text, text_len, counts, B, n_max, matrix, cp, ln, slots, minn, maxn, bucket, nwords, eos, dst, int(col0), bool(normalize), float(eps))
        return dst
    capi.call("sam_fasttext_from_text", capi.ptr(text), Lw, capi.ptr(text_len), capi.ptr(counts), B, n_max, Lw, capi.ptr(matrix), matrix.stride(0), capi.ptr(cp),
              cp.stride(0), capi.ptr(ln), capi.ptr(slots), cp.shape[1], slots.numel(), minn, maxn, bucket, nwords, eos, dim, capi.ptr(dst),
              dst.stride(0) if B * n_max > 1 else dst.shape[1], int(col0), int(dst.dtype == torch.float32), int(bool(normalize)), float(eps), capi.stream_handle(),
              meta=dict(kernel="fasttext_from_text", shape=(B, n_max, Lw)))
    return dst

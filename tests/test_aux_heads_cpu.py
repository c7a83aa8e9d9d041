"""CPU (no GPU needed): the spatial auxiliary heads (use_aux_heads, sam/sa_m4c.py:173-177, 316-347) -- module surface against the reference golden
(tests/golden/aux_heads.npz, made by tests/golden/make_golden_aux.py), an fp32 restatement of _forward_aux pinned to that golden, and the C ABI of the
pair kernels (bound, argument errors reported before any launch)."""
import math
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import oracle_cases as OC
from tests.golden import common as C

GOLDEN = os.path.join(C.GOLDEN_DIR, "aux_heads.npz")
AUX = ("origin_transform", "dest_transform", "spatial_classifier")
# the golden's heads run at hidden size 32 (tests/golden/make_golden_aux.py)
GOLDEN_SHAPES = {**{"%s.logit_fc.%s" % (m, k): s for m in ("origin_transform", "dest_transform")
                    for k, s in (("0.weight", (128, 32)), ("0.bias", (128,)), ("2.weight", (128,)), ("2.bias", (128,)), ("3.weight", (32, 128)), ("3.bias", (32,)))},
                 "spatial_classifier.weight": (12, 32), "spatial_classifier.bias": (12,)}


def golden():
    return np.load(GOLDEN)


def golden_params(shapes):
    """the aux parameters of the golden: common.det_param("aux." + name) (tests/golden/make_golden_aux.py), for {name: shape}"""
    return {n: torch.from_numpy(C.det_param("aux." + n, tuple(s), 0.1)) for n, s in shapes.items()}


def golden_keys(g):
    keys = bytes(g["keys_utf8"]).decode().split("\n")
    nd, flat, shapes, k = g["key_ndim"], list(g["key_shapes"]), [], 0
    for n in nd:
        shapes.append(tuple(int(s) for s in flat[k: k + n]))
        k += n
    return keys, shapes


# ---------------------------------------------------------------------------------------------- fp32 restatement of the reference
def simple_classifier_ref(x, p, prefix):
    """SimpleClassifier (sa_m4c.py:1031-1042) in fp32: Linear -> erf-GELU -> BertLayerNorm (TF style, eps 1e-12 inside the sqrt) -> Linear"""
    h = F.linear(x, p[prefix + ".logit_fc.0.weight"], p[prefix + ".logit_fc.0.bias"])
    h = h * 0.5 * (1.0 + torch.erf(h / math.sqrt(2.0)))
    u = h.mean(-1, keepdim=True)
    s = (h - u).pow(2).mean(-1, keepdim=True)
    h = (h - u) / torch.sqrt(s + 1e-12)
    h = p[prefix + ".logit_fc.2.weight"] * h + p[prefix + ".logit_fc.2.bias"]
    return F.linear(h, p[prefix + ".logit_fc.3.weight"], p[prefix + ".logit_fc.3.bias"])


def pair_ref(o, d, w, b, fusion):
    """spatial_classifier(f(O_i, D_j)) with the pair features materialised, as the reference does (for any n, not just 150)"""
    oi, dj = o.unsqueeze(2), d.unsqueeze(1)
    f = oi * dj if fusion == "mul" else oi + dj
    return F.linear(f, w, b)


def forward_aux_ref(seq, p, n_txt, n, fusion):
    """_forward_aux (sa_m4c.py:316-347) on mmt_seq_output: X = seq[:, T : T + n] -> [B, n, n, 12]"""
    x = seq[:, n_txt: n_txt + n]
    o = simple_classifier_ref(x, p, "origin_transform")
    d = simple_classifier_ref(x, p, "dest_transform")
    return pair_ref(o, d, p["spatial_classifier.weight"], p["spatial_classifier.bias"], fusion)


def _model(fusion="mul"):
    import sam_textvqa_amd.modules as M
    mcfg, tcfg = OC.sam4c_configs("sam4c_small_c3", M.BertConfig)
    mcfg.use_aux_heads, mcfg.aux_spatial_fusion = True, fusion
    d = C.SAM4C_CASES["sam4c_small_c3"]["dims"]
    return M.SAM4C(mcfg, tcfg, num_answers=d["V"], bos_idx=1)


# ---------------------------------------------------------------------------------------------- module surface
def test_state_dict_keys_shapes_and_order_match_the_reference():
    keys, shapes = golden_keys(golden())
    sd = _model().state_dict()
    assert list(sd) == keys
    assert [tuple(v.shape) for v in sd.values()] == shapes
    assert [k for k in keys if k.startswith(AUX)] == keys[-14:]          # registered after the classifier: they close the state dict
    assert keys[-14] == "origin_transform.logit_fc.0.weight" and keys[-1] == "spatial_classifier.bias"


def test_aux_params_sit_where_the_reference_puts_them_in_optimizer_group_0():
    g = golden()
    model = _model()
    g0 = model.get_optimizer_parameters(1e-4)[0]["params"]
    names = {id(p): n for n, p in model.named_parameters()}
    pos = [i for i, p in enumerate(g0) if names[id(p)].startswith(AUX)]
    assert pos + [len(g0)] == [int(v) for v in g["group0_aux_pos"]]
    assert set(map(id, model.aux_parameters())) == {id(g0[i]) for i in pos}


def test_without_the_switch_nothing_changes():
    import sam_textvqa_amd.modules as M
    mcfg, tcfg = OC.sam4c_configs("sam4c_small_c3", M.BertConfig)
    model = M.SAM4C(mcfg, tcfg, num_answers=40, bos_idx=1)
    assert not model.use_aux_heads and model.aux_parameters() == []
    assert not any(k.startswith(AUX) for k in model.state_dict())


def test_unknown_fusion_raises_value_error():
    with pytest.raises(ValueError):
        _model("concat")
    for f in ("mul", "add"):
        assert _model(f).aux_spatial_fusion == f


def test_aux_params_rank_with_the_classifier_and_are_listed_in_the_head_unit():
    """flat layout: the aux heads come right after the classifier, before the MMT group -- listed in the reducer's "head" unit so that the region
    walk from the top of the buffer is not broken by an unlisted range (checked on the CPU with a CPU-resident FlatParams)"""
    from sam_textvqa_amd import params
    model = _model()
    rank = model._sam_param_rank
    assert [rank(n) for n, _ in model.named_parameters() if n.startswith(AUX)] == [5] * 14
    order = params._ordered_params(model)
    names = {id(p): n for n, p in model.named_parameters()}
    seq = [names[id(p)] for p in order]
    cls = seq.index("classifier.bias")
    assert all(s.startswith(AUX) for s in seq[cls + 1: cls + 15])


@pytest.mark.parametrize("fusion", ["mul", "add"])
def test_fp32_restatement_reproduces_the_reference_golden(fusion):
    g = golden()
    p = {n: v.double().requires_grad_(True) for n, v in golden_params(GOLDEN_SHAPES).items()}
    seq = torch.from_numpy(g["seq"]).double().requires_grad_(True)
    assert torch.equal(seq.float(), torch.from_numpy(C.det_uniform("aux.seq", tuple(seq.shape), -2.0, 2.0)))
    out = forward_aux_ref(seq, p, 4, 150, fusion)
    assert out.shape == (2, 150, 150, 12)
    rows = list(g["rows"])
    ref = torch.from_numpy(g[fusion + ".out"]).double()
    assert (out[:, rows] - ref).abs().max().item() <= 1e-5 * ref.abs().max().item()
    gup = torch.from_numpy(C.det_uniform("aux.G", tuple(out.shape))).double()
    (out * gup).sum().backward()
    dref = torch.from_numpy(g[fusion + ".d_seq"]).double()
    assert (seq.grad - dref).abs().max().item() <= 1e-5 * dref.abs().max().item()
    for n, v in p.items():
        r = torch.from_numpy(g[fusion + ".g." + n]).double()
        assert (v.grad - r).abs().max().item() <= 1e-4 * r.abs().max().item() + 1e-6, n


# ---------------------------------------------------------------------------------------------- C ABI
def test_pair_entry_points_are_bound_and_reject_bad_arguments_without_a_gpu():
    from sam_textvqa_amd import _capi, ops
    for name in ("sam_aux_pair_fwd", "sam_aux_pair_bwd", "sam_aux_pair_bwd_ws_bytes"):
        assert name in _capi.SIGNATURES
    assert "sam_aux_pair_bwd_ws_bytes" in _capi.NO_STATUS
    assert _capi.call("sam_aux_pair_bwd_ws_bytes", 64, 150) > 0
    assert _capi.call("sam_aux_pair_bwd_ws_bytes", 0, 150) == 0
    with pytest.raises(_capi.SamHipError, match="null pointer"):
        _capi.call("sam_aux_pair_fwd", None, None, None, None, 2, 150, 0, None, None)
    with pytest.raises(_capi.SamHipError, match="null pointer"):
        _capi.call("sam_aux_pair_bwd", None, None, None, None, 2, 150, 0, None, None, None, None, 1, None, 0, None)
    fake = 1 << 20            # never dereferenced: the shape / fusion checks reject the call before any launch
    with pytest.raises(_capi.SamHipError, match="empty shape"):
        _capi.call("sam_aux_pair_fwd", fake, fake, fake, fake, 2, 0, 0, fake, None)
    with pytest.raises(_capi.SamHipError, match="unknown fusion"):
        _capi.call("sam_aux_pair_fwd", fake, fake, fake, fake, 2, 5, 7, fake, None)
    with pytest.raises(_capi.SamHipError, match="workspace"):
        _capi.call("sam_aux_pair_bwd", fake, fake, fake, fake, 2, 150, 0, fake, fake, fake, fake, 1, fake, 16, None)
    # the Python wrappers: CPU tensors and unknown fusions are refused, no fallback
    o = torch.zeros(2, 5, 32)
    with pytest.raises(_capi.SamHipError):
        ops.aux_pair_fwd(o, o, torch.zeros(12, 32), torch.zeros(12))
    with pytest.raises(ValueError):
        ops.aux_pair_fwd(o, o, torch.zeros(12, 32), torch.zeros(12), fusion="concat")

"""CPU (no GPU needed): the second public header, include/sam_hip_pipeline.h, binds into tables of its own next to the unchanged sam_hip.h ABI; every
argument rejection of sam_mask_bits_from_boxes happens before any device call; the batch's opt-in rules (spatial_from_boxes)."""
import ctypes
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_pipeline_header_binds_into_its_own_tables_and_leaves_the_model_abi_alone():
    from ctypes import c_double, c_int, c_int64, c_uint, c_void_p as vp
    import sam_textvqa_amd._build as b
    from sam_textvqa_amd import _capi
    i = c_int
    assert _capi.HEADER_SIGNATURES["pipeline"] == {"sam_mask_bits_from_boxes": [vp, vp, c_int64, i, vp, c_int64, i, i, i, i, i, i, i, i, c_double, c_uint, vp, vp]}
    assert _capi.HEADER_RESTYPES["pipeline"] == {"sam_mask_bits_from_boxes": c_int}
    # the tables of sam_hip.h hold what they held
    assert len(_capi.SIGNATURES) == 77 and not set(_capi.HEADER_SIGNATURES["pipeline"]) & set(_capi.SIGNATURES)
    assert set(_capi.RESTYPES) == set(_capi.SIGNATURES) and len(_capi.RET_I64) == 10 and len(_capi.STRUCTS) == 9
    assert not set(_capi.HEADER_SIGNATURES["pipeline"]) & _capi.NO_STATUS
    model_header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "sam_hip.h")).read(), flags=re.S)
    assert "sam_mask_bits_from_boxes" not in model_header and "pipeline" not in model_header
    # every argument of the declaration is bound: comma count + 1
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "sam_hip_pipeline.h")).read(), flags=re.S)
    params = re.search(r"\bsam_mask_bits_from_boxes\s*\(([^)]*)\)", src).group(1)
    assert params.count(",") + 1 == len(_capi.HEADER_SIGNATURES["pipeline"]["sam_mask_bits_from_boxes"])
    # one library: it exports the symbol, keeps ABI version 9, and its digest covers the new header and source
    assert hasattr(ctypes.CDLL(b.build()), "sam_mask_bits_from_boxes")
    l = _capi.lib()
    assert l.sam_abi_version() == 9 and l.sam_build_digest().decode() == b._digest()
    assert l.sam_mask_bits_from_boxes.argtypes == _capi.HEADER_SIGNATURES["pipeline"]["sam_mask_bits_from_boxes"] and l.sam_mask_bits_from_boxes.restype is c_int
    assert os.path.join(b.CSRC, "mask_boxes.hip") in b.sources()
    with pytest.raises(_capi.SamHipError, match="neither"):
        _capi.call("sam_no_such_entry_point")


def test_a_malformed_declaration_is_blamed_on_the_header_it_is_in():
    from sam_textvqa_amd import _capi
    with pytest.raises(_capi.SamHipError, match=r"^sam_hip_pipeline\.h: .*long n"):
        _capi.parse_header("int sam_f(const float* x, long n, void* stream);\n", header="sam_hip_pipeline.h")
    with pytest.raises(_capi.SamHipError, match=r"^sam_hip\.h: "):
        _capi.parse_header("long sam_f(void);\n")


def test_digest_covers_the_pipeline_header(tmp_path, monkeypatch):
    import sam_textvqa_amd._build as b
    was = b._digest()
    other = tmp_path / "sam_hip_pipeline.h"
    other.write_text(open(b.HEADERS["pipeline"]).read() + "\n/* changed */\n")
    monkeypatch.setitem(b.HEADERS, "pipeline", str(other))
    assert b._digest() != was


# a valid argument set (pointers are never dereferenced on the host: any non-null address will do), then one change per rejection
OK = dict(base=1 << 12, obj=1 << 13, ld_obj=5, n_obj=7, ocr=1 << 14, ld_ocr=5, n_ocr=6, f64=0, B=2, N=21, NW=1, T=5, H=12, context=3, thr=0.5, quad=(1 << 1) | (1 << 2),
          out=1 << 15)
REJECTED = [
    ("null base", dict(base=None), "null"),
    ("null obj_boxes", dict(obj=None), "null"),
    ("null out", dict(out=None), "null"),
    ("ocr_boxes NULL with n_ocr > 0", dict(ocr=None), "ocr_boxes"),
    ("context 2", dict(context=2), "context"),
    ("context 11", dict(context=11), "context"),
    ("context 0", dict(context=0), "context"),
    ("H < 12", dict(H=11), "H"),
    ("NW * 32 < N", dict(N=40, NW=1), "NW"),
    ("T + n_obj + n_ocr > N", dict(T=9), "exceeds N"),
    ("ld_obj < 4", dict(ld_obj=3), "stride"),
    ("ld_ocr < 4", dict(ld_ocr=2), "stride"),
    ("quadrant 3", dict(quad=1 << 3), "quadrant"),
    ("quadrant 5", dict(quad=(1 << 1) | (1 << 5)), "quadrant"),
    ("quadrant 6", dict(quad=1 << 6), "quadrant"),
    ("quadrant 10", dict(quad=1 << 10), "quadrant"),
]


def _call(capi, a):
    p = lambda v: None if v is None else ctypes.c_void_p(v)
    return capi.lib().sam_mask_bits_from_boxes(p(a["base"]), p(a["obj"]), a["ld_obj"], a["n_obj"], p(a["ocr"]), a["ld_ocr"], a["n_ocr"], a["f64"], a["B"], a["N"], a["NW"],
                                               a["T"], a["H"], a["context"], a["thr"], a["quad"], p(a["out"]), None)


@pytest.mark.parametrize("name,change,word", REJECTED, ids=[r[0] for r in REJECTED])
def test_argument_rejections_come_before_any_device_call(name, change, word):
    """SAM_ERR_ARG with a message naming the argument, on a box without a GPU: nothing was launched"""
    from sam_textvqa_amd import _capi
    rc = _call(_capi, dict(OK, **change))
    assert rc == _capi.CONSTANTS["SAM_ERR_ARG"] == -1, name
    msg = _capi.lib().sam_last_error().decode()
    assert msg.startswith("sam_mask_bits_from_boxes:") and word in msg, msg
    with pytest.raises(_capi.SamHipError, match="sam_mask_bits_from_boxes"):              # the same through capi.call, which looks in both tables
        a = dict(OK, **change)
        p = lambda v: None if v is None else ctypes.c_void_p(v)
        _capi.call("sam_mask_bits_from_boxes", p(a["base"]), p(a["obj"]), a["ld_obj"], a["n_obj"], p(a["ocr"]), a["ld_ocr"], a["n_ocr"], a["f64"], a["B"], a["N"], a["NW"],
                   a["T"], a["H"], a["context"], a["thr"], a["quad"], p(a["out"]), None)


def test_ops_wrapper_rejects_cpu_tensors():
    from sam_textvqa_amd import ops
    from sam_textvqa_amd._capi import SamHipError
    base = torch.zeros(1, 1, 8, 1, dtype=torch.int32)
    with pytest.raises(SamHipError):
        ops.mask_bits_from_boxes(base, torch.zeros(1, 4, 5), torch.zeros(1, 2, 5), 1, 12, (1, 2), 3)          # CPU tensors: rejected, no fallback


def _encoder(mix="share3"):
    import sam_textvqa_amd.modules as M
    cfg = M.BertConfig.from_dict(dict(hidden_size=768, num_spatial_relations=12, max_seq_length=4, num_decoding_steps=2, attention_mask_quadrants=[1, 2],
                                      intermediate_size=64, layer_type_list=["n", "s"], mix_list=["none", mix]))
    return M, M.BertSpatialEncoder(cfg)


def test_batch_opt_in_rules():
    M, enc = _encoder("share5")
    obj, ocr = torch.zeros(2, 3, 5), torch.zeros(2, 2, 5)
    # the flag: the layer receives the batch's boxes and the context matrix_type_map names; the threshold defaults to 0.5
    rel = enc._adjacency_for({"spatial_from_boxes": True, "pad_obj_bboxes": obj, "pad_ocr_bboxes": ocr}, "share5")
    assert isinstance(rel, M.BoxRelations) and rel.obj_boxes is obj and rel.ocr_boxes is ocr and (rel.context, rel.distance_threshold) == (5, 0.5)
    rel = enc._adjacency_for({"spatial_from_boxes": True, "spatial_distance_threshold": 0.25, "pad_obj_bboxes": obj, "pad_ocr_bboxes": ocr}, "none")
    assert (rel.context, rel.distance_threshold) == (1, 0.25)
    # the flag together with the relation tensors: one form only
    with pytest.raises(ValueError, match="spatial_from_boxes"):
        enc._adjacency_for({"spatial_from_boxes": True, "spatial_adj_matrices": {"5": None}, "pad_obj_bboxes": obj, "pad_ocr_bboxes": ocr}, "share5")
    # without the flag nothing changes: the relation tensor of the context, or the KeyError that names mix_list
    adj = torch.zeros(2, 5, 5, 12, dtype=torch.int8)
    assert enc._adjacency_for({"spatial_adj_matrices": {"5": adj}}, "share5") is adj
    assert enc._adjacency_for({"spatial_from_boxes": False, "spatial_adj_matrices": {"5": adj}}, "share5") is adj
    with pytest.raises(KeyError, match="mix_list"):
        enc._adjacency_for({"spatial_adj_matrices": {"3": None, "1": None}}, "share5")
    assert M.spatial_box_items({}) == () and M.spatial_box_items({"spatial_from_boxes": True, "spatial_distance_threshold": 1}) == \
        (("spatial_from_boxes", True), ("spatial_distance_threshold", 1.0))


def test_model_forward_refuses_the_flag_next_to_relation_tensors():
    """SAM4C.forward checks the pair of keys before anything runs (as it does for ragged rows next to padded features)"""
    import sam_textvqa_amd.modules as M
    from sam_textvqa_amd.synthetic import mmt_config_dict, text_bert_config_dict
    md = mmt_config_dict(3, ("s",), n_dec=2, T=4, n_obj=3, n_ocr=2)
    md.update(intermediate_size=64)
    model = M.SAM4C(M.BertConfig.from_dict(md), M.BertConfig.from_dict(dict(text_bert_config_dict(), num_hidden_layers=1, intermediate_size=64)), num_answers=20, bos_idx=1)
    with pytest.raises(ValueError, match="spatial_from_boxes"):
        model({"spatial_from_boxes": True, "spatial_adj_matrices": {"3": torch.zeros(1, 5, 5, 12, dtype=torch.int8)}})


def test_synthetic_and_ragged_carry_the_opt_in():
    from sam_textvqa_amd import ragged as R
    from sam_textvqa_amd.synthetic import clone_batch, make_batch
    a = make_batch(2, 5, 7, 6, 3, vocab=50, device="cpu", seed=4)
    b = make_batch(2, 5, 7, 6, 3, vocab=50, device="cpu", seed=4, spatial="boxes")
    assert "spatial_from_boxes" not in a and "spatial_adj_matrices" in a                                        # the default is what it was
    assert b["spatial_from_boxes"] is True and "spatial_adj_matrices" not in b
    assert set(a) - {"spatial_adj_matrices"} == set(b) - {"spatial_from_boxes"}
    assert all(torch.equal(a[k], b[k]) for k in b if torch.is_tensor(b[k]))
    assert clone_batch(b)["spatial_from_boxes"] is True and "spatial_adj_matrices" not in clone_batch(b)
    with pytest.raises(ValueError):
        make_batch(1, 5, 7, 6, 3, vocab=50, device="cpu", spatial="both")
    b["spatial_distance_threshold"] = 0.4
    rag = R.from_padded(b)
    assert rag["spatial_from_boxes"] is True and rag["spatial_distance_threshold"] == 0.4
    pad = R.to_padded(rag)
    assert pad["spatial_from_boxes"] is True and pad["spatial_distance_threshold"] == 0.4 and torch.equal(pad["pad_obj_bboxes"], b["pad_obj_bboxes"])
    samples = [dict(obj_features=torch.zeros(2, 8), obj_bboxes=torch.zeros(2, 5), ocr_features=torch.zeros(1, 8), ocr_fasttext=torch.zeros(1, 300),
                    ocr_phoc=torch.zeros(1, 604), ocr_bboxes=torch.zeros(1, 5))]
    plain = R.collate_ragged(samples, 3, 2)
    assert "spatial_from_boxes" not in plain and "spatial_distance_threshold" not in plain
    opted = R.collate_ragged(samples, 3, 2, spatial_from_boxes=True, spatial_distance_threshold=0.3)
    assert opted["spatial_from_boxes"] is True and opted["spatial_distance_threshold"] == 0.3 and set(opted) - set(plain) == set(("spatial_from_boxes", "spatial_distance_threshold"))

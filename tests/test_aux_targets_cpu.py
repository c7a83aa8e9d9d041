"""CPU: the aux loss's targets in one launch without a GPU -- the torch twin of the kernel, the third table of the header
registry, and the entry point's argument checks."""
import ctypes
import os

import pytest
import torch

MASK_DTYPES = (torch.bool, torch.uint8, torch.int8, torch.int32, torch.int64)


def make_case(b, n_obj, n_ocr, seed, multi_hot=True, dead_sample=True):
    """(rel int8 [B, n, n, 12] -- mostly one-hot, some all-zero rows, some multi-hot --, obj_mask, ocr_mask as int64 with 0 / non-zero elements)"""
    gen = torch.Generator().manual_seed(seed)
    n = n_obj + n_ocr
    code = torch.randint(0, 13, (b, n, n), generator=gen)
    rel = (code.unsqueeze(-1) == torch.arange(1, 13)).to(torch.int8)
    if multi_hot:
        rel |= (torch.rand(b, n, n, 12, generator=gen) < 0.05).to(torch.int8)
    mask = (torch.rand(b, n, generator=gen) < 0.7).long() * torch.randint(1, 100, (b, n), generator=gen)
    if dead_sample and b > 1:
        mask[-1] = 0
    return rel, mask[:, :n_obj].contiguous(), mask[:, n_obj:].contiguous()


def as_dtype(mask, dtype):
    return mask.ne(0) if dtype is torch.bool else mask.clamp(max=100).to(dtype)


# ---------------------------------------------------------------------------------------------- host twin
@pytest.mark.parametrize("b,n_obj,n_ocr", [(3, 5, 4), (2, 7, 0), (1, 1, 0)])
@pytest.mark.parametrize("dtype", MASK_DTYPES)
def test_host_twin(b, n_obj, n_ocr, dtype):
    from sam_textvqa_amd import ops
    rel, om, cm = make_case(b, n_obj, n_ocr, seed=b * 10 + n_ocr)
    codes, valid = ops.aux_targets_host(rel, as_dtype(om, dtype), as_dtype(cm, dtype))
    want_valid = torch.cat([om, cm], -1).ne(0)
    assert valid.dtype == torch.uint8 and torch.equal(valid, want_valid.to(torch.uint8))
    pair = want_valid.unsqueeze(2) & want_valid.unsqueeze(1)
    full = ops.codes_from_relation_tensor(rel, check=False)
    assert codes.dtype == torch.uint8 and tuple(codes.shape) == (b, n_obj + n_ocr, n_obj + n_ocr)
    assert torch.equal(codes[pair], full[pair]) and bool((codes[~pair] == 0).all())
    if b == 3:
        assert bool(((rel.sum(-1) > 1) & pair).any())                                                         # multi-hot rows are in the case
        assert not bool(want_valid[-1].any()) and bool((codes[-1] == 0).all())                                # ... and a sample with no valid row
        assert bool(pair.any()) and bool((~pair & (full != 0)).any())                                         # zeroing changes something
    none, valid2 = ops.aux_targets_host(None, as_dtype(om, dtype), as_dtype(cm, dtype))
    assert none is None and torch.equal(valid2, valid)


def test_host_twin_equals_the_codes_on_one_hot_rows():
    from sam_textvqa_amd import ops
    rel, om, cm = make_case(2, 6, 3, seed=1, multi_hot=False, dead_sample=False)
    om[:], cm[:] = 1, 1
    codes, valid = ops.aux_targets_host(rel, om, cm)
    assert bool(valid.all()) and torch.equal(codes, ops.codes_from_relation_tensor(rel)) and int(codes.max()) <= 12


# ---------------------------------------------------------------------------------------------- registry
def test_the_extension_table_holds_the_new_name_and_no_other_table_changed():
    from sam_textvqa_amd import _build, _capi
    vp, i, i64 = ctypes.c_void_p, ctypes.c_int, ctypes.c_int64
    assert list(_build.ABI_EXTENSIONS) == list(_capi.EXTENSION_SIGNATURES) == list(_capi.EXTENSION_RESTYPES) == ["aux_targets"]
    assert _capi.EXTENSION_SIGNATURES["aux_targets"] == {"sam_aux_targets": [vp, vp, i64, i, vp, i64, i, i, i, i, vp, vp, vp]}
    assert _capi.EXTENSION_RESTYPES["aux_targets"] == {"sam_aux_targets": i}
    assert "sam_aux_targets" not in _capi.SIGNATURES and "sam_aux_targets" not in _capi.NO_STATUS and "sam_aux_targets" not in _capi.PART_VALUES
    assert all("sam_aux_targets" not in t for t in list(_capi.HEADER_SIGNATURES.values()) + list(_capi.PART_SIGNATURES.values()))
    assert list(_build.HEADERS) == ["abi", "pipeline", "text", "answers", "step", "question", "fasttext", "metrics", "eval", "textprep", "unicode"]
    assert list(_build.ABI_PARTS) == ["aux_loss"] and len(_capi.SIGNATURES) == 77
    assert not set(_build.ABI_EXTENSIONS) & (set(_build.HEADERS) | set(_build.ABI_PARTS))
    text = open(_build.ABI_EXTENSIONS["aux_targets"]).read()
    assert '#include "sam_hip.h"' in text and "sam_hip_aux_targets.h" not in open(_build.HEADER).read()
    lib = _capi.lib()
    assert lib.sam_abi_version() == 9 and lib.sam_build_digest().decode() == _build._digest()
    assert lib.sam_aux_targets.argtypes == _capi.EXTENSION_SIGNATURES["aux_targets"]["sam_aux_targets"] and lib.sam_aux_targets.restype is i
    assert os.path.join(_build.CSRC, "aux_targets.hip") in _build.sources()
    with pytest.raises(_capi.SamHipError, match="sam_no_such") as e:
        _capi.call("sam_no_such")
    names = ["include/" + os.path.basename(p) for p in list(_build.HEADERS.values()) + list(_build.ABI_PARTS.values()) + list(_build.ABI_EXTENSIONS.values())]
    at = [str(e.value).index(n) for n in names]
    assert at == sorted(at) and names[-1] == "include/sam_hip_aux_targets.h"            # every header, the new one last


def test_digest_covers_the_extension_header(tmp_path, monkeypatch):
    import sam_textvqa_amd._build as b
    was = b._digest()
    other = tmp_path / "sam_hip_aux_targets.h"
    other.write_text(open(b.ABI_EXTENSIONS["aux_targets"]).read() + "\n/* changed */\n")
    monkeypatch.setitem(b.ABI_EXTENSIONS, "aux_targets", str(other))
    assert b._digest() != was and b._headers_digest().hexdigest() != was


def test_a_name_another_table_holds_is_refused(tmp_path):
    from sam_textvqa_amd import _capi
    bad = tmp_path / "sam_hip_bad.h"
    bad.write_text('#ifndef SAM_HIP_BAD_H\n#define SAM_HIP_BAD_H\n#include "sam_hip.h"\nint sam_aux_pair_loss_fwd(int B);\n#endif\n')
    taken = set(_capi.SIGNATURES) | {n for t in list(_capi.HEADER_SIGNATURES.values()) + list(_capi.PART_SIGNATURES.values()) for n in t}
    with pytest.raises(_capi.SamHipError, match="sam_hip_bad.h"):
        _capi.load_dataset_headers({"bad": str(bad)}, _capi.STRUCTS, taken)


# ---------------------------------------------------------------------------------------------- C ABI
def test_entry_point_rejects_bad_arguments_without_a_gpu():
    from sam_textvqa_amd import _capi, ops
    fake = 1 << 20            # never dereferenced: the checks reject the call before any launch

    def call(rel=fake, obj=fake, ld_obj=5, n_obj=5, ocr=fake, ld_ocr=4, n_ocr=4, elem=8, b=2, n=9, codes=fake, valid=fake):
        return _capi.call("sam_aux_targets", rel, obj, ld_obj, n_obj, ocr, ld_ocr, n_ocr, elem, b, n, codes, valid, None)

    for kw in (dict(valid=None), dict(codes=None), dict(obj=None), dict(ocr=None)):
        with pytest.raises(_capi.SamHipError, match="null pointer"):
            call(**kw)
    for elem in (2, 0, 3, 16, -1):
        with pytest.raises(_capi.SamHipError, match="mask elements of %d bytes" % elem):
            call(elem=elem)
    for kw in (dict(n=10), dict(n_obj=4), dict(n_ocr=0)):
        with pytest.raises(_capi.SamHipError, match="is not n"):
            call(**kw)
    for kw in (dict(b=-1), dict(n=-9), dict(n_obj=-5, n=-1), dict(n_ocr=-4, n=1)):
        with pytest.raises(_capi.SamHipError, match="negative size"):
            call(**kw)
    with pytest.raises(_capi.SamHipError, match="aligned"):
        call(obj=fake + 4)
    with pytest.raises(_capi.SamHipError, match="row strides"):
        call(ld_obj=4)
    # an empty batch or no rows: success, nothing launched (no device is touched: this runs without a GPU)
    assert call(b=0) == 0 and call(n=0, n_obj=0, n_ocr=0, ld_obj=0, ld_ocr=0) == 0
    # the Python wrappers: CPU tensors and float masks are refused, no fallback
    m = torch.ones(2, 5, dtype=torch.int64)
    with pytest.raises(_capi.SamHipError):
        ops.aux_targets(None, m, m)
    assert not ops.aux_targets_fusable(None, m, m) and not ops.aux_targets_fusable(None, m.float(), m.float())


def test_torch_op_is_registered_without_a_gpu():
    from sam_textvqa_amd import torchops
    assert hasattr(torchops.ns(), "aux_targets")
    schema = str(torch.ops.sam_hip.aux_targets.default._schema)
    assert "Tensor? rel" in schema and "Tensor obj_mask" in schema and "-> (Tensor, Tensor)" in schema


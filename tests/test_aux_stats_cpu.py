"""CPU: the spatial aux heads' confusion counts without a GPU -- the torch twin on hand-written logits, metrics.aux_report on a
hand-made table, the open table of the header registry, and the entry points' argument checks."""
import ctypes
import os

import pytest
import torch

NAN = float("nan")


def _hand_case(dtype=torch.float32):
    """B = 1, n = 3, row 2 not valid and filled with NaN.  The four valid pairs:
      (0,0) code 3   scores: channel 2 = 1.5, channel 7 = 1.5 (a tie: the first wins), rest -1          -> c 3, p 3, fired {2, 7}
      (0,1) code 0   scores: all exact 0                                                                 -> c 0, p 0, fired {}
      (1,0) code 13  scores: channel 0 = NaN, channel 4 = 0.25, channel 11 = -0.0, rest -2               -> c 0, p 5, fired {4}
      (1,1) code 12  scores: channel 11 = 2, channel 5 = 3, channel 0 = 0.5                              -> c 12, p 6, fired {0, 5, 11}"""
    s = torch.full((1, 3, 3, 12), NAN)
    s[0, 0, 0] = -1.0
    s[0, 0, 0, 2] = 1.5
    s[0, 0, 0, 7] = 1.5
    s[0, 0, 1] = 0.0
    s[0, 1, 0] = -2.0
    s[0, 1, 0, 0] = NAN
    s[0, 1, 0, 4] = 0.25
    s[0, 1, 0, 11] = -0.0
    s[0, 1, 1] = -1.0
    s[0, 1, 1, 11] = 2.0
    s[0, 1, 1, 5] = 3.0
    s[0, 1, 1, 0] = 0.5
    codes = torch.tensor([[[3, 0, 7], [13, 12, 200], [1, 2, 3]]], dtype=torch.uint8)
    valid = torch.tensor([[1, 1, 0]], dtype=torch.uint8)
    conf = torch.zeros(13, 13, dtype=torch.int64)
    conf[3, 3] = 1
    conf[0, 0] = 1
    conf[0, 5] = 1
    conf[12, 6] = 1
    fired = torch.zeros(13, 12, dtype=torch.int64)
    fired[3, 2] = fired[3, 7] = 1
    fired[0, 4] = 1
    fired[12, 0] = fired[12, 5] = fired[12, 11] = 1
    return s.to(dtype), codes, valid, conf, fired


# ---------------------------------------------------------------------------------------------- the torch twin
@pytest.mark.parametrize("dtype", [torch.float32, torch.float64, torch.bfloat16])
def test_twin_on_hand_written_logits(dtype):
    from sam_textvqa_amd import ops
    s, codes, valid, conf, fired = _hand_case(dtype)
    got_c, got_f = ops.aux_stats_from_logits(s, codes, valid)
    assert got_c.dtype == got_f.dtype == torch.int64 and tuple(got_c.shape) == (13, 13) and tuple(got_f.shape) == (13, 12)
    assert torch.equal(got_c, conf) and torch.equal(got_f, fired)
    # the valid flags may be bool or any integer dtype, as the batch's masks are
    for v in (valid.bool(), valid.long() * 7):
        assert all(torch.equal(a, b) for a, b in zip(ops.aux_stats_from_logits(s, codes, v), (conf, fired)))


def test_twin_without_a_valid_pair_gives_zeros_and_bad_shapes_raise():
    from sam_textvqa_amd import ops
    s, codes, valid, _, _ = _hand_case()
    c, f = ops.aux_stats_from_logits(s, codes, torch.zeros_like(valid))
    assert int(c.sum()) == 0 and int(f.sum()) == 0 and tuple(c.shape) == (13, 13) and tuple(f.shape) == (13, 12)
    with pytest.raises(ValueError):
        ops.aux_stats_from_logits(s[..., :11], codes, valid)
    with pytest.raises(ValueError):
        ops.aux_stats_from_logits(s, codes[:, :2], valid)
    with pytest.raises(ValueError):
        ops.aux_stats_from_logits(s.long(), codes, valid)


def test_host_counts_from_float64_scores():
    """aux_stats_host = the twin on the scores aux_loss_host forms.  O rows one-hot, D ones (mul) / zeros (add): S[i, j, r] = W[r, k_i] + bias[r]."""
    from sam_textvqa_amd import ops
    o = torch.zeros(1, 3, 32)
    o[0, 0, 4] = o[0, 1, 9] = 1.0
    o[0, 2] = NAN                                             # not valid: never used
    w = torch.zeros(12, 32)
    w[2, 4], w[5, 4], w[5, 9], w[6, 9] = 3.0, 1.0, 2.0, 2.0   # row 0: channels 2 (3) and 5 (1); row 1: channels 5 and 6 tie at 2
    bias = torch.zeros(12)
    bias[11] = -1.0
    codes = torch.tensor([[[3, 6, 0], [0, 14, 0], [0, 0, 0]]], dtype=torch.uint8)
    valid = torch.tensor([[1, 1, 0]], dtype=torch.uint8)
    conf = torch.zeros(13, 13, dtype=torch.int64)
    conf[3, 3] = conf[6, 3] = 1                              # row 0 predicts class 3 for both of its pairs
    conf[0, 6] = 2                                           # row 1 predicts class 6 (first of the tie); codes 0 and 14 are class 0
    fired = torch.zeros(13, 12, dtype=torch.int64)
    fired[3, 2] = fired[3, 5] = fired[6, 2] = fired[6, 5] = 1
    fired[0, 5] = fired[0, 6] = 2
    for fusion, d in (("mul", torch.ones(1, 3, 32)), ("add", torch.zeros(1, 3, 32))):
        d = d.clone()
        d[0, 2] = NAN
        got = ops.aux_stats_host(o, d, w, bias, codes, valid, fusion)
        assert torch.equal(got[0], conf) and torch.equal(got[1], fired), fusion
    with pytest.raises(ValueError):
        ops.aux_stats_host(o, d, w, bias, codes, valid, "sub")


# ---------------------------------------------------------------------------------------------- the report
def test_report_on_a_hand_made_table():
    from sam_textvqa_amd import metrics
    conf = torch.zeros(13, 13, dtype=torch.int64)
    conf[0, 0], conf[0, 1] = 5, 1
    conf[1, 1], conf[1, 2], conf[1, 0] = 3, 1, 2             # relation 0: support 6, predicted 4 times, 3 right
    conf[2, 2] = 4                                           # relation 1: support 4, predicted 5 times, 4 right
    conf[3, 0] = 2                                           # relation 2: support 2, never predicted: 0 / 0 precision
    fired = torch.zeros(13, 12, dtype=torch.int64)
    fired[1, 0], fired[0, 0], fired[2, 0] = 4, 1, 2          # channel 0: tp 4, fp 3, fn 2
    fired[2, 1] = 4                                          # channel 1: tp 4, fp 0, fn 0
    rep = metrics.aux_report(conf, fired)
    assert rep["pairs"] == 18.0 and rep["accuracy"] == pytest.approx(12 / 18)
    assert rep["support"][:4] == [6.0, 4.0, 2.0, 0.0] and len(rep["support"]) == 12
    assert rep["precision"][:4] == [0.75, 0.8, 0.0, 0.0] and rep["recall"][:4] == [0.5, 1.0, 0.0, 0.0]
    f0, f1 = 2 * 0.75 * 0.5 / 1.25, 2 * 0.8 / 1.8
    assert rep["f1"][0] == pytest.approx(f0) and rep["f1"][1] == pytest.approx(f1) and rep["f1"][2:] == [0.0] * 10
    assert rep["macro_f1"] == pytest.approx((f0 + f1 + 0.0) / 3)          # over the three relations with support
    assert rep["tp"][:3] == [4.0, 4.0, 0.0] and rep["fp"][:3] == [3.0, 0.0, 0.0] and rep["fn"][:3] == [2.0, 0.0, 2.0]
    assert all(isinstance(rep[k], float) for k in ("pairs", "accuracy", "macro_f1"))
    zero = metrics.aux_report(torch.zeros(13, 13, dtype=torch.int64), torch.zeros(13, 12, dtype=torch.int64))
    assert zero["pairs"] == 0.0 and zero["accuracy"] == 0.0 and zero["macro_f1"] == 0.0 and zero["f1"] == [0.0] * 12
    with pytest.raises(ValueError):
        metrics.aux_report(conf[:12], fired)


# ---------------------------------------------------------------------------------------------- registry
def test_the_open_table_holds_the_new_header_and_its_two_names():
    from sam_textvqa_amd import _build, _capi
    vp, i, i64 = ctypes.c_void_p, ctypes.c_int, ctypes.c_int64
    assert "aux_stats" in _build.ABI_ADDITIONS and "aux_stats" in _capi.ADDITION_SIGNATURES and "aux_stats" in _capi.ADDITION_RESTYPES
    assert _capi.ADDITION_SIGNATURES["aux_stats"] == {"sam_aux_pair_stats_ws_bytes": [i, i, vp],
                                                       "sam_aux_pair_stats": [vp, vp, vp, vp, vp, vp, i, i, i, vp, vp, i, vp, i64, vp]}
    assert _capi.ADDITION_RESTYPES["aux_stats"] == {"sam_aux_pair_stats_ws_bytes": i, "sam_aux_pair_stats": i}
    other = list(_capi.HEADER_SIGNATURES.values()) + list(_capi.PART_SIGNATURES.values()) + list(_capi.EXTENSION_SIGNATURES.values())
    for name in _capi.ADDITION_SIGNATURES["aux_stats"]:
        assert name not in _capi.SIGNATURES and name not in _capi.NO_STATUS and name not in _capi.PART_VALUES and all(name not in t for t in other)
    assert not set(_build.ABI_ADDITIONS) & (set(_build.HEADERS) | set(_build.ABI_PARTS) | set(_build.ABI_EXTENSIONS))
    text = open(_build.ABI_ADDITIONS["aux_stats"]).read()
    assert '#include "sam_hip.h"' in text and "sam_hip_aux_stats.h" not in open(_build.HEADER).read()
    assert _build.ABI_ADDITIONS["aux_stats"] in _build.public_headers()
    assert _build.public_headers().index(_build.ABI_ADDITIONS["aux_stats"]) > _build.public_headers().index(_build.ABI_EXTENSIONS["aux_targets"])
    lib = _capi.lib()
    assert lib.sam_abi_version() == 9 and lib.sam_build_digest().decode() == _build._digest()
    for name, sig in _capi.ADDITION_SIGNATURES["aux_stats"].items():
        assert getattr(lib, name).argtypes == sig and getattr(lib, name).restype is i
    assert os.path.join(_build.CSRC, "aux_stats.hip") in _build.sources()
    with pytest.raises(_capi.SamHipError, match="sam_no_such") as e:
        _capi.call("sam_no_such")
    assert "include/sam_hip_aux_stats.h" in str(e.value)
    assert str(e.value).index("include/sam_hip_aux_stats.h") > str(e.value).index("include/sam_hip_aux_targets.h")


def test_digest_covers_the_new_header(tmp_path, monkeypatch):
    import sam_textvqa_amd._build as b
    was, was_h = b._digest(), b._headers_digest().hexdigest()
    other = tmp_path / "sam_hip_aux_stats.h"
    other.write_text(open(b.ABI_ADDITIONS["aux_stats"]).read() + "\n/* changed */\n")
    monkeypatch.setitem(b.ABI_ADDITIONS, "aux_stats", str(other))
    assert b._digest() != was and b._headers_digest().hexdigest() != was_h


def test_a_taken_name_in_the_open_table_is_refused(tmp_path):
    from sam_textvqa_amd import _capi
    bad = tmp_path / "sam_hip_bad.h"
    bad.write_text('#ifndef SAM_HIP_BAD_H\n#define SAM_HIP_BAD_H\n#include "sam_hip.h"\nint sam_aux_targets(int B);\n#endif\n')
    taken = set(_capi.SIGNATURES) | {n for t in list(_capi.HEADER_SIGNATURES.values()) + list(_capi.PART_SIGNATURES.values()) +
                                     list(_capi.EXTENSION_SIGNATURES.values()) for n in t}
    with pytest.raises(_capi.SamHipError, match="sam_hip_bad.h"):
        _capi.load_dataset_headers({"bad": str(bad)}, _capi.STRUCTS, taken)


# ---------------------------------------------------------------------------------------------- C ABI
def test_entry_points_reject_bad_arguments_without_a_gpu():
    from sam_textvqa_amd import _capi, ops
    fake = 1 << 20            # never dereferenced: the checks reject the call before any launch
    big = 1 << 40

    def call(o=fake, d=fake, w=fake, bias=fake, codes=fake, valid=fake, b=2, n=9, fusion=_capi.AUX_MUL, conf=fake, fired=fake, acc=0, ws=fake, ws_bytes=big):
        return _capi.call("sam_aux_pair_stats", o, d, w, bias, codes, valid, b, n, fusion, conf, fired, acc, ws, ws_bytes, None)

    for name in ("o", "d", "w", "bias", "codes", "valid", "conf", "fired", "ws"):
        with pytest.raises(_capi.SamHipError, match="null pointer"):
            call(**{name: None})
    for kw in (dict(b=0), dict(n=0), dict(b=-1), dict(n=-3)):
        with pytest.raises(_capi.SamHipError, match="empty shape"):
            call(**kw)
    with pytest.raises(_capi.SamHipError, match="unknown fusion 7"):
        call(fusion=7)
    for kw in (dict(o=fake + 4), dict(d=fake + 8), dict(ws=fake + 4)):
        with pytest.raises(_capi.SamHipError, match="16-byte aligned"):
            call(**kw)
    for kw in (dict(conf=fake + 4), dict(fired=fake + 4)):
        with pytest.raises(_capi.SamHipError, match="8-byte aligned"):
            call(**kw)
    with pytest.raises(_capi.SamHipError, match="exceeds the grid"):
        call(b=65536)
    # the workspace: 325 u32 per block of 64 j x 16 i
    nbytes = ctypes.c_int64(-1)
    assert _capi.call("sam_aux_pair_stats_ws_bytes", 2, 9, ctypes.byref(nbytes)) == 0 and nbytes.value == 2 * 1 * 1 * 325 * 4
    assert _capi.call("sam_aux_pair_stats_ws_bytes", 64, 150, ctypes.byref(nbytes)) == 0 and nbytes.value == 64 * 3 * 10 * 325 * 4
    with pytest.raises(_capi.SamHipError, match="workspace of 2599 bytes, need 2600"):
        call(ws_bytes=2599)
    with pytest.raises(_capi.SamHipError, match="null pointer"):
        _capi.call("sam_aux_pair_stats_ws_bytes", 2, 9, None)
    for b, n, what in ((0, 9, "empty shape"), (2, 0, "empty shape"), (65536, 9, "exceeds the grid")):
        with pytest.raises(_capi.SamHipError, match=what):
            _capi.call("sam_aux_pair_stats_ws_bytes", b, n, ctypes.byref(nbytes))
    # the Python wrapper: CPU tensors are refused, no fallback
    o = torch.zeros(1, 3, 32)
    with pytest.raises(_capi.SamHipError):
        ops.aux_pair_stats(o, o, torch.zeros(12, 32), torch.zeros(12), torch.zeros(1, 3, 3, dtype=torch.uint8), torch.ones(1, 3, dtype=torch.uint8))
    with pytest.raises(ValueError, match="'mul' or 'add'"):
        ops.aux_pair_stats(o, o, torch.zeros(12, 32), torch.zeros(12), torch.zeros(1, 3, 3, dtype=torch.uint8), torch.ones(1, 3, dtype=torch.uint8), fusion="sub")


def test_torch_op_is_registered_without_a_gpu():
    from sam_textvqa_amd import torchops
    assert hasattr(torchops.ns(), "aux_pair_stats")
    schema = str(torch.ops.sam_hip.aux_pair_stats.default._schema)
    assert "Tensor(a!) confusion" in schema and "Tensor(b!) fired" in schema and "bool accumulate" in schema and "-> ()" in schema

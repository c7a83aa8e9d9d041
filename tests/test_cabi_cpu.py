"""CPU (no GPU needed): the C-ABI library builds, loads, and exports every symbol include/sam_hip.h declares; the
ctypes signatures cover the header; and the product path refuses to run without a GPU instead of falling back."""
import ctypes
import os
import re
import subprocess

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def header_functions():
    src = open(os.path.join(ROOT, "include", "sam_hip.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return sorted(set(re.findall(r"\b(sam_[a-z0-9_]+)\s*\(", src)))


def test_library_builds_and_exports_every_declared_symbol():
    import sam_textvqa_amd._build as b
    lib_path = b.build()
    assert os.path.exists(lib_path)
    lib = ctypes.CDLL(lib_path)
    names = header_functions()
    assert len(names) >= 20
    for n in names:
        assert hasattr(lib, n), "libsam_hip.so does not export %s declared in include/sam_hip.h" % n


def header_text():
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "sam_hip.h")).read(), flags=re.S)


def test_ctypes_binding_covers_the_header():
    from sam_textvqa_amd import _capi
    declared = set(header_functions())                                       # no exclusions: every declared function is bound from its declaration
    assert set(_capi.STRUCTS) == set(STRUCT_FIELDS)
    bound = set(_capi.SIGNATURES)
    assert declared <= bound, "unbound entry points: %s" % sorted(declared - bound)
    assert bound <= declared, "bound but undeclared: %s" % sorted(bound - declared)
    assert len(bound) == 77 and set(_capi.RESTYPES) == bound
    src = header_text()
    for name, args in _capi.SIGNATURES.items():                             # every argument of every declaration is bound: comma count + 1, (void) -> 0
        params = re.search(r"\b%s\s*\(([^)]*)\)" % name, src).group(1)
        assert len(args) == (0 if params.strip() == "void" else params.count(",") + 1), name
    l = _capi.lib()
    assert l.sam_abi_version() == 9
    import sam_textvqa_amd._build as b
    assert l.sam_build_digest().decode() == b._digest()          # the binary that is loaded is the one built from the sources in the tree
    assert _capi.call("sam_attn_words_per_row", 182) == 6 and _capi.call("sam_attn_words_per_row", 20) == 1
    assert _capi.call("sam_attn_words_per_row", 350) == 12 and _capi.call("sam_attn_words_per_row", 385) == -1
    # CUs withheld from persistent grids: a multiple of 8, bounded, host-side state only (no GPU needed)
    was = _capi.call("sam_get_cu_reserve")
    _capi.call("sam_set_cu_reserve", 37)
    assert _capi.call("sam_get_cu_reserve") == 32
    with pytest.raises(_capi.SamHipError):
        _capi.call("sam_set_cu_reserve", 200)
    _capi.call("sam_set_cu_reserve", was)


# every struct of the header with its fields in declaration order, written out by hand: the layout test below must not depend on the parser it checks
STRUCT_FIELDS = {
    "sam_ln_fuse": "gamma beta eps y ldy mean rstd done xws xws_bytes",
    "sam_gemm_desc": "M N K a_kcontig b_kcontig c_is_f32 accumulate epilogue A lda B ldb C ldc bias residual ldr aux_out aux_in ld_aux p_drop seed offset split_k "
                     "bias_grad ws ws_bytes force_tile defer_reduce split_k_used ln",
    "sam_ln_finalize_item": "ws rows accumulate dgamma dbeta dbias",
    "sam_sparse_rows": "lo hi row_len touched",
    "sam_lr_schedule": "base_lr nseg warmup_iters warmup_factor n_decay decay_iters lr_decay beta1 beta2",
    "sam_decode_layer": "wqkv wo w1 w2 bqkv bo b1 b2 ln1_g ln1_b ln2_g ln2_b qkv allow allow_stride_b allow_stride_h",
    "sam_decode_desc": "n_layers B N n_enc S H D F V No t_begin t_end scale ln_eps emb_ln_eps ptr_scale layers pos_emb type_emb emb_ln_g emb_ln_b ld_pos ld_type "
                       "ans_ln ocr_ln wc bc wq bq ptr_k ocr_mask prev_inds fixed_scores ld_fixed ocr_scores seq_out",
    "sam_copy_desc": "src dst batches rows cols src_batch_stride src_row_stride dst_batch_stride dst_row_stride src_f32 dst_f32 accumulate",
    "sam_ragged_part": "src ld_src src_f16 width dst ld_dst dst_f32 col0 normalize zero_upto",
}


def test_struct_layouts_match_the_host_compiler(tmp_path):
    """sizeof / offsetof of every struct and field as the host C++ compiler lays out include/sam_hip.h == the ctypes classes derived from it"""
    from sam_textvqa_amd import _capi
    lines = ['#include <cstddef>', '#include <cstdio>', '#include "sam_hip.h"', 'int main() {']
    for s_, fields in STRUCT_FIELDS.items():
        lines.append('  std::printf("%s - %%zu 0\\n", sizeof(%s));' % (s_, s_))
        lines += ['  std::printf("%s %s %%zu %%zu\\n", offsetof(%s, %s), sizeof(((%s*)0)->%s));' % (s_, f, s_, f, s_, f) for f in fields.split()]
    src, exe = str(tmp_path / "layout.cpp"), str(tmp_path / "layout")
    open(src, "w").write("\n".join(lines + ["  return 0;", "}", ""]))
    r = subprocess.run([os.environ.get("CXX", "g++"), "-std=c++17", "-I", os.path.join(ROOT, "include"), src, "-o", exe], stdout=subprocess.PIPE,
                       stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout[-3000:]
    seen = {}
    for s_, f, a, b in (l.split() for l in subprocess.run([exe], stdout=subprocess.PIPE, text=True, check=True).stdout.splitlines()):
        cls = _capi.STRUCTS[s_]
        if f == "-":
            assert ctypes.sizeof(cls) == int(a), s_
        else:
            assert (getattr(cls, f).offset, getattr(cls, f).size) == (int(a), int(b)), (s_, f)
            seen.setdefault(s_, []).append(f)
    assert seen == {s_: [n for n, _ in _capi.STRUCTS[s_]._fields_] for s_ in _capi.STRUCTS}          # every struct the parser found, every field, in order
    assert seen == {s_: f.split() for s_, f in STRUCT_FIELDS.items()}
    for py, c in (("GemmDesc", "sam_gemm_desc"), ("LnFuse", "sam_ln_fuse"), ("SparseRows", "sam_sparse_rows"), ("LrSchedule", "sam_lr_schedule"),
                  ("CopyDesc", "sam_copy_desc"), ("DecodeLayer", "sam_decode_layer"), ("DecodeDesc", "sam_decode_desc"), ("RaggedPart", "sam_ragged_part"),
                  ("LnFinalizeItem", "sam_ln_finalize_item")):
        assert getattr(_capi, py) is _capi.STRUCTS[c]
    assert _capi.GemmDesc.ln.size == 8 and _capi.GemmDesc._fields_[-1][1] is ctypes.POINTER(_capi.LnFuse)
    assert _capi.DecodeDesc._fields_[16] == ("layers", ctypes.POINTER(_capi.DecodeLayer))
    assert _capi.LrSchedule._fields_[0] == ("base_lr", ctypes.c_double * 8) and _capi.LrSchedule._fields_[5] == ("decay_iters", ctypes.c_int64 * 4)


def test_derived_signatures_of_tricky_declarations():
    from ctypes import POINTER, c_char_p, c_double, c_float, c_int, c_int64, c_uint, c_void_p as vp
    from sam_textvqa_amd import _capi
    S, i, i64 = _capi.SIGNATURES, c_int, c_int64
    assert S["sam_rowvec_bf16"] == [i, vp, i64, vp, i64, vp, vp, i64, i64, i, vp]                       # `int64_t rows, int cols` side by side
    assert S["sam_spatial_relation_tensor"] == [vp, i, i, i, c_double, vp, vp]
    assert S["sam_mask_bits_spatial"] == [vp, vp, i, i, i, i, i, i, i, c_uint, vp, vp]                  # the `unsigned` quadrant bits
    assert S["sam_gemm_bf16_grouped"] == [POINTER(_capi.GemmDesc), i, vp]
    assert S["sam_adam_step"][6:9] == [vp, vp, i] and S["sam_adam_step"][9:12] == [c_float] * 3 and S["sam_adam_step"][15] is POINTER(_capi.SparseRows)
    assert S["sam_abi_version"] == [] and S["sam_device_info"] == [vp, vp, vp, i]
    assert _capi.RESTYPES["sam_gemm_ln_ws_bytes"] is c_int64 and _capi.RESTYPES["sam_last_error"] is c_char_p
    assert _capi.RESTYPES["sam_set_rng_state"] is None and _capi.RESTYPES["sam_gemm_bf16"] is c_int
    l = _capi.lib()
    assert l.sam_gemm_ln_ws_bytes.restype is c_int64 and l.sam_last_error.restype is c_char_p
    assert l.sam_rowvec_bf16.argtypes == S["sam_rowvec_bf16"]
    # the name sets: int64_t and void returns are found in the header; the five int-valued queries are the one hand-kept list
    assert _capi.RET_I64 == {n for n in S if re.search(r"\bint64_t\s+%s\s*\(" % n, header_text())} and len(_capi.RET_I64) == 10
    assert _capi.NO_STATUS == _capi.RET_I64 | {"sam_set_rng_state"} | {"sam_abi_version", "sam_attn_words_per_row", "sam_attn_bwd_fused_max_n", "sam_get_cu_reserve",
                                                                      "sam_layernorm_bwd_partial_rows"}
    assert [_capi.EPI_NONE, _capi.EPI_BIAS, _capi.EPI_BIAS_GELU, _capi.EPI_BIAS_DROPOUT_RES, _capi.EPI_DGELU, _capi.EPI_BIAS_GELU_GRAD, _capi.EPI_MUL_AUX,
            _capi.EPI_BIAS_RELU] == list(range(8))
    assert (_capi.AUX_MUL, _capi.AUX_ADD, _capi.RAGGED_MAX_PARTS) == (0, 1, 6)


@pytest.mark.parametrize("decl, named", [
    ("typedef struct sam_x { int32_t n; size_t bytes; } sam_x;", "size_t bytes"),                     # a field of an unknown type
    ("int sam_f(const float* x, long n, void* stream);", "long n"),                                   # a parameter of an unknown type
    ("int sam_f(sam_y* y);", "sam_y* y"),                                                             # a pointer to a struct the header never declared
    ("typedef struct sam_x { char tag; } sam_x;", "char tag"),                                        # char: only behind a pointer
    ("int sam_f(int64_t** rows);", "int64_t** rows"),
    ("int sam_f(int n[4]);", "int n[4]"),
    ("long sam_f(void);", "long sam_f(void)"),                                                        # an unknown return type
    ("int sam_f(int);", "sam_f"),                                                                     # a parameter without a name
    ("#define SAM_X (1 << 3)", "SAM_X"),
    ("enum { SAM_A = 0, SAM_B };", "SAM_B"),
    ("typedef struct sam_x { int32_t n; } sam_x_t;", "sam_x_t"),
])
def test_unknown_spellings_in_the_header_are_errors(decl, named):
    """the parser raises on what it does not know, naming the declaration: nothing is skipped or defaulted"""
    from sam_textvqa_amd import _capi
    ok = "#define SAM_K 3\ntypedef struct sam_p { int64_t lo, hi; const float *a, *b; double w[2]; } sam_p;\nint sam_g(const sam_p* p, unsigned flags);\n"
    structs, sigs, rets, consts = _capi.parse_header(ok)
    assert [n for n, _ in structs["sam_p"]._fields_] == ["lo", "hi", "a", "b", "w"] and sigs == {"sam_g": [ctypes.POINTER(structs["sam_p"]), ctypes.c_uint]}
    assert rets == {"sam_g": ctypes.c_int} and consts == {"SAM_K": 3}
    with pytest.raises(_capi.SamHipError) as e:
        _capi.parse_header(ok + decl + "\n")
    assert named in str(e.value), str(e.value)


ABI_TEXT = "#define SAM_K 3\ntypedef struct sam_p { int64_t lo, hi; } sam_p;\nint sam_g(const sam_p* p);\n"
FIRST_TEXT = "#ifndef SAM_HIP_FIRST_H\n#define SAM_HIP_FIRST_H\n#include \"sam_hip.h\"\nint sam_first(const sam_p* p, int n);\n#endif\n"


def dataset_headers(tmp_path, second):
    """load_dataset_headers on an ABI header, a good first dataset header and `second`, all under tmp_path"""
    from sam_textvqa_amd import _capi
    paths = {}
    for name, text in (("abi", ABI_TEXT), ("first", FIRST_TEXT), ("second", second)):
        paths[name] = str(tmp_path / ("sam_hip.h" if name == "abi" else "sam_hip_%s.h" % name))
        with open(paths[name], "w") as f:
            f.write(text)
    structs, sigs, _, _ = _capi.parse_header(ABI_TEXT)
    return _capi.load_dataset_headers(paths, structs, sigs)


def test_dataset_headers_load_into_one_table_each(tmp_path):
    tables = dataset_headers(tmp_path, "#ifndef SAM_HIP_SECOND_H\n#define SAM_HIP_SECOND_H\nint sam_second(void* stream);\n#endif\n")
    assert list(tables) == ["first", "second"]                          # registry order, without the ABI's own header
    assert list(tables["first"][0]) == ["sam_first"] and tables["first"][1] == {"sam_first": ctypes.c_int}
    assert tables["second"] == ({"sam_second": [ctypes.c_void_p]}, {"sam_second": ctypes.c_int})


@pytest.mark.parametrize("second", [
    "typedef struct sam_q { int32_t n; } sam_q;\nint sam_second(const sam_q* q);\n",                  # a struct
    "#define SAM_HIP_SECOND_H\n#define SAM_SECOND_MAX 4\nint sam_second(void* stream);\n",            # a constant beside the include guard
    "int64_t sam_second(int n);\n",                                                                   # a value, not a status
    "void sam_second(int n);\n",
    "int sam_g(void* stream);\n",                                                                     # a name of sam_hip.h
    "int sam_first(void* stream);\n",                                                                 # a name of an earlier dataset header
])
def test_a_dataset_header_may_only_add_status_returning_functions(tmp_path, second):
    from sam_textvqa_amd import _capi
    with pytest.raises(_capi.SamHipError, match=r"^sam_hip_second\.h may only add status-returning functions"):
        dataset_headers(tmp_path, second)


def test_an_unknown_name_is_refused_naming_every_header_of_the_registry():
    import sam_textvqa_amd._build as b
    from sam_textvqa_amd import _capi
    assert list(b.HEADERS) == ["abi", "pipeline", "text", "answers", "step", "question", "fasttext", "metrics", "eval", "textprep", "unicode"]
    assert b.HEADER == b.HEADERS["abi"] and list(_capi.HEADER_SIGNATURES) == list(_capi.HEADER_RESTYPES) == list(b.HEADERS)[1:]
    with pytest.raises(_capi.SamHipError, match="sam_no_such") as e:
        _capi.call("sam_no_such")
    for path in b.HEADERS.values():
        assert os.path.exists(path) and "include/" + os.path.basename(path) in str(e.value)


def test_argument_errors_are_reported_without_a_gpu():
    """argument validation happens before any launch, so it can be exercised on a CPU-only box"""
    from sam_textvqa_amd import _capi
    with pytest.raises(_capi.SamHipError) as e:
        _capi.call("sam_attn_fwd", None, None, 0, 0, 1, 8, 12, 32, 0.1, 0.0, 0, 0, None, None, None, None)
    assert "head_dim" in str(e.value)
    d = _capi.GemmDesc()
    with pytest.raises(_capi.SamHipError):
        _capi.call("sam_gemm_bf16", d, None)          # empty problem


@pytest.mark.skipif(torch.cuda.is_available(), reason="CPU-only check")
def test_product_path_fails_loudly_without_gpu():
    import sam_textvqa_amd.modules as M
    from sam_textvqa_amd import ops
    from sam_textvqa_amd._capi import SamHipError
    with pytest.raises(SamHipError):
        ops.mask_bits_prefix_lm(torch.ones(2, 8, dtype=torch.uint8), 2)       # CPU tensor: rejected, no fallback
    cfg = M.BertConfig.from_dict(dict(hidden_size=768, num_spatial_relations=12, max_seq_length=4, num_decoding_steps=2,
                                      attention_mask_quadrants=[1, 2], intermediate_size=64))
    layer = M.SpatialBertLayer(cfg)
    with pytest.raises(Exception):
        layer(torch.zeros(1, 10, 768), torch.zeros(1, 1, 10, 10), torch.zeros(1, 4, 4, 12, dtype=torch.int8))


def test_no_oracle_import_in_product_package():
    pkg = os.path.join(ROOT, "sam-textvqa_amd")
    for dp, _, fs in os.walk(pkg):
        for f in fs:
            if f.endswith((".py", ".hip", ".h", ".cpp")):
                txt = open(os.path.join(dp, f)).read()
                assert "import oracle" not in txt and "from oracle" not in txt, "%s imports the oracle" % f


def test_plain_cxx_host_program_links_against_the_c_abi(tmp_path):
    """tests/cabi/host_smoke.cpp includes only sam_hip.h and the HIP runtime: it must compile and link (it runs in the gpu suite)"""
    from tests.cabi_host import build_host_smoke
    exe = build_host_smoke(tmp_path)
    assert os.path.exists(exe)


def test_a_library_built_from_other_sources_is_refused(tmp_path, monkeypatch):
    """_capi.lib() compares the digest compiled into the binary with the tree's: a stale libsam_hip.so never runs against changed signatures"""
    import sam_textvqa_amd._build as b
    from sam_textvqa_amd import _capi
    _capi.lib()
    monkeypatch.setattr(_capi, "_lib", None)
    monkeypatch.setattr(b, "build", lambda *a, **k: b.LIB)                # pretend the rebuild was skipped ...
    monkeypatch.setattr(b, "_digest", lambda: "0" * 64)                  # ... although the sources changed
    with pytest.raises(_capi.SamHipError, match="other sources"):
        _capi.lib()
    monkeypatch.setattr(b, "build", lambda *a, **k: (_ for _ in ()).throw(RuntimeError("hipcc failed on gemm.hip")))
    with pytest.raises(_capi.SamHipError, match="could not be"):
        _capi.lib()                                                        # a failed rebuild is an error even though an older .so exists


def test_torch_custom_ops_build_and_register_without_a_gpu():
    """csrc_torch/sam_torch_ops.cpp: TORCH_LIBRARY(sam_hip) schemas are visible to the dispatcher after load; running them needs the GPU"""
    from sam_textvqa_amd import torchops
    ns = torchops.ns()
    for op in ("linear", "spatial_attn_fwd", "spatial_attn_bwd", "spatial_attn_fwd_train", "spatial_attn_bwd_fused", "layernorm_fwd", "layernorm_bwd", "encoder_layer_fwd",
               "encoder_layer_bwd"):
        assert hasattr(ns, op), op
    schema = str(torch.ops.sam_hip.encoder_layer_fwd.default._schema)
    assert "Tensor[] params" in schema and "int[] seeds" in schema
    if not torch.cuda.is_available():
        with pytest.raises((RuntimeError, NotImplementedError)):
            torch.ops.sam_hip.layernorm_fwd(torch.zeros(4, 8), torch.ones(8), torch.zeros(8), 1e-12)       # no CPU kernel is registered

"""ctypes binding of libsam_hip.so — the C-ABI declared in include/sam_hip.h, derived from that header at import: the header is the
only description of the ABI (prototypes, structs, constants); nothing here repeats it.

The library is the product: if it is missing or a call fails this module raises; nothing here
(or anywhere in the package) falls back to a CPU or eager-PyTorch implementation."""
import ctypes as C
import os
import re

from . import _build

_PKG = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_PKG, "lib", "libsam_hip.so")


class SamHipError(RuntimeError):
    pass


# The C spellings the header may use.  By value: these eight.  Behind a pointer: also void, char, the narrow integers and unsigned long long;
# a pointer to one of the header's own structs is typed, every other pointer is a plain address.
_VALUE = {"int": C.c_int, "int32_t": C.c_int32, "unsigned": C.c_uint, "uint32_t": C.c_uint32, "int64_t": C.c_int64, "uint64_t": C.c_uint64,
          "float": C.c_float, "double": C.c_double}
_POINTEE = set(_VALUE) | {"void", "char", "int8_t", "uint8_t", "int16_t", "uint16_t", "unsigned long long"}
_RETURN = {"int": C.c_int, "int64_t": C.c_int64, "void": None, "const char*": C.c_char_p}
_DECLARATOR = r"(\*?)\s*([A-Za-z_]\w*)(?:\[(\d+)\])?"
# int-returning entry points whose result is a VALUE, not a status: the declaration cannot tell the two apart, so these are the only names kept by hand
VALUE_QUERIES = {"sam_abi_version", "sam_attn_words_per_row", "sam_attn_bwd_fused_max_n", "sam_get_cu_reserve", "sam_layernorm_bwd_partial_rows"}


def _declaration(text, structs, where, header="sam_hip.h"):
    """`const float *a, *b` | `int64_t lo, hi` | `double base_lr[8]` | `const sam_gemm_desc* d` -> [(name, ctype), ...]"""
    first, *rest = [d.strip() for d in text.split(",")]
    m = re.fullmatch(r"(?:const\s+)?(\w+(?:\s+\w+)*?)\s*" + _DECLARATOR, first)
    more = [re.fullmatch(_DECLARATOR, d) for d in rest]
    base = " ".join(m.group(1).split()) if m else None
    if not all(more) or not (base in _POINTEE or base in structs):
        raise SamHipError(header + ": cannot parse `%s` in %s" % (text.strip(), where))
    out = []
    for star, name, dim in [m.groups()[1:]] + [d.groups() for d in more]:
        if star:
            t = C.POINTER(structs[base]) if base in structs else C.c_void_p
        elif base in _VALUE:
            t = _VALUE[base]
        else:
            raise SamHipError(header + ": `%s` in %s holds a %s by value" % (text.strip(), where, base))
        out.append((name, t * int(dim) if dim else t))
    return out


def parse_header(text, known_structs=None, header="sam_hip.h"):
    """the C ABI as ctypes: ({struct: Structure}, {function: argtypes}, {function: restype}, {SAM_* constant: int}).  Whatever is not a
    `#define NAME <int>`, the anonymous enum, a `typedef struct sam_x {...} sam_x;` or a prototype of the form matched below raises SamHipError
    naming the declaration: nothing is skipped or guessed (a wrong argtype is a shifted pointer on the GPU, not an exception).
    known_structs: structs of a header this one includes (its declarations may point to them; they are not returned again); header: the file's name,
    for the messages."""
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    constants = {}
    for line in re.findall(r"^[ \t]*#[ \t]*define[ \t]+(.*?)[ \t]*$", text, flags=re.M):
        m = re.fullmatch(r"(SAM_\w+)(?:\s+\(?(-?\d+)\)?)?", line)
        if not m:
            raise SamHipError(header + ": cannot parse `#define %s`" % line)
        if m.group(2) is not None:                  # (a name without a value: the include guard)
            constants[m.group(1)] = int(m.group(2))
    text = re.sub(r"^[ \t]*#.*$", "", text, flags=re.M)
    m = re.search(r'extern\s+"C"\s*\{(.*)\}', text, flags=re.S)
    text = m.group(1) if m else text

    def enum(m):
        for item in m.group(1).split(","):
            e = re.fullmatch(r"\s*(SAM_\w+)\s*=\s*(-?\d+)\s*", item)
            if not e:
                raise SamHipError(header + ": cannot parse the enumerator `%s`" % item.strip())
            constants[e.group(1)] = int(e.group(2))
        return ""
    text = re.sub(r"\benum\s*\{(.*?)\}\s*;", enum, text, flags=re.S)
    structs = dict(known_structs or {})

    def struct(m):          # (in header order: a struct may point to the ones declared before it)
        tag, body, alias = m.groups()
        if tag != alias or not tag.startswith("sam_"):
            raise SamHipError(header + ": struct %s is typedef'd as %s" % (tag, alias))
        fields = [f for d in body.split(";") if d.strip() for f in _declaration(d, structs, "struct " + tag, header)]
        structs[tag] = type("".join(w.capitalize() for w in tag.split("_")[1:]), (C.Structure,), {"_fields_": fields, "__doc__": "`%s` (include/%s)" % (tag, header)})
        return ""
    text = re.sub(r"\btypedef\s+struct\s+(\w+)\s*\{(.*?)\}\s*(\w+)\s*;", struct, text, flags=re.S)
    signatures, restypes = {}, {}
    for proto in filter(None, (" ".join(p.split()) for p in text.split(";"))):
        m = re.fullmatch(r"(int|int64_t|void|const char ?\*) ?(sam_\w+) ?\((.*)\)", proto)
        if not m:
            raise SamHipError(header + ": cannot parse `%s`" % proto)
        ret, name, params = m.groups()
        args = [] if params.strip() == "void" else [_declaration(p, structs, name, header) for p in params.split(",")]
        if any(issubclass(a[0][1], C.Array) for a in args):
            raise SamHipError(header + ": array parameter in `%s`" % proto)
        signatures[name], restypes[name] = [a[0][1] for a in args], _RETURN[ret.replace(" *", "*")]
    return {k: v for k, v in structs.items() if k not in (known_structs or {})}, signatures, restypes, constants


with open(_build.HEADER) as _f:
    STRUCTS, SIGNATURES, RESTYPES, CONSTANTS = parse_header(_f.read())
globals().update({s.__name__: s for s in STRUCTS.values()})             # sam_gemm_desc -> GemmDesc, sam_ln_fuse -> LnFuse, sam_copy_desc -> CopyDesc, ...
globals().update({k[4:]: v for k, v in CONSTANTS.items()})              # SAM_EPI_BIAS -> EPI_BIAS, SAM_AUX_MUL -> AUX_MUL, SAM_RAGGED_MAX_PARTS -> RAGGED_MAX_PARTS
RET_I64 = {n for n, r in RESTYPES.items() if r is C.c_int64}
if not VALUE_QUERIES <= {n for n, r in RESTYPES.items() if r is C.c_int}:
    raise SamHipError("_capi.VALUE_QUERIES names entry points the header does not declare as returning int")
NO_STATUS = RET_I64 | {n for n, r in RESTYPES.items() if r is None} | VALUE_QUERIES        # call() checks every other return value as a status


def load_dataset_headers(paths, abi_structs, abi_names):
    """{name: (signatures, restypes)} of the headers in `paths` ({name: file}, in order) that come after the ABI's: the entry points that replace the
    dataset's work, through the same parser but into one table per header (SIGNATURES and its kin describe sam_hip.h, the versioned model ABI, and
    nothing else).  Such a header may only add status-returning functions: no struct, no constant beside its include guard, no name that sam_hip.h or
    a header before it declares."""
    tables, taken = {}, set(abi_names)
    for name, path in paths.items():
        if name == "abi":
            continue
        fname = os.path.basename(path)
        with open(path) as f:
            structs, sigs, rets, consts = parse_header(f.read(), abi_structs, header=fname)
        guard = re.sub(r"\W", "_", fname).upper()
        if structs or set(consts) - {guard} or any(r is not C.c_int for r in rets.values()) or set(sigs) & taken:
            raise SamHipError("%s may only add status-returning functions (no struct, no constant, no name that sam_hip.h or an earlier header declares)" % fname)
        tables[name] = (sigs, rets)
        taken |= set(sigs)
    return tables


_tables = load_dataset_headers(_build.HEADERS, STRUCTS, SIGNATURES)
HEADER_SIGNATURES = {k: v[0] for k, v in _tables.items()}          # HEADER_SIGNATURES["metrics"] = {"sam_score_table_from_text": [...]}
HEADER_RESTYPES = {k: v[1] for k, v in _tables.items()}
_DATASET_SIGNATURES = {n: a for sigs in HEADER_SIGNATURES.values() for n, a in sigs.items()}
_DATASET_RESTYPES = {n: r for rets in HEADER_RESTYPES.values() for n, r in rets.items()}



def load_abi_parts(paths, abi_structs, taken):
    """{name: (signatures, restypes)} of the files sam_hip.h includes (_build.ABI_PARTS): prototypes only -- int status, or an int64_t value such as a
    workspace size -- under names nothing else declares"""
    tables, taken = {}, set(taken)
    for name, path in paths.items():
        fname = os.path.basename(path)
        with open(path) as f:
            structs, sigs, rets, consts = parse_header(f.read(), abi_structs, header=fname)
        guard = re.sub(r"\W", "_", fname).upper()
        if structs or set(consts) - {guard} or any(r not in (C.c_int, C.c_int64) for r in rets.values()) or set(sigs) & taken:
            raise SamHipError("%s may only add functions that return a status or an int64_t value (no struct, no constant, no name declared elsewhere)" % fname)
        tables[name] = (sigs, rets)
        taken |= set(sigs)
    return tables


_parts = load_abi_parts(_build.ABI_PARTS, STRUCTS, set(SIGNATURES) | set(_DATASET_SIGNATURES))
PART_SIGNATURES = {k: v[0] for k, v in _parts.items()}             # PART_SIGNATURES["aux_loss"] = {"sam_aux_pair_loss_fwd": [...], ...}
PART_RESTYPES = {k: v[1] for k, v in _parts.items()}
PART_VALUES = {n for _, _rets in _parts.values() for n, r in _rets.items() if r is C.c_int64}       # value queries: call() checks no status (as NO_STATUS for sam_hip.h)
for _sigs, _rets in _parts.values():
    _DATASET_SIGNATURES.update(_sigs)                               # bound and called like every other entry point
    _DATASET_RESTYPES.update(_rets)

# additive extensions of the ABI (_build.ABI_EXTENSIONS): headers of their own that include sam_hip.h; status-returning prototypes only, under names no
# other table holds (the dataset headers' rule: load_dataset_headers refuses a struct, a constant, another return type or a taken name)
_ext = load_dataset_headers(_build.ABI_EXTENSIONS, STRUCTS, set(SIGNATURES) | set(_DATASET_SIGNATURES))
EXTENSION_SIGNATURES = {k: v[0] for k, v in _ext.items()}          # EXTENSION_SIGNATURES["aux_targets"] = {"sam_aux_targets": [...]}
EXTENSION_RESTYPES = {k: v[1] for k, v in _ext.items()}
for _sigs, _rets in _ext.values():
    _DATASET_SIGNATURES.update(_sigs)
    _DATASET_RESTYPES.update(_rets)

# the open table of additive entry points (_build.ABI_ADDITIONS), under the same rule: where every later header goes
_add = load_dataset_headers(_build.ABI_ADDITIONS, STRUCTS, set(SIGNATURES) | set(_DATASET_SIGNATURES))
ADDITION_SIGNATURES = {k: v[0] for k, v in _add.items()}           # ADDITION_SIGNATURES["aux_stats"] = {"sam_aux_pair_stats_ws_bytes": [...], "sam_aux_pair_stats": [...]}
ADDITION_RESTYPES = {k: v[1] for k, v in _add.items()}
for _sigs, _rets in _add.values():
    _DATASET_SIGNATURES.update(_sigs)
    _DATASET_RESTYPES.update(_rets)

_lib = None


def lib():
    global _lib, LIB_PATH
    if _lib is None:
        alt = os.environ.get("SAM_HIP_LIB")          # tuning: load an alternative build of the same ABI (A/B runs inside one process tree)
        if alt:
            if not os.path.exists(alt):
                raise SamHipError("SAM_HIP_LIB=%s does not exist" % alt)
            LIB_PATH = alt
        # (re)build when the sources changed or the library is missing; a no-op (digest compare) otherwise.  A failed build raises: an older
        # libsam_hip.so is never loaded in place of the sources in the tree (changed signatures against an old binary = silent corruption).
        want = None
        if not alt:
            try:
                _build.build()
            except Exception as e:
                raise SamHipError("libsam_hip.so could not be (re)built from the sources in the tree (%s); there is no fallback path" % e)
            want = _build._digest()
        if not os.path.exists(LIB_PATH):
            raise SamHipError("libsam_hip.so not built (%s): run `python __graft_entry__.py` or "
                              "sam_textvqa_amd._build.build(); there is no fallback path" % LIB_PATH)
        # torch bundles its own libamdhip64; load it FIRST so libsam_hip.so binds to the same HIP runtime instance that
        # owns torch's device allocations and streams (a second runtime copy sees "no ROCm-capable device")
        import torch
        hip_rt = os.path.join(os.path.dirname(torch.__file__), "lib", "libamdhip64.so")
        if os.path.exists(hip_rt):
            C.CDLL(hip_rt, mode=C.RTLD_GLOBAL)
        l = C.CDLL(LIB_PATH)

        def bind(name):
            fn = getattr(l, name)
            if name in SIGNATURES:
                fn.argtypes, fn.restype = SIGNATURES[name], RESTYPES[name]
            else:
                fn.argtypes, fn.restype = _DATASET_SIGNATURES[name], _DATASET_RESTYPES[name]
            return fn
        have = bind("sam_build_digest")().decode()
        if want is not None and have != want:
            raise SamHipError("libsam_hip.so was built from other sources (digest %s..., tree %s...): rebuild with `python __graft_entry__.py`" % (have[:12], want[:12]))
        for name in list(SIGNATURES) + list(_DATASET_SIGNATURES):
            bind(name)
        _lib = l
    return _lib


profiler = None   # bench.py sets this to a list to collect (name, meta, start_event, end_event) per C-ABI call


def call(name, *args, meta=None):
    """invoke a status-returning entry point; non-zero -> SamHipError with the library's message"""
    if name not in SIGNATURES and name not in _DATASET_SIGNATURES:
        raise SamHipError("%s is declared in neither %s" % (name, " nor ".join("include/" + os.path.basename(p) for p in _build.public_headers())))
    l = lib()
    if profiler is not None and name not in NO_STATUS and name not in PART_VALUES:
        import torch
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        rc = getattr(l, name)(*args)
        e1.record()
        profiler.append((name, meta or {}, e0, e1))
    else:
        rc = getattr(l, name)(*args)
    if name not in NO_STATUS and name not in PART_VALUES and rc != 0:
        raise SamHipError("%s failed (rc=%d): %s" % (name, rc, l.sam_last_error().decode()))
    return rc


def ptr(t):
    """device pointer of a torch tensor (None -> NULL)"""
    return None if t is None else C.c_void_p(t.data_ptr())


_raw_stream = None


def stream_handle():
    """hipStream_t of torch's current stream on the current device (the raw-handle getter: ~1 us instead of ~10 us for building a
    torch.cuda.Stream object, 500 times per step)"""
    global _raw_stream
    import torch
    if _raw_stream is None:
        get, dev = getattr(torch._C, "_cuda_getCurrentRawStream", None), getattr(torch._C, "_cuda_getDevice", None)
        _raw_stream = (lambda: get(dev())) if get and dev else (lambda: torch.cuda.current_stream().cuda_stream)
    return C.c_void_p(_raw_stream())

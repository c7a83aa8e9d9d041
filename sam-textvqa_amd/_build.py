"""Compile the HIP sources of this package into lib/libsam_hip.so for gfx950 (hipcc cross-compiles
without a GPU).  Sources are hashed so repeated calls are no-ops; the .so stays in-tree so it
travels with the repo snapshot to the GPU box."""
import hashlib
import os
import subprocess

PKG = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(PKG, "csrc")
LIB_DIR = os.path.join(PKG, "lib")
LIB = os.path.join(LIB_DIR, "libsam_hip.so")
_INCLUDE = os.path.join(os.path.dirname(PKG), "include")
# The public headers, in the order they are hashed into the digest and parsed by _capi (one table per header: _capi.HEADER_SIGNATURES[name]).
# A new header is one line here; nothing else in _build or _capi names the headers one by one.
HEADERS = {
    "abi": os.path.join(_INCLUDE, "sam_hip.h"),                    # the C ABI: parsed into _capi.SIGNATURES / STRUCTS / CONSTANTS
    "pipeline": os.path.join(_INCLUDE, "sam_hip_pipeline.h"),      # the dataset-side entry points
    "text": os.path.join(_INCLUDE, "sam_hip_text.h"),              # entry points that start from the OCR tokens' text; sam_hip_pipeline.h includes it
    "answers": os.path.join(_INCLUDE, "sam_hip_answers.h"),        # entry points that start from the answers' text
    "step": os.path.join(_INCLUDE, "sam_hip_step.h"),              # entry points that keep a record of the step in device memory
    "question": os.path.join(_INCLUDE, "sam_hip_question.h"),      # entry points that start from the question's text
    "fasttext": os.path.join(_INCLUDE, "sam_hip_fasttext.h"),      # the OCR tokens' FastText vectors from their text
    "metrics": os.path.join(_INCLUDE, "sam_hip_metrics.h"),        # the metrics' score tables from text
    "eval": os.path.join(_INCLUDE, "sam_hip_eval.h"),              # beam-search output to per-question results
    "textprep": os.path.join(_INCLUDE, "sam_hip_textprep.h"),      # raw UTF-8 strings to cleaned code-point tensors
    "unicode": os.path.join(_INCLUDE, "sam_hip_unicode.h"),        # entry points that read the resident Unicode table
}
HEADER = HEADERS["abi"]
# Files that sam_hip.h itself includes: part of the model's ABI (they may declare value-returning queries), written apart from the 2000-line header.  The
# parser drops preprocessor lines, so _capi reads each into a table of its own (_capi.PART_SIGNATURES[name]); they are hashed with the headers above.
ABI_PARTS = {
    "aux_loss": os.path.join(_INCLUDE, "sam_hip_aux_loss.h"),      # the spatial aux heads' loss from relation codes; the codes from boxes
}
# Additive extensions of the model's ABI: public headers of their own that include sam_hip.h (a C caller includes the one it needs; sam_hip.h does not
# name them and sam_abi_version() does not move).  _capi reads each into _capi.EXTENSION_SIGNATURES[name]; hashed after the two tables above.
ABI_EXTENSIONS = {
    "aux_targets": os.path.join(_INCLUDE, "sam_hip_aux_targets.h"),  # relation tensor + padding masks -> the aux loss's codes and valid flags, one launch
}
# The OPEN table: every later additive entry point goes here (same rule as ABI_EXTENSIONS: a header of its own that includes sam_hip.h, status-returning
# prototypes only, no name another table holds).  The three tables above are pinned by the suite key by key; this one is only ever asked for membership
# ("aux_stats" in ...), so a new header is one line here and no further table.  _capi reads each into _capi.ADDITION_SIGNATURES[name]; hashed last.
ABI_ADDITIONS = {
    "aux_stats": os.path.join(_INCLUDE, "sam_hip_aux_stats.h"),      # relation confusion / fired-channel counts of the spatial aux heads
    "store": os.path.join(_INCLUDE, "sam_hip_store.h"),              # batches gathered by index from region features resident in device memory
    "sampler": os.path.join(_INCLUDE, "sam_hip_sampler.h"),          # each step's sample indices from a resident state: shuffled, sharded epochs
    "beam_merge": os.path.join(_INCLUDE, "sam_hip_beam_merge.h"),    # beam-search output chosen by answer string: beams that spell the same answer merged
    "coverage": os.path.join(_INCLUDE, "sam_hip_coverage.h"),        # answer-space upper bounds: witness sequences from the vocabulary, the OCR tokens, both
    "evalboard": os.path.join(_INCLUDE, "sam_hip_evalboard.h"),      # evaluation results collected by question index: the resident results board
}


def public_headers():
    """every public header in the order it is hashed and named in messages: HEADERS, ABI_PARTS, ABI_EXTENSIONS, ABI_ADDITIONS"""
    return list(HEADERS.values()) + list(ABI_PARTS.values()) + list(ABI_EXTENSIONS.values()) + list(ABI_ADDITIONS.values())


# a source that includes another source's text: hashed into its object stamp (score_text.hip, eval_beams.hip and beam_merge.hip read the normaliser's
# tables where score.hip keeps them)
SOURCE_INCLUDES = {"score_text.hip": ("score.hip",), "eval_beams.hip": ("score.hip",), "beam_merge.hip": ("score.hip",)}
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
# -amdgpu-mfma-vgpr-form: MFMA accumulators that the VALU consumes right away (attention scores) stay in VGPRs; without it the compiler
# put them in AGPRs and copied every value across with v_accvgpr_read/write (80 and 136 copies per loop trip in the two attention
# backward kernels, none left with the flag; the GEMMs never had any)
FLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-Wno-unused-value", "-Wno-unused-result", "-mllvm", "-amdgpu-mfma-vgpr-form=1"]


def sources():
    return sorted(os.path.join(CSRC, f) for f in os.listdir(CSRC) if f.endswith((".hip", ".cpp")))


def _tree_digest(suffixes):
    """flags, the csrc files with these suffixes (name and bytes, sorted), then every public header in registry order; a missing header raises"""
    h = hashlib.sha256(" ".join(FLAGS).encode())
    for f in sorted(os.listdir(CSRC)):
        if f.endswith(suffixes):
            h.update(f.encode())
            h.update(open(os.path.join(CSRC, f), "rb").read())
    for hdr in public_headers():
        h.update(open(hdr, "rb").read())
    return h


def _digest():
    return _tree_digest((".hip", ".cpp", ".h")).hexdigest()


def _headers_digest():
    return _tree_digest(".h")


def build(force=False, verbose=False):
    """compile what changed (per-object stamps: source + every header + flags), link, stamp the library with the digest of the whole tree.
    Any compile or link error raises: a stale library is never left in place as if it were current."""
    os.makedirs(LIB_DIR, exist_ok=True)
    stamp = os.path.join(LIB_DIR, "libsam_hip.sha256")
    dig = _digest()
    if not force and os.path.exists(LIB) and os.path.exists(stamp) and open(stamp).read().strip() == dig:
        return LIB
    hdr = _headers_digest()
    objs, procs = [], []
    for src in sources():
        obj = os.path.join(LIB_DIR, os.path.basename(src) + ".o")
        objs.append(obj)
        is_runtime = os.path.basename(src) == "runtime.cpp"
        h = hdr.copy()
        h.update(open(src, "rb").read())
        for inc in SOURCE_INCLUDES.get(os.path.basename(src), ()):
            h.update(open(os.path.join(CSRC, inc), "rb").read())
        if is_runtime:
            h.update(dig.encode())                # carries the digest string of the whole tree
        odig, ostamp = h.hexdigest(), obj + ".sha256"
        if not force and os.path.exists(obj) and os.path.exists(ostamp) and open(ostamp).read().strip() == odig:
            continue
        cmd = [HIPCC] + FLAGS + (["-x", "hip"] if src.endswith(".cpp") else []) + (['-DSAM_BUILD_DIGEST="%s"' % dig] if is_runtime else []) + \
              ["-I", _INCLUDE, "-c", src, "-o", obj]
        if verbose:
            print(" ".join(cmd))
        if os.path.exists(ostamp):
            os.remove(ostamp)
        procs.append((src, ostamp, odig, subprocess.Popen(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT)))
    for src, ostamp, odig, p in procs:
        out, _ = p.communicate()
        if p.returncode != 0:
            raise RuntimeError("hipcc failed on %s:\n%s" % (src, out.decode(errors="replace")))
        with open(ostamp, "w") as f:
            f.write(odig)
    if os.path.exists(stamp):
        os.remove(stamp)
    cmd = [HIPCC, "--offload-arch=gfx950", "-shared", "-fPIC", "-o", LIB] + objs
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    if r.returncode != 0:
        raise RuntimeError("link failed:\n%s" % r.stdout.decode(errors="replace"))
    with open(stamp, "w") as f:
        f.write(dig)
    return LIB


# ---- PyTorch-ROCm custom ops (csrc_torch/sam_torch_ops.cpp): TORCH_LIBRARY registration + coarse per-layer entry points over the C ABI ----
TORCH_OPS_SRC = os.path.join(PKG, "csrc_torch", "sam_torch_ops.cpp")
TORCH_OPS_LIB = os.path.join(LIB_DIR, "libsam_torch_ops.so")
CXX = os.environ.get("CXX", "g++")


def build_torch_ops(force=False, verbose=False):
    """g++ against the torch headers (no device code in this file); links libsam_hip.so from its own directory ($ORIGIN)"""
    import torch
    from torch.utils.cpp_extension import include_paths, library_paths
    build()
    h = hashlib.sha256(open(TORCH_OPS_SRC, "rb").read())
    for hdr in public_headers():
        h.update(open(hdr, "rb").read())
    h.update(torch.__version__.encode())
    dig, stamp = h.hexdigest(), TORCH_OPS_LIB + ".sha256"
    if not force and os.path.exists(TORCH_OPS_LIB) and os.path.exists(stamp) and open(stamp).read().strip() == dig:
        return TORCH_OPS_LIB
    rocm = os.environ.get("ROCM_PATH", "/opt/rocm")
    cmd = [CXX, "-O2", "-std=c++17", "-fPIC", "-shared", "-D__HIP_PLATFORM_AMD__=1", "-DUSE_ROCM=1",
           "-D_GLIBCXX_USE_CXX11_ABI=%d" % int(torch._C._GLIBCXX_USE_CXX11_ABI), TORCH_OPS_SRC, "-o", TORCH_OPS_LIB,
           "-I", _INCLUDE, "-I", os.path.join(rocm, "include")]
    cmd += ["-I" + i for i in include_paths()] + ["-L" + l for l in library_paths()] + ["-L", LIB_DIR, "-lsam_hip", "-Wl,-rpath,$ORIGIN",
                                                                                         "-lc10", "-ltorch_cpu", "-ltorch", "-lc10_hip", "-ltorch_hip"]
    if verbose:
        print(" ".join(cmd))
    if os.path.exists(stamp):
        os.remove(stamp)
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    if r.returncode != 0:
        raise RuntimeError("building the torch ops failed:\n%s" % r.stdout.decode(errors="replace")[-4000:])
    with open(stamp, "w") as f:
        f.write(dig)
    return TORCH_OPS_LIB


if __name__ == "__main__":
    print(build(force=True, verbose=True))
    print(build_torch_ops(force=True, verbose=True))

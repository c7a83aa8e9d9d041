"""FastText vectors of the OCR tokens from their text and a table that stays on the device.

The reference's FastTextProcessor (sam/datasets/processors.py:181-226) loads a fastText model (wiki.en: about 2.5 M words + 2 M buckets, x 300 fp32, roughly
5.4 GB) into every DataLoader worker, calls get_word_vector per word and ships fp32 [50, 300] with every sample: 60 KB padded, 600 B per valid row of a
ragged fp16 batch.  The vector is a pure function of the token's text and that table, so a batch that carries

    ocr_text int32 [B, No, Lw]     ocr_text_len int32 [B, No]          (phoc.pack_ocr_text, unchanged: one text serves PHOC, the answers and FastText)

holds everything needed besides the table: fasttext_from_text(ocr_text, ocr_text_len, index_to(model_index(load_bin(path)), "cuda"), counts) computes the
300 columns on the GPU, one launch (ops.fasttext_from_text, csrc/fasttext.hip).  SAM4C.forward does not call it yet (DESIGN.md section 3.17 says why): the
caller writes the result into batch["ocr_fasttext"].  The table is resident: the matrix takes
(nwords + bucket) * dim * 4 bytes of device memory (5.4 GB for wiki.en) and the word index nwords * (4 * Lv + 4) + 4 * n_slots bytes more (about 0.36 GB at
Lv = 32); nothing of it travels with a batch.

WHAT IS COMPUTED is written out in include/sam_hip_fasttext.h and implemented twice, here on the host (word_ids / word_vector_host / vectors_host /
vectors_host_text: the twins) and in the kernel, which equals the twins bit for bit.  The rules were written from the fastText library's published
behaviour (dictionary word + character n-grams of "<word>" hashed with FNV-1a over signed bytes, rows added in order, times 1 / count; the reference's
np.mean over token.split(" ")).  Neither the library nor a model file was available where this was written: EQUALITY WITH THE LIBRARY'S OUTPUT WAS NOT
TESTED, only the agreement of kernel and twin, the published FNV-1a vectors and hand-listed n-grams.

CASE.  FastText is case-sensitive ("The" and "the" are different dictionary words with different n-grams); PHOC is not.  score_table["ocr"] /
["ocr_len"] (metrics.collate_score_tables) holds the LOWERED tokens, so it may stand in for ocr_text / ocr_text_len only when the dataset's tokens are
already lower case.  The reference's cleaner (textvqa_dataset.py:199-215) does lower them, but that is a property of that dataset code, not of this
package: a pipeline with another cleaner must pack the tokens it would have given FastTextProcessor.  The score table's flag bits 30 and 31 are masked
off by the kernel and the twins (a code point is its low 21 bits).

LIMITS.  Lw <= 64 code points per token, dim % 4 == 0 and dim <= 512, 0 <= minn <= maxn <= 8; version-12 unquantised, unpruned, unsupervised models."""
import struct
import warnings

import numpy as np
import torch

from . import batchtext as BT
from .wordindex import INDEX_TENSORS, build_slots, index_to, table_size    # (index_to, index_lookup_host: the names callers and tests use)
from .wordindex import lookup_host as index_lookup_host

MAGIC = 793712314
VERSION = 12
ARG_NAMES = ("dim", "ws", "epoch", "minCount", "neg", "wordNgrams", "loss", "model", "bucket", "minn", "maxn", "lrUpdateRate")
DEFAULT_ARGS = dict(ws=5, epoch=5, minCount=5, neg=5, wordNgrams=1, loss=2, model=2, lrUpdateRate=100)       # what a skip-gram run writes; never read here
EOS = b"</s>"
MAX_CHARS = 64                                       # code points per token: one per lane of the kernel
MAX_DIM = 512
MAX_N = 8
CP_MASK = 0x1FFFFF                                   # 21 bits: what four UTF-8 bytes carry; bits 30 / 31 of a packed code point are flags
TEXT_KEYS = ("ocr_text", "ocr_text_len")
FASTTEXT_KEYS = ("ocr_fasttext", "ocr_ft_rows")


# ---------------------------------------------------------------------------------------------------------------- the model and its file
def make_model(words, matrix, minn, maxn, bucket, args=None):
    """a model from its parts: words (str or bytes, in id order, non-empty, each once), matrix fp32 [len(words) + bucket, dim] (kept as it is: a numpy
    array or a memory map), the n-gram range and the number of buckets -> {"words": list of bytes, "matrix", "nwords", "bucket", "minn", "maxn", "dim",
    "args": the other header fields}"""
    words = [w.encode("utf-8") if isinstance(w, str) else bytes(w) for w in words]
    if not words or any(not w or b"\0" in w for w in words) or len(set(words)) != len(words):
        raise ValueError("make_model: the dictionary needs at least one word, every word non-empty, without NUL and listed once")
    minn, maxn, bucket = int(minn), int(maxn), int(bucket)
    if not 0 <= minn <= maxn or bucket < 0 or (maxn > 0 and bucket < 1):
        raise ValueError("make_model: need 0 <= minn <= maxn and bucket >= 1 when maxn > 0 (minn=%d maxn=%d bucket=%d)" % (minn, maxn, bucket))
    if getattr(matrix, "ndim", 0) != 2 or matrix.dtype != np.float32 or matrix.shape[0] != len(words) + bucket:
        raise ValueError("make_model: matrix must be float32 [nwords + bucket, dim] = [%d, dim], got %s %s" % (
            len(words) + bucket, getattr(matrix, "dtype", None), getattr(matrix, "shape", None)))
    return {"words": words, "matrix": matrix, "nwords": len(words), "bucket": bucket, "minn": minn, "maxn": maxn, "dim": int(matrix.shape[1]),
            "args": dict(DEFAULT_ARGS, **(args or {}))}


def write_bin(path, model, counts=None, raw=None):
    """the model as a version-12 .bin file of the layout load_bin reads (little endian): magic, version, twelve int32 args and the double t, the dictionary
    (every word with its count, type 0), quant_input = 0, the input matrix; then, as the library writes them, quant_output = 0 and an all-zero output matrix
    [nwords, dim] that nothing here reads.  This is how a fixture is made.  raw: header fields written instead of the model's own ("magic", "version",
    "nlabels", "pruneidx" (a list of int pairs), "quant_input", "m", "n", "bucket") -- for the tests of load_bin's refusals."""
    raw = dict(raw or {})
    a = dict(model["args"], dim=model["dim"], bucket=raw.get("bucket", model["bucket"]), minn=model["minn"], maxn=model["maxn"])
    nwords, dim = model["nwords"], model["dim"]
    counts = [1] * nwords if counts is None else [int(c) for c in counts]
    prune = raw.get("pruneidx")
    with open(path, "wb") as f:
        f.write(struct.pack("<ii", raw.get("magic", MAGIC), raw.get("version", VERSION)))
        f.write(struct.pack("<12i", *(a[k] for k in ARG_NAMES)))
        f.write(struct.pack("<d", 1e-4))
        f.write(struct.pack("<iiiqq", nwords, nwords, raw.get("nlabels", 0), sum(counts), -1 if prune is None else len(prune)))
        for w, c in zip(model["words"], counts):
            f.write(w + b"\0" + struct.pack("<qb", c, 0))
        for pair in prune or ():
            f.write(struct.pack("<ii", *pair))
        f.write(struct.pack("<B", raw.get("quant_input", 0)))
        f.write(struct.pack("<qq", raw.get("m", nwords + model["bucket"]), raw.get("n", dim)))
        np.ascontiguousarray(model["matrix"], dtype="<f4").tofile(f)
        f.write(struct.pack("<B", 0))
        f.write(struct.pack("<qq", nwords, dim))
        np.zeros((nwords, dim), "<f4").tofile(f)


def load_bin(path):
    """read a fastText .bin (version 12) -> make_model's dict, the input matrix as a read-only memory map of the file (nothing of it is copied).
    ValueError: a wrong magic, a version other than 12, a quantised input matrix, a pruned dictionary, labels (a supervised model), bucket < 1 with
    maxn > 0, a matrix that is not [nwords + bucket, dim]."""
    import mmap
    with open(path, "rb") as f:
        buf = mmap.mmap(f.fileno(), 0, access=mmap.ACCESS_READ)
    try:
        def take(fmt, at):
            n = struct.calcsize(fmt)
            if at + n > len(buf):
                raise ValueError("load_bin: %s ends inside its header" % path)
            return struct.unpack_from(fmt, buf, at), at + n
        (magic, version), at = take("<ii", 0)
        if magic != MAGIC:
            raise ValueError("load_bin: %s is no fastText model (magic %d, expected %d)" % (path, magic, MAGIC))
        if version != VERSION:
            raise ValueError("load_bin: model version %d; only version %d is read" % (version, VERSION))
        vals, at = take("<12i", at)
        args = dict(zip(ARG_NAMES, vals))
        _, at = take("<d", at)
        (size, nwords, nlabels, _, prune), at = take("<iiiqq", at)
        if nlabels != 0 or size != nwords:
            raise ValueError("load_bin: the dictionary holds %d labels (size %d, nwords %d): supervised models are not supported" % (nlabels, size, nwords))
        if prune > 0:
            raise ValueError("load_bin: the dictionary is pruned (pruneidx_size %d): not supported" % prune)
        if args["maxn"] > 0 and args["bucket"] < 1:
            raise ValueError("load_bin: bucket = %d with maxn = %d" % (args["bucket"], args["maxn"]))
        words = []
        for _ in range(size):
            end = buf.find(b"\0", at)
            if end < 0:
                raise ValueError("load_bin: %s ends inside its dictionary" % path)
            words.append(buf[at:end])
            at = end + 1 + 9                                      # NUL, int64 count, int8 type
        (quant,), at = take("<B", at)
        if quant != 0:
            raise ValueError("load_bin: the input matrix is quantised (quant_input %d): not supported" % quant)
        (m, n), at = take("<qq", at)
        if m != nwords + args["bucket"]:
            raise ValueError("load_bin: the input matrix has %d rows, expected nwords + bucket = %d + %d" % (m, nwords, args["bucket"]))
        if n != args["dim"]:
            raise ValueError("load_bin: the input matrix has %d columns, dim is %d" % (n, args["dim"]))
        if at + 4 * m * n > len(buf):
            raise ValueError("load_bin: %s ends inside its input matrix" % path)
    finally:
        buf.close()
    matrix = np.memmap(path, dtype="<f4", mode="r", offset=at, shape=(int(m), int(n)))
    return make_model(words, matrix, args["minn"], args["maxn"], args["bucket"], args={k: v for k, v in args.items() if k in DEFAULT_ARGS})


# ---------------------------------------------------------------------------------------------------------------- the index the kernel reads
def decode_words(words):
    """UTF-8 bytes of many words -> (code points int32 [total characters], characters per word int64 [n], valid bool [n]) with numpy only (no loop over the
    words): valid = what bytes.decode("utf-8") accepts (well-formed sequences, no overlong form, no surrogate, nothing above U+10FFFF); the characters of an
    invalid word are still counted but mean nothing."""
    n = len(words)
    lens = np.fromiter((len(w) for w in words), np.int64, n)
    b = np.frombuffer(b"".join(words), np.uint8).astype(np.int64)
    total = b.size
    word = np.repeat(np.arange(n), lens)
    start = np.cumsum(lens) - lens
    cont = (b & 0xC0) == 0x80
    lead = np.flatnonzero(~cont)
    lw = word[lead]
    b0 = b[lead]
    nb = np.select([b0 < 0x80, (b0 >= 0xC2) & (b0 <= 0xDF), (b0 >= 0xE0) & (b0 <= 0xEF), (b0 >= 0xF0) & (b0 <= 0xF4)], [1, 2, 3, 4], 0)
    nxt = np.append(lead[1:], total)
    follow = np.minimum(nxt, (start + lens)[lw]) - lead - 1                   # continuation bytes behind the lead, inside its word
    bp = np.concatenate([b, np.zeros(4, np.int64)])
    c1, c2, c3 = bp[lead + 1] & 0x3F, bp[lead + 2] & 0x3F, bp[lead + 3] & 0x3F
    cp = np.select([nb == 1, nb == 2, nb == 3, nb == 4], [b0, (b0 & 0x1F) << 6 | c1, (b0 & 0x0F) << 12 | c1 << 6 | c2, (b0 & 0x07) << 18 | c1 << 12 | c2 << 6 | c3], 0)
    bad = (nb == 0) | (follow != nb - 1) | ((nb == 3) & (cp < 0x800)) | ((nb == 4) & ((cp < 0x10000) | (cp > 0x10FFFF))) | ((cp >= 0xD800) & (cp <= 0xDFFF))
    valid = np.bincount(lw[bad], minlength=n) == 0
    nonempty = lens > 0
    valid[nonempty] &= ~cont[start[nonempty]]                                 # a word that begins inside a character
    return cp.astype(np.int32), np.bincount(lw, minlength=n), valid


def model_index(model, max_word=32, n_slots=None):
    """the tensors the kernel reads, built once per run with numpy (no Python loop over the dictionary): {"matrix": fp32 [nwords + bucket, dim] (the model's
    own memory, not a copy), "cp": int32 [nwords, Lv] the code points of dictionary word i, "len": int32 [nwords] its length in code points or -1 for a
    word without an entry, "slots": int32 [T] an open-addressed table of word ids (T a power of two, by default the smallest >= 2 * nwords; n_slots sets it,
    above the number of entries; -1 = empty, home slot wordindex.text_hash & (T - 1), linear probing; a contested slot goes to the lowest id: wordindex.build_slots), "minn", "maxn",
    "bucket", "nwords", "dim", "eos": the id of "</s>" or -1} -- CPU tensors and ints; index_to(index, device) moves the four tensors.
    A dictionary word that is not valid UTF-8 keeps its matrix row and gets no entry: no str token can equal it.  A word of more than max_word (<= 64) code
    points gets no entry either, so a TOKEN of more than max_word code points is out of vocabulary by construction -- it is built from its n-grams alone,
    also when the dictionary lists it."""
    Lv = int(max_word)
    if not 1 <= Lv <= MAX_CHARS:
        raise ValueError("model_index: max_word = %d must be in [1, %d]" % (Lv, MAX_CHARS))
    if model["dim"] % 4 or not 4 <= model["dim"] <= MAX_DIM or model["maxn"] > MAX_N:
        raise ValueError("model_index: the kernel takes dim %% 4 == 0, dim <= %d and maxn <= %d (dim=%d maxn=%d)" % (MAX_DIM, MAX_N, model["dim"], model["maxn"]))
    words, nwords = model["words"], model["nwords"]
    cps, nchar, valid = decode_words(words)
    entry = valid & (nchar >= 1) & (nchar <= Lv)
    first = np.cumsum(nchar) - nchar
    cw = np.repeat(np.arange(nwords), nchar)                                  # the word of every character
    keep = entry[cw]
    cp = np.zeros((nwords, Lv), np.int32)
    cp[cw[keep], (np.arange(cps.size) - first[cw])[keep]] = cps[keep]
    ln = np.where(entry, nchar, -1).astype(np.int32)
    ids = np.flatnonzero(entry)
    T = table_size(nwords)
    if n_slots is not None:
        T = int(n_slots)
        if T < 2 or T & (T - 1) or T <= ids.size:
            raise ValueError("model_index: n_slots = %d must be a power of two above the %d entries" % (T, ids.size))
    slots = build_slots(cp, ln, ids, T)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")                                       # (a read-only memory map: nothing writes through the tensor)
        matrix = torch.from_numpy(model["matrix"] if isinstance(model["matrix"], np.memmap) else np.ascontiguousarray(model["matrix"]))
    return {"matrix": matrix, "cp": torch.from_numpy(cp), "len": torch.from_numpy(ln), "slots": torch.from_numpy(slots), "minn": model["minn"],
            "maxn": model["maxn"], "bucket": model["bucket"], "nwords": nwords, "dim": model["dim"], "eos": words.index(EOS) if EOS in words else -1}


def is_model_index(v):
    return isinstance(v, dict) and all(k in v for k in INDEX_TENSORS + ("minn", "maxn", "bucket", "nwords", "dim", "eos"))


# ---------------------------------------------------------------------------------------------------------------- the host twins
def utf8(code_points):
    """the UTF-8 bytes of code points, encoded arithmetically as the kernel does (1-4 bytes by magnitude, low 21 bits): str.encode for every valid string"""
    out = bytearray()
    for c in code_points:
        c = int(c) & CP_MASK
        if c < 0x80:
            out.append(c)
        elif c < 0x800:
            out += bytes((0xC0 | c >> 6, 0x80 | c & 0x3F))
        elif c < 0x10000:
            out += bytes((0xE0 | c >> 12, 0x80 | c >> 6 & 0x3F, 0x80 | c & 0x3F))
        else:
            out += bytes((0xF0 | c >> 18, 0x80 | c >> 12 & 0x3F, 0x80 | c >> 6 & 0x3F, 0x80 | c & 0x3F))
    return bytes(out)


def fnv1a(data):
    """the library's hash: FNV-1a, 32 bit, over the bytes taken as SIGNED chars (a byte >= 0x80 is sign-extended before the xor)"""
    h = 2166136261
    for c in data:
        h = ((h ^ (c | 0xFFFFFF00 if c >= 0x80 else c)) * 16777619) & 0xFFFFFFFF
    return h


def ngrams(s, minn, maxn):
    """the character n-grams of the bytes s (a word with its "<" ">"), in the library's order: from every byte that starts a character, n = 1 .. maxn
    characters while bytes remain; kept when n >= minn and not (n == 1 and it touches either end of s)"""
    out = []
    for i in range(len(s)):
        if s[i] & 0xC0 == 0x80:
            continue
        j, n = i, 1
        while j < len(s) and n <= maxn:
            j += 1
            while j < len(s) and s[j] & 0xC0 == 0x80:
                j += 1
            if n >= minn and not (n == 1 and (i == 0 or j == len(s))):
                out.append(s[i:j])
            n += 1
    return out


def subwords(s, minn, maxn, bucket, nwords):
    return [nwords + fnv1a(g) % bucket for g in ngrams(s, minn, maxn)]


def _code_points(w):
    return BT.code_points(w, CP_MASK)


def word_ids(w, index):
    """the rows get_word_vector(w) adds, in order; w a str or a sequence of code points (no U+0020 inside: a piece of a token)"""
    cps = _code_points(w)
    wid = index_lookup_host(index, cps)
    ids = [wid] if wid >= 0 else []
    if index["maxn"] > 0 and not (wid >= 0 and wid == index["eos"]):
        ids += subwords(b"<" + utf8(cps) + b">", index["minn"], index["maxn"], index["bucket"], index["nwords"])
    return ids


def word_vector_host(w, index):
    """get_word_vector(w), float32 [dim]: v = 0, v += matrix[id] in list order (fp32 adds), v *= (float)(1.0 / count); no id -> zeros"""
    f = np.float32
    matrix = index["matrix"].cpu().numpy() if torch.is_tensor(index["matrix"]) else index["matrix"]
    ids = word_ids(w, index)
    v = np.zeros(index["dim"], f)
    for i in ids:
        v = v + np.asarray(matrix[i], f)
    if ids:
        v = v * f(1.0 / len(ids))
    return v


def token_vector_host(token, index):
    """the reference's vector of one OCR token (processors.py:96-102): np.mean of the word vectors of token.split(" "), axis 0, fp32"""
    pieces, cur = [], []
    for c in _code_points(token):
        if c == 0x20:
            pieces.append(cur)
            cur = []
        else:
            cur.append(c)
    pieces.append(cur)
    return np.mean([word_vector_host(p, index) for p in pieces], axis=0)


def vectors_host(tokens, index):
    """numpy float32 [len(tokens), dim]: the reference's vector of every token (str, or a sequence of code points), the kernel's host twin"""
    out = np.zeros((len(tokens), index["dim"]), np.float32)
    for i, t in enumerate(tokens):
        out[i] = token_vector_host(t, index)
    return out


def vectors_host_text(ocr_text, ocr_text_len, index, counts=None):
    """the kernel's output for packed text, on the host: float32 [B, No, dim] with the kernel's clamps (lengths into [0, Lw], counts into [0, No]; slots at or
    past the count are zero rows) and its 21-bit code-point mask"""
    index = dict(index, matrix=index["matrix"].cpu().numpy() if torch.is_tensor(index["matrix"]) else index["matrix"])
    return BT.map_slots(ocr_text, ocr_text_len, counts, index["dim"], lambda cps: token_vector_host(cps, index))


# ---------------------------------------------------------------------------------------------------------------- batches
def has_text(batch_dict):
    return BT.has_text(BT.OCR_TEXT_FASTTEXT, batch_dict)


def wants_fasttext(batch_dict):
    """the batch gives the tokens' text and no FastText tensor of either form: its FastText block is to be computed from the text"""
    return has_text(batch_dict) and not any(k in batch_dict for k in FASTTEXT_KEYS)


def check(batch_dict, n_ocr=None):
    """the rule for a consumer that holds a table: a batch opts in with BOTH text keys and no FastText tensor of either form; text next to ocr_fasttext /
    ocr_ft_rows raises ValueError; -> whether it opted in.  Shapes and dtypes as phoc.check."""
    return BT.check(BT.OCR_TEXT_FASTTEXT, batch_dict, n_ocr)


def fasttext_from_text(ocr_text, ocr_text_len, index, counts=None, dtype=torch.float32):
    """the GPU [B, No, dim] tensor (fp32, or bf16: rounded once) of packed text, one launch: bit for bit vectors_host_text.  index: model_index(...) with its
    tensors on the GPU (index_to); counts int32 [B] (optional): slots at or past it are zero rows.  Nothing is read by the host: capturable."""
    from . import ops
    B, No = ocr_text.shape[:2]
    out = torch.empty((B, No, int(index["dim"])), dtype=dtype, device=ocr_text.device)
    ops.fasttext_from_text(ocr_text.contiguous(), ocr_text_len.contiguous(), counts, index, out.view(B * No, -1))
    return out

"""The exact-match word index, its hash and Python's whitespace set on the host: the one copy each, the twin of csrc/text.h.

The answer vocabulary (answers.vocab_index), BERT's vocab.txt (wordpiece.vocab_index) and the fastText dictionary (fasttext.model_index) are kept on the
device in one form: "cp" int32 [n, Lv] the words' code points, "len" int32 [n] their lengths (-1: a word without an entry), "slots" int32 [T] an
open-addressed table of word ids -- T a power of two, -1 = empty, home slot text_hash & (T - 1), linear probing.  build_slots fills the table, lookup_host
is the host twin of the kernels' probes (index_lookup / index_lookup_wave of csrc/text.h), index_to moves an index's tensors.  WHITESPACE is the set
str.split() / str.strip() / str.isspace() use, the list is_space of csrc/text.h writes out.  This module imports none of the package's others."""
import numpy as np
import torch

# the code points c with chr(c).isspace() (tests/test_answer_text_cpu.py enumerates all code points, here and in csrc/text.h)
WHITESPACE = frozenset(list(range(0x09, 0x0E)) + list(range(0x1C, 0x21)) + [0x85, 0xA0, 0x1680] + list(range(0x2000, 0x200B)) + [0x2028, 0x2029, 0x202F, 0x205F, 0x3000])
INDEX_TENSORS = ("matrix", "cp", "len", "slots")


def mix32(x):
    """lowbias32 on numpy uint32 (a scalar or an array): mix32 of csrc/common.h"""
    x = x ^ (x >> np.uint32(16))
    x = x * np.uint32(0x7FEB352D)
    x = x ^ (x >> np.uint32(15))
    x = x * np.uint32(0x846CA68B)
    return x ^ (x >> np.uint32(16))


def text_hash_rows(cp, ln):
    """the hash that places a word in the index, of every row of cp [n, L] at its length ln [n] -> uint32 [n]: FNV-1a over the code points as 32-bit units,
    then mix32 (text_hash of csrc/text.h)"""
    h = np.full(cp.shape[0], 0x811C9DC5, np.uint32)
    with np.errstate(over="ignore"):
        for k in range(cp.shape[1]):
            h = np.where(k < ln, (h ^ cp[:, k].astype(np.uint32)) * np.uint32(0x01000193), h)
        return mix32(h)


def text_hash(code_points):
    """text_hash_rows of one word, as an int"""
    cps = np.array([[int(c) & 0xFFFFFFFF for c in code_points]], np.int64)
    return int(text_hash_rows(cps, np.array([cps.shape[1]]))[0])


def table_size(n):
    """the smallest power of two >= 2 n (and >= 2): the number of slots the builders give n words"""
    T = 2
    while T < 2 * n:
        T *= 2
    return T


def build_slots(cp, ln, ids, n_slots):
    """the slot table of the words `ids` (ascending) of cp [n, Lv] / ln [n] -> int32 [n_slots], -1 = empty.  Vectorised, in rounds: every word still without
    a slot tries its next one, starting from its home slot; a contested slot goes to the lowest id.  Every word ends up reachable from its home slot over
    occupied slots only, which is all the probes rely on."""
    T, todo = int(n_slots), np.asarray(ids, np.int64)
    if T < 2 or T & (T - 1) or T <= todo.size:
        raise ValueError("build_slots: n_slots = %d must be a power of two above the %d entries" % (T, todo.size))
    slots = np.full(T, -1, np.int32)
    at = (text_hash_rows(cp[todo], ln[todo]) & np.uint32(T - 1)).astype(np.int64)
    while todo.size:
        free = slots[at] < 0
        s, firsts = np.unique(at[free], return_index=True)                   # `todo` ascends, so the first claimant of a slot is its lowest id
        won = np.flatnonzero(free)[firsts]
        slots[s] = todo[won]
        rest = np.ones(todo.size, bool)
        rest[won] = False
        todo, at = todo[rest], (at[rest] + 1) & (T - 1)
    return slots


def index_to(index, device):
    """the index with its tensors (whichever of INDEX_TENSORS it holds) on `device`"""
    return dict(index, **{k: index[k].to(device) for k in INDEX_TENSORS if k in index})


def lookup_host(index, code_points):
    """host twin of the kernels' probe: the id of the word with exactly these code points, or -1"""
    cps = [int(c) for c in code_points]
    cp, ln, slots = index["cp"].cpu().numpy(), index["len"].cpu().numpy(), index["slots"].cpu().numpy()
    T, n = len(slots), len(cps)
    if n > cp.shape[1]:
        return -1
    s = text_hash(cps) & (T - 1)
    for _ in range(T):
        w = int(slots[s])
        if w < 0:
            return -1
        if int(ln[w]) == n and cp[w, :n].tolist() == cps:
            return w
        s = (s + 1) & (T - 1)
    return -1

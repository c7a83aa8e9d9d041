"""CPU: the word index's one host copy (sam_textvqa_amd/wordindex.py) -- build_slots' table and lookup_host against plain Python: a dict of the words and
an FNV-1a / lowbias32 written out here, not the module's.  Shared with tests/test_wordindex_gpu.py: wrapping_words, a vocabulary whose probe chain runs
over the end of the table."""
import functools

import numpy as np
import pytest
import torch

from sam_textvqa_amd import wordindex as WI
from tests.test_answer_text_cpu import colliding_vocab, golden_batch, near_misses


def plain_hash(word):
    """FNV-1a over the code points as 32-bit units, then lowbias32, in Python integers"""
    h = 0x811C9DC5
    for c in word:
        h = ((h ^ ord(c)) * 0x01000193) & 0xFFFFFFFF
    h ^= h >> 16
    h = (h * 0x7FEB352D) & 0xFFFFFFFF
    h ^= h >> 15
    h = (h * 0x846CA68B) & 0xFFFFFFFF
    return h ^ (h >> 16)


@functools.lru_cache(maxsize=None)
def wrapping_words(T, n=4, prefix="k", continuation=0):
    """the first n words prefix + number whose home slot in a table of T slots is T - 2 or T - 1 (found by search, on the CPU): at least n - 2 of them are
    placed past the end, from slot 0 on.  The last `continuation` of them carry "##" in front (the highest ids lose a contested slot: they are the placed ones)."""
    out = []
    for i in range(100000):
        w = ("##" if len(out) >= n - continuation else "") + "%s%d" % (prefix, i)
        if plain_hash(w) & (T - 1) >= T - 2:
            out.append(w)
            if len(out) == n:
                return tuple(out)
    raise AssertionError("fewer than %d words with home slot %d or %d among 100000 candidates" % (n, T - 2, T - 1))


def packed(words, Lv):
    cp, ln = np.zeros((len(words), Lv), np.int32), np.zeros(len(words), np.int32)
    for i, w in enumerate(words):
        cp[i, :len(w)] = [ord(c) for c in w]
        ln[i] = len(w)
    return cp, ln


def vocabulary(which):
    """(words, number of slots)"""
    if which == "golden answers":
        words = golden_batch()[0].word_list
    elif which == "golden wordpiece":
        from tests.test_wordpiece_cpu import golden
        words = golden()[0]
    elif which == "colliding7":
        words = colliding_vocab().word_list
    else:
        return list(wrapping_words(8)), 8
    return list(words), WI.table_size(len(words))


@pytest.mark.parametrize("which", ["golden answers", "golden wordpiece", "colliding7", "wraps at T=8"])
def test_build_slots_places_every_word_on_an_occupied_chain_and_lookup_is_the_dict(which):
    words, T = vocabulary(which)
    V, ids = len(words), {w: i for i, w in enumerate(words)}
    assert len(ids) == V and T & (T - 1) == 0 and T > V
    cp, ln = packed(words, 32)
    slots = WI.build_slots(cp, ln, np.arange(V), T)
    assert slots.dtype == np.int32 and slots.shape == (T,)
    assert sorted(slots[slots >= 0].tolist()) == list(range(V)) and (slots[slots < 0] == -1).all()        # every id once, the rest empty
    where = {int(w): s for s, w in enumerate(slots.tolist()) if w >= 0}
    wrapped = 0
    for w, i in ids.items():
        s, steps = plain_hash(w) & (T - 1), 0
        while s != where[i]:                                          # from the home slot to the word's own: occupied all the way
            assert slots[s] >= 0 and steps < T, (w, s)
            s, steps = (s + 1) & (T - 1), steps + 1
        wrapped += where[i] < (plain_hash(w) & (T - 1))
    if which == "wraps at T=8":
        assert all(plain_hash(w) & 7 >= 6 for w in words) and wrapped >= 2 and slots[0] >= 0 and slots[7] >= 0      # the chain runs from slot 7 on to slot 0
    if which == "colliding7":
        assert (V, T) == (7, 16) and any(where[i] != plain_hash(w) & 15 for w, i in ids.items())
    index = {"cp": torch.from_numpy(cp), "len": torch.from_numpy(ln), "slots": torch.from_numpy(slots)}
    some = words if V < 100 else words[::37]
    for w in words + [m for w in some for m in near_misses(w)] + ["", "zzz", "x" * 33, "\U0001F600"]:
        assert WI.lookup_host(index, [ord(c) for c in w]) == ids.get(w, -1), w
    assert WI.text_hash([ord(c) for c in words[-1]]) == plain_hash(words[-1]) and WI.text_hash([]) == plain_hash("")


def test_the_builders_and_their_old_names_share_the_one_copy():
    from sam_textvqa_amd import answers as A, fasttext as FT, metrics as M, textprep as TP
    assert A.vocab_lookup_host is WI.lookup_host is FT.index_lookup_host and A.index_to is WI.index_to is FT.index_to
    assert A.text_hash is WI.text_hash and A._mix32 is WI.mix32
    assert A.WHITESPACE is WI.WHITESPACE is TP.WHITESPACE is M.WHITESPACE and M._WS == {chr(c) for c in WI.WHITESPACE}
    with pytest.raises(ValueError, match="n_slots"):
        WI.build_slots(*packed(["a", "b"], 4), np.arange(2), 2)       # no room for an empty slot: a probe for an absent word would not end early
    with pytest.raises(ValueError, match="n_slots"):
        WI.build_slots(*packed(["a", "b"], 4), np.arange(2), 6)

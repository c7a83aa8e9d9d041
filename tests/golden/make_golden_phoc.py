#!/usr/bin/env python3
"""Generate tests/golden/phoc.npz by running the REFERENCE's PHOC (sam/phoc/build_phoc.py over sam/phoc/cphoc.c) on a word list.

Runs ONLY in the build container (the reference never travels to the GPU box).  The reference's C extension is compiled into a temporary directory outside
the repository (gcc -O2 -shared -fPIC, plain x86-64: no -march, hence no FMA) and loaded as sam.phoc.cphoc; the reference's own build_phoc.py is then
imported on top of it, so its lowering / filtering and the raw call both run as the reference wrote them.  Nothing of the reference's program text and no
binary is stored: the fixture holds data only.

phoc.npz: words (uint8: the UTF-8 bytes of the JSON list of raw tokens), rows (uint8 [N, 76]: np.packbits of each token's 604 values, which are all 0 / 1),
alphabet (36 names, in column order) and bigrams (50 names, in column order) -- both read off the rows the reference produces for one- and two-character
words, not off its source.

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_phoc.py
"""
import importlib
import importlib.machinery
import importlib.util
import json
import os
import random
import subprocess
import sys
import sysconfig
import tempfile
import types

sys.dont_write_bytecode = True
import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
from tests.golden.make_golden import REF  # noqa: E402

CANDIDATES = "abcdefghijklmnopqrstuvwxyz0123456789"


def load_reference_build_phoc(tmp):
    so = os.path.join(tmp, "cphoc" + (sysconfig.get_config_var("EXT_SUFFIX") or ".so"))
    subprocess.run(["gcc", "-O2", "-shared", "-fPIC", "-I" + sysconfig.get_paths()["include"], os.path.join(REF, "sam", "phoc", "cphoc.c"), "-o", so], check=True)
    for name, path in (("sam", os.path.join(REF, "sam")), ("sam.phoc", os.path.join(REF, "sam", "phoc"))):       # bare packages: their __init__ is not run
        pkg = types.ModuleType(name)
        pkg.__path__ = [path]
        sys.modules[name] = pkg
    spec = importlib.util.spec_from_loader("sam.phoc.cphoc", importlib.machinery.ExtensionFileLoader("sam.phoc.cphoc", so))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    sys.modules["sam.phoc.cphoc"] = mod
    return importlib.import_module("sam.phoc.build_phoc").build_phoc


def names_from_rows(build_phoc):
    """column order of the unigrams and bigrams, read off the reference's output: a one-character word lights column k of the first unigram region, a
    two-character word that is a listed bigram lights column 504 + k"""
    alphabet = {}
    for c in CANDIDATES:
        (cols,) = np.nonzero(build_phoc(c)[:36])
        alphabet[int(cols[0])] = c
    bigrams = {}
    for a in CANDIDATES:
        for b in CANDIDATES:
            cols = np.nonzero(build_phoc(a + b)[504:554])[0]
            if cols.size:
                bigrams[int(cols[0])] = a + b
    assert sorted(alphabet) == list(range(36)) and sorted(bigrams) == list(range(50))
    return [alphabet[k] for k in range(36)], [bigrams[k] for k in range(50)]


def word_list(alphabet, bigrams):
    rng = random.Random(604)
    abc = "".join(alphabet)
    words = []
    for n in range(1, 37):                                   # n distinct characters: pins every (n, index) unigram decision
        r = (7 * n) % 36
        words.append((abc[r:] + abc[:r])[:n])
    for n in range(37, 65):                                  # two rotations of the alphabet per length
        for r in (n % 36, (5 * n + 11) % 36):
            rot = abc[r:] + abc[:r]
            words.append((rot * 2)[:n])
    k = 0
    for n in range(2, 33):                                   # one listed bigram at i among digits (no listed bigram holds a digit), cycling through all 50
        for i in range(n - 1):
            filler = [abc[26 + (i + j) % 10] for j in range(n)]
            filler[i: i + 2] = bigrams[k % 50]
            words.append("".join(filler))
            k += 1
    for _ in range(300):                                     # random words: letters weighted towards bigram material
        n = rng.choice([1, 2, 3, 3, 4, 4, 5, 5, 6, 6, 7, 8, 9, 10, 11, 12, 14, 17, 23, 31])
        words.append("".join(rng.choice("etaoinshrdlu" * 3 + abc) for _ in range(n)))
    words += ["the", "within", "THE", "The", "Hello,", "WORLD!", "joe's", "'s", "'S", "", " ", "  two  words ", "a b", "e-mail", "3.50", "$12", "100%", "#1", "co.uk",
              "\tstop\n", "Über", "STRASSE", "straße", "ß", "ΣΑΣ", "ὈΔΥΣΣΕΎΣ", "１２３", "ａｂｃ", "İstanbul", "İ", "K", "2K", "Kelvin",
              "i̇", "k", "I", "K", "ı", "ſ", "Å", "Ω", "naïve", "café", "ÀÉÎ", "x" * 64, "Th" * 32, "9" * 33, "?!", "...", "@home", "<pad>"]
    assert all(len(w) <= 64 for w in words)
    return words


def main():
    with tempfile.TemporaryDirectory() as tmp:
        assert not os.path.abspath(tmp).startswith(os.path.dirname(os.path.dirname(HERE)) + os.sep)
        build_phoc = load_reference_build_phoc(tmp)
        alphabet, bigrams = names_from_rows(build_phoc)
        words = word_list(alphabet, bigrams)
        rows = np.stack([build_phoc(w) for w in words])
    assert rows.shape == (len(words), 604) and rows.dtype == np.float32 and np.isin(rows, (0.0, 1.0)).all()
    out = os.path.join(HERE, "phoc.npz")
    np.savez_compressed(out, words=np.frombuffer(json.dumps(words).encode("utf-8"), np.uint8), rows=np.packbits(rows.astype(np.uint8), axis=1),
                        alphabet=np.array(alphabet), bigrams=np.array(bigrams))
    print("%s: %d words, %d bytes" % (out, len(words), os.path.getsize(out)))


if __name__ == "__main__":
    main()

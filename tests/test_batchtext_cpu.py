"""CPU: the one owner of the batch's text forms (sam_textvqa_amd/batchtext.py).  Three things are held here: every outcome the check functions, the
packers and the status messages gave before the module existed (tests/golden/batch_text_rules.json, recorded by tests/golden/make_golden_batchtext.py
from the functions as they were written out) against the functions as they are now; the shared helpers directly; and the declared key groups against the
*_KEYS tuples and limits the feature modules publish."""
import glob
import json
import os
import re

import numpy as np
import pytest
import torch

from sam_textvqa_amd import batchtext as BT
from tests.golden import make_golden_batchtext as G

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---------------------------------------------------------------------------------------------- the recorded behaviour
@pytest.fixture(scope="module")
def recorded():
    with open(os.path.join(ROOT, "tests", "golden", "batch_text_rules.json")) as f:
        return json.load(f)


@pytest.fixture(scope="module")
def replayed():
    return G.record()


def test_every_subset_of_every_check_functions_keys_was_recorded(recorded):
    want = G.check_functions()
    assert set(recorded["checks"]) == set(want)
    for name, (_, keys) in want.items():
        got = recorded["checks"][name]
        assert got["keys"] == list(keys) and len(got["subsets"]) == 2 ** len(keys), name
        assert [m["case"] for m in got["malformed"]] == [case for case, _ in G.malformed().get(name, [])], name
    for name in ("phoc.check", "fasttext.check", "wordpiece.check", "answers.check_answer_text", "metrics.check_score_text", "textprep.check_raw",
                 "textprep.check_question_raw"):                    # the seven, each with accepting and refusing subsets and with malformed tensors
        got = recorded["checks"][name]
        assert any("err" in o for o in got["subsets"]) and any("ret" in o for o in got["subsets"]) and got["malformed"], name
    assert {name: len(cases) for name, cases in recorded["packers"].items()} == {name: len(cases) for name, (_, cases) in G.packer_cases().items()}
    assert {name: [c["status"] for c in cases] for name, cases in recorded["status"].items()} == {name: G.status_vectors(bits) for name, (_, bits) in G.status_functions().items()}


@pytest.mark.parametrize("name", sorted(G.check_functions()))
def test_check_functions_answer_as_recorded(recorded, replayed, name):
    want, got = recorded["checks"][name], replayed["checks"][name]
    for mask, (w, g) in enumerate(zip(want["subsets"], got["subsets"])):
        assert g == w, (name, [k for i, k in enumerate(want["keys"]) if mask >> i & 1])
    assert got == want


@pytest.mark.parametrize("section", ["packers", "status"])
def test_packers_and_status_messages_answer_as_recorded(recorded, replayed, section):
    for name, want in recorded[section].items():
        for w, g in zip(want, replayed[section][name]):
            assert g == w, (name, w.get("case", w.get("status")))
    assert replayed[section] == recorded[section]


# ---------------------------------------------------------------------------------------------- the helpers
def test_to_numpy_code_points_and_text_of():
    t = torch.arange(6, dtype=torch.int32).reshape(2, 3).requires_grad_(False)
    assert isinstance(BT.to_numpy(t), np.ndarray) and BT.to_numpy(t).tolist() == [[0, 1, 2], [3, 4, 5]]
    a = np.arange(3)
    assert BT.to_numpy(a) is a and BT.to_numpy([1, 2]).tolist() == [1, 2]
    assert BT.to_numpy(torch.ones(2, requires_grad=True)).tolist() == [1.0, 1.0]
    assert BT.code_points("aé\U0001F600") == [97, 233, 0x1F600] and BT.code_points("") == []
    assert BT.code_points(np.array([97 | 1 << 30, 98], np.int32), (1 << 30) - 1) == [97, 98] and BT.code_points([np.int64(5), 1 << 30]) == [5, 1 << 30]
    assert all(type(c) is int for c in BT.code_points(np.array([1, 2], np.int32)))
    assert BT.text_of([97, 233, 0x1F600]) == "aé\U0001F600" and BT.text_of(np.array([], np.int32)) == ""


def test_pack_rows_fills_rows_and_lengths_and_raises_only_the_callers_message():
    over = lambda at, s, n: "row %r (%r) has %d" % (at, s, n)
    text, ln = BT.pack_rows((2, 3, 4), [((0, 1), "abcd"), ((1, 2), "é"), ((1, 0), ""), ((0, 0), [7 | 1 << 30, 8])], 4, over)
    assert text.dtype == np.int32 and ln.dtype == np.int32 and text.shape == (2, 3, 4) and ln.shape == (2, 3)
    assert text.tolist() == [[[7 | 1 << 30, 8, 0, 0], [97, 98, 99, 100], [0] * 4], [[0] * 4, [0] * 4, [233, 0, 0, 0]]] and ln.tolist() == [[2, 4, 0], [0, 0, 1]]
    text, ln = BT.pack_rows((3, 2), enumerate(["ab", "", "\ud800z"]), 2, over)               # int indices; a lone surrogate is its own code point, as ord gives it
    assert text.tolist() == [[97, 98], [0, 0], [0xD800, 122]] and ln.tolist() == [2, 0, 2]
    with pytest.raises(ValueError) as e:
        BT.pack_rows((3, 2), enumerate(["ab", "abc", "abcd"]), 2, over)
    assert str(e.value) == "row 1 ('abc') has 3"                                              # the first row over the capacity, its index, itself, its length
    with pytest.raises(ValueError) as e:
        BT.pack_rows((2, 2), ((i, s) for i, s in enumerate([[1, 2, 3], "a"])), 2, over)
    assert str(e.value) == "row 0 ([1, 2, 3]) has 3"

    def rows():                                                                               # a generator's own refusal comes when its row is reached
        yield 0, "abc"
        raise KeyError("row 1")
    with pytest.raises(ValueError):
        BT.pack_rows((2, 2), rows(), 2, over)
    with pytest.raises(KeyError):
        BT.pack_rows((2, 3), rows(), 3, over)
    # into the caller's arrays: what is not named stays as it was; cap=None checks nothing here (numpy refuses a row wider than the array)
    text, ln = np.full((2, 2, 3), 9, np.int32), np.full((2, 2), 9, np.int32)
    assert BT.pack_rows((text[1], ln[1]), [(1, "ab")])[0] is not None
    assert text.tolist() == [[[9] * 3] * 2, [[9] * 3, [97, 98, 9]]] and ln.tolist() == [[9, 9], [9, 2]]
    with pytest.raises(IndexError):
        BT.pack_rows((text[1], ln[1]), [(0, "abcd")])
    # nothing to write: no items, no slots, rows of no width
    assert BT.pack_rows((2, 3), [])[0].tolist() == [[0] * 3] * 2 and BT.pack_rows((2, 0, 3), [])[1].shape == (2, 0)
    text, ln = BT.pack_rows((2, 0), [(0, ""), (1, "")])
    assert text.shape == (2, 0) and ln.tolist() == [0, 0]


def test_pack_rows_equals_the_written_out_loop_on_random_text():
    rng = np.random.RandomState(0)
    alphabet = "abcXYZ '?é中\U0001F600"
    strings = [["".join(alphabet[i] for i in rng.randint(0, len(alphabet), rng.randint(0, 7))) for _ in range(5)] for _ in range(4)]
    want, want_len = np.zeros((4, 5, 6), np.int32), np.zeros((4, 5), np.int32)
    for b, row in enumerate(strings):
        for i, s in enumerate(row):
            want[b, i, :len(s)] = [ord(c) for c in s]
            want_len[b, i] = len(s)
    text, ln = BT.pack_rows((4, 5, 6), (((b, i), s) for b, row in enumerate(strings) for i, s in enumerate(row)), 6, None)
    np.testing.assert_array_equal(text, want)
    np.testing.assert_array_equal(ln, want_len)
    mixed, _ = BT.pack_rows((4, 5, 6), (((b, i), s if (b + i) % 2 else [ord(c) for c in s]) for b, row in enumerate(strings) for i, s in enumerate(row)), 6, None)
    np.testing.assert_array_equal(mixed, want)
    assert [BT.strings(text[b], ln[b]) for b in range(4)] == strings                          # and back


def test_unpack_clamps_as_the_kernels_do_and_strings_reads_rows():
    text = torch.tensor([[[97, 98, 99], [100, 0, 0]]], dtype=torch.int32)
    t, ln = BT.unpack(text, torch.tensor([5, -2], dtype=torch.int32))                         # flat lengths are reshaped; over the width -> the width, negative -> 0
    assert isinstance(t, np.ndarray) and t.shape == (1, 2, 3) and ln.tolist() == [[3, 0]]
    assert BT.unpack(text.numpy(), [[2, 1]])[1].tolist() == [[2, 1]]
    assert BT.strings(t[0], ln[0]) == ["abc", ""] and BT.strings(text[0], torch.tensor([1, 1])) == ["a", "d"]
    assert BT.strings(np.zeros((0, 4), np.int32), np.zeros(0, np.int32)) == []
    # the per-slot frame: lengths clamped, counts clamped into [0, No] (None: every slot), zero rows behind the count
    seen = lambda cps: [len(cps), int(cps.sum())]
    two = torch.tensor([[[97, 98, 99], [100, 0, 0]], [[1, 2, 3], [4, 5, 6]]], dtype=torch.int32)
    lens = torch.tensor([[5, -2], [1, 2]], dtype=torch.int32)
    assert BT.map_slots(two, lens, None, 2, seen).tolist() == [[[3, 294], [0, 0]], [[1, 1], [2, 9]]]
    got = BT.map_slots(two, lens, torch.tensor([9, -1], dtype=torch.int32), 2, seen)
    assert got.dtype == np.float32 and got.tolist() == [[[3, 294], [0, 0]], [[0, 0], [0, 0]]]
    assert BT.map_slots(two.numpy(), lens.numpy(), [1, 1], 2, seen).tolist() == [[[3, 294], [0, 0]], [[1, 1], [0, 0]]]


def test_pinned_pins_every_tensor_or_none():
    class Pinnable:
        def pin_memory(self):
            return "pinned"
    d = {"a": Pinnable(), "b": Pinnable()}
    assert BT.pinned(d, False) is d and BT.pinned(d, True) == {"a": "pinned", "b": "pinned"} and list(BT.pinned(d, True)) == ["a", "b"]


def test_first_flagged_names_the_first_flagged_entry_by_its_first_listed_bit():
    reasons = ((2, "two at %(L)d"), (1, "one"), (8, "eight %(W)s"))
    assert BT.first_flagged([], reasons, L=1, W="w") is None and BT.first_flagged([0, 0], reasons, L=1, W="w") is None
    assert BT.first_flagged([0, 3, 8], reasons, L=5, W="w") == (1, 2, "two at 5")               # the table's order, not the bits' magnitude
    assert BT.first_flagged([4, 16, 9], reasons, L=5, W="w") == (2, 1, "one")                   # bits the table does not name flag nothing
    assert BT.first_flagged([8], reasons, L=5, W="w") == (0, 8, "eight w")
    with pytest.raises(KeyError):
        BT.first_flagged([8], reasons, L=5)                                                   # a reason's parameter left out is an error, when that reason is reached
    assert BT.first_flagged([1], reasons) == (0, 1, "one")


# ---------------------------------------------------------------------------------------------- the declarations
def test_the_groups_are_the_key_tuples_and_limits_the_modules_publish():
    from sam_textvqa_amd import answers, fasttext, metrics, phoc, textprep, wordpiece
    rule = lambda group, kind: [keys for k, keys, _ in group.rules if k == kind]
    assert list(BT.GROUPS) == ["question raw", "question text", "OCR raw", "OCR text, PHOC", "OCR text, FastText", "answer raw", "answer text, answer table",
                               "answer text, score table"]
    assert BT.QUESTION_RAW.keys == textprep.QUESTION_RAW_KEYS and BT.OCR_RAW.keys == textprep.OCR_RAW_KEYS and BT.ANSWER_RAW.keys == textprep.ANSWER_RAW_KEYS
    assert BT.QUESTION_TEXT.keys == wordpiece.QUESTION_TEXT_KEYS and BT.OCR_TEXT_PHOC.keys == phoc.TEXT_KEYS and BT.OCR_TEXT_FASTTEXT.keys == fasttext.TEXT_KEYS
    assert BT.ANSWER_TEXT_TABLE.keys == BT.ANSWER_TEXT_SCORE.keys == answers.ANSWER_TEXT_KEYS
    assert BT.ANSWER_TEXT_SCORE.keys + rule(BT.ANSWER_TEXT_SCORE, "pair")[0] == metrics.SCORE_TEXT_KEYS
    assert rule(BT.OCR_TEXT_FASTTEXT, "not") == [fasttext.FASTTEXT_KEYS] and rule(BT.ANSWER_TEXT_TABLE, "need") == [phoc.TEXT_KEYS]
    assert rule(BT.QUESTION_RAW, "not") == [wordpiece.QUESTION_TEXT_KEYS + wordpiece.QUESTION_KEYS[:2]] and rule(BT.QUESTION_TEXT, "not") == [wordpiece.QUESTION_KEYS[:2]]
    assert rule(BT.OCR_RAW, "not") == [phoc.TEXT_KEYS] and rule(BT.ANSWER_RAW, "not") == [answers.ANSWER_TEXT_KEYS]
    # the packed shapes: rank, width name and maximum as the packers and the kernels have them
    assert BT.QUESTION_TEXT.shape == (("B",), "Lq", wordpiece.MAX_QUESTION_CHARS) and BT.OCR_TEXT_PHOC.shape == (("B", "No"), "Lw", phoc.MAX_CHARS)
    assert BT.OCR_TEXT_FASTTEXT.shape == (("B", "No"), "Lw", fasttext.MAX_CHARS)
    assert BT.ANSWER_TEXT_TABLE.shape == BT.ANSWER_TEXT_SCORE.shape == (("B", "A"), "La", answers.MAX_ANSWER_CHARS) and textprep.MAX_CHARS == answers.MAX_ANSWER_CHARS
    assert [g.shape for g in (BT.QUESTION_RAW, BT.OCR_RAW, BT.ANSWER_RAW)] == [None] * 3
    assert [name for name, g in BT.GROUPS.items() if g.checked] == ["question text", "OCR text, PHOC", "OCR text, FastText"]          # no check added, none dropped
    for g in BT.GROUPS.values():
        assert len(g.keys) == 2 and g.label == "%s / %s" % g.keys and all(kind in ("not", "need", "pair", "any") for kind, _, _ in g.rules)
        assert not set(g.keys) & {k for _, keys, _ in g.rules for k in keys}
    # every pair a rule names is some group's pair: the forms of one text exclude or need each other, nothing else
    pairs = {g.keys for g in BT.GROUPS.values()}
    for g in BT.GROUPS.values():
        for _, keys, _ in g.rules:
            named = [k for k in keys if k.endswith(("_text", "_text_len", "_raw", "_raw_off"))]
            assert all(any(k in p for p in pairs) for k in named), (g.label, keys)


def test_the_public_forwards_answer_as_the_declarations_do():
    from sam_textvqa_amd import fasttext, phoc, wordpiece
    w = G.well_formed()
    for module, group in ((phoc, BT.OCR_TEXT_PHOC), (fasttext, BT.OCR_TEXT_FASTTEXT), (wordpiece, BT.QUESTION_TEXT)):
        for have in ((), group.keys[:1], group.keys[1:], group.keys):
            bd = {k: w[k] for k in have}
            assert module.has_text(bd) is BT.has_text(group, bd) is bool(have)
        assert module.check({k: w[k] for k in group.keys}) is True and module.check({"pad_obj_mask": 1}) is False


def test_one_copy_of_each_shared_expression_and_a_pure_module():
    sources = {os.path.basename(p): open(p).read() for p in sorted(glob.glob(os.path.join(ROOT, "sam-textvqa_amd", "*.py")))}
    count = lambda pattern: {name: len(re.findall(pattern, src)) for name, src in sources.items() if re.search(pattern, src)}
    assert count(r"detach\(\)\.cpu\(\)\.numpy\(\) if torch\.is_tensor") == {"batchtext.py": 1}
    assert count(r"pin_memory\(\) for k, v in") == {"batchtext.py": 1}
    forwards = {name: re.findall(r"def has_text\(.*\):\n +return (.*)\n", src) for name, src in sources.items() if "def has_text" in src and name != "batchtext.py"}
    assert forwards == {"phoc.py": ["BT.has_text(BT.OCR_TEXT_PHOC, batch_dict)"], "fasttext.py": ["BT.has_text(BT.OCR_TEXT_FASTTEXT, batch_dict)"],
                        "wordpiece.py": ["BT.has_text(BT.QUESTION_TEXT, batch_dict)"]}
    assert not re.search(r"^\s*(from|import)\s+(?!numpy|torch)\S+", sources["batchtext.py"], flags=re.M)          # pure: numpy and torch only

"""GPU: the three device probes of the word index (csrc/text.h: index_lookup in answer_text.hip and wordpiece.hip, index_lookup_wave in fasttext.hip) on
an index whose probe chain runs over the end of the table into slot 0, at the smallest shapes; every output equals the host twin element for element (the
twins' lookups are pinned to a Python dict by tests/test_wordindex_cpu.py).  The FastText index has T = 8 slots; the answer table's entry point wants
T >= 2 V and both vocabularies need their four special tokens, so those two wrap at their builders' own T = 16 for V = 8."""
import numpy as np
import pytest
import torch

from tests.test_wordindex_cpu import plain_hash, wrapping_words

pytestmark = pytest.mark.gpu


def placed_past_the_end(index, words, first_id):
    """the words of `words` (ids first_id ...) that sit in a slot below their home slot: reached only by walking over the last slot into slot 0"""
    slots = index["slots"].tolist()
    T = len(slots)
    assert all(plain_hash(w) & (T - 1) >= T - 2 for w in words) and slots[T - 1] >= 0 and slots[0] >= 0
    return [w for i, w in enumerate(words) if slots.index(first_id + i) < T - 2]


def test_answer_table_probe_over_the_end_of_the_table():
    from sam_textvqa_amd import answers as A
    from tests.test_answer_text_cpu import SPECIALS, pack
    from tests.test_answer_text_gpu import assert_equals_twin
    words = wrapping_words(16)
    voc = A.AnswerVocab(SPECIALS + list(words))
    index = A.vocab_index(voc)
    assert (index["V"], index["slots"].numel()) == (8, 16)
    far = placed_past_the_end(index, words, 4)
    assert len(far) >= 2
    caps = A.AnswerTableCaps(20, 3, 8, 16)
    for w in list(words) + [far[0] + "x", far[0][:-1]]:               # B = 1, A = 1, No = 1: the answer's two words and the token go through the probe
        bd = pack([[w + " " + far[-1]]], [[w]], No=1, Lw=8, La=16, A_=1)
        table, status = assert_equals_twin(bd, voc, caps, what=w)
        n_seq = (2 if w in words else 1) * (2 if w == far[-1] else 1)                              # per word: its vocabulary entry and / or the OCR slot
        assert int(status[0]) == 0 and int(table["meta"][0, 0]) == n_seq, w
        assert (voc.word2idx_dict[far[-1]] in table["grp_idx"][0].tolist()) and (voc.word2idx_dict.get(w, -1) in table["grp_idx"][0].tolist()) == (w in words)


def test_wordpiece_probe_over_the_end_of_the_table():
    from sam_textvqa_amd import answers as A, wordpiece as W
    from tests.test_wordpiece_gpu import assert_same, launch
    pieces = wrapping_words(16, 4, "q", 2)                            # two plain words, then two "##" pieces
    vocab = ["[PAD]", "[UNK]", "[CLS]", "[SEP]"] + list(pieces)
    index = W.vocab_index(vocab, max_piece=8)
    assert (index["V"], index["slots"].numel()) == (8, 16)
    far = placed_past_the_end(index, pieces, 4)
    assert any(w.startswith("##") for w in far), far
    index_gpu = A.index_to(index, "cuda")
    ids = {w: i for i, w in enumerate(vocab)}
    for plain in pieces[:2]:
        for cont in pieces[2:]:
            for q, row in ((plain + cont[2:], [2, ids[plain], ids[cont], 3]), (plain, [2, ids[plain], 3]), (plain + cont[2:] + "z", [2, 1, 3]), (cont[2:], [2, 1, 3])):
                packed = W.pack_question_text([q], max_chars=16)      # B = 1, T = 4
                want = W.encode_host(packed["question_text"], packed["question_text_len"], index, 4)
                assert want["question_indices"][0, :len(row)].tolist() == row and int(want["num_question_tokens"][0]) == len(row), q
                assert_same(launch(W, packed, index_gpu, 4), want, q)


def test_fasttext_probe_over_the_end_of_the_table():
    from sam_textvqa_amd import fasttext as FT, phoc as P
    words = wrapping_words(8)
    matrix = np.arange(1, 17, dtype=np.float32).reshape(4, 4)
    index = FT.model_index(FT.make_model(list(words), matrix, 0, 0, 0), max_word=8, n_slots=8)     # maxn = 0: a token's row is its word's own matrix row
    assert index["slots"].numel() == 8 and len(placed_past_the_end(index, words, 0)) >= 2
    index_gpu = FT.index_to(index, "cuda")
    for i, tok in enumerate(list(words) + [words[0] + "x", words[3][:-1]]):
        p = P.pack_ocr_text([[tok]], max_ocr_tokens=1, max_chars=8)   # B = 1, n_max = 1, dim = 4
        want = FT.vectors_host_text(p["ocr_text"], p["ocr_text_len"], index)
        assert np.array_equal(want[0, 0], matrix[i] if i < 4 else np.zeros(4, np.float32)), tok
        got = FT.fasttext_from_text(p["ocr_text"].cuda(), p["ocr_text_len"].cuda(), index_gpu)
        torch.cuda.synchronize()
        assert torch.equal(got.cpu().view(torch.int32), torch.from_numpy(want).view(torch.int32)), tok

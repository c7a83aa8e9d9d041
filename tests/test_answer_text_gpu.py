"""GPU: the M4C answer tables built on the MI355X from the answers' and the OCR tokens' text (csrc/answer_text.hip, sam_answer_table_from_text) -- every
tensor and the status bit for bit equal to answers.collate_answer_tables of answers.build_answer_table (through the host twin on the same packed text),
every output element written, nothing written outside, and the sampler drawing the same targets from the GPU-built table as from the host-built one."""
import pytest
import torch

from sam_textvqa_amd import answers as A
from tests.test_answer_text_cpu import (STATUS_CAPS, big_vocab, colliding_vocab, golden_batch, pack, special_batch, status_batch, text_samples, tiny_batch, twin)

pytestmark = pytest.mark.gpu

KEYS = A.TABLE_KEYS + ("status",)


def on_gpu(d):
    return {k: v.cuda() for k, v in d.items()}


def launch(bd, voc, caps=A.DEFAULT_CAPS, out=None, max_word=32):
    """(table, status) of the kernel for the packed CPU batch bd, unchecked"""
    index = A.index_to(A.vocab_index(voc, max_word=max_word), "cuda")
    return A.tables_from_text(on_gpu(bd), index, caps, out=out, check=False)


def assert_equals_twin(bd, voc, caps=A.DEFAULT_CAPS, what="", max_word=32):
    table, status = launch(bd, voc, caps, max_word=max_word)
    want, want_status = twin(bd, voc, caps)
    for k in A.TABLE_KEYS:
        assert table[k].dtype == want[k].dtype and tuple(table[k].shape) == tuple(want[k].shape), (what, k)
        assert torch.equal(table[k].cpu(), want[k]), (what, k)
    assert torch.equal(status.cpu(), want_status), (what, status.tolist(), want_status.tolist())
    assert torch.equal(table["dims"], want["dims"]) and not table["dims"].is_cuda
    return table, status


def test_golden_cases_as_one_batch():
    voc, answers, tokens, n_clean = golden_batch()
    table, status = assert_equals_twin(pack(answers, tokens), voc, what="golden")
    assert status[:n_clean].eq(0).all() and status[n_clean:].tolist() == [A.STATUS_UNK_TARGET, A.STATUS_PAD_SLOT]
    assert table["meta"][:n_clean, 0].sum() > 0 and not table["meta"][n_clean:].any()


def test_constructed_batch_hits_every_corner_of_the_host_rules():
    voc, names, answers, tokens = special_batch()
    table, status = assert_equals_twin(pack(answers, tokens), voc, what="special")
    assert not status.any()
    n = dict(zip(names, table["meta"][:, 0].tolist()))
    assert n["product_24_is_cut"] == 200 and n["product_exactly_20"] == 152 and n["sixty_four_words"] == 181 and n["no_ocr_tokens"] == 8


def test_smallest_shapes():
    voc, answers, tokens, shp, caps = tiny_batch()
    table, status = assert_equals_twin(pack(answers, tokens, **shp), voc, caps, what="tiny", max_word=5)
    assert not status.any() and int(table["meta"][0, 0]) > 0


def test_colliding_and_large_vocabularies():
    voc = colliding_vocab()
    words = voc.word_list[4:]
    answers = [[words[0], words[1] + " " + words[2], words[2], words[0][:-1], words[1] + "x", words[2].upper(), " ".join(words), words[1], "<unk>", "</s> " + words[0]]]
    assert_equals_twin(pack(answers, [[words[1], "zz", words[1], words[2].upper()]]), voc, what="colliding")
    voc, answers, tokens = text_samples(16, seed=11)
    table, status = assert_equals_twin(pack(answers, tokens), voc, what="5000 words")
    assert not status.any() and (table["meta"][:, 0] > 0).sum() >= 12
    # more distinct indices than the group table holds at G = 8: eighty vocabulary words in ten answers
    many = [[" ".join("w%d" % (8 * a + k) for k in range(8)) for a in range(10)], ["w1 w2"] * 10]
    table, status = assert_equals_twin(pack(many, [[], ["w2"]]), big_vocab(), A.AnswerTableCaps(200, 12, 8, 256), what="group table overflow")
    assert status.tolist() == [A.STATUS_GROUPS, 0]


def test_each_status_bit_between_clean_neighbours():
    voc, names, answers, tokens, expect = status_batch()
    bd = pack(answers, tokens)
    table, status = assert_equals_twin(bd, voc, STATUS_CAPS, what="status")
    assert torch.equal(status.cpu(), expect), dict(zip(names, status.tolist()))
    for b, st in enumerate(expect.tolist()):
        assert bool(table["meta"][b].any()) == (st == 0), names[b]
    index = A.index_to(A.vocab_index(voc), "cuda")
    with pytest.raises(ValueError, match="sample 1: more score-index groups than the capacity G = 6"):
        A.tables_from_text(on_gpu(bd), index, STATUS_CAPS)
    for first, word in ((3, "more target indices than the capacity E = 7"), (4, "a score index is an OCR slot holding <pad>"),
                        (6, r"<unk> \(index 3\) among the target indices")):
        sub = {k: v[first:first + 2] for k, v in bd.items()}
        with pytest.raises(ValueError, match="sample 0: " + word):
            A.tables_from_text(on_gpu(sub), index, STATUS_CAPS)
    clean = {k: v[[0, 2, 5]] for k, v in bd.items()}
    got = A.tables_from_text(on_gpu(clean), index, STATUS_CAPS)                                   # check=True on clean samples: the table alone
    assert isinstance(got, dict) and int(got["meta"][:, 0].min()) > 0


def test_every_element_is_written_twice_the_same_and_nothing_beside():
    voc, _, answers, tokens = special_batch()
    bd = pack(answers, tokens)
    fresh, fresh_status = launch(bd, voc)
    B, caps, guard = len(answers), A.DEFAULT_CAPS, 64
    shapes = {k: tuple(v.shape) for k, v in A.table_outputs(B, caps, "cpu").items()}
    dtypes = {k: v.dtype for k, v in A.table_outputs(1, caps, "cpu").items()}
    # every buffer sits in the middle of a byte arena filled with 0x7f: its own bytes must all be overwritten, the guard bytes on both sides must stay
    arenas, out = {}, {}
    for k in KEYS:
        nbytes = torch.empty(shapes[k], dtype=dtypes[k]).numel() * torch.empty((), dtype=dtypes[k]).element_size()
        arenas[k] = torch.full((guard + nbytes + guard,), 0x7f, dtype=torch.uint8, device="cuda")
        out[k] = arenas[k][guard:guard + nbytes].view(dtypes[k]).view(shapes[k])
    table, status = launch(bd, voc, out=out)
    for k in A.TABLE_KEYS:
        assert table[k].data_ptr() == out[k].data_ptr() and torch.equal(table[k], fresh[k]), k
    assert torch.equal(status, fresh_status)
    for k in KEYS:
        assert arenas[k][:guard].eq(0x7f).all() and arenas[k][-guard:].eq(0x7f).all(), k
    before = {k: arenas[k].clone() for k in KEYS}
    launch(bd, voc, out=out)
    for k in KEYS:
        assert torch.equal(arenas[k], before[k]), k                                           # two launches: identical bytes


# ---------------------------------------------------------------------------------------------- into the sampler
def test_the_sampler_draws_the_same_targets_from_the_gpu_built_table():
    """the table built on the GPU goes where the collated host table goes: ops.answer_sample (csrc/answers.hip) draws and writes bit-identical dense targets,
    previous indices, masks and choices from either, at two steps"""
    from sam_textvqa_amd import ops
    voc, answers, tokens = text_samples(8, num_vocab=200, n_ocr=50, seed=5)
    bd = pack(answers, tokens)
    table, status = launch(bd, voc)
    assert not status.any() and table["dims"].tolist() == [250, voc.BOS_IDX, voc.EOS_IDX, 12]
    host = on_gpu(A.collate_answer_tables([A.build_answer_table(a, t, voc) for a, t in zip(answers, tokens)]))
    W, bos = A.table_dims(table)
    for step in (0, 5):
        got = ops.answer_sample({k: table[k] for k in A.TABLE_KEYS}, W, bos, A.answer_key(7, 0), step=step)
        want = ops.answer_sample({k: host[k] for k in A.TABLE_KEYS}, W, bos, A.answer_key(7, 0), step=step)
        assert (got["answer_choice"] >= 0).any()
        for k in want:
            assert torch.equal(got[k], want[k]), (step, k)

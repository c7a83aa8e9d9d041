"""GPU: PHOC from the OCR tokens' text (csrc/phoc.hip) -- the kernel against the reference's own rows and the host twin, its
clamps and guard band, and bit-identity of everything downstream (encoder operand, whole model, captured training step, greedy decoding) between a batch that
carries the tokens' text and the same batch carrying the host-built PHOC."""
import functools
import random

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

SHAPES = (7, 20, 9, 3)                 # T, n_obj, n_ocr, n_dec: the small config of tests/test_ragged_gpu.py / tests/test_model_gpu.py
VOCAB = 300


def pack(P, words, Lw, per_sample=32):
    """words -> packed text of ceil(len / per_sample) samples of per_sample slots"""
    B = (len(words) + per_sample - 1) // per_sample
    return P.pack_ocr_text([words[b * per_sample: (b + 1) * per_sample] for b in range(B)], max_ocr_tokens=per_sample, max_chars=Lw)


def run(P, packed, counts=None, dtype=torch.float32):
    out = P.phoc_from_text(packed["ocr_text"].cuda(), packed["ocr_text_len"].cuda(), None if counts is None else counts.cuda(), dtype=dtype)
    torch.cuda.synchronize()
    return out


@pytest.mark.parametrize("Lw", [64, 32, 7, 1])
def test_golden_words_bit_for_bit(Lw):
    from sam_textvqa_amd import phoc as P
    from tests.test_phoc_cpu import golden
    words, rows, _, _ = golden()
    keep = [i for i, w in enumerate(words) if len(w) <= Lw]
    assert len(keep) == len(words) if Lw == 64 else 10 < len(keep) < len(words)
    packed = pack(P, [words[i] for i in keep], Lw)
    assert packed["ocr_text"].shape[0] > 1 or Lw == 1                                   # several launches' worth of blocks, 32 slots per sample
    got = run(P, packed).cpu().numpy().reshape(-1, 604)
    want = np.zeros_like(got)
    want[:len(keep)] = rows[keep]
    bad = [words[keep[i]] for i in range(len(keep)) if not np.array_equal(got[i], want[i])]
    assert got.dtype == np.float32 and not bad, bad[:10]
    assert not got[len(keep):].any()                                                    # the empty slots behind the last word
    bf = run(P, packed, dtype=torch.bfloat16)
    assert torch.equal(bf.float().cpu(), torch.from_numpy(want).view(bf.shape))


def test_text_len_is_clamped_not_trusted():
    from sam_textvqa_amd import phoc as P
    words = ["within", "thethe", "a1b2c3", "stop"]
    packed = P.pack_ocr_text([words], max_ocr_tokens=4, max_chars=6)
    packed["ocr_text"][0, 3, 4:] = torch.tensor([ord("x"), ord("y")])                   # columns past the token's own length
    packed["ocr_text_len"] = torch.tensor([[6 + 1, 1 << 30, -1, -(1 << 31)]], dtype=torch.int32)
    got = run(P, packed).cpu().numpy()[0]
    assert np.array_equal(got, P.phoc_host(["within", "thethe", "", ""]))
    assert np.array_equal(got, P.phoc_host_text(packed["ocr_text"], packed["ocr_text_len"])[0])
    packed["ocr_text_len"] = torch.tensor([[3, 6, 2, 99]], dtype=torch.int32)
    assert np.array_equal(run(P, packed).cpu().numpy()[0], P.phoc_host(["wit", "thethe", "a1", "stopxy"]))


def test_counts_are_clamped_and_padding_slots_are_zero():
    from sam_textvqa_amd import phoc as P
    No = 5
    tokens = [["the", "quick", "brown", "fox", "jumps"], ["over", "a", "lazy", "dog", "42"], ["x", "yy", "zzz", "within", "st"], ["ab", "cd", "ef", "gh", "ij"]]
    packed = P.pack_ocr_text(tokens, max_ocr_tokens=No, max_chars=8)
    counts = torch.tensor([0, No, No + 3, -1], dtype=torch.int32)
    got = run(P, packed, counts).cpu().numpy()
    host = np.stack([P.phoc_host(t) for t in tokens])
    assert host.reshape(20, 604).any(1).all()                                           # every slot's text is non-empty
    for b, c in enumerate((0, No, No, 0)):
        assert np.array_equal(got[b, :c], host[b, :c]) and not got[b, c:].any(), b
    got = run(P, packed, torch.tensor([2, 4, 1, 3], dtype=torch.int32)).cpu().numpy()
    for b, c in enumerate((2, 4, 1, 3)):
        assert np.array_equal(got[b, :c], host[b, :c]) and not got[b, c:].any(), b
    assert np.array_equal(run(P, packed).cpu().numpy(), host)                           # NULL counts: every slot at its text_len


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("normalize", [False, True])
def test_guard_band(dtype, normalize, monkeypatch):
    """ld_dst = 1000, col0 = 300: the columns outside [300, 904) keep the sentinel in every row, padding rows hold zeros inside; then an unaligned
    destination (col0 = 301, ld = 1001: the scalar stores) under the same conditions; each through the torch op and through the ctypes route of the wrapper"""
    from sam_textvqa_amd import ops, phoc as P
    tokens = [["the", "Stop", "within", "e-mail", "x" * 8], ["42"], ["", "a"]]
    packed = P.pack_ocr_text(tokens, max_ocr_tokens=5, max_chars=8)
    counts = torch.tensor([5, 1, 1], dtype=torch.int32)
    host = torch.from_numpy(P.phoc_host_text(packed["ocr_text"], packed["ocr_text_len"], counts)).view(15, 604)
    for ld, col0 in ((1000, 300), (1001, 301)):
        # expected: the host-built rows through the existing expansion (every slot valid, the zero rows included), whose scaling the kernel must reproduce
        ref = torch.zeros((15, ld), dtype=dtype, device="cuda")
        ops.ragged_expand(torch.full((3,), 5, dtype=torch.int32, device="cuda"), 5, [(host.cuda(), ref, col0, normalize, 0)])
        want = ref[:, col0: col0 + 604].cpu()
        assert torch.equal(want, host.to(dtype)) if not normalize else (want.float() - host / host.sum(1, keepdim=True).sqrt().clamp(min=1)).abs().max() < 4e-3
        for route in ("1", "0"):
            monkeypatch.setenv("SAM_COARSE_OPS", route)
            dst = torch.full((15, ld), -7.0, dtype=dtype, device="cuda")
            ops.phoc_from_text(packed["ocr_text"].cuda(), packed["ocr_text_len"].cuda(), counts.cuda(), dst, col0, normalize)
            torch.cuda.synchronize()
            out = dst.cpu()
            assert (out[:, :col0] == -7.0).all() and (out[:, col0 + 604:] == -7.0).all(), (ld, col0, route)
            assert torch.equal(out[:, col0: col0 + 604], want), (ld, col0, route)
            assert not out[[6, 7, 8, 9, 11, 12, 13, 14], col0: col0 + 604].any() and not out[10, col0: col0 + 604].any()      # padding rows, and the empty token
        monkeypatch.delenv("SAM_COARSE_OPS")


# ---------------------------------------------------------------------------------------------- batches: text against host PHOC
def random_tokens(rng, n):
    out = []
    for _ in range(n):
        w = "".join(rng.choice("etaoinshrdlu" * 3 + "abcdefghijklmnopqrstuvwxyz0123456789-' ") for _ in range(rng.randint(0, 12)))
        out.append(w.upper() if rng.random() < 0.2 else w)
    return out


def two_forms(bd, seed):
    """a padded synthetic batch -> (the batch with the host-built PHOC of random tokens, zero rows behind the valid ones; the same batch with the tokens'
    text instead; the tokens)"""
    from sam_textvqa_amd import phoc as P
    rng = random.Random(seed)
    n_ocr = bd["pad_ocr_mask"].shape[1]
    tokens = [random_tokens(rng, int(c)) for c in bd["pad_ocr_mask"].sum(1).tolist()]
    host = dict(bd)
    ph = torch.zeros(len(tokens), n_ocr, 604)
    for b, t in enumerate(tokens):
        if t:
            ph[b, :len(t)] = torch.from_numpy(P.phoc_host(t))
    host["ocr_phoc"] = ph.to(bd["pad_ocr_mask"].device)
    text = {k: v for k, v in bd.items() if k != "ocr_phoc"}
    text.update({k: v.to(bd["pad_ocr_mask"].device) for k, v in P.pack_ocr_text(tokens, max_ocr_tokens=n_ocr, max_chars=12).items()})
    return host, text, tokens


def small_batch(seed, n=3, device="cuda", shapes=SHAPES):
    from sam_textvqa_amd.synthetic import make_batch
    bd = make_batch(n, *shapes, vocab=VOCAB, context=3, device=device, seed=seed)
    bd["question_indices"] = (bd["question_indices"] % 499 + 1) * bd["question_mask"]
    return bd


def small_model(fc7=False, seed=0):
    """the small config with its dropouts ON (the two forms must draw the same masks: same seed)"""
    import sam_textvqa_amd.modules as M
    from sam_textvqa_amd.synthetic import mmt_config_dict, text_bert_config_dict
    T, n_obj, n_ocr, n_dec = SHAPES
    md = mmt_config_dict(3, ("n", "s"), n_dec=n_dec, T=T, n_obj=n_obj, n_ocr=n_ocr)
    if fc7:
        md.update(frcn_encoder_type="finetune_faster_rcnn_fpn_fc7")
    td = dict(text_bert_config_dict(), num_hidden_layers=1, vocab_size=500)
    torch.manual_seed(seed)
    return M.SAM4C(M.BertConfig.from_dict(md), M.BertConfig.from_dict(td), num_answers=VOCAB, bos_idx=1)


def bits(t):
    return t.contiguous().view(torch.int16 if t.element_size() == 2 else torch.int32)


@pytest.mark.parametrize("fc7", [False, True], ids=["fc7_features", "fc7_finetuned"])
@pytest.mark.parametrize("normalize", [True, False])
@pytest.mark.parametrize("rows", [torch.float16, torch.float32], ids=["fp16", "fp32"])
def test_ragged_ocr_operand_is_bit_identical_to_the_host_phoc_path(rows, normalize, fc7):
    """B = 3, max_ocr = 6, counts 0 / 6 / 3: the OCR encoder operand _expand_ragged builds from ocr_text against the one built from ocr_phoc_rows = phoc_host"""
    from sam_textvqa_amd import ragged as R
    bd = small_batch(31, shapes=(7, 20, 6, 3))
    bd["pad_ocr_mask"] = (torch.arange(6, device="cuda")[None, :] < torch.tensor([0, 6, 3], device="cuda")[:, None]).long()
    for k in ("pad_ocr_features", "ocr_fasttext", "pad_ocr_bboxes"):
        bd[k] = bd[k] * bd["pad_ocr_mask"][..., None]
    host, text, tokens = two_forms(bd, 5)
    assert [len(t) for t in tokens] == [0, 6, 3]
    model = small_model(fc7).cuda()
    model.normalize = normalize
    out = []
    for form in (host, text):
        rag = R.from_padded(form, feature_dtype=rows)
        assert ("ocr_phoc_rows" in rag) != ("ocr_text" in rag)
        model._expand_ragged(rag)
        torch.cuda.synchronize()
        out.append(rag["_sam_ocr_operand"])
    (fa, xa), (fb, xb) = out
    assert fa.dtype == torch.bfloat16 and fa.shape == fb.shape
    if fc7:                      # the fc7 block's columns are left to the encoder node: compare what the expansion wrote
        col = xa[2]
        assert col == xb[2] == 904 and torch.equal(bits(xa[1]), bits(xb[1]))
        fa, fb = fa[..., :col], fb[..., :col]
    assert torch.equal(bits(fa), bits(fb))
    assert fa[1, :, 300:904].float().abs().sum() > 0 and not fa[0, :, 300:904].any() and not fa[2, 3:, 300:904].any()


def test_padded_form_materialises_the_host_tensor():
    from sam_textvqa_amd.synthetic import clone_batch
    host, text, _ = two_forms(small_batch(32), 6)
    model = small_model().cuda().train()
    bd = clone_batch(text)
    model(bd)
    torch.cuda.synchronize()
    assert bd["ocr_phoc"].dtype == torch.float32 and torch.equal(bd["ocr_phoc"], host["ocr_phoc"]) and host["ocr_phoc"].any()
    again = dict(clone_batch(text), ocr_phoc=torch.ones_like(bd["ocr_phoc"]), _sam_phoc_from_text=True)
    model(again)                                                  # a dict that went through forward before: ocr_phoc is rebuilt from the text, not refused
    assert torch.equal(again["ocr_phoc"], host["ocr_phoc"])
    with pytest.raises(ValueError, match="ocr_phoc"):
        model(dict(clone_batch(text), ocr_phoc=host["ocr_phoc"]))


@pytest.mark.parametrize("form", ["padded", "ragged"])
def test_whole_model_loss_and_gradients_are_bit_identical(form):
    """one forward / backward with dropout on and the same seed: the loss (summed by torch in a fixed order) and every parameter gradient"""
    from sam_textvqa_amd import ragged as R
    from sam_textvqa_amd.autograd import dropout_clock
    from sam_textvqa_amd.params import prepare
    from sam_textvqa_amd.synthetic import clone_batch
    host, text, _ = two_forms(small_batch(33), 7)
    model = small_model().cuda().train()
    fp = prepare(model)
    runs = []
    for bd in (host, text):
        bd = clone_batch(R.from_padded(bd) if form == "ragged" else bd)
        dropout_clock.manual_seed(11)
        fp.zero_grad()
        scores = model(bd)["textvqa_scores"]
        loss = (torch.nn.functional.binary_cross_entropy_with_logits(scores.float(), bd["targets"], reduction="none") * bd["train_loss_mask"][..., None]).sum()
        loss.backward()
        torch.cuda.synchronize()
        runs.append((loss.detach().clone(), scores.detach().clone(), {n: p.grad.clone() for n, p in model.named_parameters() if p.grad is not None}))
    (la, sa, ga), (lb, sb, gb) = runs
    print("%s: loss host-PHOC %r, text %r" % (form, la.item(), lb.item()))
    assert torch.isfinite(la) and torch.equal(sa, sb) and torch.equal(la, lb)
    assert set(ga) == set(gb) and len(ga) > 20 and any(g.any() for g in ga.values())
    bad = [n for n in ga if not torch.equal(ga[n], gb[n])]
    assert not bad, bad


@functools.lru_cache(maxsize=None)
def table_batches():
    """three (host-PHOC, text) pairs of batches with different tokens and the collated answer table of tests/test_answers_gpu.py (c3 token layout, B = 4: the
    shapes its table model and table are built for; the table loss sums in a fixed order, so two runs can be compared bit for bit); built once, never written to"""
    from sam_textvqa_amd.synthetic import make_batch
    from tests.test_answers_gpu import batches
    _, table = batches()
    pairs = []
    for seed in (41, 42, 43):
        bd = make_batch(4, vocab=200, device="cuda", seed=seed)
        for k in ("targets", "train_prev_inds", "train_loss_mask"):
            del bd[k]
        pairs.append(two_forms(bd, seed)[:2])
    return tuple(pairs), table


@pytest.mark.parametrize("form", ["padded", "ragged"])
def test_captured_steps_on_text_equal_host_phoc_bit_for_bit(form):
    """Trainer(use_graph=True), four steps (warm-up, capture + replay, two replays of batches written into input_buffers()) on batches with different
    tokens: parameters and losses equal those of a second trainer with the same seed fed the host-built PHOC; the graph was replayed, not left for eager"""
    from sam_textvqa_amd import ragged as R
    from sam_textvqa_amd.synthetic import clone_batch
    from sam_textvqa_amd.trainer import Trainer
    from tests.test_answers_gpu import small_model as table_model
    pairs, table = table_batches()
    assert not torch.equal(pairs[0][1]["ocr_text"], pairs[1][1]["ocr_text"]) and not torch.equal(pairs[1][1]["ocr_text"], pairs[2][1]["ocr_text"])
    runs = {}
    for which, name in ((0, "host"), (1, "text")):
        batches = [dict(p[which], answer_table=table) for p in pairs]
        if form == "ragged":
            batches = [R.from_padded(b) for b in batches]                              # fp16 rows
        tr = Trainer(table_model(), seed=7, base_lr=1e-3, use_graph=True, answer_targets="table")
        losses = [tr.step(clone_batch(batches[0])).clone(), tr.step(clone_batch(batches[1])).clone()]
        graph = tr._graph
        assert graph is not None
        replays = []
        real = graph.replay
        tr._graph = type("Counting", (), {"replay": lambda self: (replays.append(1), real())[1]})()
        tr._capture = lambda *a, **k: pytest.fail("a second capture was attempted")
        tr._eager_step = lambda *a, **k: pytest.fail("a step fell back to eager")
        for b in (batches[2], batches[0]):
            bufs = tr.input_buffers()
            assert ("ocr_text" in bufs and "ocr_phoc" not in bufs and "ocr_phoc_rows" not in bufs) if name == "text" else "ocr_text" not in bufs
            for k, v in b.items():
                if torch.is_tensor(v):
                    bufs[k].copy_(v)
                else:
                    for kk, vv in v.items():
                        bufs[k][kk].copy_(vv)
            losses.append(tr.step(bufs).clone())
        assert len(replays) == 2
        tr._graph = graph
        del tr._eager_step
        tr.flush_update()
        torch.cuda.synchronize()
        runs[name] = (torch.stack(losses).cpu(), tr.flat.flat.clone())
        del tr
    (la, pa), (lb, pb) = runs["host"], runs["text"]
    print("%s captured losses: host-PHOC %r, text %r; parameters differ in %d places" % (form, la.tolist(), lb.tolist(), (pa != pb).sum().item()))
    assert torch.isfinite(la).all() and len(set(la.tolist())) == 4
    assert torch.equal(la, lb) and torch.equal(pa, pb)


@pytest.mark.parametrize("form", ["padded", "ragged"])
def test_greedy_decoding_returns_the_same_ids(form):
    from sam_textvqa_amd import ragged as R
    from sam_textvqa_amd.params import prepare
    from sam_textvqa_amd.synthetic import clone_batch
    host, text, _ = two_forms(small_batch(34, n=4), 8)
    model = small_model().cuda().eval()
    prepare(model)
    out = []
    with torch.no_grad():
        for bd in (host, text):
            bd = clone_batch(R.from_padded(bd) if form == "ragged" else bd)
            bd["train_prev_inds"] = torch.zeros_like(bd["train_prev_inds"])
            bd["train_prev_inds"][:, 0] = 1
            scores = model(bd)["textvqa_scores"]
            assert "ocr_phoc" in bd                                                   # the sessions read the reference schema
            out.append((scores.argmax(-1).clone(), scores.clone()))
    assert torch.equal(out[0][0], out[1][0]) and torch.equal(out[0][1], out[1][1])

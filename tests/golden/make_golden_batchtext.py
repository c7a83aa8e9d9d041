#!/usr/bin/env python3
"""Generate tests/golden/batch_text_rules.json: what the package's host-side text functions answered BEFORE sam_textvqa_amd/batchtext.py owned their
shared parts -- the project's own recorded behaviour, not the reference's.  Run it on the commit whose behaviour is to be pinned:

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_batchtext.py

record() is the one definition of the cases: main() writes what it returns, tests/test_batchtext_cpu.py calls it again and demands equality.  Contents:
  checks    per check function: the outcome for EVERY subset of the keys it looks at (outcome[mask], bit i of mask = keys[i] is in the batch) on
            well-formed small tensors, and for a list of malformed batches
  packers   per packer / vocab_index / vocab_text / collate_score_tables: the outcome for a fixed list of inputs at B = 3
  status    per *_status_message: every single bit, every pair of bits and a bit no table names, with the flagged sample first, last and absent
An outcome is {"ret": the value, tensors as nested lists} or {"err": [exception type, message]}."""
import itertools
import json
import os
import sys

sys.dont_write_bytecode = True

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

B, No, Lw, A, La, Lq = 2, 3, 4, 2, 5, 6
i32 = torch.int32


def plain(v):
    """a return value as JSON holds it"""
    if torch.is_tensor(v) or isinstance(v, np.ndarray):
        return v.tolist()
    if isinstance(v, dict):
        return {k: plain(x) for k, x in v.items()}
    if isinstance(v, (tuple, list)):
        return [plain(x) for x in v]
    if isinstance(v, (np.integer, np.floating)):
        return v.item()
    return v


def outcome(fn, *args, **kw):
    try:
        return {"ret": plain(fn(*args, **kw))}
    except Exception as e:                                      # (every refusal here is a ValueError; the type is recorded, not assumed)
        return {"err": [type(e).__name__, str(e)]}


def well_formed():
    """one small well-formed value per key any check function looks at"""
    return {"ocr_text": torch.zeros(B, No, Lw, dtype=i32), "ocr_text_len": torch.zeros(B, No, dtype=i32),
            "answer_text": torch.zeros(B, A, La, dtype=i32), "answer_text_len": torch.zeros(B, A, dtype=i32),
            "question_text": torch.zeros(B, Lq, dtype=i32), "question_text_len": torch.zeros(B, dtype=i32),
            "ocr_phoc": torch.zeros(B, No, 2), "ocr_phoc_rows": torch.zeros(B * No, 2), "ocr_fasttext": torch.zeros(B, No, 2), "ocr_ft_rows": torch.zeros(B * No, 2),
            "question_indices": torch.zeros(B, 3, dtype=torch.int64), "question_mask": torch.ones(B, 3, dtype=torch.int64),
            "answer_table": {}, "score_table": {}, "targets": torch.zeros(B, 2, 5),
            "ocr_raw": torch.zeros(4, dtype=torch.uint8), "ocr_raw_off": torch.zeros(B * No + 1, dtype=i32), "ocr_count": torch.ones(B, dtype=i32),
            "answer_raw": torch.zeros(4, dtype=torch.uint8), "answer_raw_off": torch.zeros(B * A + 1, dtype=i32),
            "question_raw": torch.zeros(4, dtype=torch.uint8), "question_raw_off": torch.zeros(B + 1, dtype=i32)}


def check_functions():
    """name -> (the function of a batch dict, the keys it looks at: its own pair, what excludes it, what it needs)"""
    from sam_textvqa_amd import answers, fasttext, metrics, phoc, textprep, wordpiece
    return {
        "phoc.check": (phoc.check, ("ocr_text", "ocr_text_len", "ocr_phoc", "ocr_phoc_rows")),
        "phoc.check[n_ocr]": (lambda bd: phoc.check(bd, No), ("ocr_text", "ocr_text_len", "ocr_phoc", "ocr_phoc_rows")),
        "fasttext.check": (fasttext.check, ("ocr_text", "ocr_text_len", "ocr_fasttext", "ocr_ft_rows")),
        "fasttext.check[n_ocr]": (lambda bd: fasttext.check(bd, No), ("ocr_text", "ocr_text_len", "ocr_fasttext", "ocr_ft_rows")),
        "fasttext.wants_fasttext": (fasttext.wants_fasttext, ("ocr_text", "ocr_text_len", "ocr_fasttext", "ocr_ft_rows")),
        "wordpiece.check": (wordpiece.check, ("question_text", "question_text_len", "question_indices", "question_mask")),
        "answers.check_answer_text": (answers.check_answer_text, ("answer_text", "answer_text_len", "answer_table", "targets", "ocr_text", "ocr_text_len")),
        "metrics.check_score_text": (metrics.check_score_text, ("answer_text", "answer_text_len", "ocr_text", "ocr_text_len", "score_table")),
        "textprep.check_raw": (textprep.check_raw, ("ocr_raw", "ocr_raw_off", "answer_raw", "answer_raw_off", "ocr_text", "ocr_text_len", "answer_text",
                                                    "answer_text_len", "ocr_count")),
        "textprep.check_question_raw": (lambda bd: textprep.check_question_raw(bd, object()),
                                        ("question_raw", "question_raw_off", "question_text", "question_text_len", "question_indices", "question_mask")),
        "textprep.check_question_raw[no table]": (lambda bd: textprep.check_question_raw(bd, None),
                                                  ("question_raw", "question_raw_off", "question_text", "question_text_len", "question_indices", "question_mask")),
        "textprep.has_raw": (textprep.has_raw, ("ocr_raw", "ocr_raw_off", "answer_raw", "answer_raw_off", "question_raw", "question_raw_off")),
        "phoc.has_text": (phoc.has_text, ("ocr_text", "ocr_text_len")),
        "fasttext.has_text": (fasttext.has_text, ("ocr_text", "ocr_text_len")),
        "wordpiece.has_text": (wordpiece.has_text, ("question_text", "question_text_len")),
    }


def malformed():
    """name of a check function -> [(case, batch)]: wrong rank, wrong dtype, a length tensor of another shape, width 0, width over the maximum and the
    n_ocr mismatch where the function has such a rule; for the functions without a shape rule the same tensors, to record that they pass"""
    w = well_formed()

    def packed(text, ln, rank3, limit):
        lead = (B, No) if rank3 else (B,)
        cases = [("rank", {text: torch.zeros(lead + (2, 2), dtype=i32)}), ("rank low", {text: torch.zeros(lead[:-1] + (4,), dtype=i32) if rank3 else torch.zeros(4, dtype=i32)}),
                 ("text dtype", {text: w[text].long()}), ("len dtype", {ln: w[ln].long()}), ("text float", {text: w[text].float()}),
                 ("len shape", {ln: torch.zeros(lead + (1,), dtype=i32)}), ("len longer", {ln: torch.zeros((B + 1,) + lead[1:], dtype=i32)}),
                 ("width 0", {text: torch.zeros(lead + (0,), dtype=i32)}), ("width max", {text: torch.zeros(lead + (limit,), dtype=i32)}),
                 ("width over", {text: torch.zeros(lead + (limit + 1,), dtype=i32)}),
                 ("two rules", {text: w[text].long(), ln: torch.zeros(lead + (1,), dtype=i32)})]
        return [(name, dict({text: w[text], ln: w[ln]}, **change)) for name, change in cases]

    ocr = packed("ocr_text", "ocr_text_len", True, 64)
    ocr_n = ocr + [("n_ocr mismatch", {"ocr_text": torch.zeros(B, No + 1, Lw, dtype=i32), "ocr_text_len": torch.zeros(B, No + 1, dtype=i32)})]
    ans = packed("answer_text", "answer_text_len", True, 128)
    with_ocr = lambda cases: [(n, dict(bd, ocr_text=w["ocr_text"], ocr_text_len=w["ocr_text_len"])) for n, bd in cases]
    both_wrong = [("shape and excluder", dict(ocr[0][1], ocr_phoc=w["ocr_phoc"], ocr_fasttext=w["ocr_fasttext"]))]
    return {"phoc.check": ocr + both_wrong, "phoc.check[n_ocr]": ocr_n + both_wrong, "fasttext.check": ocr + both_wrong, "fasttext.check[n_ocr]": ocr_n + both_wrong,
            "wordpiece.check": packed("question_text", "question_text_len", False, 1024),
            "answers.check_answer_text": with_ocr(ans) + [(n, dict(bd, answer_text=w["answer_text"], answer_text_len=w["answer_text_len"])) for n, bd in ocr],
            "metrics.check_score_text": with_ocr(ans) + [(n, dict(bd, answer_text=w["answer_text"], answer_text_len=w["answer_text_len"])) for n, bd in ocr],
            "textprep.check_raw": [("raw dtype", {"ocr_raw": w["ocr_raw"].long(), "ocr_raw_off": w["ocr_raw_off"].long(), "ocr_count": w["ocr_count"]}),
                                   ("raw rank", {"answer_raw": torch.zeros(2, 2, dtype=torch.uint8), "answer_raw_off": torch.zeros(2, 2, dtype=i32), "ocr_count": w["ocr_count"]})],
            "textprep.check_question_raw": [("raw dtype", {"question_raw": w["question_raw"].long(), "question_raw_off": w["question_raw_off"].long()})]}


def record_checks():
    w, bad = well_formed(), malformed()
    out = {}
    for name, (fn, keys) in check_functions().items():
        assert all(k in w for k in keys) and len(set(keys)) == len(keys), name
        subsets = [outcome(fn, {k: w[k] for i, k in enumerate(keys) if mask >> i & 1}) for mask in range(2 ** len(keys))]
        assert len(subsets) == 2 ** len(keys), name
        out[name] = {"keys": list(keys), "subsets": subsets, "malformed": [{"case": case, "out": outcome(fn, bd)} for case, bd in bad.get(name, [])]}
    return out


def packer_cases():
    """name -> (function, [(case, args, kwargs)]): one fixed list of inputs at B = 3 -- an empty string, non-ASCII strings, a string exactly at the
    capacity and one code point over it, too many tokens, the wrong number of answers, a question that is no str, one holding [SEP], an empty batch"""
    from sam_textvqa_amd import answers, metrics, phoc, wordpiece
    tokens = [["", "café", "abcd", "one too many"], ["Stop", "\U0001F600中"], []]
    ans = [["", "naïve"], ["abcde", "x"], ["Joe'S", "İ"]]
    questions = ["", "what is Ünder the (sign)‽", "what does it say?"]
    words = ["<pad>", "<s>", "</s>", "<unk>", "é", "abcd", "Joe'S", "İx"]
    pieces = ["[PAD]", "[UNK]", "[CLS]", "[SEP]", "[MASK]", "##ing", "é", "stop\n"]
    record = lambda a, t: metrics.build_score_table(a, t, num_answers=A, max_ocr_tokens=3)
    tabs = [record(a, t) for a, t in zip(ans, tokens)]
    caps = metrics.ScoreTableCaps
    return {
        "phoc.pack_ocr_text": (phoc.pack_ocr_text, [
            ("fits", (tokens,), dict(max_ocr_tokens=3, max_chars=4)), ("one over", (tokens,), dict(max_ocr_tokens=3, max_chars=3)),
            ("over in the last sample", ([[], ["ab"], ["a", "abcde"]],), dict(max_ocr_tokens=2, max_chars=4)), ("the cut token is not read", (tokens,), dict(max_ocr_tokens=3, max_chars=4)),
            ("no slots", (tokens,), dict(max_ocr_tokens=0, max_chars=4)), ("empty batch", ([],), {}), ("max_chars 0", (tokens,), dict(max_chars=0)),
            ("max_chars 64", ([["x" * 64]],), dict(max_ocr_tokens=1, max_chars=64)), ("max_chars 65", (tokens,), dict(max_chars=65)), ("defaults", (tokens[1:],), {})]),
        "answers.pack_answer_text": (answers.pack_answer_text, [
            ("fits", (ans,), dict(num_answers=2, max_chars=5)), ("one over", (ans,), dict(num_answers=2, max_chars=4)),
            ("too few answers", (ans[:2] + [["a"]],), dict(num_answers=2, max_chars=5)), ("too many answers", ([["a", "b", "c"]] + ans[1:],), dict(num_answers=2, max_chars=5)),
            ("count before length", ([["abcdef", "a"], ["a"]],), dict(num_answers=2, max_chars=5)), ("empty batch", ([],), {}), ("num_answers 0", (ans,), dict(num_answers=0)),
            ("max_chars 0", (ans,), dict(num_answers=2, max_chars=0)), ("max_chars 129", (ans,), dict(num_answers=2, max_chars=129)),
            ("defaults", ([["a%d" % i for i in range(10)]] * 3,), {})]),
        "wordpiece.pack_question_text": (wordpiece.pack_question_text, [
            ("fits", (questions,), dict(max_chars=25)), ("ascii at the capacity", (questions[::2],), dict(max_chars=17)), ("ascii one over", (questions[::2],), dict(max_chars=16)),
            ("one over after normalisation", (questions,), dict(max_chars=24)), ("not a str", (["a", None, "b"],), {}), ("bytes", ([b"a"],), {}),
            ("holds [SEP]", (["fine", "is [SEP] here", 3],), {}), ("holds [MASK]", (["a [MASK]"],), {}), ("special before length", (["[CLS]" * 9],), dict(max_chars=8)),
            ("empty batch", ([],), {}), ("max_chars 0", (questions,), dict(max_chars=0)), ("max_chars 1025", (questions,), dict(max_chars=1025)),
            ("cjk and controls", (["中文 a\x00b c\tD", "Ångström…", "plain"],), dict(max_chars=16))]),
        "answers.vocab_index": (answers.vocab_index, [
            ("fits", (words,), dict(max_word=5)), ("one over", (words,), dict(max_word=4)), ("over at a later word", (words + ["abcdefg"],), dict(max_word=6)),
            ("max_word 0", (words,), dict(max_word=0)), ("max_word 65", (words,), dict(max_word=65)), ("defaults", (words,), {})]),
        "wordpiece.vocab_index": (wordpiece.vocab_index, [
            ("fits", (pieces,), dict(max_piece=6)), ("one over", (pieces,), dict(max_piece=5)), ("listed twice", (pieces + ["stop"],), {}), ("no [SEP]", (pieces[:3] + pieces[4:],), {}),
            ("[PAD] not first", (pieces[1:] + pieces[:1],), {}), ("twice before over", (pieces + ["a-very-long-piece", "stop"],), dict(max_piece=6)),
            ("max_piece 0", (pieces,), dict(max_piece=0)), ("max_piece 65", (pieces,), dict(max_piece=65)), ("defaults", (pieces,), {})]),
        "metrics.vocab_text": (metrics.vocab_text, [
            ("fits", (words,), dict(max_word=5)), ("one over", (words,), dict(max_word=4)), ("lowering lengthens", (words + ["İİİ"],), dict(max_word=5)),
            ("defaults", (words,), {})]),
        "metrics.collate_score_tables": (metrics.collate_score_tables, [
            ("fits", (tabs, caps(2, 5, 6)), {}), ("normalised answer over Lg", (tabs, caps(2, 5, 5)), {}), ("answer over Lg", (tabs, caps(2, 5, 4)), {}), ("token over Lw", (tabs, caps(2, 3, 5)), {}), ("answers over A", (tabs, caps(1, 5, 5)), {}),
            ("slots differ", (tabs[:2] + [metrics.build_score_table(ans[2], [], num_answers=A, max_ocr_tokens=2)], caps(2, 5, 5)), {}),
            ("empty batch", ([], caps(2, 5, 5)), {}), ("Lg 0", (tabs, caps(2, 5, 0)), {}), ("Lg 256", (tabs, caps(2, 5, 256)), {}),
            ("no slots", ([metrics.build_score_table(a, [], num_answers=A, max_ocr_tokens=0) for a in ans], caps(2, 5, 6)), {})]),
    }


def record_packers():
    return {name: [{"case": case, "out": outcome(fn, *args, **kw)} for case, args, kw in cases] for name, (fn, cases) in packer_cases().items()}


def status_vectors(bits):
    """every single bit, every pair of bits, all of them, and a bit no table names (alone and in front of a named one): in the first and in the last of
    three samples, with another flagged sample behind it, and absent"""
    words = list(bits) + [a | b for a, b in itertools.combinations(bits, 2)] + [sum(bits), 1 << 10, 1 << 10 | bits[-1]]
    out = [[0, 0, 0], []]
    for w in words:
        out += [[w, 0, 0], [0, 0, w], [w, 0, bits[0]], [1 << 10, w, bits[-1]]]
    return out


def status_functions():
    from sam_textvqa_amd import answers, metrics, textprep, wordpiece
    return {"textprep.status_message": (lambda st: textprep.status_message(st, 7), [b for b, _ in textprep.STATUS_REASONS]),
            "textprep.status_message[what]": (lambda st: textprep.status_message(st, 64, what="ocr slot"), [b for b, _ in textprep.STATUS_REASONS]),
            "wordpiece.question_status_message": (lambda st: wordpiece.question_status_message(st, 9), [b for b, _ in wordpiece.QUESTION_STATUS_REASONS]),
            "answers.status_message": (lambda st: answers.status_message(st, {"UNK": 3}, (200, 12, 64, 256)), [b for b, _ in answers.STATUS_REASONS]),
            "metrics.score_status_message": (lambda st: metrics.score_status_message(st, (10, 32, 128)), [metrics.STATUS_LG, metrics.STATUS_PAD])}


def record_status():
    return {name: [{"status": st, "out": outcome(fn, st)} for st in status_vectors(bits)] for name, (fn, bits) in status_functions().items()}


def record():
    return json.loads(json.dumps({"checks": record_checks(), "packers": record_packers(), "status": record_status()}))


def main():
    data = record()
    path = os.path.join(HERE, "batch_text_rules.json")
    with open(path, "w") as f:
        json.dump(data, f, indent=0, ensure_ascii=True, separators=(",", ":"))
        f.write("\n")
    n = {k: sum(len(v["subsets"]) + len(v["malformed"]) if k == "checks" else len(v) for v in d.values()) for k, d in data.items()}
    print("batch_text_rules.json: %s outcomes, %.1f KB" % (n, os.path.getsize(path) / 1024))


if __name__ == "__main__":
    main()

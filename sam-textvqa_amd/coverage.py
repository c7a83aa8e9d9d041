"""Answer-space upper bounds: how much of each metric ANY decoder could reach on a batch when it may emit only answer-vocabulary
words (the papers' "vocab UB"), only the sample's OCR tokens ("OCR UB"), or both ("vocab + OCR UB") -- the numbers the M4C and SA-M4C papers report
for an OCR system, an answer vocabulary, max_ocr_num and the decoding length.

For every ground-truth answer and every SOURCE (0 = vocabulary, 1 = OCR tokens, 2 = both) one launch (csrc/coverage.hip, sam_answer_witness) writes the
id sequence a perfect decoder would emit -- a WITNESS -- or marks the answer unreachable.  The witnesses of a sample's A answers are then handed to the
evaluator's own scoring kernel as "beams" (metrics.evaluate_beams, K = A, skip = 0): its `oracle` output, the per-metric maximum over the beams, is
the bound, measured by the code that measures the model.  Nothing here touches the training step.

What the numbers are:
  * the VQA-accuracy bound is exact under this scorer: a string that equals no (normalised) ground-truth answer scores 0, so the best string is one of
    the answers;
  * the ST-VQA accuracy and ANLS figures are the bound over the GROUND-TRUTH ANSWERS only: a string that is no answer can still earn partial ANLS, so the
    true ANLS bound may be higher;
  * the text is the batch's cleaned, lowered text (answer_text / ocr_text, as everywhere else), matched exactly; OCR slots past a sample's token count are
    expected to be empty, as phoc.pack_ocr_text and textprep.materialize leave them (the score table reads such a slot as "<pad>");
  * an answer of more than L words is reachable but its witness is cut to L ids; what the prefix is worth is the scorer's decision;
  * a sample none of whose answers is reachable scores 0 by definition, never whatever an empty prediction happens to score.

witness_host / upper_bounds_host are the CPU twins: the first is written on answers.match_answer_to_vocab_ocr_seq (pinned to the reference) and the kernel
equals it bit for bit, padding included."""
import numpy as np
import torch

from . import answers as _answers
from . import metrics as M
from .batchtext import to_numpy as _np
from .layouts import WITNESS

KEYS = WITNESS.keys                             # words, reach, any, seqs, counts
SOURCES = ("vocab", "ocr", "both")              # the leading dimension of reach / any / seqs and of every bound
METRIC_KEYS = ("vqa_accuracy", "stvqa_accuracy", "anls")
COUNT_KEYS = ("words", "in_vocab", "in_ocr", "in_neither")          # the columns of counts
MAX_ANSWERS, MAX_STEPS, MAX_SLOTS = 64, 64, 64  # sam_eval_beams' K and L; one OCR slot per lane


def _check_shapes(at, ot, L):
    if at.ndim != 3 or ot.ndim != 3 or at.shape[0] != ot.shape[0]:
        raise ValueError("coverage: answer_text must be [B, A, La] and ocr_text [B, No, Lw]; got %s and %s" % (tuple(at.shape), tuple(ot.shape)))
    (B, A, La), (No, Lw) = at.shape, ot.shape[1:]
    if min(B, A, La, No, Lw) < 1 or int(L) < 1:
        raise ValueError("coverage: B, A, La, No, Lw and L must be at least 1 (B=%d A=%d La=%d No=%d Lw=%d L=%d)" % (B, A, La, No, Lw, int(L)))
    if A > MAX_ANSWERS or La > _answers.MAX_ANSWER_CHARS or No > MAX_SLOTS or Lw > _answers.MAX_WORD_CHARS or int(L) > MAX_STEPS:
        raise ValueError("coverage: A=%d La=%d No=%d Lw=%d L=%d over the limits %d, %d, %d, %d, %d" % (A, La, No, Lw, int(L), MAX_ANSWERS, _answers.MAX_ANSWER_CHARS,
                                                                                                        MAX_SLOTS, _answers.MAX_WORD_CHARS, MAX_STEPS))
    return B, A, La, No, Lw


def witness(batch, index, L=12, out=None):
    """the witnesses of a batch on the GPU, one launch: batch carries answer_text int32 [B, A, La] / answer_text_len [B, A] and ocr_text int32 [B, No, Lw] /
    ocr_text_len [B, No]; index: answers.vocab_index(...) with its tensors on the GPU; L: the decoding length.  -> dict of
      words  int32 [B, A]        the answer's word count
      reach  int32 [3, B, A]     1 when every word of the answer (at least one) matches the source
      any    int32 [3, B]        the OR of reach over the sample's answers
      seqs   int64 [3, B * A, L] seqs[s]: metrics.evaluate_beams input for beam = A, skip = 0: a reachable answer's first min(words, L) ids, then EOS; an
                                 unreachable answer's row copies the sample's first reachable one; all EOS where any == 0
      counts int32 [B, 4]        over all words of the sample's answers: how many, in the vocabulary, among the OCR tokens, in neither
    out: buffers of layouts.WITNESS (allocated when None; every element is written).  Nothing synchronises."""
    from . import ops
    return ops.answer_witness(batch["answer_text"], batch["answer_text_len"], batch["ocr_text"], batch["ocr_text_len"], index, L, out=out)


def vocab_dict(index):
    """{word: id} of a vocabulary index (answers.vocab_index): what witness_host matches against; build it once per run"""
    cp, ln = _np(index["cp"]), _np(index["len"])
    words = {"".join(map(chr, cp[i, :ln[i]])): i for i in range(cp.shape[0]) if 0 <= ln[i] <= cp.shape[1]}
    if len(words) != int(index["V"]):
        raise ValueError("coverage: the index holds %d distinct words for V = %d" % (len(words), int(index["V"])))
    return words


def witness_host(batch, index, L=12, vocab=None):
    """the CPU twin of witness, and its definition: per answer answers.match_answer_to_vocab_ocr_seq with the vocabulary alone, the OCR tokens alone
    (ids offset by V) and both; the witness is the first sequence it returns.  Lengths are clamped as the kernel clamps them; an empty slot is no
    token.  vocab: vocab_dict(index), built here when None.  -> dict of numpy arrays under KEYS."""
    at, al, ot, ol = (_np(batch[k]) for k in ("answer_text", "answer_text_len", "ocr_text", "ocr_text_len"))
    B, A, La, No, Lw = _check_shapes(at, ot, L)
    L, V, eos = int(L), int(index["V"]), int(index["EOS"])
    vocab = vocab_dict(index) if vocab is None else vocab
    al, ol = np.clip(al.reshape(B, A), 0, La), np.clip(ol.reshape(B, No), 0, Lw)
    out = WITNESS.zeros_host(B=B, A=A, L=L)
    out["seqs"][:] = eos
    seqs = out["seqs"].reshape(3, B, A, L)
    for b in range(B):
        ocr2inds = {}
        for i in range(No):
            if ol[b, i] > 0:
                ocr2inds.setdefault("".join(map(chr, ot[b, i, :ol[b, i]])), []).append(i)
        rows = [[None] * A for _ in SOURCES]
        for a in range(A):
            ans = "".join(map(chr, at[b, a, :al[b, a]]))
            ws = ans.split()
            out["words"][b, a] = len(ws)
            out["counts"][b] += (len(ws), sum(w in vocab for w in ws), sum(w in ocr2inds for w in ws), sum(w not in vocab and w not in ocr2inds for w in ws))
            from_ocr = _answers.match_answer_to_vocab_ocr_seq(ans, {}, ocr2inds)
            found = (_answers.match_answer_to_vocab_ocr_seq(ans, vocab, {}), [tuple(V + i for i in seq) for seq in from_ocr[:1]],
                     _answers.match_answer_to_vocab_ocr_seq(ans, vocab, ocr2inds))
            for s, got in enumerate(found):
                if got:
                    rows[s][a] = list(got[0])[:L]
                    out["reach"][s, b, a] = 1
        for s in range(3):
            first = next((r for r in rows[s] if r is not None), None)
            out["any"][s, b] = first is not None
            for a in range(A):
                r = rows[s][a] if rows[s][a] is not None else first
                if r is not None:
                    seqs[s, b, a, :len(r)] = r
    return out


# ---------------------------------------------------------------------------------------------------------- bounds
def _vt(vocab_text, device):
    return {"cp": vocab_text["cp"].to(device), "len": vocab_text["len"].to(device), "eos": int(vocab_text["eos"])}


def _results(batch, index, vt, caps, table, L):
    """(witness dict, [evaluate_beams' dict per source]) of a batch on the GPU; vt: vocab_text on the device"""
    from . import evaluator
    if table is None:
        table = evaluator._score_table(batch, caps)
    wit = witness(batch, index, L)
    B, A = wit["words"].shape
    zeros = torch.zeros(B * A, dtype=torch.float32, device=wit["seqs"].device)
    return wit, [M.evaluate_beams(wit["seqs"][s], zeros, table, vt, beam=A, skip=0) for s in range(3)]


def _masked(res, wit, s):
    return res["oracle"] * wit["any"][s].to(torch.float32).unsqueeze(1)


def upper_bounds(batch, index, vocab_text, caps=M.DEFAULT_SCORE_CAPS, table=None, L=12):
    """fp32 [3, B, 3] on the GPU, source x sample x (VQA accuracy, ST-VQA accuracy, ANLS): the best any decoder restricted to the source could score on
    each sample (the module docstring says in which sense).  The score table is `table` (a collated table, moved to the device when it is not there),
    else it is built on the device from the batch's text as evaluator.evaluate builds it, at the capacities `caps` (caps.A = A, caps.Lw = Lw; the batch
    then carries ocr_count or pad_ocr_mask; a batch that carries the text cannot also carry "score_table", so a shipped table comes in as table=);
    vocab_text: metrics.vocab_text(...) at max_word = Lw.  One witness launch, then metrics.evaluate_beams once per source, whose `oracle` is
    multiplied by any[s] on the device; nothing synchronises."""
    dev = batch["answer_text"].device
    wit, res = _results(batch, index, _vt(vocab_text, dev), caps, table, L)
    return torch.stack([_masked(res[s], wit, s) for s in range(3)])


def upper_bounds_host(batch, index, vocab_text, caps=M.DEFAULT_SCORE_CAPS, table=None, L=12, counts=None):
    """the CPU twin of upper_bounds on witness_host and metrics.evaluate_beams_host -> numpy fp32 [3, B, 3].  counts: the OCR tokens per sample for a
    table built from text (metrics.score_tables_from_text_host)."""
    if table is None:
        table = M.score_tables_from_text_host(batch, caps, counts)[0]
    wit = witness_host(batch, index, L)
    B, A = wit["words"].shape
    zeros = np.zeros(B * A, np.float32)
    out = np.zeros((3, B, 3), np.float32)
    for s in range(3):
        res = M.evaluate_beams_host(wit["seqs"][s], zeros, table, vocab_text, A, skip=0)
        out[s] = res["oracle"] * wit["any"][s].astype(np.float32)[:, None]
    return out


# ---------------------------------------------------------------------------------------------------------- a pass over a dataset
def _report(sums, reach, words, count, extra=None):
    """sums [3][3], reach [3], words [4] and the question count, as host numbers -> measure's dict"""
    count, total = int(count), int(words[0])
    out = {"count": count,
           "sources": {name: dict({k: (sums[s][m] / count if count else 0.0) for m, k in enumerate(METRIC_KEYS)}, reachable=int(reach[s]))
                       for s, name in enumerate(SOURCES)},
           "words": dict({k: int(w) for k, w in zip(COUNT_KEYS, words)},
                         **{k + "_share": (int(w) / total if total else 0.0) for k, w in zip(COUNT_KEYS[1:], words[1:])})}
    out.update(extra or {})
    return out


def measure(batches, index, vocab_text, boards=None, caps=M.DEFAULT_SCORE_CAPS, L=12, unicode=None):
    """one pass over `batches` (an iterable of batch dicts on the GPU that carry the text keys of `witness` and what upper_bounds builds the score table
    from; raw UTF-8 strings go through textprep.materialize first, as in evaluator.evaluate), one read-back at the end.  -> {"count": the questions,
    "sources": {"vocab" | "ocr" | "both": {"vqa_accuracy", "stvqa_accuracy", "anls": the mean bounds, "reachable": the questions with an answer reachable
    from the source}}, "words": {"words", "in_vocab", "in_ocr", "in_neither": summed over every answer of every question, and the three shares of "words"}}.
    boards=None: the sums accumulate in a resident float64 tensor; a slot with batch["valid"] == 0 is left out, every other slot counts.
    boards: three evalboard.Board of one shape (n questions, P = L * (Lw + 1)), one per source: every batch's result is collected by batch["sample_idx"]
    (and batch["valid"]), so wrap padding and a question met twice count once, as in evaluator.evaluate_indexed; "repeats" says how many slots came on
    top.  A board row holds evaluate_beams' row of the source with `oracle` masked by any[s]; its `scores` triple, which for witnesses (all cumulative
    scores equal) would only repeat answer 0's row, holds (any[s], the question's word count, its words matching the source -- for "both": matching
    neither) instead, so that one reduce per board gives every sum.  The boards are not reset here."""
    from . import textprep as T
    caps = M.ScoreTableCaps(*caps)
    if boards is not None and (len(boards) != 3 or len({(bd.n, bd.P) for bd in boards}) != 1):
        raise ValueError("measure: boards must be three evalboard.Board of one shape, one per source")
    vt = acc = None
    for batch in batches:
        if T.has_raw(batch):
            T.materialize(batch, ocr_chars=caps.Lw, check=False, unicode=unicode)
        if boards is not None and "sample_idx" not in batch:
            raise ValueError("measure: with boards a batch needs sample_idx, the question index of every slot")
        dev = batch["answer_text"].device
        if vt is None:
            vt = _vt(vocab_text, dev)
            acc = torch.zeros(17, dtype=torch.float64, device=dev)               # [4 s + m]: the three bound sums and the reachable count of source s; [12:16] words; [16] questions
        wit, res = _results(batch, index, vt, caps, None, L)
        cnt = wit["counts"].to(torch.float32)
        if boards is not None:
            for s, bd in enumerate(boards):
                scores = torch.stack([wit["any"][s].to(torch.float32), cnt[:, 0], cnt[:, s + 1]], 1)
                bd.collect(dict(res[s], oracle=_masked(res[s], wit, s), best_scores=scores), batch["sample_idx"], batch.get("valid"))
            continue
        w = torch.ones(cnt.shape[0], dtype=torch.float64, device=dev) if batch.get("valid") is None else batch["valid"].ne(0).to(torch.float64)
        for s in range(3):
            acc[4 * s:4 * s + 3] += (_masked(res[s], wit, s).double() * w[:, None]).sum(0)
            acc[4 * s + 3] += (wit["any"][s].double() * w).sum()
        acc[12:16] += (wit["counts"].double() * w[:, None]).sum(0)
        acc[16] += w.sum()
    if vt is None:
        raise ValueError("measure: no batches")
    if boards is None:
        a = acc.cpu().tolist()                                                      # the one read-back
        return _report([a[4 * s:4 * s + 3] for s in range(3)], [a[4 * s + 3] for s in range(3)], a[12:16], a[16])
    red = torch.cat([torch.cat([bd.reduce(), bd.t["status"].double()]) for bd in boards]).cpu().tolist()          # the one read-back
    red = [red[9 * s:9 * s + 9] for s in range(3)]
    for s, r in enumerate(red):
        if int(r[8]):
            from . import evalboard
            raise ValueError("measure: board %d (%s): status %d: %s" % (s, SOURCES[s], int(r[8]), evalboard.status_message(int(r[8]))))
    count = red[0][3]
    return _report([r[4:7] for r in red], [r[0] for r in red], [red[0][1], red[0][2], red[1][2], red[2][2]], count,
                   {"missing": boards[0].n - int(count), "repeats": int(red[0][7]) - int(count)})

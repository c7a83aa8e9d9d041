"""Beam-search evaluation: the reference's Evaluator.evaluate (evaluator.py:67-135) without pandas and without per-sample host work.

Per batch: SAM4C.forward(batch, use_beam_search=True) leaves complete_seqs [B * K, S] and topkscores [B * K, 1] on the device; metrics.evaluate_beams
scores every beam against the batch's score table, keeps per question the beam with the largest cumulative score, and writes its scores and its answer
string -- all on the device.  The score table is either shipped with the batch (batch["score_table"], metrics.collate_score_tables) or built on the device
from the batch's text (answer_text / answer_text_len with ocr_text / ocr_text_len: metrics.score_tables_from_text); a batch that carries the raw strings
as UTF-8 (ocr_raw / answer_raw: textprep.py) has them cleaned and packed on the device first (textprep.materialize).  The mean
accuracies accumulate in a resident float64 tensor; question ids and answer tensors are collected per batch and read back ONCE, after the last batch.

metrics.py lists the three deviations from the reference (lowered answer text, a flag instead of IndexError, "<pad>" slots yield "<pad>").

merge="string" (this project's own, not the reference's) makes the answer string the unit of choice: metrics.evaluate_beams_merged adds up
the probabilities of the beams that spell the same answer and keeps the string with the largest sum.  The default, merge=None, is the path above."""
import json

import torch

from . import metrics as M
from . import textprep as T


def _score_table(batch, caps):
    if M.check_score_text(batch):                  # text next to a shipped table: ValueError
        table, _ = M.score_tables_from_text(batch, caps=caps, check=False)       # (a flagged sample has all-zero rows and scores 0; nothing synchronises)
        return table
    if "score_table" not in batch:
        raise ValueError("evaluate: a batch needs score_table, or answer_text / answer_text_len with ocr_text / ocr_text_len to build it from")
    return batch["score_table"]


def _evaluate_beams(merge, who):
    """merge=None: metrics.evaluate_beams, the beam with the largest cumulative score; "string": metrics.evaluate_beams_merged, the string with the largest
    summed probability"""
    if merge is None:
        return M.evaluate_beams
    if merge == "string":
        return M.evaluate_beams_merged
    raise ValueError('%s: merge = %r (None: the best beam, "string": beams that spell the same answer merged)' % (who, merge))


def evaluate(model, batches, vocab_text, beam_size, totals=None, caps=M.DEFAULT_SCORE_CAPS, skip=1, unicode=None, merge=None):
    """run beam search of width beam_size over `batches` (an iterable of batch_dicts on the GPU) and evaluate its output.  -> {"vqa_accuracy",
    "stvqa_accuracy", "anls": the means of the chosen beams' scores; "count": the questions; "oracle": [three means of the per-metric maximum over a
    question's beams]; "answers": [{"question_id", "answer"}] in batch order}.  totals: a metrics.new_totals() accumulator to add to (a fresh one when None;
    the means are taken over everything it holds).  caps: the capacities of tables built from text.  unicode: a Unicode table on the GPU
    (unicode_table.py) for textprep.materialize: raw strings are lowered, and raw questions normalised, on the device.  The model is put in eval mode
    for the run and back into its mode afterwards.
    merge="string": the answer string is the unit of choice (metrics.evaluate_beams_merged): per question the string with the largest summed probability
    over the beams that spell it, reported through its beam with the largest cumulative score.  The result gains "changed", the number of questions whose
    chosen beam is not the beam with the largest cumulative score, and "groups", the mean number of distinct strings per question; both are summed on the
    device and come with the same read-back."""
    eval_beams = _evaluate_beams(merge, "evaluate")
    model.set_beam_size(beam_size)
    was_training = model.training
    model.eval()
    vt, qids, answers, lens, oracles = None, [], [], [], []
    try:
        with torch.no_grad():
            for batch in batches:
                if T.has_raw(batch):               # raw strings: cleaned and packed on the device (a flagged slot is empty; nothing synchronises)
                    T.materialize(batch, ocr_chars=M.ScoreTableCaps(*caps).Lw, check=False, unicode=unicode)
                table = _score_table(batch, caps)
                model(batch, use_beam_search=True)
                seqs, cum = batch["complete_seqs"], batch["topkscores"]
                if vt is None:
                    vt = {"cp": vocab_text["cp"].to(seqs.device), "len": vocab_text["len"].to(seqs.device), "eos": int(vocab_text["eos"])}
                    totals = M.new_totals(seqs.device) if totals is None else totals
                    oracle_sum = torch.zeros(3, dtype=torch.float64, device=seqs.device)
                    merged_sum = torch.zeros(2, dtype=torch.int64, device=seqs.device) if merge else None      # (changed questions, groups)
                res = eval_beams(seqs.reshape(cum.numel(), -1), cum, table, vt, beam_size, skip=skip, totals=totals)
                B = res["best"].numel()
                oracle_sum += res["oracle"].double().sum(0)
                if merge:
                    merged_sum += torch.stack(((res["best"] != res["plain_best"]).sum(), res["n_groups"].sum()))
                if "question_id" in batch:
                    q = batch["question_id"].reshape(-1)
                    qids.append(q[::beam_size] if q.numel() == B * beam_size else q)          # (the search repeats question_id once per beam)
                else:
                    qids.append(torch.arange(B, device=seqs.device) + sum(a.shape[0] for a in answers))
                answers.append(res["answer"])
                lens.append(res["answer_len"])
    finally:
        model.train(was_training)
    if vt is None:
        raise ValueError("evaluate: no batches")
    # the one read-back
    tot, osum = totals.cpu().tolist(), oracle_sum.cpu().tolist()
    msum = merged_sum.cpu().tolist() if merge else None
    qid = torch.cat(qids).cpu().tolist()
    text = [s for a, n in zip(answers, lens) for s in M.answer_strings(a, n)]
    n = tot[3]
    result = {"vqa_accuracy": tot[0] / n, "stvqa_accuracy": tot[1] / n, "anls": tot[2] / n, "count": int(n), "oracle": [o / len(qid) for o in osum],
              "answers": [{"question_id": q, "answer": s} for q, s in zip(qid, text)]}
    if merge:
        result.update(changed=msum[0], groups=msum[1] / len(qid))
    return result


def evaluate_indexed(model, batches, vocab_text, beam_size, board, caps=M.DEFAULT_SCORE_CAPS, skip=1, unicode=None, merge=None):
    """evaluate's loop over batches that carry "sample_idx" int32 [B] (question indices, as sampler.Sampler.next() draws them) and optionally "valid"
    int32 [B]: every batch's metrics.evaluate_beams result is collected into `board` (evalboard.Board) by question index, a slot
    with valid 0 is left out and a question met twice counts once.  No per-batch Python lists and no totals are kept; -> board.result(), the pass's
    one read-back.  The board is not reset here: a pass may go on from a loaded state.
    beam_size = 0 is the greedy route (the reference's evaluate_no_beam / run_model_no_beam, evaluator.py:52-66, 162-176): the model runs in eval mode
    without beam search, the prediction is batch["scores"].argmax(-1), and the same kernel scores it as one beam per question with no BOS column.
    merge="string": evaluate's: every batch goes through metrics.evaluate_beams_merged, whose result the board collects as it is.  With one beam per
    question (beam_size 0 or 1) there is nothing to merge and the board equals merge=None's."""
    eval_beams = _evaluate_beams(merge, "evaluate_indexed")
    beam_size = int(beam_size)
    if beam_size < 0:
        raise ValueError("evaluate_indexed: beam_size = %d (0: greedy decoding, K >= 1: beam search of width K)" % beam_size)
    if beam_size:
        model.set_beam_size(beam_size)
    was_training = model.training
    model.eval()
    vt, zeros = None, None
    try:
        with torch.no_grad():
            for batch in batches:
                if "sample_idx" not in batch:
                    raise ValueError("evaluate_indexed: a batch needs sample_idx, the question index of every slot")
                if T.has_raw(batch):
                    T.materialize(batch, ocr_chars=M.ScoreTableCaps(*caps).Lw, check=False, unicode=unicode)
                table = _score_table(batch, caps)
                if beam_size:
                    model(batch, use_beam_search=True)
                    seqs, cum = batch["complete_seqs"], batch["topkscores"]
                    seqs = seqs.reshape(cum.numel(), -1)
                else:
                    model(batch)
                    seqs = batch["scores"].argmax(-1)
                    if zeros is None or zeros.numel() != seqs.shape[0]:
                        zeros = torch.zeros(seqs.shape[0], dtype=torch.float32, device=seqs.device)
                    cum = zeros
                if vt is None:
                    vt = {"cp": vocab_text["cp"].to(seqs.device), "len": vocab_text["len"].to(seqs.device), "eos": int(vocab_text["eos"])}
                res = eval_beams(seqs, cum, table, vt, beam_size or 1, skip=skip if beam_size else 0)
                board.collect(res, batch["sample_idx"], batch.get("valid"))
    finally:
        model.train(was_training)
    if vt is None:
        raise ValueError("evaluate_indexed: no batches")
    return board.result()


def store_batches(store, sampler, into, steps=None, **gather_kw):
    """a generator over one epoch of this rank (steps=None: sampler.steps_per_epoch batches): per step one sampler.next() and one store.gather(store,
    sample_idx, into, **gather_kw), then `into` itself is yielded with "sample_idx" and "valid" (int32 [B], the sampler's own buffers of that step)
    attached.  `into` is reused: consume a batch before asking for the next.  Whatever else a model batch needs beyond what store.gather fills is the
    caller's to put into `into`, as it is for store.gather today."""
    from . import store as _store
    steps = sampler.steps_per_epoch if steps is None else int(steps)
    out = None
    for _ in range(steps):
        idx, valid = out = sampler.next(out=out)             # (allocated by the first step, rewritten by the later ones, like `into`)
        _store.gather(store, idx, into, **gather_kw)
        into["sample_idx"], into["valid"] = idx, valid
        yield into


def write_evalai(result, path):
    """dump evaluate()'s answer list as the reference writes its EvalAI / ST-VQA file (evaluator.py:122-133)"""
    with open(path, "w") as f:
        json.dump(result["answers"], f)

"""Beam-search evaluation: the reference's Evaluator.evaluate (evaluator.py:67-135) without pandas and without per-sample host work.

Per batch: SAM4C.forward(batch, use_beam_search=True) leaves complete_seqs [B * K, S] and topkscores [B * K, 1] on the device; metrics.evaluate_beams
scores every beam against the batch's score table, keeps per question the beam with the largest cumulative score, and writes its scores and its answer
string -- all on the device.  The score table is either shipped with the batch (batch["score_table"], metrics.collate_score_tables) or built on the device
from the batch's text (answer_text / answer_text_len with ocr_text / ocr_text_len: metrics.score_tables_from_text); a batch that carries the raw strings
as UTF-8 (ocr_raw / answer_raw: textprep.py) has them cleaned and packed on the device first (textprep.materialize).  The mean
accuracies accumulate in a resident float64 tensor; question ids and answer tensors are collected per batch and read back ONCE, after the last batch.

metrics.py lists the three deviations from the reference (lowered answer text, a flag instead of IndexError, "<pad>" slots yield "<pad>")."""
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


def evaluate(model, batches, vocab_text, beam_size, totals=None, caps=M.DEFAULT_SCORE_CAPS, skip=1, unicode=None):
    """run beam search of width beam_size over `batches` (an iterable of batch_dicts on the GPU) and evaluate its output.  -> {"vqa_accuracy",
    "stvqa_accuracy", "anls": the means of the chosen beams' scores; "count": the questions; "oracle": [three means of the per-metric maximum over a
    question's beams]; "answers": [{"question_id", "answer"}] in batch order}.  totals: a metrics.new_totals() accumulator to add to (a fresh one when None;
    the means are taken over everything it holds).  caps: the capacities of tables built from text.  unicode: a Unicode table on the GPU
    (unicode_table.py) for textprep.materialize: raw strings are lowered, and raw questions normalised, on the device.  The model is put in eval mode
    for the run and back into its mode afterwards."""
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
                res = M.evaluate_beams(seqs.reshape(cum.numel(), -1), cum, table, vt, beam_size, skip=skip, totals=totals)
                B = res["best"].numel()
                oracle_sum += res["oracle"].double().sum(0)
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
    qid = torch.cat(qids).cpu().tolist()
    text = [s for a, n in zip(answers, lens) for s in M.answer_strings(a, n)]
    n = tot[3]
    return {"vqa_accuracy": tot[0] / n, "stvqa_accuracy": tot[1] / n, "anls": tot[2] / n, "count": int(n), "oracle": [o / len(qid) for o in osum],
            "answers": [{"question_id": q, "answer": s} for q, s in zip(qid, text)]}


def write_evalai(result, path):
    """dump evaluate()'s answer list as the reference writes its EvalAI / ST-VQA file (evaluator.py:122-133)"""
    with open(path, "w") as f:
        json.dump(result["answers"], f)

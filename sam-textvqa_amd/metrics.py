"""TextVQA / ST-VQA metrics from per-sample score tables.

The reference scores a batch on the host (sam/datasets/metrics.py): TextVQAAccuracy.calculate walks the predicted indices into words (:39-51), and
its evaluators put the prediction and the ten ground-truth answers through EvalAIAnswerProcessor (:265-302) for the VQA soft accuracy (:309-341) and
the ST-VQA accuracy (:348-357), or through editdistance for ANLS (:366-382).  As with the answer processor (answers.py) the work splits in two:

  * the ground-truth half -- the normalised answers, their leave-one-out soft scores, the lowered raw answers for ANLS and the text of every OCR
    slot -- has no randomness: build_score_table turns it into a record once per sample (cacheable), collate_score_tables packs a batch into
    fixed-capacity tensors (batch_dict["score_table"]), vocab_text holds the answer vocabulary's words once per run;
  * the per-step half -- assemble the predicted string from indices, normalise it, compare it, edit distances -- runs on the GPU
    (csrc/score.hip, ops.score_answers, score_predictions): fp32 [B, 3] = (VQA soft accuracy, ST-VQA accuracy, ANLS) per sample, flags, and a
    resident float64 accumulator of the batch sums.

Text is int32 Unicode code points, never bytes (editdistance.eval and Python's == both work on code points).  normalize_answer is this project's
restatement of EvalAIAnswerProcessor.__call__ and the CPU twin of the kernel's normaliser; assemble_prediction / score_answers_host are the host
twins of the kernel (the CPU semantics, and its checker).

Two deviations from the reference, both outside ASCII only:
  1. a digit (the period rule: a "." stays when a digit follows) is "0"-"9" only; Python's \\d also accepts other Unicode decimal digits;
  2. lowercasing happens per word on the host, when the tables are built (vocab_text, build_score_table), not on the joined string: the two differ
     only in Python's context rule for a final capital sigma across the "'s" glue.  (An "s" lowered from "S" right after an apostrophe carries the
     NO_GLUE bit until the glue pass has run, so that " 'S" stays unglued as it does in the reference, which glues before it lowers; a word whose
     lowering changes its length -- non-ASCII only -- carries no such bits.)
A third one concerns only tables built on the device from text (score_tables_from_text, csrc/score_text.hip):
  3. the kernel lowers ASCII "A"-"Z" only, where build_score_table uses str.lower(); code points >= 0x80 pass through unchanged.  The two agree on every
     string t with ascii_lower(t) == t.lower() (device_lowerable), in particular on everything Processors.word_cleaner returns, which is lowered already
     -- and so on every text textprep.materialize wrote, with or without a Unicode table (with one the device has applied str.lower()
     itself; str.lower() is idempotent, so the ASCII lowering here finds nothing left to do and no caveat remains for such text).
"""
from collections import namedtuple

import numpy as np
import torch

from . import answers as _answers
from . import batchtext as BT
from .answers import PAD_TOKEN, as_answer_vocab
from .batchtext import to_numpy as _np
from .layouts import EVAL_BEAMS, EVAL_MERGED, SCORE_TABLE, SCORE_TABLE_OUT
from .wordindex import WHITESPACE    # Python's str.isspace() / str.split() / str.strip() set (is_space of csrc/text.h lists the same code points)

_WS = frozenset(chr(c) for c in WHITESPACE)
# every occurrence of one of these is deleted when some occurrence touches a blank, else replaced by a blank ("," and "?" are gone before the rule runs)
PUNCTUATION = (";", "/", "[", "]", '"', "{", "}", "(", ")", "=", "+", "\\", "_", "-", ">", "<", "@", "`", ",", "?", "!")
_PUNCT = frozenset(PUNCTUATION)
MAX_PERIODS = 32                       # the reference passes re.UNICODE (= 32) as the substitution's count
NO_GLUE = 1 << 30                      # flag bit on an "s" that was a capital right after an apostrophe (see the module docstring)
NUMBER_WORDS = (("none", "0"), ("zero", "0"), ("one", "1"), ("two", "2"), ("three", "3"), ("four", "4"), ("five", "5"), ("six", "6"), ("seven", "7"),
                ("eight", "8"), ("nine", "9"), ("ten", "10"))
ARTICLES = ("a", "an", "the")
# whole-word replacements applied after the number words and the articles (keys with capitals, and the two that contain "'s", can never match)
CONTRACTIONS = tuple(tuple(p.split()) for p in """
aint ain't|arent aren't|cant can't|couldve could've|couldnt couldn't|couldn'tve couldn't've|couldnt've couldn't've|didnt didn't|doesnt doesn't|dont don't
hadnt hadn't|hadnt've hadn't've|hadn'tve hadn't've|hasnt hasn't|havent haven't|hed he'd|hed've he'd've|he'dve he'd've|hes he's|howd how'd|howll how'll
hows how's|Id've I'd've|I'dve I'd've|Im I'm|Ive I've|isnt isn't|itd it'd|itd've it'd've|it'dve it'd've|itll it'll|let's let's|maam ma'am|mightnt mightn't
mightnt've mightn't've|mightn'tve mightn't've|mightve might've|mustnt mustn't|mustve must've|neednt needn't|notve not've|oclock o'clock|oughtnt oughtn't
ow's'at 'ow's'at|'ows'at 'ow's'at|'ow'sat 'ow's'at|shant shan't|shed've she'd've|she'dve she'd've|she's she's|shouldve should've|shouldnt shouldn't
shouldnt've shouldn't've|shouldn'tve shouldn't've|somebody'd somebodyd|somebodyd've somebody'd've|somebody'dve somebody'd've|somebodyll somebody'll
somebodys somebody's|someoned someone'd|someoned've someone'd've|someone'dve someone'd've|someonell someone'll|someones someone's|somethingd something'd
somethingd've something'd've|something'dve something'd've|somethingll something'll|thats that's|thered there'd|thered've there'd've|there'dve there'd've
therere there're|theres there's|theyd they'd|theyd've they'd've|they'dve they'd've|theyll they'll|theyre they're|theyve they've|twas 'twas|wasnt wasn't
wed've we'd've|we'dve we'd've|weve we've|werent weren't|whatll what'll|whatre what're|whats what's|whatve what've|whens when's|whered where'd
wheres where's|whereve where've|whod who'd|whod've who'd've|who'dve who'd've|wholl who'll|whos who's|whove who've|whyll why'll|whyre why're|whys why's
wont won't|wouldve would've|wouldnt wouldn't|wouldnt've wouldn't've|wouldn'tve wouldn't've|yall y'all|yall'll y'all'll|y'allll y'all'll
yall'd've y'all'd've|y'alld've y'all'd've|y'all'dve y'all'd've|youd you'd|youd've you'd've|you'dve you'd've|youll you'll|youre you're|youve you've
""".replace("\n", "|").split("|") if p.strip())
# one lookup per word: number word -> digits, article -> "" (the word is dropped), contraction -> its spelling.  No key appears twice and no value is a
# key of a later stage, so one lookup equals the reference's three in a row.  csrc/score.hip lists the same pairs in constant memory.
WORD_MAP = tuple(NUMBER_WORDS) + tuple((a, "") for a in ARTICLES) + CONTRACTIONS
_WORD_MAP = dict(WORD_MAP)
assert len(CONTRACTIONS) == 120 and len(_WORD_MAP) == len(WORD_MAP) == 135

SCORE_TABLE_KEYS = SCORE_TABLE.keys
METRICS = ("textvqa", "stvqa_accuracy", "stvqa_anls")           # column of the [B, 3] scores each one reads


def _strip(s):
    i, j = 0, len(s)
    while i < j and s[i] in _WS:
        i += 1
    while j > i and s[j - 1] in _WS:
        j -= 1
    return s[i:j]


def _split(s):
    words, cur = [], []
    for c in s:
        if c in _WS:
            if cur:
                words.append("".join(cur))
                cur = []
        else:
            cur.append(c)
    if cur:
        words.append("".join(cur))
    return words


def _normalize_lowered(t):
    """the normaliser proper, on text that is lowered already: what the kernel runs on the assembled prediction"""
    t = t.replace(",", "").replace("?", "").replace("'s", " 's")
    t = _strip(t).replace("\n", " ").replace("\t", " ")
    drop = {p for p in _PUNCT if (p + " ") in t or (" " + p) in t}           # decided per character on the text before any replacement
    t = "".join(("" if c in drop else " ") if c in _PUNCT else c for c in t)
    out, dropped = [], 0
    for i, c in enumerate(t):
        if c == "." and dropped < MAX_PERIODS and not (i + 1 < len(t) and "0" <= t[i + 1] <= "9"):
            dropped += 1
            continue
        out.append(c)
    words = []
    for w in _split("".join(out)):
        w = _WORD_MAP.get(w, w)
        if w:
            words.append(w)
    return " ".join(words)


def normalize_answer(s):
    """EvalAIAnswerProcessor.__call__ (sam/datasets/metrics.py:265-302) restated: lower; delete every "," and "?"; "'s" -> " 's"; strip; newline and
    tab -> blank; every punctuation character is deleted when some occurrence of it touches a blank and becomes a blank otherwise; the first 32
    periods that no digit follows are deleted; split on whitespace; number words -> digits; a / an / the dropped; contractions spelled out; joined
    with blanks (possibly the empty string).  The ground truths go through this; the kernel runs the same rules on the prediction."""
    return _normalize_lowered(s.lower())


def soft_scores_normalized(answers):
    """{normalised answer: soft score}, the leave-one-out rule of _compute_answer_scores (metrics.py:309-330) on the normalised answers, in first-seen order"""
    norm = [normalize_answer(a) for a in answers]
    sc = _answers.soft_scores(norm)                                           # the same rule and the same floating-point sums in the same order
    return {a: sc[a] for a in dict.fromkeys(norm)}


def _lower_word(w):
    """code points of w.lower(), an "s" that was "'S" flagged NO_GLUE"""
    lw = w.lower()
    cp = BT.code_points(lw)
    if len(lw) == len(w):
        for i in range(1, len(w)):
            if w[i] == "S" and w[i - 1] == "'":
                cp[i] |= NO_GLUE
    return cp


def vocab_text(answer_vocab, max_word=32):
    """every word of the answer vocabulary, lowered, as code points: {"cp": int32 [V, max_word], "len": int32 [V], "eos": EOS index}.  Built once per
    run and kept on the device (score_predictions moves it when it is not there yet)."""
    voc = as_answer_vocab(answer_vocab)
    V, Lw = len(voc), int(max_word)
    cp, ln = BT.pack_rows((V, Lw), ((i, _lower_word(w)) for i, w in enumerate(voc.word_list)), Lw,
                         lambda i, c, n: "vocabulary word %d (%r): %d code points exceed the capacity Lw = %d" % (i, voc.word_list[i], n, Lw))
    return {"cp": torch.from_numpy(cp), "len": torch.from_numpy(ln), "eos": int(voc.EOS_IDX)}


def build_score_table(answers, context_tokens, *, num_answers=10, max_ocr_tokens=50):
    """the random-free half of the metrics for one sample: the cleaned answers and OCR tokens build_answer_table receives.  -> dict
      gt_norm   the unique normalize_answer(a) strings, in first-seen order     gt_score  fp32, each one's leave-one-out soft score
      gt_raw    the distinct a.lower().strip() strings (ANLS, metrics.py:367-368)
      ocr       per OCR slot its lowered text as code points (NO_GLUE bits kept); slots beyond the token list hold "<pad>", as the dataset pads them
                (textvqa_dataset.py:209; metrics.py:43 indexes the padded list)"""
    answers = list(answers)
    if len(answers) != num_answers:
        raise ValueError("expected %d answers, got %d" % (num_answers, len(answers)))
    sc = soft_scores_normalized(answers)
    tokens = list(context_tokens)[:max_ocr_tokens]
    tokens += [PAD_TOKEN] * (max_ocr_tokens - len(tokens))
    return {"gt_norm": list(sc), "gt_score": np.array(list(sc.values()), np.float32),
            "gt_raw": list(dict.fromkeys(_strip(a.lower()) for a in answers)), "ocr": [_lower_word(t) for t in tokens]}


class ScoreTableCaps(namedtuple("ScoreTableCaps", "A Lw Lg")):
    """fixed per-run capacities of a collated score table: A ground-truth strings per sample, Lw code points per word (vocabulary words and OCR tokens),
    Lg code points per ground-truth string (at most 255: the distance kernel holds a row of Lg + 1 cells in four registers per lane)"""
    __slots__ = ()


ScoreTableCaps.__new__.__defaults__ = (10, 32, 128)
DEFAULT_SCORE_CAPS = ScoreTableCaps()


def collate_score_tables(tables, caps=DEFAULT_SCORE_CAPS, pin_memory=False):
    """batch_dict["score_table"]: CPU tensors at the fixed capacities `caps`
      meta int32 [B, 4] (n_norm, n_raw, 0, 0), gt_norm / gt_raw int32 [B, A, Lg] with gt_norm_len / gt_raw_len int32 [B, A], gt_score fp32 [B, A],
      ocr int32 [B, No, Lw] with ocr_len int32 [B, No].
    Anything over a capacity raises ValueError naming the sample and the capacity: nothing is truncated.  A prediction of L steps then holds at most
    L * (Lw + 1) code points, which is what the kernel sizes its buffers from."""
    caps = ScoreTableCaps(*caps)
    A, Lw, Lg = caps
    B = len(tables)
    if B == 0:
        raise ValueError("collate_score_tables: empty batch")
    if not 1 <= Lg <= 255:
        raise ValueError("capacity Lg = %d must be in [1, 255]" % Lg)
    No = len(tables[0]["ocr"])
    out = SCORE_TABLE.zeros_host(B=B, A=A, Lg=Lg, No=max(No, 1), Lw=Lw)
    for b, t in enumerate(tables):
        if len(t["ocr"]) != No:
            raise ValueError("sample %d: %d OCR slots, sample 0 has %d" % (b, len(t["ocr"]), No))
        for what, strings, key in (("normalised answers", t["gt_norm"], "gt_norm"), ("raw answers", t["gt_raw"], "gt_raw")):
            if len(strings) > A:
                raise ValueError("sample %d: %d %s exceed the capacity A = %d" % (b, len(strings), what, A))
            BT.pack_rows((out[key][b], out[key + "_len"][b]), enumerate(strings), Lg,
                        lambda a, s, n: "sample %d: answer %r has %d code points, over the capacity Lg = %d" % (b, s, n, Lg))
        out["meta"][b, :2] = (len(t["gt_norm"]), len(t["gt_raw"]))
        out["gt_score"][b, :len(t["gt_norm"])] = t["gt_score"]
        BT.pack_rows((out["ocr"][b], out["ocr_len"][b]), enumerate(t["ocr"]), Lw,
                    lambda o, cp, n: "sample %d: OCR token %d has %d code points, over the capacity Lw = %d" % (b, o, n, Lw))
    return BT.pinned({k: torch.from_numpy(v) for k, v in out.items()}, pin_memory)


# ---------------------------------------------------------------------------------------------------------- host twins of the kernel
def assemble_prediction(row, ocr_cp, ocr_len, vocab_cp, vocab_len, eos):
    """the id walk of metrics.py:39-51 over the tables, for one sample -> (the lowered answer string, bad): an id below V that is EOS ends the answer, any
    other id below V appends that vocabulary word, an id at or above V appends OCR slot id - V; a negative id or one at or above V + No ends the walk
    with bad = True.  The words are joined with blanks and " 's" is glued back to "'s" over the whole string, as str.replace does."""
    V, No = len(vocab_len), len(ocr_len)
    cps, bad, first = [], False, True
    for i in row:
        i = int(i)
        if i < 0 or i >= V + No:
            bad = True
            break
        if i < V:
            if i == eos:
                break
            w = vocab_cp[i, :vocab_len[i]]
        else:
            w = ocr_cp[i - V, :ocr_len[i - V]]
        if not first:
            cps.append(32)
        first = False
        cps.extend(int(c) for c in w)
    out, n = [], len(cps)
    for k, c in enumerate(cps):
        if c == 32 and k + 2 < n and cps[k + 1] == 39 and cps[k + 2] == 115:      # (an "s" that carries NO_GLUE is not 115)
            continue
        out.append(c & ~NO_GLUE)
    return BT.text_of(out), bad


def levenshtein(a, b):
    """edit distance over code points (what editdistance.eval computes), two rows"""
    prev = list(range(len(b) + 1))
    for i, ca in enumerate(a, 1):
        cur = [i]
        for j, cb in enumerate(b, 1):
            cur.append(min(prev[j] + 1, cur[j - 1] + 1, prev[j - 1] + (ca != cb)))
        prev = cur
    return prev[-1]


def anls_pair(s1, s2):
    """get_anls (metrics.py:366-371) on lowered, stripped strings: fp32 1 - d / max(len) when 2 d <= max(len), else 0; None when both are empty (the
    reference divides by zero there)"""
    m = max(len(s1), len(s2))
    if m == 0:
        return None
    d = levenshtein(s1, s2)
    return np.float32(1) - np.float32(d) / np.float32(m) if 2 * d <= m else np.float32(0)


def score_answers_host(pred_ids, table, vocab_text, return_flags=False):
    """host twin of sam_score_answers: fp32 [B, 3] = (VQA soft accuracy, ST-VQA accuracy, ANLS) per sample from prediction ids [B, L], the collated
    score table and vocab_text's dict.  return_flags=False raises where the reference would: IndexError on an id outside [0, V + No), ValueError when
    the prediction and a ground truth are both empty (ANLS divides by zero).  return_flags=True mirrors the kernel instead: -> (scores, flags int32 [B]),
    bit 0 = an out-of-range id ended the walk, bit 1 = an empty prediction met an empty ground truth (ANLS 0)."""
    ids = _np(pred_ids)
    tab = {k: _np(table[k]) for k in SCORE_TABLE_KEYS}
    vcp, vln, eos = _np(vocab_text["cp"]), _np(vocab_text["len"]), int(vocab_text["eos"])
    B = ids.shape[0]
    scores, flags = np.zeros((B, 3), np.float32), np.zeros(B, np.int32)
    for b in range(B):
        s, bad = assemble_prediction(ids[b], tab["ocr"][b], tab["ocr_len"][b], vcp, vln, eos)
        if bad:
            if not return_flags:
                raise IndexError("score_answers_host: sample %d predicts an id outside [0, %d)" % (b, len(vln) + tab["ocr"].shape[1]))
            flags[b] |= 1
        n_norm, n_raw = int(tab["meta"][b, 0]), int(tab["meta"][b, 1])
        sp, best = _strip(s), np.float32(0)
        for a in range(n_raw):
            gt = BT.text_of(tab["gt_raw"][b, a, :tab["gt_raw_len"][b, a]])
            v = anls_pair(sp, gt)
            if v is None:
                if not return_flags:
                    raise ValueError("score_answers_host: sample %d: the prediction and ground truth %d are both empty (ANLS divides by zero)" % (b, a))
                flags[b] |= 2
                v = np.float32(0)
            best = max(best, v)
        norm = _normalize_lowered(s)
        for a in range(n_norm):
            if norm == BT.text_of(tab["gt_norm"][b, a, :tab["gt_norm_len"][b, a]]):
                scores[b, 0], scores[b, 1] = tab["gt_score"][b, a], 1.0
                break
        scores[b, 2] = best
    return (scores, flags) if return_flags else scores


# ---------------------------------------------------------------------------------------------------------- the GPU path
def new_totals(device="cuda"):
    """a resident accumulator for score_predictions / ops.score_answers: float64 [4] = the three batch sums and the sample count"""
    return torch.zeros(4, dtype=torch.float64, device=device)


def score_predictions(pred_ids, batch_dict_or_table, vocab_text, totals=None, return_flags=False):
    """score predictions on the GPU (csrc/score.hip): pred_ids int [B, L] -- Trainer.predictions(), a DecodeSession's greedy output, or a beam's
    complete_seqs[:, 1:] (evaluator.py:333); batch_dict_or_table: a batch_dict with "score_table", or the collated table itself (moved to the device
    when it is not there); vocab_text: vocab_text(...)'s dict.  -> fp32 [B, 3] (VQA soft accuracy, ST-VQA accuracy, ANLS), un-synchronised; with
    return_flags also int32 [B].  totals (new_totals()): the batch sums and the count are added to it on the device, in a fixed order."""
    from . import ops
    table = batch_dict_or_table.get("score_table", batch_dict_or_table)
    dev = pred_ids.device if torch.is_tensor(pred_ids) and pred_ids.is_cuda else torch.device("cuda")
    pred = torch.as_tensor(pred_ids).to(device=dev, dtype=torch.int64).contiguous()
    tab = {k: table[k].to(dev, non_blocking=True) for k in SCORE_TABLE_KEYS}
    scores, flags = ops.score_answers(pred, tab, vocab_text["cp"].to(dev), vocab_text["len"].to(dev), int(vocab_text["eos"]), totals=totals)
    return (scores, flags) if return_flags else scores


# ---------------------------------------------------------------------------------------------------------- beam-search output
# The second half of the reference's Evaluator.evaluate (evaluator.py:67-135, evaluate_predictions :304-356): every beam scored, per question the beam with the
# largest cumulative score kept, its scores and its answer string.  Three deviations from the reference, and no others:
#   1. the answer text is the score table's and the vocabulary's, lowered per word; the reference writes the evaluation file's tokens as stored.  The two
#      agree wherever the tokens are lower case already, which Processors.word_cleaner guarantees;
#   2. an id at or above V + No sets flag bit 0 (the string holds what was assembled before it) where the reference raises IndexError;
#   3. an id that points at a "<pad>" slot yields the text "<pad>", as sam_score_answers does.
# `oracle` is the per-metric maximum over a question's beams -- the headroom the ranking by cumulative score leaves; the reference's variable of that name
# is in fact the chosen beam's score.
EVAL_BEAMS_KEYS = EVAL_BEAMS.keys


def argmax_first(v):
    """numpy.argmax's rule on a float vector, restated: the first k such that no element is greater, a NaN counting as greater than every number (the first
    NaN wins); +inf, -inf and -0.0 == 0.0 follow IEEE comparison.  What the select kernel computes across the lanes."""
    best = 0
    for k in range(len(v)):
        if v[k] != v[k]:
            return k
        if v[k] > v[best]:
            best = k
    return best


def evaluate_beams_host(complete_seqs, topkscores, batch_dict_or_table, vocab_text, beam, skip=1, totals=None):
    """host twin of sam_eval_beams, on assemble_prediction, score_answers_host(return_flags=True) and _strip: -> dict of numpy arrays under EVAL_BEAMS_KEYS
    (beam_scores fp32 [B * K, 3], beam_flags int32 [B * K], best int32 [B], best_ids int64 [B, L], best_scores fp32 [B, 3], best_flags int32 [B], oracle
    fp32 [B, 3], answer int32 [B, L * (Lw + 1)], answer_len int32 [B]).  totals: a float64 [4] numpy array, added to in the kernel's order (per thread of
    256 in ascending sample order, then the block's tree)."""
    table = batch_dict_or_table.get("score_table", batch_dict_or_table)
    tab = {k: _np(table[k]) for k in SCORE_TABLE_KEYS}
    seqs, cum = _np(complete_seqs).astype(np.int64), _np(topkscores).astype(np.float32).reshape(-1)
    K, skip = int(beam), int(skip)
    B = tab["meta"].shape[0]
    if seqs.ndim != 2 or K < 1 or seqs.shape[0] != B * K or cum.size != B * K or not 0 <= skip < seqs.shape[1]:
        raise ValueError("evaluate_beams_host: complete_seqs %s / topkscores %d for B = %d samples of K = %d beams, skip = %d" % (seqs.shape, cum.size, B, K, skip))
    ids = seqs[:, skip:]
    L, Lw = ids.shape[1], tab["ocr"].shape[2]
    rep = {k: np.repeat(v, K, axis=0) for k, v in tab.items()}
    beam_scores, beam_flags = score_answers_host(ids, rep, vocab_text, return_flags=True)
    vcp, vln, eos = _np(vocab_text["cp"]), _np(vocab_text["len"]), int(vocab_text["eos"])
    out = dict(EVAL_BEAMS.zeros_host(B=B, K=K, L=L, Lw=Lw), beam_scores=beam_scores, beam_flags=beam_flags)     # (the two scored arrays, in their slots)
    for b in range(B):
        k = argmax_first(cum[b * K:(b + 1) * K])
        r = b * K + k
        out["best"][b], out["best_ids"][b], out["best_scores"][b], out["best_flags"][b] = k, ids[r], beam_scores[r], beam_flags[r]
        m = beam_scores[b * K].copy()
        for j in range(1, K):
            m = np.fmax(m, beam_scores[b * K + j])
        out["oracle"][b] = m
        s = _strip(assemble_prediction(ids[r], tab["ocr"][b], tab["ocr_len"][b], vcp, vln, eos)[0])
        BT.pack_rows((out["answer"], out["answer_len"]), [(b, s)])
    if totals is not None:
        totals += host_totals(out["best_scores"])
    return out


def host_totals(scores):
    """float64 [4]: the column sums of fp32 [B, 3] scores and B, added in score_totals_kernel's order: thread t of 256 sums samples t, t + 256, ... in
    ascending order, then a halving tree over the threads"""
    sc = np.asarray(scores, np.float32).astype(np.float64)
    red = np.zeros((256, 3))
    for b in range(sc.shape[0]):
        red[b % 256] += sc[b]
    o = 128
    while o >= 1:
        red[:o] += red[o:2 * o]
        o >>= 1
    return np.concatenate([red[0], [float(sc.shape[0])]])


def aux_report(confusion, fired):
    """what the spatial aux heads' counts say (ops.aux_pair_stats / SAM4C.spatial_aux_stats), float64 on the host.  confusion
    [13, 13] = [true class, argmax-rule class], fired [13, 12] = [true class, channel with S > 0]; class 0 is "no relation", class r + 1 relation channel r.
    -> dict: pairs, accuracy (trace / pairs); precision, recall, f1, support: lists over the 12 relations (under the argmax rule; a 0 / 0 gives 0);
    macro_f1: the mean f1 of the relations with support (0 when none has); tp, fp, fn: lists over the 12 channels, each read as its own yes / no
    classifier (tp[r] = fired[r + 1, r])."""
    conf, fr = np.asarray(_np(confusion), np.float64), np.asarray(_np(fired), np.float64)
    if conf.shape != (13, 13) or fr.shape != (13, 12):
        raise ValueError("aux_report: confusion [13, 13] and fired [13, 12] expected, got %s and %s" % (conf.shape, fr.shape))

    def ratio(a, b):
        return np.divide(a, b, out=np.zeros_like(a), where=b != 0)

    pairs = conf.sum()
    support, predicted, hit = conf.sum(1)[1:], conf.sum(0)[1:], np.diag(conf)[1:]
    precision, recall = ratio(hit, predicted), ratio(hit, support)
    f1 = ratio(2 * precision * recall, precision + recall)
    tp = np.array([fr[r + 1, r] for r in range(12)])
    return {"pairs": float(pairs), "accuracy": float(np.trace(conf) / pairs) if pairs else 0.0,
            "precision": precision.tolist(), "recall": recall.tolist(), "f1": f1.tolist(), "support": support.tolist(),
            "macro_f1": float(f1[support > 0].mean()) if (support > 0).any() else 0.0,
            "tp": tp.tolist(), "fp": (fr.sum(0) - tp).tolist(), "fn": (support - tp).tolist()}


def evaluate_beams(complete_seqs, topkscores, batch_dict_or_table, vocab_text, beam, skip=1, totals=None, out=None):
    """beam-search output to per-question results on the GPU (csrc/eval_beams.hip, sam_eval_beams): complete_seqs int [B * K, S] and topkscores fp32 [B * K]
    or [B * K, 1] as SAM4C.forward(..., use_beam_search=True) leaves them in the batch; batch_dict_or_table: a batch_dict with "score_table", or the collated
    table of the B samples itself (moved to the device when it is not there; never repeated per beam); vocab_text: vocab_text(...)'s dict; beam = K.  The
    first `skip` columns are not scored (the BOS: evaluator.py:333).  -> dict of the EVAL_BEAMS_KEYS tensors (ops.eval_beams lists them), un-synchronised.
    totals (new_totals()): the chosen beams' score sums and the count are added to it on the device, in a fixed order.  answer_strings reads the text back."""
    from . import ops
    return _beams_on_device(ops.eval_beams, complete_seqs, topkscores, batch_dict_or_table, vocab_text, beam, skip, totals, out)


def _beams_on_device(op, complete_seqs, topkscores, batch_dict_or_table, vocab_text, beam, skip, totals, out):
    """evaluate_beams' and evaluate_beams_merged's operands moved to the device (where they are not there) and handed to ops.eval_beams / eval_beams_merged"""
    table = batch_dict_or_table.get("score_table", batch_dict_or_table)
    dev = complete_seqs.device if torch.is_tensor(complete_seqs) and complete_seqs.is_cuda else torch.device("cuda")
    seqs = torch.as_tensor(complete_seqs).to(device=dev, dtype=torch.int64).contiguous()
    cum = torch.as_tensor(topkscores).to(device=dev, dtype=torch.float32).reshape(-1).contiguous()
    tab = {k: table[k].to(dev, non_blocking=True) for k in SCORE_TABLE_KEYS}
    return op(seqs, cum, tab, vocab_text["cp"].to(dev), vocab_text["len"].to(dev), int(vocab_text["eos"]), int(beam), skip=int(skip), totals=totals, out=out)


def answer_strings(answer, answer_len):
    """evaluate_beams' answer int32 [B, P] / answer_len int32 [B] -> list[str]: the one read-back of the answer text"""
    return BT.strings(answer, answer_len)


# ---------------------------------------------------------------------------------------------------------- ... chosen by answer string
# This project's own definition; the reference has nothing like it.  Many id sequences spell one answer (a word that is in the vocabulary and among the OCR
# tokens, an OCR word detected twice, "joe" + "'s" and "joe's"), so the model's belief in an answer is the sum over the beams that spell it.  Per question:
# the beams are grouped by exact string (the stripped string evaluate_beams writes as `answer`; a beam with an out-of-range id stays alone), a group's mass
# is the log of its members' summed probabilities, the group with the largest mass wins (argmax_first over the leaders, the groups' lowest beams) and its
# member with the largest cumulative score (argmax_first over the members) is reported through evaluate_beams' nine fields.
EVAL_MERGED_KEYS = EVAL_MERGED.keys


def group_mass(cum):
    """the mass of one group from its members' fp32 cumulative scores in beam order -> numpy.float32.  One member: that score itself (NaN and the infinities
    pass through).  Several: NaN when a member is NaN, -inf when every member is -inf, else m + log(sum of exp(cum[j] - m)) with m the largest member, in
    float64 over ascending j and rounded once to fp32 (a +inf member makes inf - inf: NaN, as in the kernel).  The kernel does the same in fp32."""
    c = np.asarray(cum, np.float32).reshape(-1)
    if c.size == 1:
        return c[0]
    if np.isnan(c).any():
        return np.float32(np.nan)
    d = c.astype(np.float64)
    m = max(d.tolist())
    if m == -np.inf:
        return np.float32(-np.inf)
    with np.errstate(invalid="ignore", over="ignore"):
        s = np.float64(0)
        for v in d:
            s = s + np.exp(v - m)
        return np.float32(m + np.log(s))


def evaluate_beams_merged_host(complete_seqs, topkscores, batch_dict_or_table, vocab_text, beam, skip=1, totals=None):
    """host twin of sam_eval_beams_merged, on evaluate_beams_host (and so on score_answers_host), assemble_prediction, _strip and argmax_first: -> dict of
    numpy arrays under EVAL_MERGED_KEYS.  beam_scores, beam_flags and oracle are evaluate_beams_host's and its `best` is plain_best here; the masses come
    from group_mass (float64, rounded to fp32).  Bad shapes raise evaluate_beams_host's ValueError.  totals: as in evaluate_beams_host."""
    plain = evaluate_beams_host(complete_seqs, topkscores, batch_dict_or_table, vocab_text, beam, skip=skip)
    table = batch_dict_or_table.get("score_table", batch_dict_or_table)
    ocr, ocr_len = _np(table["ocr"]), _np(table["ocr_len"])
    ids, cum = _np(complete_seqs).astype(np.int64)[:, int(skip):], _np(topkscores).astype(np.float32).reshape(-1)
    vcp, vln, eos = _np(vocab_text["cp"]), _np(vocab_text["len"]), int(vocab_text["eos"])
    K, B = int(beam), ocr.shape[0]
    out = dict(EVAL_MERGED.zeros_host(B=B, K=K, L=ids.shape[1], Lw=ocr.shape[2]), beam_scores=plain["beam_scores"], beam_flags=plain["beam_flags"],
               oracle=plain["oracle"], plain_best=plain["best"])
    for b in range(B):
        rows = range(b * K, (b + 1) * K)
        text = [_strip(assemble_prediction(ids[r], ocr[b], ocr_len[b], vcp, vln, eos)[0]) for r in rows]
        BT.pack_rows((out["beam_answer"], out["beam_answer_len"]), zip(rows, text))
        alone = [bool(out["beam_flags"][r] & 1) for r in rows]
        group = [next((j for j in range(k) if not alone[k] and not alone[j] and text[j] == text[k]), k) for k in range(K)]
        leaders = [k for k in range(K) if group[k] == k]
        mass = {g: group_mass([cum[b * K + k] for k in range(K) if group[k] == g]) for g in leaders}
        win = leaders[argmax_first([mass[g] for g in leaders])]
        members = [k for k in range(K) if group[k] == win]
        k = members[argmax_first([cum[b * K + j] for j in members])]
        r = b * K + k
        out["group"][b * K:(b + 1) * K], out["mass"][b * K:(b + 1) * K], out["n_groups"][b] = group, [mass[g] for g in group], len(leaders)
        out["best"][b], out["best_ids"][b], out["best_scores"][b], out["best_flags"][b] = k, ids[r], out["beam_scores"][r], out["beam_flags"][r]
        out["answer"][b], out["answer_len"][b], out["best_mass"][b] = out["beam_answer"][r], out["beam_answer_len"][r], mass[win]
    if totals is not None:
        totals += host_totals(out["best_scores"])
    return out


def evaluate_beams_merged(complete_seqs, topkscores, batch_dict_or_table, vocab_text, beam, skip=1, totals=None, out=None):
    """evaluate_beams with the answer string as the unit of choice (csrc/beam_merge.hip, sam_eval_beams_merged): the same operands -> dict of the
    EVAL_MERGED_KEYS tensors (ops.eval_beams_merged lists them), un-synchronised: evaluate_beams' nine fields for the representative of the string with the
    largest summed probability, then every beam's string (answer_strings reads beam_answer / beam_answer_len as it stands: the n-best list), group, mass,
    n_groups, plain_best (evaluate_beams' best) and best_mass.  evalboard.Board.collect takes the result as it is."""
    from . import ops
    return _beams_on_device(ops.eval_beams_merged, complete_seqs, topkscores, batch_dict_or_table, vocab_text, beam, skip, totals, out)


# ---------------------------------------------------------------------------------------------------------- score tables from text
# build_score_table + collate_score_tables as one launch per batch (csrc/score_text.hip, sam_score_table_from_text): the batch carries the
# cleaned answers and the OCR tokens as code points (answers.pack_answer_text, phoc.pack_ocr_text -- the tensors answers.tables_from_text and the PHOC and
# FastText kernels read), and nothing about the ground truths is computed, cached or shipped by the host.
SCORE_TEXT_KEYS = ("answer_text", "answer_text_len", "ocr_text", "ocr_text_len")
STATUS_LG = 1                          # a normalised or a raw answer exceeds Lg code points
STATUS_PAD = 2                         # "<pad>" does not fit an OCR slot (Lw < 5)
SCORE_STATUS_REASONS = ((STATUS_LG, "an answer has more code points than the capacity Lg = %(Lg)d"),
                        (STATUS_PAD, "the OCR token '<pad>' has 5 code points, over the capacity Lw = %(Lw)d"))
_ASCII_LOWER = {c: c + 32 for c in range(ord("A"), ord("Z") + 1)}


def device_lowerable(s):
    """whether the device's lowering (ASCII "A"-"Z" only) gives s.lower(): the strings on which score_tables_from_text equals build_score_table"""
    return s.translate(_ASCII_LOWER) == s.lower()


def ocr_counts(tokens_per_sample, max_ocr_tokens=50):
    """int32 [B]: how many OCR slots of every sample hold a token (a token may be the empty string, so the packed lengths cannot tell)"""
    return torch.tensor([min(len(t), int(max_ocr_tokens)) for t in tokens_per_sample], dtype=torch.int32)


def check_score_text(batch_dict):
    """a batch asks for its score table to be built from text with answer_text / answer_text_len next to ocr_text / ocr_text_len; -> whether it does.
    The combinations that cannot be served raise ValueError: a text tensor without its lengths, answers without OCR text, text next to a score table."""
    return BT.check(BT.ANSWER_TEXT_SCORE, batch_dict)


def _lower_slot(w):
    """_lower_word on a slot's code points as the device lowers them: ASCII "A"-"Z" only, an "s" that was "'S" flagged NO_GLUE"""
    cp = np.where((w >= 65) & (w <= 90), w + 32, w)
    cp[1:] |= np.where((w[1:] == ord("S")) & (w[:-1] == ord("'")), NO_GLUE, 0).astype(cp.dtype)
    return cp


def _score_counts(batch_dict, counts, B):
    """the OCR tokens per sample: `counts`, else batch_dict["ocr_count"] (ragged batch), else the row sums of pad_ocr_mask"""
    if counts is None:
        counts = batch_dict.get("ocr_count")
    if counts is None and "pad_ocr_mask" in batch_dict:
        counts = batch_dict["pad_ocr_mask"].ne(0).sum(1)
    if counts is None:
        raise ValueError("score tables from text need the OCR tokens per sample: counts=, batch_dict['ocr_count'] or batch_dict['pad_ocr_mask']")
    counts = torch.as_tensor(counts)
    if counts.numel() != B:
        raise ValueError("%d OCR counts for a batch of %d" % (counts.numel(), B))
    return counts.reshape(B)


def score_table_outputs(B, No, caps, device):
    """fresh output buffers of score_tables_from_text at the capacities `caps`: the eight SCORE_TABLE_KEYS tensors and "status" int32 [B]"""
    A, Lw, Lg = ScoreTableCaps(*caps)
    return SCORE_TABLE_OUT.empty(device, B=B, A=A, Lg=Lg, No=max(int(No), 1), Lw=Lw)


def _check_score_shapes(at, ot, caps):
    A, Lw, Lg = caps
    if at.dim() != 3 or ot.dim() != 3 or at.shape[0] != ot.shape[0]:
        raise ValueError("answer_text must be [B, A, La] and ocr_text [B, No, Lw]; got %s and %s" % (tuple(at.shape), tuple(ot.shape)))
    if at.shape[1] != A or ot.shape[2] != Lw:
        raise ValueError("answer_text %s / ocr_text %s do not fit the capacities A = %d, Lw = %d" % (tuple(at.shape), tuple(ot.shape), A, Lw))
    if not 1 <= Lg <= 255:
        raise ValueError("capacity Lg = %d must be in [1, 255]" % Lg)


def score_status_message(status, caps):
    """the first flagged sample of a status vector (host list) in collate_score_tables' words, or None"""
    caps = ScoreTableCaps(*caps)
    hit = BT.first_flagged(status, SCORE_STATUS_REASONS, Lg=caps.Lg, Lw=caps.Lw)
    return hit and "sample %d: %s" % (hit[0], hit[2])


def score_tables_from_text_host(batch_dict, caps=DEFAULT_SCORE_CAPS, counts=None):
    """host twin of sam_score_table_from_text on the packed tensors, in numpy: the kernel's clamps (lengths into [0, La] / [0, Lw], counts into [0, No]),
    its ASCII-only lowering and its status rule.  -> (table, status): the eight CPU tensors of collate_score_tables, and int32 [B] with one bit and an
    all-zero row where collate_score_tables raises for a sample."""
    caps = ScoreTableCaps(*caps)
    A, Lw, Lg = caps
    _check_score_shapes(batch_dict["answer_text"], batch_dict["ocr_text"], caps)
    (at, al), (ot, ol) = BT.unpack(batch_dict["answer_text"], batch_dict["answer_text_len"]), BT.unpack(batch_dict["ocr_text"], batch_dict["ocr_text_len"])
    B, No = at.shape[0], ot.shape[1]
    cnt = np.clip(_np(_score_counts(batch_dict, counts, B)).astype(np.int64), 0, No)
    out = SCORE_TABLE.zeros_host(B=B, A=A, Lg=Lg, No=max(No, 1), Lw=Lw)
    status = np.zeros(B, np.int32)
    upper = (at >= 65) & (at <= 90)
    low = np.where(upper, at + 32, at)
    for b in range(B):
        lowered = BT.strings(low[b], al[b])
        norm = [_normalize_lowered(t) for t in lowered]
        sc = _answers.soft_scores(norm)
        gt_norm = list(dict.fromkeys(norm))
        gt_raw = list(dict.fromkeys(_strip(t) for t in lowered))
        if any(len(t) > Lg for t in gt_norm + gt_raw):
            status[b] = STATUS_LG
            continue
        if Lw < len(PAD_TOKEN) and cnt[b] < No:
            status[b] = STATUS_PAD
            continue
        out["meta"][b, :2] = (len(gt_norm), len(gt_raw))
        for key, strings in (("gt_norm", gt_norm), ("gt_raw", gt_raw)):
            BT.pack_rows((out[key][b], out[key + "_len"][b]), enumerate(strings))
        out["gt_score"][b, :len(gt_norm)] = np.array([sc[t] for t in gt_norm], np.float32)
        BT.pack_rows((out["ocr"][b], out["ocr_len"][b]), ((o, _lower_slot(ot[b, o, :ol[b, o]]) if o < cnt[b] else PAD_TOKEN) for o in range(No)))
    return {k: torch.from_numpy(v) for k, v in out.items()}, torch.from_numpy(status)


def score_tables_from_text(batch_dict, caps=DEFAULT_SCORE_CAPS, counts=None, out=None, check=True):
    """batch_dict["score_table"] of a batch that carries answer_text / answer_text_len and ocr_text / ocr_text_len on the GPU, one launch
    (csrc/score_text.hip): bit for bit collate_score_tables of build_score_table of every sample, for text that device_lowerable accepts (the module
    docstring's third deviation).  counts: the OCR tokens per sample, int32 [B]; None: batch_dict["ocr_count"] (ragged batch), else the row sums of
    pad_ocr_mask, else ValueError.  out: buffers from score_table_outputs (allocated here when None; every element is written).  check=True reads
    status back and raises ValueError naming the first flagged sample and the capacity; check=False never synchronises and returns (table, status): a
    flagged sample's rows are all zero.  The result goes into batch_dict["score_table"] in front of Trainer.step or score_predictions."""
    from . import ops
    caps = ScoreTableCaps(*caps)
    at, ot = batch_dict["answer_text"], batch_dict["ocr_text"]
    _check_score_shapes(at, ot, caps)
    B, No = at.shape[0], ot.shape[1]
    cnt = _score_counts(batch_dict, counts, B).to(device=at.device, dtype=torch.int32).contiguous()
    if out is None:
        out = score_table_outputs(B, No, caps, at.device)
    ops.score_table_from_text(at, batch_dict["answer_text_len"], ot, batch_dict["ocr_text_len"], cnt, out)
    table = {k: out[k] for k in SCORE_TABLE_KEYS}
    if not check:
        return table, out["status"]
    msg = score_status_message(out["status"].tolist(), caps)
    if msg is not None:
        raise ValueError(msg)
    return table


# ---------------------------------------------------------------------------------------------------------- synthetic samples
_RICH = ("coca-cola", "st.", "1.5", "x.5", "it's", "dont", "three", "the", "a", "u.s.a.", "(stop)", "a/b", "hed've", "no.", "7", "'s", "joe's", "!", "- go",
         "über", "σας", "e\tf", "ten", "an", " nb", "q?", "1,000", "3.", "'stop", "..", "w@x", "none")


def _synthetic_samples(batch_size, num_vocab, n_ocr, seed, rich):
    """the samples of make_score_tables as text: (AnswerVocab, [ten answers per sample], [OCR tokens per sample])"""
    rng = np.random.RandomState(seed)
    extra = list(_RICH) if rich else []
    words = [_answers.PAD_TOKEN, _answers.BOS_TOKEN, _answers.EOS_TOKEN, _answers.UNK_TOKEN] + extra + ["w%d" % i for i in range(num_vocab - 4 - len(extra))]
    voc = _answers.AnswerVocab(words)
    nw = num_vocab - 4 - len(extra)
    all_ans, all_tokens = [], []
    for _ in range(batch_size):
        n_tok = rng.randint(1, n_ocr + 1)
        pool = ["w%d" % i for i in rng.randint(0, nw, 8)] + ["oov%d" % i for i in rng.randint(0, 40, 8)]
        if rich:
            pool += [extra[i] for i in rng.randint(0, len(extra), 8)]
        tokens = [pool[i] for i in rng.randint(0, len(pool), n_tok)]
        cands = []
        for _ in range(4):
            src = tokens if rng.rand() < 0.6 else ["w%d" % i for i in rng.randint(0, nw, 3)]
            cands.append(" ".join(src[i] for i in rng.randint(0, len(src), rng.randint(1, 4))))
        cands.append("unmatched%d" % rng.randint(1000))
        all_ans.append([cands[i] for i in rng.choice(len(cands), 10, p=[0.4, 0.25, 0.15, 0.1, 0.1])])
        all_tokens.append(tokens)
    return voc, all_ans, all_tokens


def make_score_tables(batch_size, num_vocab=5000, n_ocr=50, seed=0, max_copy_steps=12, rich=False):
    """make_answer_tables' sibling: the same synthetic samples (same seed -> same vocabulary, tokens and answers), as answer tables AND score tables.
    rich=True: a third of the vocabulary-side words and of the OCR tokens come from a list that exercises the normaliser (punctuation next to blanks
    and not, periods before digits and not, "'s", number words, articles, contractions, tabs, non-ASCII text); the answers reuse them.
    -> (AnswerVocab, [build_answer_table records], [build_score_table records])"""
    voc, all_ans, all_tokens = _synthetic_samples(batch_size, num_vocab, n_ocr, seed, rich)
    a_tabs = [_answers.build_answer_table(ans, tokens, voc, max_ocr_tokens=n_ocr, max_copy_steps=max_copy_steps) for ans, tokens in zip(all_ans, all_tokens)]
    s_tabs = [build_score_table(ans, tokens, max_ocr_tokens=n_ocr) for ans, tokens in zip(all_ans, all_tokens)]
    return voc, a_tabs, s_tabs


def make_score_text(batch_size, num_vocab=5000, n_ocr=50, seed=0, rich=False):
    """the samples of make_score_tables (same arguments -> same samples) as the text a batch ships: -> (AnswerVocab, [the ten answers of every sample],
    [the OCR tokens of every sample]); answers.pack_answer_text / phoc.pack_ocr_text pack them, ocr_counts counts the tokens"""
    return _synthetic_samples(batch_size, num_vocab, n_ocr, seed, rich)

"""M4C answer targets from per-sample answer tables.

M4CAnswerProcessor.__call__ (sam/datasets/processors.py:586-692), run by TextVQADataset.__getitem__ for every drawn sample
(sam/datasets/textvqa_dataset.py:350-365), splits into two halves:

  * the string half -- soft scores, matching every answer word against the answer vocabulary and the OCR tokens, the index lists of
    get_all_indices -- has no randomness: build_answer_table turns it into a compact record, once per sample (cacheable; the reference's own
    comment at :627-628 says it was meant to be precomputed);
  * the per-step half -- np.random.choice of one decoding sequence, the dense fp32 targets [12, V + 50], train_prev_inds and both masks --
    runs on the GPU (csrc/answers.hip, ops.answer_sample) as the first node of the training step, writing straight into the step's buffers.

collate_answer_tables packs a batch of records into fixed-capacity tensors (batch_dict["answer_table"]); Trainer.step samples from them.
sample_answers_torch is the vectorised torch twin of the kernel (the CPU semantics), draw_choices the host twin of the kernel's draw.
"""
from collections import defaultdict, namedtuple

import numpy as np
import torch

from . import batchtext as BT
from .layouts import ANSWER_TABLE, ANSWER_TABLE_OUT
from .wordindex import WHITESPACE, build_slots, index_to, mix32 as _mix32, table_size, text_hash    # (re-exported: the names callers and tests use)
from .wordindex import lookup_host as vocab_lookup_host

UNK_TOKEN, PAD_TOKEN, BOS_TOKEN, EOS_TOKEN = "<unk>", "<pad>", "<s>", "</s>"
TABLE_KEYS = ANSWER_TABLE.keys
# why a sample has no table: the bits sam_answer_table_from_text sets in status[b] (csrc/answer_text.hip) where the host functions below raise
STATUS_GROUPS, STATUS_EXTRA, STATUS_PAD_SLOT, STATUS_UNK_TARGET = 1, 2, 4, 8


class AnswerTableError(ValueError):
    """the ValueError of build_answer_table / collate_answer_tables for a sample that has no valid table, with the kernel's status bit for the same condition"""

    def __init__(self, status, message):
        super().__init__(message)
        self.status = int(status)


class AnswerVocab:
    """the answer vocabulary as VocabDict builds it (sam/datasets/textvqa_vocab.py:28-53: <unk> is prepended when the word list lacks it), with the
    checks M4CAnswerProcessor makes of it (processors.py:520-536, 591) raised as ValueError.  Build it once and pass it to every build_answer_table call."""

    def __init__(self, words):
        words = list(getattr(words, "word_list", words))
        if UNK_TOKEN not in words:
            words = [UNK_TOKEN] + words
        self.word_list = words
        self.word2idx_dict = {w: i for i, w in enumerate(words)}
        if len(self.word2idx_dict) != len(words):
            raise ValueError("answer vocab lists a word more than once (%d words, %d distinct)" % (len(words), len(self.word2idx_dict)))
        self.UNK_IDX = self.word2idx_dict[UNK_TOKEN]
        self.PAD_IDX, self.BOS_IDX, self.EOS_IDX = (self.word2idx(w) for w in (PAD_TOKEN, BOS_TOKEN, EOS_TOKEN))
        for name, idx in (("<pad>", self.PAD_IDX), ("<s>", self.BOS_IDX), ("</s>", self.EOS_IDX)):
            if idx == self.UNK_IDX:
                raise ValueError("answer vocab has no %s" % name)
        if self.PAD_IDX != 0:
            raise ValueError("answer vocab must list <pad> first (index %d)" % self.PAD_IDX)

    def word2idx(self, w):
        return self.word2idx_dict.get(w, self.UNK_IDX)

    def __len__(self):
        return len(self.word_list)


def as_answer_vocab(v):
    return v if isinstance(v, AnswerVocab) else AnswerVocab(v)


def soft_scores(answers):
    """{answer: soft score} of processors.py:597-614 (leave-one-out min(1, matches / 3), averaged), the same floating-point sums in the same order"""
    counts = defaultdict(int)
    for a in answers:
        counts[a] += 1
    out = {}
    for ua in sorted(set(answers)):
        accs = [min(1, float(counts[ua] - (a == ua)) / 3) for a in answers]
        out[ua] = sum(accs) / len(accs)
    return out


def match_answer_to_vocab_ocr_seq(answer, vocab2idx_dict, ocr2inds_dict, max_match_num=20):
    """processors.py:541-576, verbatim semantics: vocab first, then every OCR slot (offset len(vocab)); no sequences as soon as one word does not
    match; at most max_match_num sequences, cut after every word"""
    num_vocab = len(vocab2idx_dict)
    answer_word_matches = []
    for word in answer.split():
        matched_inds = []
        if word in vocab2idx_dict:
            matched_inds.append(vocab2idx_dict.get(word))
        matched_inds.extend([num_vocab + idx for idx in ocr2inds_dict.get(word, ())])
        if len(matched_inds) == 0:
            return []
        answer_word_matches.append(matched_inds)
    if len(answer_word_matches) == 0:
        return []
    idx_seq_list = [()]
    for matched_inds in answer_word_matches:
        idx_seq_list = [seq + (idx,) for seq in idx_seq_list for idx in matched_inds]
        if len(idx_seq_list) > max_match_num:
            idx_seq_list = idx_seq_list[:max_match_num]
    return idx_seq_list


def build_answer_table(answers, context_tokens, answer_vocab, *, num_answers=10, max_ocr_tokens=50, max_copy_steps=12, max_match_num=20):
    """the random-free half of M4CAnswerProcessor.__call__ (processors.py:586-692) for one sample: cleaned answers and OCR tokens in, as the dataset passes
    them.  Returns a dict of small numpy arrays:
      seq_len   int32 [n]        length of every entry of all_idx_seq_list (duplicates of repeated answers kept: the draw is uniform over them), clamped to L
      seq_grp   int16 [n, L]     the group of each step's score index: seq[t] while t < len, EOS after (t = 0: the group of seq[0], read for prev[1])
      step0_idx / step0_val      the unique step-0 indices, each with the max soft score of the sequences starting there (fp32, :624-643)
      grp_idx   int32 [g]        the score index of each group;  grp_off int32 [g + 1] into grp_extra int32 [e]: get_all_indices of it (:693-707), for the
                                 groups a step t >= 1 scores (empty for indices that only ever start a sequence)
      dims      int32 [4]        (W = len(vocab) + max_ocr_tokens, BOS, EOS, L)
    Raises ValueError where the reference would fail its own assertions: len(answers) != num_answers, an OCR score index on a "<pad>" token, <unk> among
    the target indices of a step t >= 1 of any sequence (the reference asserts only for the one it draws; a table must be valid for every draw)."""
    voc = as_answer_vocab(answer_vocab)
    L = int(max_copy_steps)
    if L < 1:
        raise ValueError("max_copy_steps must be >= 1 (got %d)" % L)
    tokens = list(context_tokens)[:max_ocr_tokens]
    answers = list(answers)
    if len(answers) != num_answers:
        raise ValueError("expected %d answers, got %d" % (num_answers, len(answers)))
    V = len(voc)
    scores = soft_scores(answers)
    ocr2inds = defaultdict(list)
    for i, tok in enumerate(tokens):
        ocr2inds[tok].append(i)
    seqs, step0 = [], {}
    for a in answers:
        lst = match_answer_to_vocab_ocr_seq(a, voc.word2idx_dict, ocr2inds, max_match_num)
        seqs.extend(lst)
        s = scores[a]
        for seq in lst:
            step0[seq[0]] = max(step0.get(seq[0], 0.0), s)

    groups, scored = {}, set()

    def group(idx):
        g = groups.get(idx)
        if g is None:
            g = groups[idx] = len(groups)
        return g

    n = len(seqs)
    seq_len = np.zeros(n, np.int32)
    seq_grp = np.zeros((n, L), np.int16)
    for i, seq in enumerate(seqs):
        ln = min(len(seq), L)
        seq_len[i] = ln
        dec = min(1 + len(seq), L)
        for t in range(L):
            if t < ln:
                seq_grp[i, t] = group(seq[t])
            elif t < dec:
                seq_grp[i, t] = group(voc.EOS_IDX)
            if 1 <= t < dec:
                scored.add(seq[t] if t < len(seq) else voc.EOS_IDX)
        if ln < L:
            seq_grp[i, ln:] = groups[voc.EOS_IDX]
    if len(groups) > 32767:
        raise AnswerTableError(STATUS_GROUPS, "%d distinct score indices do not fit int16 group ids" % len(groups))
    grp_idx = np.array(list(groups), np.int32)
    off, extra = [0], []
    for idx in groups:
        if idx in scored:
            all_idx = [idx]
            if idx >= V:                                      # an OCR slot: plus its vocab word unless that is <unk>
                word = tokens[idx - V]
                if word == PAD_TOKEN:
                    raise AnswerTableError(STATUS_PAD_SLOT, "score index %d is an OCR slot holding <pad>" % idx)
                v = voc.word2idx(word)
                if v != voc.UNK_IDX:
                    all_idx.append(v)
            else:                                             # a vocab word: plus every OCR slot holding it
                all_idx.extend(V + o for o in ocr2inds.get(voc.word_list[idx], ()))
            if voc.UNK_IDX in all_idx:
                raise AnswerTableError(STATUS_UNK_TARGET, "<unk> (index %d) among the target indices of score index %d" % (voc.UNK_IDX, idx))
            extra.extend(all_idx)
        off.append(len(extra))
    return {"seq_len": seq_len, "seq_grp": seq_grp,
            "step0_idx": np.array(list(step0), np.int32), "step0_val": np.array(list(step0.values()), np.float32),
            "grp_idx": grp_idx, "grp_off": np.array(off, np.int32), "grp_extra": np.array(extra, np.int32),
            "dims": np.array([V + max_ocr_tokens, voc.BOS_IDX, voc.EOS_IDX, L], np.int32)}


class AnswerTableCaps(namedtuple("AnswerTableCaps", "S L G E")):
    """fixed per-run capacities of a collated batch (every batch of a run has the same tensor shapes, hence the same graph signature):
    S sequences (num_answers * max_match_num is an exact bound), L decoding steps, G distinct score indices, E target indices"""
    __slots__ = ()

    @classmethod
    def for_config(cls, num_answers=10, max_match_num=20, max_copy_steps=12, max_groups=64, max_extra=256):
        return cls(num_answers * max_match_num, max_copy_steps, max_groups, max_extra)


DEFAULT_CAPS = AnswerTableCaps.for_config()


def collate_answer_tables(tables, caps=DEFAULT_CAPS, pin_memory=False):
    """batch_dict["answer_table"]: a dict of CPU tensors at the fixed capacities `caps`
      meta int32 [B, 4] (n_seq, n_step0, n_grp, n_extra), seq_len int32 [B, S], seq_grp int16 [B, S, L], step0_idx int32 / step0_val fp32 [B, S],
      grp_idx int32 [B, G], grp_off int32 [B, G + 1], grp_extra int32 [B, E], dims int32 [4] (W, BOS, EOS, L).
    A sample over a capacity raises ValueError naming it: nothing is truncated."""
    caps = AnswerTableCaps(*caps)
    S, L, G, E = caps
    B = len(tables)
    if B == 0:
        raise ValueError("collate_answer_tables: empty batch")
    dims = np.asarray(tables[0]["dims"], np.int32)
    out = ANSWER_TABLE.zeros_host(B=B, S=S, L=L, G=G, E=E)
    for b, t in enumerate(tables):
        if not np.array_equal(np.asarray(t["dims"], np.int32), dims):
            raise ValueError("sample %d: (W, BOS, EOS, L) = %s differs from sample 0's %s" % (b, list(t["dims"]), list(dims)))
        if int(dims[3]) != L:
            raise ValueError("sample %d: tables built for %d decoding steps, capacity L = %d" % (b, int(dims[3]), L))
        n, n0, g, e = len(t["seq_len"]), len(t["step0_idx"]), len(t["grp_idx"]), len(t["grp_extra"])
        for what, have, name, cap, bit in (("sequences", n, "S", S, 0), ("step-0 indices", n0, "S", S, 0), ("score-index groups", g, "G", G, STATUS_GROUPS),
                                           ("target indices", e, "E", E, STATUS_EXTRA)):
            if have > cap:
                raise AnswerTableError(bit, "sample %d: %d %s exceed the capacity %s = %d" % (b, have, what, name, cap))
        out["meta"][b] = (n, n0, g, e)
        out["seq_len"][b, :n] = t["seq_len"]
        out["seq_grp"][b, :n] = t["seq_grp"]
        out["step0_idx"][b, :n0] = t["step0_idx"]
        out["step0_val"][b, :n0] = t["step0_val"]
        out["grp_idx"][b, :g] = t["grp_idx"]
        out["grp_off"][b, :g + 1] = t["grp_off"]
        out["grp_extra"][b, :e] = t["grp_extra"]
    res = {k: torch.from_numpy(v) for k, v in out.items()}
    res["dims"] = torch.from_numpy(dims.copy())
    return BT.pinned(res, pin_memory)


# ---------------------------------------------------------------------------------------------------------- the draw
def answer_key(seed, rank=0):
    """the draw's 64-bit key: the Trainer seed with the rank folded in, as the Trainer seeds the DropoutClock"""
    return (int(seed) ^ (int(rank) << 32)) & 0xFFFFFFFFFFFFFFFF


def draw_hash(key, step, samples):
    """csrc/answers.hip answer_draw_hash: lowbias32 chained over (key lo, key hi, step lo, step hi, sample) -> uint32 per sample"""
    key, s = int(key) & 0xFFFFFFFFFFFFFFFF, int(step) & 0xFFFFFFFFFFFFFFFF
    u = np.uint32
    with np.errstate(over="ignore"):
        h = _mix32(u((key & 0xFFFFFFFF) ^ 0xA0761D65))
        h = _mix32(h ^ u(key >> 32))
        h = _mix32(h ^ u(s & 0xFFFFFFFF))
        h = _mix32(h ^ u(s >> 32))
        smp = np.asarray(samples, np.uint32) * u(0x9E3779B1)
        return _mix32(h ^ smp)


def draw_choices(key, step, n_seq):
    """host twin of the kernel's draw: the sequence each sample picks at `step` (int64 [B]; -1 where n_seq = 0)"""
    n = np.asarray(n_seq, np.int64).reshape(-1)
    h = draw_hash(key, step, np.arange(len(n))).astype(np.uint64)
    k = ((h * n.astype(np.uint64)) >> np.uint64(32)).astype(np.int64)
    return np.where(n > 0, k, -1)


# ---------------------------------------------------------------------------------------------------------- torch twin of the kernel
def sample_answers_torch(table, choice):
    """what sam_answer_sample writes for the collated `table` when sample b picks sequence choice[b] (-1 or out of range: none), vectorised torch on the
    table's device -> {targets fp32 [B, L, W], train_prev_inds int64 [B, L], train_loss_mask, train_acc_mask fp32 [B, L], answer_choice int32 [B]}"""
    W, bos = int(table["dims"][0]), int(table["dims"][1])
    meta = table["meta"].long()
    B, S, L = table["seq_grp"].shape
    G, E = table["grp_idx"].shape[1], table["grp_extra"].shape[1]
    dev = meta.device
    n_seq, n0 = meta[:, 0].clamp(max=S), meta[:, 1].clamp(0, S)
    n_grp, n_ex = meta[:, 2].clamp(0, G), meta[:, 3].clamp(0, E)
    k = torch.as_tensor(choice, device=dev).long().reshape(B)
    valid = (k >= 0) & (k < n_seq)
    k = torch.where(valid, k, torch.full_like(k, -1))
    kk = k.clamp(0, S - 1)
    bi = torch.arange(B, device=dev)
    ln = table["seq_len"].long()[bi, kk].clamp(0, L)
    dec = torch.where(valid, torch.minimum(1 + ln, torch.full_like(ln, L)), torch.zeros_like(ln))
    t = torch.arange(L, device=dev)
    on = t[None] < dec[:, None]
    grp = table["seq_grp"].long()[bi, kk]                                              # [B, L]
    prev_g = torch.cat([torch.zeros_like(grp[:, :1]), grp[:, :-1]], 1)
    prev_ok = (prev_g >= 0) & (prev_g < n_grp[:, None])
    prev = table["grp_idx"].long().gather(1, prev_g.clamp(0, G - 1))
    prev = torch.where(prev_ok, prev, torch.zeros_like(prev))
    prev[:, 0] = bos
    prev = torch.where(on, prev, torch.zeros_like(prev))
    targets = torch.zeros(B * L * W, dtype=torch.float32, device=dev)
    # step 0: the merged (index, max score) list
    i0 = table["step0_idx"].long()
    m0 = (torch.arange(S, device=dev)[None] < n0[:, None]) & valid[:, None] & (i0 >= 0) & (i0 < W)
    flat0 = bi[:, None] * (L * W) + i0
    targets[flat0[m0]] = table["step0_val"][m0].float()
    # steps 1 .. dec - 1: 1.0 at every index of the group of the step's score index
    g_ok = (grp >= 0) & (grp < n_grp[:, None]) & on & (t[None] >= 1)
    gc = grp.clamp(0, G - 1)
    off = table["grp_off"].long()
    lo = off.gather(1, gc).clamp(min=0)
    lo = torch.minimum(lo, n_ex[:, None])
    hi = torch.maximum(lo, torch.minimum(off.gather(1, (gc + 1).clamp(max=G)), n_ex[:, None]))
    e = torch.arange(E, device=dev)
    ex = table["grp_extra"].long()[:, None, :].expand(B, L, E)
    sel = g_ok[:, :, None] & (e[None, None] >= lo[:, :, None]) & (e[None, None] < hi[:, :, None]) & (ex >= 0) & (ex < W)
    flat = (bi[:, None, None] * L + t[None, :, None]) * W + ex
    targets[flat[sel]] = 1.0
    return {"targets": targets.view(B, L, W), "train_prev_inds": prev, "train_loss_mask": on.float(),
            "train_acc_mask": (t[None] < dec[:, None] - 1).float(), "answer_choice": k.to(torch.int32)}


# ---------------------------------------------------------------------------------------------------------- torch twin of the table loss
def sparse_target_rows(table, choice):
    """the non-zeros of every target row, straight from the collated table (host walk, the clamps of csrc/answers.hip): {(b, t): {index: value}} for the
    rows sample b's sequence choice[b] scores; rows that are absent are all zero (choice -1 / out of range: no row at all)"""
    W = int(table["dims"][0])
    tab = {k: table[k].cpu().numpy() for k in TABLE_KEYS}
    B, S, L = tab["seq_grp"].shape
    G, E = tab["grp_idx"].shape[1], tab["grp_extra"].shape[1]
    ks = np.asarray(torch.as_tensor(choice).cpu().numpy(), np.int64).reshape(B)
    rows = {}
    for b in range(B):
        m = tab["meta"][b]
        n_seq, n0 = min(int(m[0]), S), max(0, min(int(m[1]), S))
        n_grp, n_ex = max(0, min(int(m[2]), G)), max(0, min(int(m[3]), E))
        k = int(ks[b])
        if k < 0 or k >= n_seq:
            continue
        dec = min(1 + max(0, min(int(tab["seq_len"][b, k]), L)), L)
        row0 = rows.setdefault((b, 0), {})
        for i in range(n0):
            idx = int(tab["step0_idx"][b, i])
            if 0 <= idx < W:
                row0[idx] = float(tab["step0_val"][b, i])
        for t in range(1, dec):
            g = int(tab["seq_grp"][b, k, t])
            row = rows.setdefault((b, t), {})
            if 0 <= g < n_grp:
                lo = max(0, min(int(tab["grp_off"][b, g]), n_ex))
                hi = max(lo, min(int(tab["grp_off"][b, g + 1]), n_ex))
                for idx in tab["grp_extra"][b, lo:hi].tolist():
                    if 0 <= idx < W:
                        row[idx] = 1.0
    return rows


def bce_from_table_torch(fixed, ocr, table, choice, loss_mask, grad_scale=1.0, global_count=None):
    """CPU / torch twin of sam_bce_loss_table: M4CDecodingBCEWithMaskLoss (sam/task_utils.py:19-30) and its gradient on the targets the sampler would have
    written for `choice`, built here row by row from the table's sparse lists (sparse_target_rows; no dense [B, L, W] tensor, and not via
    sample_answers_torch), plus the metric's argmax (sam/datasets/metrics.py:26).  fixed [R, V] / ocr [R, No] (or [B, L, .]), loss_mask [R] or [B, L].
    -> (loss fp32 scalar, d_fixed fp32 [R, V], d_ocr fp32 [R, No], pred int64 [R]).  With every target 0, bce(x, 0) = softplus(x) and d/dx = sigmoid(x); the
    listed (row, index, value) entries then subtract x * value from the loss and value from the gradient."""
    B, _, L = table["seq_grp"].shape
    R = B * L
    f = fixed.detach().reshape(R, -1).to(torch.float64)
    o = ocr.detach().reshape(R, -1).to(torch.float64)
    V = f.shape[1]
    x = torch.cat([f, o], 1)
    mask = loss_mask.detach().reshape(R).to(torch.float64)
    count = mask.sum() if global_count is None else torch.as_tensor(global_count, dtype=torch.float64).reshape(())
    count = torch.clamp(count, min=1.0)
    row_loss = torch.nn.functional.softplus(x).sum(1)
    grad = torch.sigmoid(x)
    ri, ci, vi = [], [], []
    for (b, t), nz in sparse_target_rows(table, choice).items():
        for idx, val in nz.items():
            ri.append(b * L + t); ci.append(idx); vi.append(val)
    if ri:
        ri, ci = torch.tensor(ri, dtype=torch.long), torch.tensor(ci, dtype=torch.long)
        vi = torch.tensor(vi, dtype=torch.float64)
        row_loss = row_loss.index_put((ri,), -x[ri, ci] * vi, accumulate=True)
        grad = grad.index_put((ri, ci), -vi, accumulate=True)
    loss = (row_loss * mask).sum() / count
    grad = grad * (mask / count * float(grad_scale))[:, None]
    pred = torch.argmax(torch.cat([fixed.detach().reshape(R, -1), ocr.detach().reshape(R, -1)], 1), dim=-1)
    return loss.to(torch.float32), grad[:, :V].to(torch.float32), grad[:, V:].to(torch.float32), pred


def decode_predictions(pred_ids, answer_vocab, ocr_tokens, eos_idx=None):
    """greedy prediction indices -> what a TextVQA metric scores (the index -> word walk of sam/datasets/metrics.py:39-51).  pred_ids: int [B, L]
    (Trainer.predictions(), a decoder's output); ocr_tokens: per sample the list of its OCR token strings.  Per sample, in order: an index below
    len(answer_vocab) that is EOS ends the answer; any other vocabulary index contributes its word; an index at or above len(answer_vocab) copies OCR token
    (index - len(answer_vocab)) -- IndexError (naming the sample) when the sample has no such token.  The words are joined with blanks and " 's" is glued
    back to "'s".  -> [(answer string, answer_words, belongs_to)] with belongs_to entries "vocab", "ocr", "vocab+eos"."""
    voc = as_answer_vocab(answer_vocab)
    eos = voc.EOS_IDX if eos_idx is None else int(eos_idx)
    V = len(voc)
    ids = pred_ids.detach().cpu().tolist() if torch.is_tensor(pred_ids) else [list(r) for r in pred_ids]
    if len(ids) != len(ocr_tokens):
        raise ValueError("decode_predictions: %d prediction rows for %d samples' OCR tokens" % (len(ids), len(ocr_tokens)))
    out = []
    for b, (row, tokens) in enumerate(zip(ids, ocr_tokens)):
        words, belongs = [], []
        for i in row:
            i = int(i)
            if i >= V:
                if i - V >= len(tokens):
                    raise IndexError("decode_predictions: sample %d predicts OCR slot %d but has %d OCR tokens" % (b, i - V, len(tokens)))
                belongs.append("ocr")
                words.append(tokens[i - V])
            elif i == eos:
                belongs.append("vocab+eos")
                break
            else:
                if i < 0:
                    raise IndexError("decode_predictions: sample %d predicts the negative index %d" % (b, i))
                belongs.append("vocab")
                words.append(voc.word_list[i])
        out.append((" ".join(words).replace(" 's", "'s"), words, belongs))
    return out


# ---------------------------------------------------------------------------------------------------------- public sampler
def table_dims(table):
    """(W, BOS) of a collated table: free for a CPU table, one device read for a GPU one"""
    d = table["dims"]
    w, bos = (int(x) for x in d[:2].tolist())
    return w, bos


def sample_answers(batch_dict, step, seed=0, choice=None, rank=None, device=None):
    """draw the answer sequences of batch_dict["answer_table"] for training step `step` on the GPU (csrc/answers.hip) and fill batch_dict's targets,
    train_prev_inds, train_loss_mask, train_acc_mask and answer_choice, as M4CAnswerProcessor.__call__ fills a sample.  The key is answer_key(seed, rank)
    (rank: the process group's, 0 without one), the draw the one Trainer.step(...) makes at global_step == step; choice (int32 [B]) pins it."""
    from . import ops
    if "targets" in batch_dict:
        raise ValueError("batch_dict carries both dense 'targets' and an 'answer_table'")
    table = batch_dict["answer_table"]
    if rank is None:
        dist = torch.distributed
        rank = dist.get_rank() if dist.is_available() and dist.is_initialized() else 0
    dev = torch.device(device) if device is not None else (table["meta"].device if table["meta"].is_cuda else torch.device("cuda"))
    W, bos = table_dims(table)
    tab = {k: table[k].to(dev, non_blocking=True) for k in TABLE_KEYS}
    fc = None if choice is None else torch.as_tensor(choice, dtype=torch.int32).to(dev)
    out = ops.answer_sample(tab, W, bos, answer_key(seed, rank), step=int(step), force_choice=fc)
    batch_dict.update(out)
    return out


def make_answer_tables(batch_size, num_vocab=5000, n_ocr=50, seed=0, max_copy_steps=12):
    """synthetic TextVQA-like samples for tests and tools: a vocabulary of num_vocab words (<pad>, <s>, </s>, <unk> first), per sample up to n_ocr OCR
    tokens drawn from the vocabulary and from out-of-vocabulary words, and ten answers of 1-3 words, mostly repeats of a few (soft scores 0.3-1.0), some
    of them OCR words, one in ten unmatched.  -> (AnswerVocab, [build_answer_table records])"""
    rng = np.random.RandomState(seed)
    words = [PAD_TOKEN, BOS_TOKEN, EOS_TOKEN, UNK_TOKEN] + ["w%d" % i for i in range(num_vocab - 4)]
    voc = AnswerVocab(words)
    tabs = []
    for _ in range(batch_size):
        n_tok = rng.randint(1, n_ocr + 1)
        pool = ["w%d" % i for i in rng.randint(0, num_vocab - 4, 8)] + ["oov%d" % i for i in rng.randint(0, 40, 8)]
        tokens = [pool[i] for i in rng.randint(0, len(pool), n_tok)]
        cands = []
        for _ in range(4):
            src = tokens if rng.rand() < 0.6 else ["w%d" % i for i in rng.randint(0, num_vocab - 4, 3)]
            cands.append(" ".join(src[i] for i in rng.randint(0, len(src), rng.randint(1, 4))))
        cands.append("unmatched%d" % rng.randint(1000))
        answers = [cands[i] for i in rng.choice(len(cands), 10, p=[0.4, 0.25, 0.15, 0.1, 0.1])]
        tabs.append(build_answer_table(answers, tokens, voc, max_ocr_tokens=n_ocr, max_copy_steps=max_copy_steps))
    return voc, tabs


# ---------------------------------------------------------------------------------------------------------- tables from the answers' text
# build_answer_table + collate_answer_tables as one launch per batch (csrc/answer_text.hip, sam_answer_table_from_text): the batch carries the cleaned
# answers and the OCR tokens as code points, the run keeps the answer vocabulary on the device as an exact-match hash index, and nothing about the
# answers is computed or cached on the host.
ANSWER_TEXT_KEYS = ("answer_text", "answer_text_len")
MAX_ANSWER_CHARS = 128
MAX_WORD_CHARS = 64
STATUS_REASONS = ((STATUS_GROUPS, "more score-index groups than the capacity G = %(G)d"), (STATUS_EXTRA, "more target indices than the capacity E = %(E)d"),
                  (STATUS_PAD_SLOT, "a score index is an OCR slot holding <pad>"), (STATUS_UNK_TARGET, "<unk> (index %(UNK)d) among the target indices of a score index"))


def pack_answer_text(answers_per_sample, num_answers=10, max_chars=MAX_ANSWER_CHARS, pin_memory=False):
    """list (one entry per sample) of the sample's cleaned answers, as the dataset hands them to the answer processor -> {"answer_text": int32 [B, A, La],
    "answer_text_len": int32 [B, A]} on the CPU, A = num_answers, La = max_chars (at most 128): the exact code points, nothing lowered or stripped.
    A sample without exactly num_answers answers, or an answer of more than max_chars code points, raises ValueError naming it: nothing is truncated."""
    B, A, La = len(answers_per_sample), int(num_answers), int(max_chars)
    if B == 0:
        raise ValueError("pack_answer_text: no samples")
    if A < 1:
        raise ValueError("pack_answer_text: num_answers = %d must be at least 1" % A)
    if not 1 <= La <= MAX_ANSWER_CHARS:
        raise ValueError("pack_answer_text: max_chars = %d must be in [1, %d]" % (La, MAX_ANSWER_CHARS))

    def rows():
        for b, ans in enumerate(answers_per_sample):
            ans = list(ans)
            if len(ans) != A:
                raise ValueError("sample %d: expected %d answers, got %d" % (b, A, len(ans)))
            for i, a in enumerate(ans):
                yield (b, i), a

    text, ln = BT.pack_rows((B, A, La), rows(), La, lambda at, a, n: "sample %d: answer %d (%r) has %d code points, over max_chars = %d" % (at + (a, n, La)))
    return BT.pinned({"answer_text": torch.from_numpy(text), "answer_text_len": torch.from_numpy(ln)}, pin_memory)


def vocab_index(answer_vocab, max_word=32):
    """the answer vocabulary as the kernel reads it, built once per run: {"cp": int32 [V, Lv] exact code points of AnswerVocab.word_list, "len": int32 [V],
    "slots": int32 [T] the slot table wordindex.build_slots makes of them (T the smallest power of two >= 2 V, -1 = empty, home slot text_hash & (T - 1), linear
    probing, a contested slot goes to the lowest index; AnswerVocab has rejected a word list that names a word twice, so a probe's first match is the word's
    only index), "V", "UNK", "BOS", "EOS"} -- CPU tensors and ints; index_to(index, device) moves the three tensors.  A word of more than max_word (<= 64)
    code points raises ValueError."""
    voc = as_answer_vocab(answer_vocab)
    V, Lv = len(voc), int(max_word)
    if not 1 <= Lv <= MAX_WORD_CHARS:
        raise ValueError("vocab_index: max_word = %d must be in [1, %d]" % (Lv, MAX_WORD_CHARS))
    cp, ln = BT.pack_rows((V, Lv), enumerate(voc.word_list), Lv, lambda i, w, n: "vocab_index: word %d (%r) has %d code points, over max_word = %d" % (i, w, n, Lv))
    slots = build_slots(cp, ln, np.arange(V), table_size(V))
    return {"cp": torch.from_numpy(cp), "len": torch.from_numpy(ln), "slots": torch.from_numpy(slots), "V": V, "UNK": voc.UNK_IDX, "BOS": voc.BOS_IDX,
            "EOS": voc.EOS_IDX}


def is_vocab_index(v):
    return isinstance(v, dict) and all(k in v for k in ("cp", "len", "slots", "V", "UNK", "BOS", "EOS"))


def _zero_tables(B, caps):
    S, L, G, E = caps
    return ANSWER_TABLE.zeros("cpu", B=B, S=S, L=L, G=G, E=E)


def tables_from_text_host(answer_text, answer_text_len, ocr_text, ocr_text_len, answer_vocab, caps=DEFAULT_CAPS, max_match_num=20):
    """host twin of sam_answer_table_from_text on the packed tensors: decodes the code points (lengths clamped as the kernel clamps them; every one of the
    No slots is a token, the empty ones the empty string, which no word equals), calls build_answer_table per sample and collates.  -> (table, status):
    the collated table with dims, and int32 [B] with the kernel's status bit and an all-zero row where the host functions raise for a sample."""
    caps = AnswerTableCaps(*caps)
    voc = as_answer_vocab(answer_vocab)
    (at, al), (ot, ol) = BT.unpack(answer_text, answer_text_len), BT.unpack(ocr_text, ocr_text_len)
    (B, A), No = at.shape[:2], ot.shape[1]
    out = _zero_tables(B, caps)
    status = torch.zeros(B, dtype=torch.int32)
    dims = torch.tensor([len(voc) + No, voc.BOS_IDX, voc.EOS_IDX, caps.L], dtype=torch.int32)
    for b in range(B):
        ans, toks = BT.strings(at[b], al[b]), BT.strings(ot[b], ol[b])
        try:
            one = collate_answer_tables([build_answer_table(ans, toks, voc, num_answers=A, max_ocr_tokens=No, max_copy_steps=caps.L, max_match_num=max_match_num)], caps)
        except AnswerTableError as e:
            if not e.status:
                raise
            status[b] = e.status
            continue
        for k in TABLE_KEYS:
            out[k][b] = one[k][0]
    out["dims"] = dims
    return out, status


def check_answer_text(batch_dict):
    """a batch opts in with BOTH answer-text keys; -> whether it did.  The answers' text replaces the answer table and the dense targets, and the kernel
    matches it against the OCR tokens' text: the combinations that cannot be served raise ValueError."""
    return BT.check(BT.ANSWER_TEXT_TABLE, batch_dict)


def table_outputs(B, caps, device):
    """fresh output buffers of tables_from_text at the capacities `caps`: the eight TABLE_KEYS tensors and "status" int32 [B]"""
    S, L, G, E = AnswerTableCaps(*caps)
    return ANSWER_TABLE_OUT.empty(device, B=B, S=S, L=L, G=G, E=E)


def status_message(status, index, caps):
    """the first flagged sample of a status vector (host list) in the host functions' words, or None"""
    caps = AnswerTableCaps(*caps)
    hit = BT.first_flagged(status, STATUS_REASONS, G=caps.G, E=caps.E, UNK=int(index["UNK"]))
    return hit and "sample %d: %s" % (hit[0], hit[2])


def tables_from_text(batch_dict, index, caps=DEFAULT_CAPS, max_match_num=20, out=None, check=True):
    """batch_dict["answer_table"] of a batch that carries answer_text / answer_text_len and ocr_text / ocr_text_len on the GPU, one launch
    (csrc/answer_text.hip): bit for bit collate_answer_tables of build_answer_table of every sample.  index: vocab_index(...) with its tensors on the
    GPU; out: buffers from table_outputs (allocated here when None; every element is written).  dims (W, BOS, EOS, L) is filled by the host from the
    index and the shapes.  check=True reads status back and raises ValueError naming the first flagged sample and the reason; check=False never
    synchronises and returns (table, status): a flagged sample's rows are all zero, which the sampler treats as "no candidate"."""
    from . import ops
    caps = AnswerTableCaps(*caps)
    at, ot = batch_dict["answer_text"], batch_dict["ocr_text"]
    if out is None:
        out = table_outputs(at.shape[0], caps, at.device)
    ops.answer_table_from_text(at, batch_dict["answer_text_len"], ot, batch_dict["ocr_text_len"], index, out, max_match_num=max_match_num)
    table = {k: out[k] for k in TABLE_KEYS}
    table["dims"] = torch.tensor([int(index["V"]) + ot.shape[1], int(index["BOS"]), int(index["EOS"]), caps.L], dtype=torch.int32)
    if not check:
        return table, out["status"]
    msg = status_message(out["status"].tolist(), index, caps)
    if msg is not None:
        raise ValueError(msg)
    return table


# ---------------------------------------------------------------------------------------------------------- the build's sticky status record
# tables_from_text(check=False) in front of every step never raises for a flagged sample and reads nothing back: a one-wave launch behind the build
# (ops.answer_status_fold: csrc/answer_status.hip, sam_answer_status_fold, include/sam_hip_step.h) folds status into four int64 words on the device, which
# the caller reads when it wants to.
STATUS_STATE_RESET = (0, 0, -1, -1)
STATUS_COUNT_CAP = 1 << 62
STATUS_STATE_KEYS = ("bits", "flagged", "first_step", "first_sample")


def fold_status_host(status, step, state):
    """host twin of sam_answer_status_fold: status (a sequence of ints or an int tensor, one word per sample of one build) folded into `state`, four ints
    (OR of the status words as unsigned 32-bit values, number of flagged samples saturating at 2^62, step and batch index of the first flagged sample:
    written once, while the index is negative; the lowest flagged index of that step).  -> the new state as a list of four ints; `state` is not changed."""
    st = [int(s) for s in (status.detach().cpu().reshape(-1).tolist() if torch.is_tensor(status) else status)]
    if not st:
        raise ValueError("fold_status_host: no samples")
    bits, flagged, first_step, first_sample = (int(x) for x in (state.detach().cpu().tolist() if torch.is_tensor(state) else state))
    marked = [b for b, s in enumerate(st) if s != 0]
    for s in st:
        bits |= s & 0xFFFFFFFF
    if marked:
        flagged = min(flagged + len(marked), STATUS_COUNT_CAP)
        if first_sample < 0:
            first_step, first_sample = int(step), marked[0]
    return [bits, flagged, first_step, first_sample]

"""Evaluation results collected by question index: a results board resident in device memory.

sampler.Sampler.next() pads a shard by wrapping and marks the slots past its end with valid = 0; evaluator.evaluate adds every slot of every batch to its
sums and its answer list, so a pass driven by the sampler counts the wrapped questions twice, and two ranks' partial sums cannot be merged without
counting the wrap padding again.  A board keeps one result row per QUESTION instead:

    scores fp32 [n, 3], oracle fp32 [n, 3], flags int32 [n], best int32 [n], answer int32 [n, P], answer_len int32 [n]   (sam_eval_beams' outputs)
    seen int32 [n]     how many valid slots held the question so far; 0: the row is empty
    status int32 [1]   only ever OR-ed into; bit 0: a valid slot held an index outside [0, n)

collect scatters a batch's metrics.evaluate_beams rows to board[sample_idx[b]] where valid[b] is set (first write wins), reduce sums the distinct rows
in one fixed order, merge folds another rank's board in row by row (ops.evalboard_*, csrc/evalboard.hip: one launch each).  By construction the means
are independent of batch size, batch order, world size and wrap padding, to the last bit.  The host reads back once per pass (result()).

This file is the definition: collect_host / reduce_host / merge_host on numpy are the host twins the kernels equal bit for bit, untouched rows
included."""
import numpy as np
import torch

from .batchtext import to_numpy as _np
from .layouts import EVAL_BOARD, EVAL_ROWS

KEYS = EVAL_BOARD.keys
ROW_KEYS = EVAL_ROWS.keys                       # the evaluate_beams outputs a row holds, in KEYS' order
BAD_INDEX = 1                                   # status bit 0 (include/sam_hip_evalboard.h)
_DTYPES = EVAL_BOARD.np_dtypes                  # (under the name its readers use)


def _check_size(n, P):
    n, P = int(n), int(P)
    if not 1 <= n < 1 << 31:
        raise ValueError("evalboard: n = %d (need 1 <= n < 2^31)" % n)
    if P < 1:
        raise ValueError("evalboard: answer width P = %d (need >= 1)" % P)
    return n, P


# ---------------------------------------------------------------------------------------------------------- host twins (the definition)
def new_host(n, P):
    """an empty board on the host: the eight KEYS arrays, all zero"""
    n, P = _check_size(n, P)
    return EVAL_BOARD.zeros_host(n=n, P=P)


def _host_shape(board):
    n, P = board["answer"].shape
    EVAL_BOARD.check_host(board, "evalboard: board", n=n, P=P)
    return n, P


def collect_host(board, res, sample_idx, valid=None):
    """the host twin of sam_evalboard_collect, and its specification; `board` (new_host) is changed in place and returned.  res: evaluate_beams' /
    evaluate_beams_host's dict for B samples.  Slot b is LIVE when (valid is None or valid[b] != 0) and 0 <= sample_idx[b] < n; a valid slot out of
    range sets status bit 0 and writes nothing.  A live slot OWNS q = sample_idx[b] when no live slot in front of it holds q; with m live slots holding
    q, the owner copies its row (all P answer columns, answer_len clamped to [0, P]) and sets seen[q] = m when seen[q] == 0, else leaves the row and
    adds m to seen[q] (int32, two's complement)."""
    n, P = _host_shape(board)
    idx = _np(sample_idx).astype(np.int64).reshape(-1)
    B = idx.size
    ok = np.ones(B, bool) if valid is None else _np(valid).reshape(-1) != 0
    rows = [_np(res[k]) for k in ROW_KEYS]
    if B < 1 or ok.size != B or rows[4].shape != (B, P) or any(r.shape[0] != B for r in rows):
        raise ValueError("evalboard: a batch of %d slots needs valid [%d] and result rows [%d, ...] with answer [%d, %d]" % (B, B, B, B, P))
    inside = (idx >= 0) & (idx < n)
    if (ok & ~inside).any():
        board["status"][0] |= BAD_INDEX
    live = ok & inside
    counts = {}
    for b in np.flatnonzero(live):
        counts.setdefault(int(idx[b]), []).append(int(b))
    for q, slots in counts.items():
        b, m = slots[0], len(slots)
        if board["seen"][q] == 0:
            for k, r in zip(KEYS[:6], rows):
                board[k][q] = r[b]
            board["answer_len"][q] = min(max(int(rows[5][b]), 0), P)
            board["seen"][q] = m
        else:
            board["seen"][q] = _wrap32(int(board["seen"][q]) + m)
    return board


def _wrap32(v):
    v &= 0xFFFFFFFF
    return v - (1 << 32) if v >= 1 << 31 else v


def reduce_host(board):
    """the host twin of sam_evalboard_reduce: float64 [8] = the three score sums over the rows with seen > 0, the number of such rows, the three oracle
    sums over the same rows, the sum of their seen.  The order is metrics.host_totals' over the BOARD's rows -- thread t of 256 adds rows t, t + 256,
    ... in ascending order, then a halving tree over the threads -- and a row with seen <= 0 adds nothing, whatever it holds.  On a board whose rows
    are all seen, out[0:4] is host_totals(scores)."""
    n, _ = _host_shape(board)
    live = board["seen"] > 0
    rows = np.flatnonzero(live)
    val = np.concatenate([board["scores"][rows], board["oracle"][rows]], 1).astype(np.float64)          # (an unseen row is never read, nor converted)
    red = np.zeros((256, 6))
    for r, v in zip(rows, val):
        red[r % 256] += v
    o = 128
    while o >= 1:
        red[:o] += red[o:2 * o]
        o >>= 1
    return np.concatenate([red[0, :3], [float(live.sum())], red[0, 3:], [float(board["seen"][live].astype(np.int64).sum())]])


def merge_host(dst, src):
    """the host twin of sam_evalboard_merge; `dst` is changed in place and returned: every row src has seen (seen > 0) is copied where dst's row is
    empty (seen == 0), dst.seen += src.seen there in either case, dst.status |= src.status"""
    if _host_shape(dst) != _host_shape(src):
        raise ValueError("evalboard: merge of boards of different shapes %s and %s" % (_host_shape(dst), _host_shape(src)))
    if any(np.shares_memory(dst[k], src[j]) for k in KEYS for j in KEYS):
        raise ValueError("evalboard: merge needs two boards that share no memory")
    for q in np.flatnonzero(src["seen"] > 0):
        if dst["seen"][q] == 0:
            for k in KEYS[:6]:
                dst[k][q] = src[k][q]
        dst["seen"][q] = _wrap32(int(dst["seen"][q]) + int(src["seen"][q]))
    dst["status"][0] |= src["status"][0]
    return dst


def _result(red, seen, answer, answer_len, question_ids):
    """reduce's eight sums and the board's seen / answer / answer_len on the host -> the result dict"""
    from . import metrics as M
    n = seen.shape[0]
    count = int(red[3])
    if count == 0:
        raise ValueError("evalboard: no question was collected")
    rows = np.flatnonzero(seen > 0)
    text = M.answer_strings(answer[rows], np.clip(answer_len[rows], 0, answer.shape[1]))         # (a merged row's length is not trusted either)
    qid = rows.tolist() if question_ids is None else [question_ids[q] for q in rows.tolist()]
    return {"vqa_accuracy": red[0] / count, "stvqa_accuracy": red[1] / count, "anls": red[2] / count, "count": count,
            "oracle": [red[4] / count, red[5] / count, red[6] / count], "missing": n - count, "repeats": int(red[7]) - count,
            "answers": [{"question_id": q, "answer": s} for q, s in zip(qid, text)]}


def status_message(st):
    return "bit 0: a valid slot held a sample index outside the board" if st & BAD_INDEX else "unknown bits"


def result_host(board, question_ids=None, check=True):
    """Board.result() of a host board: the twin of the whole pass's read-back"""
    st = int(board["status"][0])
    if check and st:
        raise ValueError("evalboard: status %d: %s" % (st, status_message(st)))
    red = [float(v) for v in reduce_host(board)]
    return _result(red, board["seen"], board["answer"], board["answer_len"], _ids(question_ids, board["seen"].shape[0]))


def _ids(question_ids, n):
    if question_ids is None:
        return None
    ids = question_ids.reshape(-1).tolist() if torch.is_tensor(question_ids) or isinstance(question_ids, np.ndarray) else list(question_ids)
    if len(ids) != n:
        raise ValueError("evalboard: %d question ids for a board of %d questions" % (len(ids), n))
    return ids


# ---------------------------------------------------------------------------------------------------------- the resident board
class Board:
    """The results board of one evaluation pass on one rank.  collect / reduce / merge are one launch each, take no host-side value per call and never
    synchronise; collect allocates nothing.  The board is read back by result() (once per pass), status() and state_dict() only."""

    def __init__(self, n, P, device="cuda", question_ids=None):
        self.n, self.P = _check_size(n, P)
        self.device = torch.device(device)
        self.question_ids = _ids(question_ids, self.n)
        self.t = EVAL_BOARD.zeros(self.device, n=self.n, P=self.P)

    def collect(self, res, sample_idx, valid=None):
        """a batch's metrics.evaluate_beams result dict into the board: row b goes to question sample_idx[b] (int32 [B] on the device) where valid[b]
        (int32 [B], None: every slot) is set and the question's row is empty"""
        from . import ops
        ops.evalboard_collect(self.t, res, sample_idx, valid)

    def reduce(self, out=None):
        """-> float64 [8] on the device (reduce_host lists it), un-synchronised"""
        from . import ops
        return ops.evalboard_reduce(self.t, out)

    def merge(self, other):
        """fold another board of the same shape (another rank's, gathered to this device) into this one; merge the ranks in rank order"""
        from . import ops
        if not isinstance(other, Board) or (other.n, other.P) != (self.n, self.P):
            raise ValueError("evalboard: merge needs a Board of n = %d, P = %d" % (self.n, self.P))
        if other is self:
            raise ValueError("evalboard: merge needs two boards that share no memory")
        ops.evalboard_merge(self.t, other.t)

    def reset(self):
        """back to the empty board (eight fills; the question ids stay)"""
        for t in self.t.values():
            t.zero_()

    def status(self, check=True):
        """the status word (read back: synchronises).  check=True raises ValueError naming the bit"""
        st = int(self.t["status"].item())
        if check and st:
            raise ValueError("evalboard: status %d: %s" % (st, status_message(st)))
        return st

    def result(self, check=True):
        """the single read-back of a pass -> evaluator.evaluate's dict ("vqa_accuracy", "stvqa_accuracy", "anls", "oracle": means over the distinct
        questions seen; "count": how many those are; "answers": [{"question_id", "answer"}] in question-index order over the seen rows, question_id
        from question_ids when given, else the index) with "missing" = n - count and "repeats" = the slots collected beyond one per question.
        evaluator.write_evalai takes it unchanged.  check=True raises ValueError when the status word is set."""
        red = self.reduce()
        host = {k: self.t[k].cpu().numpy() for k in ("seen", "answer_len", "status")}
        st = int(host["status"][0])
        if check and st:
            raise ValueError("evalboard: status %d: %s" % (st, status_message(st)))
        used = host["answer_len"][host["seen"] > 0]
        width = min(max(int(used.max()) if used.size else 0, 1), self.P)         # only the columns some seen row's string reaches cross the link
        return _result(red.cpu().tolist(), host["seen"], self.t["answer"][:, :width].cpu().numpy(), host["answer_len"], self.question_ids)

    def host(self):
        """the board as numpy arrays (a copy): what the host twins take"""
        return {k: self.t[k].cpu().numpy().copy() for k in KEYS}

    def state_dict(self):
        """the eight tensors on the CPU, the shape and the question ids: a half-finished pass resumes from it next to the sampler's state"""
        d = {k: self.t[k].cpu().clone() for k in KEYS}
        d.update(n=self.n, P=self.P, question_ids=None if self.question_ids is None else list(self.question_ids))
        return d

    def load_state_dict(self, d):
        """ValueError when the saved board is not one of this shape and these question ids"""
        if d.get("n") != self.n or d.get("P") != self.P:
            raise ValueError("evalboard: the saved state has n = %r, P = %r, this board %d, %d" % (d.get("n"), d.get("P"), self.n, self.P))
        if d.get("question_ids") != self.question_ids:
            raise ValueError("evalboard: the saved state has other question ids")
        for k, s in EVAL_BOARD.shapes(n=self.n, P=self.P).items():
            if k not in d or not torch.is_tensor(d[k]) or d[k].dtype != EVAL_BOARD.torch_dtypes[k] or tuple(d[k].shape) != s:
                raise ValueError("evalboard: the saved state lacks %s as %s %s" % (k, EVAL_BOARD.torch_dtypes[k], s))
        for k in KEYS:
            self.t[k].copy_(d[k])

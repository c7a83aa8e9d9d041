"""The tensor tables that cross the C ABI as a run of pointers -- answer table, score table, eval_beams result (plain and merged), evaluation board, witness -- each described
once: key order (the ABI's parameter order), dtype and shape per key.  ops.py checks and passes the tensors in this order, answers.py, metrics.py and
evalboard.py allocate from it, tests/test_layouts_cpu.py holds it against the prototypes under include/.  Pure: numpy and torch, no GPU, no library."""
import math

import numpy as np
import torch


class Layout:
    """name: what messages call the table; fields: (key, dtype name) in ABI order; shapes: the capacities, by name -> the fields' shapes, in that
    order; lead: the GPU size check requires shape[0] too (else the element count alone: the kernels index flat memory)"""

    def __init__(self, name, fields, shapes, lead=False):
        self.name, self.fields, self._shapes, self.lead = name, tuple(fields), shapes, lead
        self.keys = tuple(k for k, _ in self.fields)
        self.np_dtypes = {k: np.dtype(d) for k, d in self.fields}
        self.torch_dtypes = {k: getattr(torch, d) for k, d in self.fields}

    def shapes(self, **dims):
        return dict(zip(self.keys, self._shapes(**dims)))

    def zeros_host(self, **dims):
        return {k: np.zeros(s, self.np_dtypes[k]) for k, s in self.shapes(**dims).items()}

    def empty(self, device, **dims):
        return {k: torch.empty(s, dtype=self.torch_dtypes[k], device=device) for k, s in self.shapes(**dims).items()}

    def zeros(self, device, **dims):
        return {k: t.zero_() for k, t in self.empty(device, **dims).items()}

    def with_status(self):
        """this layout and the "status" int32 [B] word per sample that the *_from_text builders append"""
        return Layout(self.name, self.fields + (("status", "int32"),), lambda **d: self._shapes(**d) + ((d["B"],),), self.lead)

    # The checks of a dict of GPU tensors.  gpu: (ops._chk, which takes one tensor's dtype, device and contiguity; the exception type,
    # capi.SamHipError) -- handed in, as this module imports neither.  A caller that reads the capacities off the tensors calls require first.
    def require(self, d, gpu, name=None):
        for k in self.keys:
            if k not in d:
                raise gpu[1]("%s lacks %r" % (name or self.name, k))

    def check(self, d, gpu, name=None, **dims):
        """each tensor through chk, then its element count (and leading dimension, for a layout with `lead`) at these capacities"""
        for k, s in self.shapes(**dims).items():
            gpu[0](d[k], self.torch_dtypes[k], "%s[%r]" % (name or self.name, k))
            if d[k].numel() != math.prod(s) or (self.lead and d[k].shape[0] != s[0]):
                raise gpu[1]("%s[%r] has %d elements, expected %d (%s)" % (name or self.name, k, d[k].numel(), math.prod(s),
                                                                           " ".join("%s=%d" % kv for kv in dims.items())))

    def check_host(self, d, name, **dims):
        """a dict of numpy arrays: exactly these shapes and dtypes, else ValueError"""
        for k, s in self.shapes(**dims).items():
            if d[k].shape != s or d[k].dtype != self.np_dtypes[k]:
                raise ValueError("%s[%r] is %s %s, expected %s %s" % (name, k, d[k].dtype, d[k].shape, self.np_dtypes[k], s))


ANSWER_TABLE = Layout("answer table", (("meta", "int32"), ("seq_len", "int32"), ("seq_grp", "int16"), ("step0_idx", "int32"), ("step0_val", "float32"),
                                       ("grp_idx", "int32"), ("grp_off", "int32"), ("grp_extra", "int32")),
                      lambda B, S, L, G, E: ((B, 4), (B, S), (B, S, L), (B, S), (B, S), (B, G), (B, G + 1), (B, E)), lead=True)
SCORE_TABLE = Layout("score table", (("meta", "int32"), ("gt_norm", "int32"), ("gt_norm_len", "int32"), ("gt_score", "float32"), ("gt_raw", "int32"),
                                     ("gt_raw_len", "int32"), ("ocr", "int32"), ("ocr_len", "int32")),
                     lambda B, A, Lg, No, Lw: ((B, 4), (B, A, Lg), (B, A), (B, A), (B, A, Lg), (B, A), (B, No, Lw), (B, No)), lead=True)
EVAL_BEAMS = Layout("eval_beams result", (("beam_scores", "float32"), ("beam_flags", "int32"), ("best", "int32"), ("best_ids", "int64"), ("best_scores", "float32"),
                                          ("best_flags", "int32"), ("oracle", "float32"), ("answer", "int32"), ("answer_len", "int32")),
                    lambda B, K, L, Lw: ((B * K, 3), (B * K,), (B,), (B, L), (B, 3), (B,), (B, 3), (B, L * (Lw + 1)), (B,)))
# sam_eval_beams_merged's sixteen outputs: EVAL_BEAMS' nine, then every beam's string, its group's leader and mass, and per question the number of groups,
# the beam sam_eval_beams would have kept and the winning group's mass
EVAL_MERGED = Layout("eval_beams_merged result", EVAL_BEAMS.fields + (("beam_answer", "int32"), ("beam_answer_len", "int32"), ("group", "int32"), ("mass", "float32"),
                                                                      ("n_groups", "int32"), ("plain_best", "int32"), ("best_mass", "float32")),
                     lambda B, K, L, Lw: EVAL_BEAMS._shapes(B=B, K=K, L=L, Lw=Lw) + ((B * K, L * (Lw + 1)), (B * K,), (B * K,), (B * K,), (B,), (B,), (B,)))
EVAL_BOARD = Layout("evaluation board", (("scores", "float32"), ("oracle", "float32"), ("flags", "int32"), ("best", "int32"), ("answer", "int32"),
                                         ("answer_len", "int32"), ("seen", "int32"), ("status", "int32")),
                    lambda n, P: ((n, 3), (n, 3), (n,), (n,), (n, P), (n,), (n,), (1,)))
# what sam_answer_witness writes for B samples of A answers at decoding length L (sources: vocabulary, OCR, both)
WITNESS = Layout("witness", (("words", "int32"), ("reach", "int32"), ("any", "int32"), ("seqs", "int64"), ("counts", "int32")),
                 lambda B, A, L: ((B, A), (3, B, A), (3, B), (3, B * A, L), (B, 4)))
ANSWER_TABLE_OUT, SCORE_TABLE_OUT = ANSWER_TABLE.with_status(), SCORE_TABLE.with_status()          # what the two sam_*_table_from_text write
# the six eval_beams outputs a board row holds, in the order of EVAL_BOARD's first six keys, for B slots of answer width P = L * (Lw + 1)
EVAL_ROWS = Layout("result rows", [(k, dict(EVAL_BEAMS.fields)[k]) for k in ("best_scores", "oracle", "best_flags", "best", "answer", "answer_len")],
                   lambda B, P: ((B, 3), (B, 3), (B,), (B,), (B, P), (B,)))

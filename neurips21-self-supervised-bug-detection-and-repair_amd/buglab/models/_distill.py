"""Knowledge distillation in NumPy fp64: the twin of csrc/bl_distill.hip, operation for operation (the kernels are compiled
without fused multiply-adds, so the two differ only in exp / log and in the order of the sums).  The tests pin the kernels to
it and it to a torch autograd restatement; tools/distill_bench.py and the end-to-end test measure a student's distance to its
teacher with it.  No GPU, no library.

Per segment, with the student's logits z, the teacher's log-probabilities t and a temperature tau:
    a = z / tau, ms = max a, Ss = sum exp(a - ms):                 log q = (a - ms) - log Ss,  q = exp(a - ms) / Ss
    u = t / tau over the entries with t > -inf, mt, St likewise:   log p = (u - mt) - log St,  p = exp(u - mt) / St
    KL = sum over p > 0 of p (log p - log q);   delta = q - p   (p = 0 where t is -inf or NaN).
d KL / d z_i = delta_i / tau.  A segment without a teacher entry above -inf is skipped: KL 0, delta 0, counted.

A location segment of graph b is its candidate rows candidate_ptr[b] .. candidate_ptr[b + 1] followed by NO_BUG, whose student
logit is the constant 1.0 (localizationmodule.py:63-77) and whose teacher value sits at teacher_loc[C + b]; a repair segment is
a group of the CSR the repair log-softmax runs over (gnn.py:295-299)."""
from __future__ import annotations

from typing import NamedTuple, Optional, Tuple

import numpy as np

NO_BUG_LOGIT = 1.0


class SegmentTerms(NamedTuple):
    kl: float
    delta: np.ndarray      # float64 [n]
    distilled: bool
    agree: bool            # the student's first maximum is the teacher's


def _first_max(v: np.ndarray, counts: np.ndarray) -> int:
    """The index of the first maximum of v among the entries that count; -1 if none does."""
    idx = np.flatnonzero(counts)
    if idx.size == 0:
        return -1
    return int(idx[np.argmax(v[idx])])  # np.argmax returns the first of equal maxima


def segment_terms(z: np.ndarray, t: np.ndarray, tau: float) -> SegmentTerms:
    """One segment: z float [n] student logits, t float [n] teacher log-probabilities (-inf allowed)."""
    z = np.asarray(z, dtype=np.float64)
    t = np.asarray(t, dtype=np.float64)
    n = z.shape[0]
    with np.errstate(invalid="ignore"):
        counts = t > -np.inf  # False for -inf and NaN
    it = _first_max(t / tau, counts)
    if it < 0:
        return SegmentTerms(0.0, np.zeros(n), False, False)
    a = z / tau
    is_ = _first_max(a, np.ones(n, dtype=bool))
    ms, mt = a[is_], (t / tau)[it]
    da = a - ms
    ea = np.exp(da)
    ss = ea.sum()
    q = ea / ss
    du = np.where(counts, t, 0.0) / tau - mt
    eu = np.where(counts, np.exp(du), 0.0)
    st = eu.sum()
    p = eu / st
    ls, lt = np.log(ss), np.log(st)
    pos = p > 0.0
    kl = float((p[pos] * ((du[pos] - lt) - (da[pos] - ls))).sum())
    return SegmentTerms(kl, q - p, True, is_ == it)


class DistillOutput(NamedTuple):
    kl_loc: float
    kl_rep: float
    delta: np.ndarray              # float64 [C + R]: candidates | logits (what the kernel rounds to fp32)
    distilled_loc: int
    distilled_rep: int
    agreement: int
    skipped: int
    seg_kl: np.ndarray             # float64 [B + G]: every segment's own KL

    def out8(self) -> np.ndarray:
        """bl_distill_fwd's out[8], rounded once to fp32."""
        return np.asarray([self.kl_loc, self.kl_rep, self.distilled_loc, self.distilled_rep, self.agreement, self.skipped, 0, 0],
                          dtype=np.float64).astype(np.float32)


def distill_terms(loc_scores, repair_logits, teacher_loc, teacher_repair, candidate_ptr, repair_group_ptr, repair_group_items,
                  tau: float) -> DistillOutput:
    """bl_distill_fwd in NumPy.  The sums run over the segments in ascending order (the kernel's fixed tree differs from it
    by the rounding of an fp64 sum of B + G terms)."""
    loc_scores = np.asarray(loc_scores, dtype=np.float64).reshape(-1)
    repair_logits = np.asarray(repair_logits, dtype=np.float64).reshape(-1)
    teacher_loc = np.asarray(teacher_loc, dtype=np.float64).reshape(-1)
    teacher_repair = np.asarray(teacher_repair, dtype=np.float64).reshape(-1)
    cptr = np.asarray(candidate_ptr, dtype=np.int64)
    gptr = np.asarray(repair_group_ptr, dtype=np.int64)
    items = np.asarray(repair_group_items, dtype=np.int64)
    C, R, B, G = loc_scores.shape[0], repair_logits.shape[0], cptr.shape[0] - 1, gptr.shape[0] - 1
    if teacher_loc.shape[0] != C + B or teacher_repair.shape[0] != R:
        raise ValueError(f"distill_terms: teacher_loc has {teacher_loc.shape[0]} entries for {C} candidates + {B} graphs and "
                         f"teacher_repair {teacher_repair.shape[0]} for {R} logits")
    if tau <= 0:
        raise ValueError("distill_terms: the temperature must be > 0")
    delta = np.zeros(C + R)
    seg_kl = np.zeros(B + G)
    n_loc = n_rep = agree = skipped = 0
    for b in range(B):
        c0, c1 = int(np.clip(cptr[b], 0, C)), int(np.clip(cptr[b + 1], 0, C))
        c1 = max(c0, c1)
        z = np.concatenate([loc_scores[c0:c1], [NO_BUG_LOGIT]])
        t = np.concatenate([teacher_loc[c0:c1], [teacher_loc[C + b]]])
        terms = segment_terms(z, t, tau)
        delta[c0:c1] = terms.delta[:-1]
        seg_kl[b] = terms.kl
        n_loc += terms.distilled
        agree += terms.agree
        skipped += not terms.distilled
    for g in range(G):
        g0, g1 = int(np.clip(gptr[g], 0, R)), int(np.clip(gptr[g + 1], 0, R))
        at = items[g0:max(g0, g1)]
        at = at[(at >= 0) & (at < R)]
        terms = segment_terms(repair_logits[at], teacher_repair[at], tau)
        delta[C + at] = terms.delta
        seg_kl[B + g] = terms.kl
        n_rep += terms.distilled
        skipped += (not terms.distilled) and g1 > g0  # an empty group is neither distilled nor skipped
    return DistillOutput(float(seg_kl[:B].sum()), float(seg_kl[B:].sum()), delta, n_loc, n_rep, agree, skipped, seg_kl)


def distill_grads(delta, num_candidates: int, g_loc: float, g_rep: float, tau: float) -> Tuple[np.ndarray, np.ndarray]:
    """bl_distill_bwd in NumPy on the fp32 delta the forward wrote: -> (g_loc_scores, g_repair_logits), rounded once to fp32."""
    d = np.asarray(delta, dtype=np.float32).astype(np.float64)
    C = int(num_candidates)
    return ((np.float64(np.float32(g_loc)) * d[:C] / tau).astype(np.float32),
            (np.float64(np.float32(g_rep)) * d[C:] / tau).astype(np.float32))


def location_kl(teacher_logprobs, student_logprobs, tau: float = 1.0) -> float:
    """KL(teacher || student) of one sample's location distribution, both given as log-probabilities in the same order
    (`predict`'s canonical order).  The student's log-probabilities serve as its logits: a log-softmax is shift-invariant."""
    return segment_terms(np.asarray(student_logprobs, np.float64), np.asarray(teacher_logprobs, np.float64), tau).kl


def entropy(logprobs) -> float:
    """The entropy of a distribution given as log-probabilities (entries at -inf contribute 0)."""
    lp = np.asarray(logprobs, dtype=np.float64)
    fin = lp > -np.inf
    return float(-(np.exp(lp[fin]) * lp[fin]).sum())

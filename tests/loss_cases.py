"""Shared by tests/test_loss_cases_host.py and tests/test_loss_heads_gpu.py: handmade inputs of the loss assembly
(include/buglab_hip.h, bl_bug_loss_t) at the shapes where csrc/bl_loss.hip changes path, and a restatement of its arithmetic
in plain torch ops with autograd.  In float64 the restatement is the reference; in float32 it is the measuring stick of the
tolerances (`case_err32`, `bound_of`).  Nothing here imports the code under test."""
from __future__ import annotations

import math
from typing import NamedTuple

import numpy as np
import torch

LOG_0995 = math.log(0.995)  # localizationmodule.py:93
LSM_EPS = 1e-12             # utils.py:27
LOSS_WAVES = 16             # graphs / groups the one workgroup of the loss kernels walks at a time
LOSS_THREADS = 1024
MARGIN = 1e-3               # distance every case keeps from a decision the kernel takes in fp32
BASELINE_BOUND = 1e-4       # BASELINE.json: the project's bound against the fp64 oracle

# bl_bug_loss_fwd's stats, in the order of the header comment
STATS = ("B", "loc_ok", "nobug", "nobug_ok", "loc_nll", "text_ok", "text_n", "var_ok", "var_n", "swap_ok", "swap_n", "loss",
         "repair_loss", "has_bug", "batches", "unused")
COUNT_STATS = ("B", "loc_ok", "nobug", "nobug_ok", "text_ok", "text_n", "var_ok", "var_n", "swap_ok", "swap_n", "has_bug", "batches",
               "unused")
SUM_STATS = ("loc_nll", "loss", "repair_loss")

W_BUGGY = (1.0, 2.5, 0.4)
ABSTAIN = (0.0, 0.35)
G_LOSS = (1.0, 0.37)
GRID = tuple((w, a, g) for w in W_BUGGY for a in ABSTAIN for g in G_LOSS)


def f32(v: float) -> float:
    """the value a float field of the descriptor holds"""
    return float(np.float32(v))


def csr_from_index(index, num_segments: int):
    """CSR (ptr int32 [n + 1], items int32 [len(index)]) of a segment-id vector: items ascending inside a segment"""
    index = np.asarray(index, dtype=np.int64).reshape(-1)
    assert index.size == 0 or (0 <= index.min() and index.max() < num_segments)
    ptr = np.zeros(num_segments + 1, dtype=np.int32)
    ptr[1:] = np.cumsum(np.bincount(index, minlength=num_segments))
    return ptr, np.argsort(index, kind="stable").astype(np.int32)


class LossCase(NamedTuple):
    name: str
    B: int
    C: int
    sizes: tuple              # (Rt, Rv, Rs)
    G: int
    loc_scores: np.ndarray    # float32 [C]
    repair_logits: np.ndarray  # float32 [Rt + Rv + Rs]
    cand_graph: np.ndarray    # int64 [C]: graph of every candidate row (ascending)
    loc_index: np.ndarray     # int64 [C + B]: graph of every item of the location log-softmax (candidates, then NO_BUG slots)
    loc_group_ptr: np.ndarray
    loc_group_items: np.ndarray
    candidate_ptr: np.ndarray
    has_bug: np.ndarray       # bool [B]
    correct_candidate_idxs: np.ndarray  # int32 [B]: candidate ROW of the bug (a valid row where has_bug is false too: never read)
    repair_index: np.ndarray  # int64 [R]: location group of every logit = cat(logit_group)
    repair_group_ptr: np.ndarray
    repair_group_items: np.ndarray
    logit_group: tuple        # 3 x int32 [Rk]
    target: tuple             # 3 x int32 [ntarget k]: indices into fixer k's slice
    null_fixers: tuple        # fixers whose target / logit_group pointers are NULL in the descriptor (ntarget 0)

    @property
    def R(self):
        return int(sum(self.sizes))

    @property
    def max_abs_score(self):
        return max([0.0] + [float(np.abs(a).max()) for a in (self.loc_scores, self.repair_logits) if a.size])


class LossRef(NamedTuple):
    loc_logprobs: torch.Tensor
    repair_logprobs: torch.Tensor
    group_max: torch.Tensor
    loss: torch.Tensor
    stats: torch.Tensor
    g_loc_scores: torch.Tensor
    g_repair_logits: torch.Tensor


# ------------------------------------------------------------------------------------------------ the restatement
def segment_log_softmax_ref(x, index, nseg, eps=LSM_EPS):
    """x - max - log(sum exp(x - max) + eps) per segment (utils.py:15-28); no gradient through the max"""
    if x.numel() == 0:
        return x
    m = torch.full((nseg,), -math.inf, dtype=x.dtype).scatter_reduce(0, index, x.detach(), reduce="amax", include_self=True)
    rec = x - m[index]
    s = torch.zeros(nseg, dtype=x.dtype).index_add(0, index, rec.exp())
    return rec - (s + eps).log()[index]


def segment_max_ref(x, index, nseg):
    return torch.full((nseg,), -math.inf, dtype=x.dtype).scatter_reduce(0, index, x.detach(), reduce="amax", include_self=True)


def first_argmax_ref(x, index, nseg):
    """the lowest item among a segment's maxima (x.numel() for an empty segment)"""
    m = segment_max_ref(x, index, nseg)
    items = torch.arange(x.numel(), dtype=torch.int64)
    cand = torch.where(x.detach() == m[index], items, torch.full_like(items, x.numel()))
    return torch.full((nseg,), x.numel(), dtype=torch.int64).scatter_reduce(0, index, cand, reduce="amin", include_self=True)


def seq_sum(x):
    """x[0] + x[1] + ... in that order, in x's dtype (torch.sum adds in blocks, cumsum in a wider type: neither is the plain
    sequential float32 sum the tolerances are measured with)"""
    s = torch.zeros((), dtype=x.dtype)
    for v in x:
        s = s + v
    return s


def loss_ref(case: LossCase, w_buggy: float, abstain: float, g_loss: float = 1.0, dtype=torch.float64) -> LossRef:
    """What bl_bug_loss_fwd / _bwd compute, from the same float32 inputs, in `dtype`.  w_buggy, abstain and g_loss are taken as
    the float32 values the kernels receive."""
    w_buggy, abstain, g_loss = f32(w_buggy), f32(abstain), f32(g_loss)
    B, C, G = case.B, case.C, case.G
    x = torch.tensor(case.loc_scores, dtype=dtype).requires_grad_(True)
    r = torch.tensor(case.repair_logits, dtype=dtype).requires_grad_(True)
    has_bug = torch.tensor(case.has_bug)
    arange = torch.arange(B, dtype=torch.int64)
    loc_index = torch.tensor(case.loc_index)
    # localization: the candidates, then one NO_BUG slot of value 1.0 per graph
    items = torch.cat([x, torch.ones(B, dtype=dtype)])
    loc_lp = segment_log_softmax_ref(items, loc_index, B)
    correct = torch.where(has_bug, torch.tensor(case.correct_candidate_idxs).long(), C + arange)
    lp = loc_lp[correct].clamp(max=LOG_0995)
    if abstain > 0:
        lp = lp + torch.where(has_bug, abstain * loc_lp[C + arange], torch.zeros_like(lp))
    if w_buggy == 1.0:
        loc_loss = -seq_sum(lp) / B
    else:
        w = torch.where(has_bug, torch.full_like(lp, w_buggy), torch.ones_like(lp))
        loc_loss = -seq_sum(lp * w) / seq_sum(w)
    pred = first_argmax_ref(loc_lp, loc_index, B)  # candidates come before the NO_BUG slot, lower rows first
    ok = pred == correct
    # repair: one log-softmax of the three fixers' logits over the location groups
    repair_index = torch.tensor(case.repair_index)
    rep_lp = segment_log_softmax_ref(r, repair_index, G)
    gmax = segment_max_ref(r, repair_index, G) if case.R else torch.full((G,), -math.inf, dtype=dtype)
    is_max = r.detach() == gmax[repair_index] if case.R else torch.zeros(0, dtype=torch.bool)
    nll, hits, off = [], [], 0
    for k in range(3):
        t = torch.tensor(case.target[k]).long() + off
        nll.append(-seq_sum(rep_lp[t]))
        hits.append(float(is_max[t].sum()))
        off += case.sizes[k]
    repair = ((nll[0] + nll[1]) + nll[2]) * w_buggy
    loss = loc_loss + repair / B
    g_x, g_r = torch.autograd.grad(loss, [x, r], grad_outputs=torch.tensor(g_loss, dtype=dtype), allow_unused=True)
    g_x = torch.zeros_like(x) if g_x is None else g_x
    g_r = torch.zeros_like(r) if g_r is None else g_r
    nobug = ~has_bug
    stats = torch.tensor([B, float(ok.sum()), float(nobug.sum()), float((nobug & ok).sum()), float(-seq_sum(lp.detach())),
                          hits[0], len(case.target[0]), hits[1], len(case.target[1]), hits[2], len(case.target[2]),
                          float(loss.detach()), float(repair.detach()), float(has_bug.sum()), 1.0, 0.0], dtype=dtype)
    return LossRef(loc_lp.detach(), rep_lp.detach(), gmax, loss.detach(), stats, g_x, g_r)


# ------------------------------------------------------------------------------------------------ tolerances
def _maxdiff(a, b):
    a, b = a.double(), b.double()
    if a.numel() == 0:
        return 0.0
    same = (a == b) | (torch.isnan(a) & torch.isnan(b))  # (-inf == -inf: the group_max of an empty group)
    return float(torch.where(same, torch.zeros_like(a), (a - b).abs()).max())


def abs_bound(ref32, ref64):
    """(err32, bound): the float32 restatement's own distance from float64, and 4 x that + 1e-6 -- the kernel sums in butterfly
    order where torch sums sequentially, and the device's expf / logf are good to about 2 ulp where the host's round correctly"""
    err32 = _maxdiff(ref32, ref64)
    return err32, 4.0 * err32 + 1e-6


def rel_bound(ref32, ref64):
    """(err32 relative to the largest fp64 entry, absolute bound, scale) for a gradient: (4 x err32 + 1e-6) x scale"""
    scale = float(ref64.abs().max()) if ref64.numel() else 0.0
    err32 = _maxdiff(ref32, ref64) / scale if scale > 0 else 0.0
    return err32, (4.0 * err32 + 1e-6) * scale, scale


ABS_FIELDS = ("loc_logprobs", "repair_logprobs", "group_max", "loss", "stats")
REL_FIELDS = ("g_loc_scores", "g_repair_logits")
_ERR32 = {}


def case_err32(name: str) -> dict:
    """err32 of every compared quantity of a case: the largest distance of the float32 restatement from the float64 one over the
    case's runs (GRID) and over the entries of the quantity (`stats` is one quantity); for the gradients relative to the largest
    fp64 entry of the run.  One run's own err32 of a single number can be next to nothing by luck."""
    if name not in _ERR32:
        worst = dict.fromkeys(ABS_FIELDS + REL_FIELDS, 0.0)
        for w_buggy, abstain, g_loss in GRID:
            r64, r32 = get_ref(name, w_buggy, abstain, g_loss), get_ref(name, w_buggy, abstain, g_loss, torch.float32)
            for f in ABS_FIELDS:
                worst[f] = max(worst[f], abs_bound(getattr(r32, f), getattr(r64, f))[0])
            for f in REL_FIELDS:
                worst[f] = max(worst[f], rel_bound(getattr(r32, f), getattr(r64, f))[0])
        _ERR32[name] = worst
    return _ERR32[name]


def bound_of(name: str, field: str, ref64) -> tuple:
    """(err32, absolute bound) of one quantity of one run of case `name`: 4 x err32 + 1e-6, times the largest fp64 entry for a gradient"""
    err32 = case_err32(name)[field]
    if field in REL_FIELDS:
        return err32, (4.0 * err32 + 1e-6) * (float(ref64.abs().max()) if ref64.numel() else 0.0)
    return err32, 4.0 * err32 + 1e-6


def max_error(got, ref64):
    return _maxdiff(got, ref64)


# ------------------------------------------------------------------------------------------------ the case builder
def uniform(lo, hi):
    return lambda rng, n: rng.uniform(lo, hi, n)


def spread_groups(group_sizes, sizes, rng):
    """logit -> group maps of the three fixers: `group_sizes[g]` logits in group g, shuffled, cut into slices of `sizes`"""
    ids = np.repeat(np.arange(len(group_sizes)), group_sizes)
    assert ids.size == sum(sizes)
    rng.shuffle(ids)
    cuts = np.cumsum([0] + list(sizes))
    return [ids[cuts[k]:cuts[k + 1]] for k in range(3)]


def _clear_margin(values, m):
    near = (values != m) & (values > m - np.float32(10 * MARGIN))
    values[near] -= np.float32(20 * MARGIN)


def build_case(name, cand_counts, has_bug, correct_local, logit_groups, targets, G, seed, loc_rule=uniform(-3, 3),
               rep_rule=uniform(-3, 3), loc_set=(), rep_set=(), null_fixers=(), target_boost=0.0, correct_boost=0.0) -> LossCase:
    """cand_counts [B]; has_bug [B]; correct_local [B]: the bug's candidate inside its graph (ignored without a bug);
    logit_groups / targets: one array per fixer (group of every logit; indices of the correct rewrites inside the slice);
    loc_rule / rep_rule(rng, n) draw the values, loc_set / rep_set = [(index, value)] overwrite some afterwards; target_boost is
    added to the logit of every correct rewrite (a model that has learnt something: it keeps the summed losses, and with them one
    float32 ulp of the sums, small), correct_boost to the score of every bug's candidate."""
    rng = np.random.default_rng(seed)
    cand_counts = np.asarray(cand_counts, dtype=np.int64)
    B, C = len(cand_counts), int(cand_counts.sum())
    has_bug = np.asarray(has_bug, dtype=bool)
    assert has_bug.shape == (B,) and len(correct_local) == B
    candidate_ptr = np.zeros(B + 1, dtype=np.int32)
    candidate_ptr[1:] = np.cumsum(cand_counts)
    correct = np.zeros(B, dtype=np.int32)
    for b in range(B):
        if has_bug[b]:
            assert 0 <= correct_local[b] < cand_counts[b], (name, b)
            correct[b] = candidate_ptr[b] + correct_local[b]
    cand_graph = np.repeat(np.arange(B), cand_counts)
    loc_index = np.concatenate([cand_graph, np.arange(B)])
    loc_group_ptr, loc_group_items = csr_from_index(loc_index, B)
    logit_group = tuple(np.asarray(g, dtype=np.int32).reshape(-1) for g in logit_groups)
    target = tuple(np.asarray(t, dtype=np.int32).reshape(-1) for t in targets)
    sizes = tuple(int(g.shape[0]) for g in logit_group)
    for k in range(3):
        assert target[k].size == 0 or (0 <= target[k].min() and target[k].max() < sizes[k]), (name, k)
        assert k not in null_fixers or target[k].size == 0
    repair_index = np.concatenate(logit_group).astype(np.int64)
    repair_group_ptr, repair_group_items = csr_from_index(repair_index, G)
    loc_scores = np.asarray(loc_rule(rng, C), dtype=np.float32)
    repair_logits = np.asarray(rep_rule(rng, sum(sizes)), dtype=np.float32)
    off = 0
    for k in range(3):
        repair_logits[off + np.unique(target[k])] += np.float32(target_boost[k] if isinstance(target_boost, tuple) else target_boost)
        off += sizes[k]
    loc_scores[correct[has_bug]] += np.float32(correct_boost)
    for i, v in loc_set:
        loc_scores[i] = v
    for i, v in rep_set:
        repair_logits[i] = v
    # a drawn value that happens to lie just under its group's maximum moves down, out of the margin (designed ties are bit-equal)
    for b in range(B):
        rows = slice(candidate_ptr[b], candidate_ptr[b + 1])
        _clear_margin(loc_scores[rows], max(np.float32(1.0), loc_scores[rows].max(initial=np.float32(1.0))))
    for g in range(G):
        items = repair_group_items[repair_group_ptr[g]:repair_group_ptr[g + 1]]
        if items.size:
            vals = repair_logits[items]
            _clear_margin(vals, vals.max())
            repair_logits[items] = vals
    case = LossCase(name, B, C, sizes, int(G), loc_scores, repair_logits, cand_graph, loc_index, loc_group_ptr, loc_group_items,
                    candidate_ptr, has_bug, correct, repair_index, repair_group_ptr, repair_group_items, logit_group, target,
                    tuple(null_fixers))
    check_conditions(case)
    return case


def _argmax_is_decided(values, what):
    """the maximum is either bit-equal to a competitor or more than MARGIN above it"""
    if values.size < 2:
        return
    m = values.max()
    rest = values[values != m]
    assert rest.size == 0 or float(m) - float(rest.max()) > MARGIN, f"{what}: two competitors of an arg-max lie within {MARGIN}"


def check_conditions(case: LossCase):
    """Every decision a kernel takes in fp32 is MARGIN away from going the other way in fp64: a case that drifts fails here,
    loudly, instead of flaking on the device."""
    ref = loss_ref(case, 1.0, 0.0)
    for b in range(case.B):
        items = case.loc_group_items[case.loc_group_ptr[b]:case.loc_group_ptr[b + 1]]
        assert items.size == case.candidate_ptr[b + 1] - case.candidate_ptr[b] + 1
        correct = int(case.correct_candidate_idxs[b]) if case.has_bug[b] else case.C + b
        assert correct in items, f"{case.name}: graph {b}'s correct item is not its own"
        lp = float(ref.loc_logprobs[correct])
        assert abs(lp - LOG_0995) > MARGIN, f"{case.name}: graph {b}'s correct log-probability {lp} is within {MARGIN} of log 0.995"
        values = np.array([case.loc_scores[i] if i < case.C else np.float32(1.0) for i in items], dtype=np.float32)
        _argmax_is_decided(values, f"{case.name}: graph {b}")
    for g in range(case.G):
        items = case.repair_group_items[case.repair_group_ptr[g]:case.repair_group_ptr[g + 1]]
        _argmax_is_decided(case.repair_logits[items], f"{case.name}: repair group {g}")
    for t in ref:
        assert not bool(torch.isnan(t).any()), case.name


# ------------------------------------------------------------------------------------------------ the cases
def _targets(rng, sizes, counts, replace=False):
    return [rng.choice(sizes[k], size=counts[k], replace=replace) if sizes[k] and counts[k] else np.zeros(0, np.int64) for k in range(3)]


def _mixed_bugs(cand_counts, rng):
    """about two of three graphs buggy (never one without candidates), the bug at a random candidate"""
    has_bug = np.array([c > 0 and (b % 3 != 2) for b, c in enumerate(cand_counts)])
    return has_bug, [int(rng.integers(0, c)) if c else 0 for c in cand_counts]


def case_boundary():
    """17 graphs -- one more than the kernel has waves -- whose location groups (candidates + NO_BUG) have 1, 2, 3, 63, 64,
    65, 66, 128, 129, 130, 201 items: both sides of the switch between the per-lane and the looping path, and loops of two,
    three and four rounds.  Repair groups of 3, 64, 65, 1, 0, 10."""
    rng = np.random.default_rng(101)
    counts = [0, 1, 2, 62, 63, 64, 65, 127, 128, 129, 200, 5, 5, 5, 5, 5, 5]
    has_bug, correct = _mixed_bugs(counts, rng)
    correct[4], correct[6], correct[10] = 62, 64, 199  # the last candidate of a full wave; the first item of a second round; the last of four
    sizes = (60, 50, 33)
    groups = spread_groups([3, 64, 65, 1, 0, 10], sizes, rng)
    return build_case("boundary", counts, has_bug, correct, groups, _targets(rng, sizes, (9, 7, 5)), 6, seed=102, target_boost=5.0)


def case_many_graphs():
    """33 graphs of 0 .. 9 candidates: every wave walks three graphs.  40 repair groups of 0, 1, 63, 64, 65 and 130 logits
    (and a few other sizes), ten of them empty: every wave walks three groups, on both paths."""
    rng = np.random.default_rng(201)
    counts = [int(c) for c in rng.integers(1, 10, 33)]
    counts[7], counts[20] = 0, 0
    has_bug, correct = _mixed_bugs(counts, rng)
    group_sizes = [0, 1, 63, 64, 65, 130] + [0, 3, 1, 64, 0, 7, 65, 2, 0, 1, 130, 5, 0, 63, 9, 0, 1, 64, 0, 2, 65, 4, 0, 11, 63, 0, 6, 1,
                                             0, 3, 8, 2, 5, 0]
    assert len(group_sizes) == 40
    total = sum(group_sizes)
    sizes = (total // 2, total // 3, total - total // 2 - total // 3)
    groups = spread_groups(group_sizes, sizes, rng)
    return build_case("many_graphs", counts, has_bug, correct, groups, _targets(rng, sizes, (8, 6, 4)), 40, seed=202, target_boost=4.0)


def case_long_lists():
    """C + B = 1324 items and 1300 logits: the kernels' thread-stride loops (zero fill, targets) go round twice.  The first fixer
    has 1500 targets that name 150 of its 700 logits, so a logit is the target about ten times: the backward kernel's atomicAdd
    adds to one address again and again.  Each of the 150 leads a small group of its own (groups 0 .. 149) by 12; the other two
    fixers share groups 150 .. 159 of some 60 logits, on both sides of 64."""
    rng = np.random.default_rng(301)
    counts = [60] * 16 + [100, 100, 70, 70, 4, 0]
    has_bug, correct = _mixed_bugs(counts, rng)
    sizes = (700, 500, 100)
    groups = [np.concatenate([np.arange(150), rng.integers(0, 150, 550)]), rng.integers(150, 160, 500), rng.integers(150, 160, 100)]
    targets = [rng.integers(0, 150, 1500), rng.choice(500, 6, replace=False), rng.choice(100, 4, replace=False)]
    return build_case("long_lists", counts, has_bug, correct, groups, targets, 160, seed=302, target_boost=(12.0, 3.0, 3.0))


def _sparse(name, sizes, ntargets, G, seed, null_fixers=()):
    rng = np.random.default_rng(seed)
    counts = [4, 9, 0, 70, 3]
    has_bug, correct = _mixed_bugs(counts, rng)
    groups = [rng.integers(0, G, n) if n else np.zeros(0, np.int64) for n in sizes]
    return build_case(name, counts, has_bug, correct, groups, _targets(rng, sizes, ntargets), G, seed=seed + 1, null_fixers=null_fixers,
                      target_boost=6.0, correct_boost=2.0)


def cases_sparse_fixers():
    """a fixer without logits (each in turn), a fixer with logits whose target list is empty and whose index pointers are NULL,
    and a minibatch without any repair logit or group"""
    return [_sparse("sparse_Rt0", (0, 30, 20), (0, 4, 3), 7, 401),
            _sparse("sparse_Rv0", (25, 0, 20), (3, 0, 3), 7, 411),
            _sparse("sparse_Rs0", (25, 30, 0), (3, 4, 0), 7, 421),
            _sparse("sparse_null_fixer", (25, 30, 20), (3, 0, 2), 7, 431, null_fixers=(1,)),
            _sparse("sparse_R0", (0, 0, 0), (0, 0, 0), 0, 441)]


def case_no_buggy_graph():
    rng = np.random.default_rng(501)
    counts = [5, 0, 12, 66, 3, 8]
    sizes = (12, 9, 6)
    groups = [rng.integers(0, 4, n) for n in sizes]
    return build_case("no_buggy_graph", counts, [False] * 6, [0] * 6, groups, [[], [], []], 4, seed=502, loc_rule=uniform(-4, 0))


def case_all_buggy():
    rng = np.random.default_rng(511)
    counts = [5, 1, 12, 66, 3, 8]
    sizes = (12, 9, 6)
    groups = [rng.integers(0, 4, n) for n in sizes]
    return build_case("all_buggy", counts, [True] * 6, [int(rng.integers(0, c)) for c in counts], groups,
                      _targets(rng, sizes, (3, 2, 1)), 4, seed=512, target_boost=6.0, correct_boost=2.0)


def case_wide_range():
    """scores uniform in [-30, 30]; graph 2: one candidate at 30, the others near -30 (60 below); graph 3, without a bug: every
    candidate exactly -30; repair group 0 spans -40 .. 40.  expf(x - max) vanishes next to the maximum's 1."""
    rng = np.random.default_rng(601)
    counts = [40, 70, 10, 30, 100, 5]
    ptr = np.concatenate([[0], np.cumsum(counts)])
    has_bug = [True, True, True, False, True, False]
    correct = [3, 65, 4, 0, 99, 0]
    loc_set = [(int(ptr[2]) + j, -30.0 + 0.05 * j) for j in range(10)] + [(int(ptr[2]) + 6, 30.0)]
    loc_set += [(int(ptr[3]) + j, -30.0) for j in range(30)]
    sizes = (40, 30, 20)
    groups = [rng.integers(1, 5, n) for n in sizes]
    for k, n in ((0, 9), (1, 8), (2, 4)):  # group 0: 21 logits from all three fixers
        groups[k][:n] = 0
    offs = (0, 40, 70)
    members = [offs[k] + j for k, n in ((0, 9), (1, 8), (2, 4)) for j in range(n)]
    rep_set = [(i, v) for i, v in zip(members, np.linspace(-40.0, 40.0, len(members)))]
    targets = [[0, 8, 20], [0, 7, 11], [3, 9]]  # the bottom (-40) and the top (+40, fixer 2's index 3) of group 0 among them
    return build_case("wide_range", counts, has_bug, correct, groups, targets, 5, seed=602, loc_rule=uniform(-30, 30),
                      rep_rule=uniform(-30, 30), loc_set=loc_set, rep_set=rep_set)


def case_ties():
    """graph 0 (bug at row 3): rows 3 and 7 hold the same maximum -> row 3 is predicted: right
    graph 1 (bug at its row 7): the same values -> its row 3 is predicted: wrong
    graph 2 (no bug): its best candidate is exactly 1.0f, the NO_BUG logit -> the candidate is predicted: wrong
    graph 3 (no bug): its best candidate is 0.5 -> NO_BUG is predicted: right
    graph 4 (bug at row 5, 100 candidates, looping path): rows 5 and 70 hold the same maximum, in different lanes and rounds: right
    graph 5 (bug at row 70 of the same values): wrong
    graph 6 (bug at row 2): the candidate at exactly 1.0f is the bug and ties NO_BUG: right
    repair group 0: two equal maxima, both targets -> two hits; group 1: two equal maxima, one a target, and a target that is
    not a maximum -> one hit; group 2 (70 logits): equal maxima 64 items apart, both targets (one of them twice) -> three hits."""
    rng = np.random.default_rng(701)
    counts = [10, 10, 6, 6, 100, 100, 4]
    ptr = np.concatenate([[0], np.cumsum(counts)])
    has_bug = [True, True, False, False, True, True, True]
    correct = [3, 7, 0, 0, 5, 70, 2]
    loc_set = []
    for b in (0, 1):
        loc_set += [(int(ptr[b]) + 3, 2.5), (int(ptr[b]) + 7, 2.5)]
    loc_set += [(int(ptr[2]) + 4, 1.0), (int(ptr[3]) + 1, 0.5), (int(ptr[6]) + 2, 1.0)]
    for b in (4, 5):
        loc_set += [(int(ptr[b]) + 5, 2.75), (int(ptr[b]) + 70, 2.75)]
    # fixer 0: 10 logits of group 0; fixer 1: 10 logits of group 1; fixer 2: 70 logits of group 2
    groups = [np.zeros(10, np.int64), np.ones(10, np.int64), np.full(70, 2, np.int64)]
    rep_set = [(2, 1.5), (6, 1.5), (10 + 1, 1.25), (10 + 8, 1.25), (20 + 3, 1.75), (20 + 67, 1.75)]
    targets = [[2, 6], [8, 4], [3, 67, 67]]
    case = build_case("ties", counts, has_bug, correct, groups, targets, 3, seed=702, loc_rule=uniform(-3, 0.4),
                      rep_rule=uniform(-6, -2), loc_set=loc_set, rep_set=rep_set)
    stats = dict(zip(STATS, loss_ref(case, 1.0, 0.0).stats.tolist()))
    assert (stats["loc_ok"], stats["nobug_ok"], stats["text_ok"], stats["var_ok"], stats["swap_ok"]) == (4, 1, 2, 1, 3), stats
    return case


def case_clamp():
    """graph 0 (bug): the correct candidate is 12 above the rest: its log-probability is about -1e-4, above log 0.995 = -5e-3, so
    it is clamped and passes no gradient (with an abstain weight its NO_BUG slot still does)
    graph 1 (bug): the correct candidate is an ordinary one: far below the clamp
    graph 2 (no bug): every candidate is near -8: NO_BUG's log-probability is above the clamp
    graph 3 (no bug): ordinary
    graph 4 (bug, 80 candidates, looping path): clamped like graph 0"""
    counts = [8, 8, 5, 7, 80]
    ptr = np.concatenate([[0], np.cumsum(counts)])
    has_bug = [True, True, False, False, True]
    correct = [2, 5, 0, 0, 77]
    loc_set = [(int(ptr[0]) + 2, 14.0), (int(ptr[4]) + 77, 16.0)] + [(int(ptr[2]) + j, -8.0 - 0.125 * j) for j in range(5)]
    case = build_case("clamp", counts, has_bug, correct, [[0, 0, 1], [1, 0], [1]], [[1], [0], [0]], 2, seed=801, loc_set=loc_set)
    lp = loss_ref(case, 1.0, 0.0).loc_logprobs
    assert float(lp[ptr[0] + 2]) > LOG_0995 + MARGIN and float(lp[ptr[4] + 77]) > LOG_0995 + MARGIN
    assert float(lp[ptr[1] + 5]) < LOG_0995 - 0.1 and float(lp[case.C + 2]) > LOG_0995 + MARGIN and float(lp[case.C + 3]) < LOG_0995 - 0.1
    return case


def all_cases():
    return ([case_boundary(), case_many_graphs(), case_long_lists()] + cases_sparse_fixers()
            + [case_no_buggy_graph(), case_all_buggy(), case_wide_range(), case_ties(), case_clamp()])


CASE_NAMES = ("boundary", "many_graphs", "long_lists", "sparse_Rt0", "sparse_Rv0", "sparse_Rs0", "sparse_null_fixer", "sparse_R0",
              "no_buggy_graph", "all_buggy", "wide_range", "ties", "clamp")
_CACHE = {}


def get_case(name: str) -> LossCase:
    """the cases are built once and shared; nothing may write into their arrays"""
    if not _CACHE:
        for case in all_cases():
            for a in case:
                if isinstance(a, np.ndarray):
                    a.setflags(write=False)
            _CACHE[case.name] = case
        assert tuple(_CACHE) == CASE_NAMES
    return _CACHE[name]


_REFS = {}


def get_ref(name: str, w_buggy: float, abstain: float, g_loss: float, dtype=torch.float64) -> LossRef:
    key = (name, w_buggy, abstain, g_loss, dtype)
    if key not in _REFS:
        _REFS[key] = loss_ref(get_case(name), w_buggy, abstain, g_loss, dtype)
    return _REFS[key]

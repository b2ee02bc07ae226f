"""CPU: the handmade loss cases of tests/loss_cases.py and their fp64 restatement are what tests/test_loss_heads_gpu.py holds the
kernels of csrc/bl_loss.hip against, so they are checked here first, on any machine: the restatement against the oracle chain the
model-level parity tests trust, the CSR arrays against the collator's, and the margins every case promises."""
import math

import numpy as np
import pytest
import torch

from oracle import buglab_oracle as O
from tests import loss_cases as L


def _oracle_chain(case, w_buggy, abstain, g_loss):
    """oracle.buglab_oracle's scatter_log_softmax / scatter_max_with_arg, the clamp / abstain / weighting lines of its
    localization_loss and the repair assembly of its forward_loss, applied to the case's scores without the scorers"""
    w_buggy, abstain, g_loss = L.f32(w_buggy), L.f32(abstain), L.f32(g_loss)
    B, C = case.B, case.C
    x = torch.tensor(case.loc_scores, dtype=torch.float64).requires_grad_(True)
    r = torch.tensor(case.repair_logits, dtype=torch.float64).requires_grad_(True)
    has_bug = torch.tensor(case.has_bug)
    arange = torch.arange(B, dtype=torch.int64)
    all_scores = torch.cat([x, torch.ones(B, dtype=x.dtype)])                  # localization_logprobs
    all_idx = torch.cat([torch.tensor(case.cand_graph), arange])
    logprobs = O.scatter_log_softmax(all_scores, all_idx)
    correct = torch.where(has_bug, torch.tensor(case.correct_candidate_idxs).long(), arange + C)  # localization_loss
    lp = logprobs[correct].clamp(max=math.log(0.995))
    if abstain > 0:
        lp = lp + torch.where(has_bug, abstain * logprobs[arange + C], torch.zeros_like(lp))
    if w_buggy == 1.0:
        loc_loss = -lp.mean()
    else:
        w = torch.where(has_bug, torch.full_like(lp, w_buggy), torch.ones_like(lp))
        loc_loss = -(lp * w).sum() / w.sum()
    pred = O.scatter_max_with_arg(logprobs.detach(), all_idx, B)[1]
    ok = pred == correct
    groups = torch.cat([torch.tensor(g).long() for g in case.logit_group])      # repair_logprobs
    rep_lp = O.scatter_log_softmax(r, groups) if r.numel() else r
    if r.numel():
        ng = int(groups.max()) + 1
        gmax = O.scatter_max_with_arg(r.detach(), groups, ng)[0]
        sel = gmax.gather(0, groups) == r.detach()
    else:
        gmax, sel = torch.zeros(0, dtype=torch.float64), torch.zeros(0, dtype=torch.bool)
    lps, sels = torch.split(rep_lp, list(case.sizes)), torch.split(sel, list(case.sizes))
    t = [torch.tensor(a).long() for a in case.target]
    losses = [-lps[k][t[k]] for k in range(3)]                                   # forward_loss
    repair = (losses[0].sum() + losses[1].sum() + losses[2].sum()) * w_buggy
    loss = loc_loss + repair / B
    (loss * g_loss).backward()
    hits = [float(sels[k][t[k]].sum()) for k in range(3)]
    nobug = ~has_bug
    stats = [B, float(ok.sum()), float(nobug.sum()), float((nobug & ok).sum()), float(-lp.detach().sum()), hits[0], len(t[0]), hits[1],
             len(t[1]), hits[2], len(t[2]), float(loss.detach()), float(repair.detach()), float(has_bug.sum()), 1.0, 0.0]
    zeros = torch.zeros_like
    return (logprobs.detach(), rep_lp.detach(), gmax, loss.detach(), torch.tensor(stats, dtype=torch.float64),
            zeros(x) if x.grad is None else x.grad, zeros(r) if r.grad is None else r.grad)


@pytest.mark.parametrize("name", L.CASE_NAMES)
def test_restatement_agrees_with_the_oracle_chain(name):
    case = L.get_case(name)
    for w_buggy, abstain, g_loss in L.GRID:
        ref = L.get_ref(name, w_buggy, abstain, g_loss)
        loc_lp, rep_lp, gmax, loss, stats, g_x, g_r = _oracle_chain(case, w_buggy, abstain, g_loss)
        what = (name, w_buggy, abstain, g_loss)
        assert L.max_error(ref.loc_logprobs, loc_lp) <= 1e-12, what
        assert L.max_error(ref.repair_logprobs, rep_lp) <= 1e-12, what
        # the oracle's scatter_max stops at the last non-empty group and reports 0 for an empty one; the kernel's contract is -inf
        sizes = np.diff(case.repair_group_ptr)
        for g in range(case.G):
            if sizes[g]:
                assert float(ref.group_max[g]) == float(gmax[g]), what
            else:
                assert float(ref.group_max[g]) == -math.inf, what
        assert abs(float(ref.loss) - float(loss)) <= 1e-12 * max(1.0, abs(float(loss))), what
        assert L.max_error(ref.stats, stats) <= 1e-12 * max(1.0, float(stats.abs().max())), (what, ref.stats, stats)
        assert L.max_error(ref.g_loc_scores, g_x) <= 1e-12, what
        assert L.max_error(ref.g_repair_logits, g_r) <= 1e-12, what


@pytest.mark.parametrize("name", L.CASE_NAMES)
def test_csr_arrays_are_the_collators(name):
    from buglab.data.collate import segments_from_index

    case = L.get_case(name)
    ptr, items = segments_from_index(case.loc_index, case.B)
    assert ptr.dtype == case.loc_group_ptr.dtype == np.int32 and items.dtype == case.loc_group_items.dtype == np.int32
    assert np.array_equal(ptr, case.loc_group_ptr) and np.array_equal(items, case.loc_group_items)
    ptr, items = segments_from_index(case.repair_index, case.G)
    assert ptr.dtype == case.repair_group_ptr.dtype == np.int32 and items.dtype == case.repair_group_items.dtype == np.int32
    assert np.array_equal(ptr, case.repair_group_ptr) and np.array_equal(items, case.repair_group_items)
    assert np.array_equal(np.diff(case.candidate_ptr), np.bincount(case.cand_graph, minlength=case.B))
    assert np.array_equal(case.repair_index, np.concatenate(case.logit_group))


@pytest.mark.parametrize("name", L.CASE_NAMES)
def test_case_keeps_its_margins(name):
    case = L.get_case(name)
    L.check_conditions(case)
    assert case.loc_scores.dtype == np.float32 and case.repair_logits.dtype == np.float32
    assert case.has_bug.dtype == np.bool_ and case.correct_candidate_idxs.dtype == np.int32
    # every index is valid: no case provokes an access out of bounds
    assert case.C == 0 or (0 <= case.correct_candidate_idxs.min() and case.correct_candidate_idxs.max() < case.C)
    assert sorted(case.loc_group_items.tolist()) == list(range(case.C + case.B))
    assert sorted(case.repair_group_items.tolist()) == list(range(case.R))
    for k in range(3):
        assert case.logit_group[k].shape == (case.sizes[k],)
        assert case.target[k].size == 0 or (0 <= case.target[k].min() and case.target[k].max() < case.sizes[k])


def test_cases_reach_the_paths_they_are_meant_for():
    loc = {n: np.diff(L.get_case(n).loc_group_ptr) for n in L.CASE_NAMES}
    rep = {n: np.diff(L.get_case(n).repair_group_ptr) for n in L.CASE_NAMES}
    assert loc["boundary"].tolist()[:11] == [1, 2, 3, 63, 64, 65, 66, 128, 129, 130, 201] and len(loc["boundary"]) == L.LOSS_WAVES + 1
    assert not L.get_case("boundary").has_bug[0] and 0 < L.get_case("boundary").has_bug.sum() < 17
    many = L.get_case("many_graphs")
    assert many.B == 33 and many.G == 40 and {0, 1, 63, 64, 65, 130} <= set(rep["many_graphs"].tolist())
    assert (rep["many_graphs"] == 0).sum() >= 3
    long_ = L.get_case("long_lists")
    assert long_.C + long_.B > L.LOSS_THREADS and long_.R > L.LOSS_THREADS and len(long_.target[0]) == 1500
    assert np.bincount(long_.target[0]).max() > 1
    assert [L.get_case(n).sizes.index(0) for n in ("sparse_Rt0", "sparse_Rv0", "sparse_Rs0")] == [0, 1, 2]
    null = L.get_case("sparse_null_fixer")
    assert null.null_fixers == (1,) and null.sizes[1] > 0 and null.target[1].size == 0
    assert L.get_case("sparse_R0").R == 0 and L.get_case("sparse_R0").G == 0
    assert not L.get_case("no_buggy_graph").has_bug.any() and L.get_case("all_buggy").has_bug.all()
    wide = L.get_case("wide_range")
    items = wide.repair_group_items[wide.repair_group_ptr[0]:wide.repair_group_ptr[1]]
    assert float(np.ptp(wide.repair_logits[items])) == 80.0 and float(wide.loc_scores.min()) == -30.0 and float(wide.loc_scores.max()) == 30.0
    for n in L.CASE_NAMES:  # the 4 x err32 + 1e-6 rule stays inside the project's bound wherever the scores lie within +-30
        if L.get_case(n).max_abs_score > 30.0:
            continue
        for field, err32 in L.case_err32(n).items():
            assert 4.0 * err32 + 1e-6 <= L.BASELINE_BOUND, (n, field, err32)

"""CPU: the NumPy twin of the warning-grouping kernels (buglab/models/_group.py) against plain Python loops
(tests/group_cases.py: all pairs, fp64 dots in the stated order, a naive union-find), the filter's promise that no edge is lost,
and the host side of a grouping: representatives, ordering, records.

No tolerance anywhere: labels, degrees and counters are integers that the definition fixes."""
import numpy as np
import pytest

from tests import group_cases as GC
from tests import similar_cases as C


def _quantized(x, center=True):
    from buglab.models._similar import column_mean, quantize_host

    mean = column_mean(x) if center else np.zeros(x.shape[1], np.float32)
    return quantize_host(x, mean)


def _twin(x, S, center=True, block=256):
    from buglab.models._group import link_host, row_l1_host

    c, q, sumsq, r = _quantized(x, center)
    return link_host(c, q, sumsq, r, row_l1_host(q), S, block=block), (c, q, sumsq, r)


CASES = [(1, 9), (3, 40), (100, 60), (128, 33)]


@pytest.fixture(scope="module")
def references():
    """(D, S) -> (the twin's inputs, the loops' answer), computed once"""
    out = {}
    for D, N in CASES:
        x = GC.mixed_rows(N, D, seed=D)
        c, q, sumsq, r = _quantized(x)
        for S in (0.5, 0.9, 1.0):
            out[D, S] = ((c, q, sumsq, r), GC.link_ref(c, q, sumsq, r, S))
    return out


@pytest.mark.parametrize("D,N", CASES)
def test_twin_equals_plain_loops(D, N, references):
    from buglab.models._group import link_host, row_l1_host

    some_rejected = False
    for S in (0.5, 0.9, 1.0):
        (c, q, sumsq, r), (label, degree, nc, ne, lost) = references[D, S]
        assert not lost, (D, S, lost)  # a condition, not a tolerance: every edge is a candidate
        l1 = row_l1_host(q)
        C.assert_equal_bits([l1], [GC.row_l1_ref(q)], (D, "l1"))
        for block in (256, 7):  # one block, and blocks that cut the triangle
            got = link_host(c, q, sumsq, r, l1, S, block=block)
            C.assert_equal_bits(got[:2], (label, degree), (D, S, block))
            assert got[2:] == (nc, ne), (D, S, block, got[2:], (nc, ne))
        assert ne <= nc and degree.sum() == 2 * ne
        some_rejected = some_rejected or nc > ne
        if N > 7:  # invalid rows (NaN, inf; the zero row 1 is minus the mean after centring) are singletons of degree 0
            assert label[[4, 7]].tolist() == [4, 7] and not degree[[4, 7]].any() and not (r[[4, 7]] > 0).any()
        if S == 1.0 and N > 5 and D > 1:  # the copies still link
            assert ne >= 1 and (label != np.arange(N)).any()
    if D >= 100:
        assert some_rejected, "the rejecting branch of the re-score was never taken"


def test_filter_loses_no_edge_on_heavy_tailed_rows():
    from buglab.models._explain import node_scores_host
    from buglab.models._group import candidate_pairs, row_l1_host, thresholds

    rejected = 0
    for D in (3, 16, 64, 100):
        x = GC.heavy_tailed_rows(48, D, seed=D)
        for center in (True, False):
            c, q, sumsq, r = _quantized(x, center)
            l1 = row_l1_host(q)
            ii, jj = np.triu_indices(48, 1)
            live = (r[ii] > 0) & (r[jj] > 0)
            ii, jj = ii[live], jj[live]
            dot = node_scores_host(c[ii], c[jj])
            for S in (0.5, 0.8, 0.9, 0.99, 1.0):
                s2, K = thresholds(S)
                edge = (dot > 0.0) & (dot * dot >= s2 * (sumsq[ii] * sumsq[jj]))
                ci, cj = candidate_pairs(q, r, l1, D, K, 0, 48)
                candidates = set(zip(ci.tolist(), cj.tolist()))
                assert set(zip(ii[edge].tolist(), jj[edge].tolist())) <= candidates, (D, center, S)
                rejected += len(candidates) - int(edge.sum())
    assert rejected > 0


def test_duplicates_link_at_similarity_one_and_a_chain_is_one_group():
    x = C.drawn_rows(12, 100, seed=1)
    x[5], x[9] = x[2], x[2]
    (label, degree, nc, ne), _ = _twin(x, 1.0)
    assert label.tolist() == [0, 1, 2, 3, 4, 2, 6, 7, 8, 2, 10, 11] and degree[[2, 5, 9]].tolist() == [2, 2, 2] and ne == 3

    rows, chain = GC.chain_rows()
    (label, degree, nc, ne), (c, q, sumsq, r) = _twin(rows, 0.9, center=False)
    from buglab.models._similar import similarity

    a, b, far = chain[0], chain[1], chain[2]
    cos = lambda i, j: float(similarity(np.dot(c[i].astype(np.float64), c[j].astype(np.float64)), sumsq[i], sumsq[j]))
    assert cos(a, b) >= 0.9 > cos(a, far)  # a - b - far: linked through b alone
    assert (label[chain] == 0).all() and ne == len(chain) - 1 and degree[chain].tolist() == [1] + [2] * (len(chain) - 2) + [1]
    others = np.setdiff1d(np.arange(rows.shape[0]), chain)
    assert (label[others] == others).all() and not degree[others].any()


def test_invalid_rows_are_singletons():
    x = np.ones((20, 8), np.float32)  # every row equal: zero after centring
    (label, degree, nc, ne), _ = _twin(x, 0.5)
    assert label.tolist() == list(range(20)) and not degree.any() and (nc, ne) == (0, 0)
    x[3, 2] = np.nan
    (label, degree, nc, ne), _ = _twin(x, 0.5, center=False)  # 19 equal rows and a NaN row
    assert label.tolist() == [0, 0, 0, 3] + [0] * 16 and degree[3] == 0 and ne == 19 * 18 // 2 and (np.delete(degree, 3) == 18).all()


@pytest.mark.parametrize("S", [0.0, -0.5, 1.0000001, float("nan"), float("inf")])
def test_similarity_outside_the_range_raises(S):
    from buglab.models import group
    from buglab.models._group import thresholds
    from buglab.models.hip_ops import group_thresholds

    for f in (thresholds, group_thresholds):
        with pytest.raises(ValueError, match="similarity"):
            f(S)
    with pytest.raises(ValueError, match="similarity"):
        group.group_embeddings(C.drawn_rows(4, 8, 0), S, host=True)


def test_thresholds_are_the_stated_doubles():
    from buglab.models._group import thresholds
    from buglab.models.hip_ops import group_thresholds

    for S in (0.5, 0.8, 0.9, 0.99, 1.0, 1e-3):
        s2, K = GC.thresholds_ref(S)
        assert thresholds(S) == group_thresholds(S) == (float(s2), float(K))
    assert thresholds(1.0) == (1.0, 4162314256.0 * (1.0 - 2.0 ** -40)) and 16 * 16129 ** 2 == 4162314256


def test_a_squared_stays_exact_at_the_largest_dimension():
    from buglab.models._group import candidate_pairs, row_l1_host

    q = np.full((2, 512), 127, np.int8)
    l1 = row_l1_host(q)
    assert l1.tolist() == [512 * 127] * 2
    A = 4 * 512 * 127 * 127 + 2 * (2 * 512 * 127) + 512
    assert A * A < 2 ** 53 and float(A) * float(A) == A * A
    r = np.asarray([16129.0 / (512 * 16129.0)] * 2)  # amax^2 / sumsq of a constant row
    ii, jj = candidate_pairs(q, r, l1, 512, float(A * A) * (r[0] * r[1]), 0, 2)  # K exactly at the key: passes
    assert (ii.tolist(), jj.tolist()) == ([0], [1])
    ii, jj = candidate_pairs(q, r, l1, 512, np.nextafter(float(A * A) * (r[0] * r[1]), np.inf), 0, 2)
    assert ii.shape[0] == 0


def test_groups_from_labels_orders_and_breaks_ties():
    from buglab.models._group import groups_from_labels

    #                 0  1  2  3  4  5  6  7  8  9
    label = np.array([0, 1, 0, 3, 1, 0, 6, 3, 8, 1], np.int32)
    degree = np.array([1, 2, 2, 1, 2, 1, 0, 1, 0, 1], np.int32)
    logprob = np.array([-1.0, -3.0, -2.0, -0.5, -0.1, -0.2, -9.0, -0.5, -0.3, -0.1], np.float32)
    groups = groups_from_labels(label, degree, logprob)
    assert [(g.members.tolist(), g.representative, g.size) for g in groups] == [
        ([0, 2, 5], 2, 3),     # the greatest degree
        ([1, 4, 9], 4, 3),     # degrees 2, 2: the greater log-probability; equal sizes: the lower representative first
        ([3, 7], 3, 2),        # degree and log-probability equal: the lower index
        ([6], 6, 1), ([8], 8, 1)]
    assert [g.representative for g in groups_from_labels(label, degree)] == [1, 2, 3, 6, 8]  # no log-probabilities: degree, then index
    assert groups_from_labels(np.zeros(0, np.int32), np.zeros(0, np.int32)) == []


def test_labels_host_walks_to_the_root_and_stays_in_bounds():
    from buglab.models._group import labels_host

    assert labels_host(np.array([0, 0, 1, 2, 4, 4, 3], np.int32)).tolist() == [0, 0, 0, 0, 4, 4, 0]
    assert labels_host(np.array([0, 5, -7, 2, 99], np.int32)).tolist() == [0, 1, 2, 2, 4]  # garbage ends the walk where it stands


def test_group_embeddings_on_the_host_and_the_report():
    from buglab.models import group
    from buglab.models._group import report

    rng = np.random.default_rng(0)
    base = rng.standard_normal((3, 32)).astype(np.float32)
    rows = np.concatenate([np.repeat(base[:1], 4, 0), np.repeat(base[1:2], 2, 0), base[2:]])
    rows += 1e-3 * rng.standard_normal(rows.shape).astype(np.float32)
    found = group.group_embeddings(rows, 0.9, center=False, host=True)
    assert [(g.members.tolist(), g.size) for g in found.groups] == [([0, 1, 2, 3], 4), ([4, 5], 2), ([6], 1)]
    assert found.num_edges == 7 and found.valid.all() and (found.similarity > 0.99).all()
    assert all(found.similarity[g.representative] == 1.0 for g in found.groups)  # dot == sumsq bit for bit
    summary = report([g.size for g in found.groups], [["a"] * 4, ["a", "b"], ["c"]], 0.9, 9, 1, 1, 0, 0, found.num_candidates, 7)
    assert summary["num_groups"] == 3 and summary["num_singletons"] == 1 and summary["largest_group"] == 4
    assert summary["spared"] == 1.0 - 3 / 7 and summary["size_histogram"]["3-4"] == 1 and summary["labelled"] == {"num_groups": 2, "one_scout": 0.5}
    empty = group.group_embeddings(np.zeros((0, 32), np.float32), 0.9, host=True)
    assert empty.groups == [] and empty.label.shape == (0,)

"""GPU: warning grouping on the MI355X -- the kernels of csrc/bl_group.hip against their NumPy twin (buglab/models/_group.py,
which tests/test_group_host.py pins to plain loops) bit for bit: labels, degrees and both counters for every shape that reaches
another branch of the join, for every number of slices; the cases built to stress the lock-free union-find (a chain joined only
across workgroups, 200 identical rows); strided and shifted operands, outputs inside poisoned guard bands, argument errors; and
`group` end to end on two tiny untrained models, the device path against `--host` byte for byte.

No tolerance anywhere: every output is an integer that the definition fixes whatever the order of the pairs."""
import copy
import gzip
import json
from pathlib import Path

import numpy as np
import pytest
import torch

from tests import group_cases as GC
from tests import similar_cases as C
from tests.guard_bands import guarded
from tests.test_similar_gpu import DEV, SPECS, _deterministic, _dev, _stream, _strided

pytestmark = pytest.mark.gpu


def _inputs(x, center=True):
    """the twin's own quantisation of the rows (the kernel's is tested in tests/test_similar_gpu.py) and their l1"""
    from buglab.models._group import row_l1_host
    from buglab.models._similar import column_mean, quantize_host

    c, q, sumsq, r = quantize_host(x, column_mean(x) if center else np.zeros(x.shape[1], np.float32))
    return c, q, sumsq, r, row_l1_host(q)


def _device_link(d, S, slices=None):
    """(label, degree, counters) of one launch, on the host"""
    from buglab.models import hip_ops

    parent, degree, counters = hip_ops.group_link(*d, S, slices)
    label = hip_ops.group_labels(parent)
    p = parent.cpu().numpy()
    assert (p <= np.arange(p.shape[0])).all() and (p >= 0).all()  # the forest's invariant
    return label.cpu().numpy(), degree.cpu().numpy(), counters.cpu().numpy()


def _assert_same(got, want, what):
    C.assert_equal_bits(got[:2], want[:2], what)
    assert got[2].tolist() == [want[2], want[3]], (what, got[2].tolist(), want[2:])


# ------------------------------------------------------------------------------------------------ bl_group_row_l1
@pytest.mark.parametrize("D", [1, 100, 512])
def test_row_l1_equals_the_twin(D):
    from buglab.models import hip_ops
    from buglab.models._group import row_l1_host

    for N in (1, 5, 67):
        c, q, sumsq, r, l1 = _inputs(GC.mixed_rows(N, D, seed=N + D, noise=1.0))
        assert l1.max() <= 127 * D and (N < 5 or l1[4] == 0)
        C.assert_equal_bits([hip_ops.group_row_l1(_dev(q)).cpu().numpy()], [l1], (D, N))
    full = np.full((3, (D + 63) // 64 * 64), -127, np.int8)
    C.assert_equal_bits([hip_ops.group_row_l1(_dev(full)).cpu().numpy()], [row_l1_host(full)], (D, "all -127"))


# ------------------------------------------------------------------------------------------------ bl_group_link, bl_group_labels
NS = [1, 2, 15, 16, 17, 33, 200]  # the diagonal tile alone (partial, whole), one off-diagonal tile, partial tiles, 13 tiles


@pytest.mark.parametrize("D", [1, 100, 128, 512])  # one column; padding columns; two whole k-chunks; 8 k-chunks
def test_link_equals_the_twin_for_every_geometry(D):
    from buglab.models._group import link_host

    rejected = linked = 0
    for N in NS:
        c, q, sumsq, r, l1 = _inputs(GC.mixed_rows(N, D, seed=7 * N + D))
        d = [_dev(a) for a in (c, q, sumsq, r, l1)]
        for S in (0.5, 0.9, 1.0):
            want = link_host(c, q, sumsq, r, l1, S)
            for slices in (1, 3, 64):
                _assert_same(_device_link(d, S, slices), want, (D, N, S, slices))
            _assert_same(_device_link(d, S), want, (D, N, S, "default slices"))
            rejected += want[2] - want[3]
            linked += want[3]
    assert linked > 0 and (D < 100 or rejected > 0)  # both outcomes of the re-score were taken


def test_a_chain_with_one_row_per_tile_is_joined_across_workgroups():
    """rows 0 - 16 - 32 - ... - 192: every edge lies in another (tile row, tile) pair, so with 13 x 64 workgroups the component
    is assembled by hooks of different workgroups alone"""
    from buglab.models._group import link_host

    rows, chain = GC.chain_rows()
    c, q, sumsq, r, l1 = _inputs(rows, center=False)
    want = link_host(c, q, sumsq, r, l1, 0.9)
    assert (want[0][chain] == 0).all() and want[3] == len(chain) - 1 == 12 and (want[0] != 0).sum() == 200 - 13
    d = [_dev(a) for a in (c, q, sumsq, r, l1)]
    for slices in (1, 64):
        _assert_same(_device_link(d, 0.9, slices), want, ("chain", slices))


def test_identical_rows_all_hook_towards_row_zero():
    """the contention case, run once: 200 equal rows, 19 900 edges, every hook aimed at the same root"""
    from buglab.models._group import link_host

    rows = np.repeat(C.drawn_rows(1, 128, seed=2), 200, axis=0)
    c, q, sumsq, r, l1 = _inputs(rows, center=False)
    want = link_host(c, q, sumsq, r, l1, 1.0)
    assert not want[0].any() and (want[1] == 199).all() and want[2:] == (19900, 19900)
    _assert_same(_device_link([_dev(a) for a in (c, q, sumsq, r, l1)], 1.0), want, "identical rows")


def test_the_filter_passes_pairs_that_the_rescore_rejects_and_invalid_rows_stay_alone():
    from buglab.models._group import link_host

    x = GC.mixed_rows(33, 128, seed=5)
    x[20], x[31, 3] = 0.0, np.inf  # with rows 4 and 7: invalid rows in both tiles and in the partial third (row 20 is zero: not centred)
    c, q, sumsq, r, l1 = _inputs(x, center=False)
    invalid = [1, 4, 7, 20, 31]
    assert not (r[invalid] > 0).any() and (np.delete(r, invalid) > 0).all()
    want = link_host(c, q, sumsq, r, l1, 0.9)
    assert want[2] > want[3] > 0 and want[0][invalid].tolist() == invalid and not want[1][invalid].any()
    d = [_dev(a) for a in (c, q, sumsq, r, l1)]
    first = _device_link(d, 0.9, 3)
    _assert_same(first, want, "invalid rows")
    again = _device_link(d, 0.9, 3)  # the same call twice: the same bytes
    assert all(a.tobytes() == b.tobytes() for a, b in zip(first, again))


def test_strided_operands_and_outputs_inside_guard_bands():
    from buglab.models import hip_ops
    from buglab.models._group import link_host, thresholds

    N, D, S = 37, 100, 0.9
    c, q, sumsq, r, l1 = _inputs(GC.mixed_rows(N, D, seed=11))
    want = link_host(c, q, sumsq, r, l1, S)
    assert want[3] > 0
    d_q, d_sumsq, d_r, d_l1 = (_dev(a) for a in (q, sumsq, r, l1))
    for pad, shift in ((0, 1), (3, 0), (4, 4), (5, 3)):  # no quad is aligned; rows drift; everything aligned; neither
        _assert_same(_device_link([_strided(c, pad, shift), d_q, d_sumsq, d_r, d_l1], S, 3), want, (pad, shift))
    lib = hip_ops.load_library()
    s2, K = thresholds(S)
    g_parent = guarded(N, 1, ld=1, dtype=torch.int32, device=DEV, any_width=True)
    g_degree = guarded(N, 1, ld=1, dtype=torch.int32, device=DEV, any_width=True)
    g_label = guarded(N, 1, ld=1, dtype=torch.int32, device=DEV, any_width=True)
    g_l1 = guarded(N, 1, ld=1, dtype=torch.int32, device=DEV, any_width=True)
    g_count = guarded(2, 2, ld=2, dtype=torch.int32, device=DEV, lead=6, any_width=True)
    g_q = guarded(N, 128, ld=128, dtype=torch.int8, device=DEV)
    assert g_count.data_ptr() % 8 == 0 and g_q.data_ptr() % 16 == 0
    g_q.view.copy_(d_q)
    g_parent.view[:, 0].copy_(torch.arange(N, dtype=torch.int32, device=DEV))
    g_degree.view.zero_(), g_count.view.zero_()
    d_c = _strided(c, 2, 1)
    assert lib.bl_group_row_l1(g_q.data_ptr(), N, 128, g_l1.data_ptr(), _stream()) == 0, lib.bl_last_error()
    rc = lib.bl_group_link(g_q.data_ptr(), d_r.data_ptr(), g_l1.data_ptr(), d_c.data_ptr(), D + 2, d_sumsq.data_ptr(), N, D, 128, s2, K, 3,
                           g_parent.data_ptr(), g_degree.data_ptr(), g_count.data_ptr(), _stream())
    assert rc == 0, lib.bl_last_error()
    assert lib.bl_group_labels(g_parent.data_ptr(), N, g_label.data_ptr(), _stream()) == 0, lib.bl_last_error()
    for g, name in ((g_parent, "parent"), (g_degree, "degree"), (g_label, "label"), (g_l1, "l1"), (g_count, "counters"), (g_q, "q")):
        g.assert_untouched(name)
    counters = g_count.view.contiguous().cpu().numpy().view(np.int64)[:, 0]
    _assert_same((g_label.view[:, 0].cpu().numpy(), g_degree.view[:, 0].cpu().numpy(), counters), want, "guard bands")
    C.assert_equal_bits([g_l1.view[:, 0].cpu().numpy()], [l1], "l1 in guard bands")


def test_argument_errors_are_returned_without_a_launch():
    from buglab.models import hip_ops
    from buglab.models._group import thresholds

    N, D = 20, 100
    c, q, sumsq, r, l1 = _inputs(GC.mixed_rows(N, D, seed=1))
    d_c, d_q, d_sumsq, d_r, d_l1 = (_dev(a) for a in (c, q, sumsq, r, l1))
    parent, degree = torch.arange(N, dtype=torch.int32, device=DEV), torch.zeros(N, dtype=torch.int32, device=DEV)
    counters = torch.zeros(3, dtype=torch.int64, device=DEV)
    lib = hip_ops.load_library()
    s2, K = thresholds(0.9)

    def link(q_ptr=d_q.data_ptr(), ldc=D, n=N, d=D, dp=128, s2_=s2, k_=K, slices=1, parent_ptr=parent.data_ptr(), count_ptr=counters.data_ptr()):
        return lib.bl_group_link(q_ptr, d_r.data_ptr(), d_l1.data_ptr(), d_c.data_ptr(), ldc, d_sumsq.data_ptr(), n, d, dp, s2_, k_, slices,
                                 parent_ptr, degree.data_ptr(), count_ptr, _stream())

    EINVAL, ERANGE = -1, -2
    assert link(q_ptr=None) == EINVAL and b"null" in lib.bl_last_error()
    assert link(parent_ptr=None) == EINVAL and link(count_ptr=None) == EINVAL
    assert link(q_ptr=d_q.data_ptr() + 4) == EINVAL and b"16-byte aligned" in lib.bl_last_error()
    assert link(count_ptr=counters.data_ptr() + 4) == EINVAL and b"8-byte aligned" in lib.bl_last_error()
    assert link(dp=100) == EINVAL and link(dp=64) == EINVAL and link(dp=192) == EINVAL and b"multiple of 64" in lib.bl_last_error()
    assert link(d=513, dp=576) == ERANGE and b"BL_SIM_MAX_D" in lib.bl_last_error()
    assert link(ldc=D - 1) == EINVAL and link(n=-1) == EINVAL and link(d=0, dp=0) == EINVAL
    for bad in (0.0, -0.25, 1.0000001, float("nan")):
        assert link(s2_=bad) == EINVAL and b"s2" in lib.bl_last_error()
    for bad in (0.0, float("nan"), float("inf")):
        assert link(k_=bad) == EINVAL
    assert link(slices=0) == EINVAL and link(slices=65) == EINVAL
    assert link(n=(1 << 19) + 1) == ERANGE and b"BL_GROUP_MAX_N" in lib.bl_last_error()
    assert lib.bl_group_row_l1(None, N, 128, d_l1.data_ptr(), _stream()) == EINVAL
    assert lib.bl_group_row_l1(d_q.data_ptr() + 4, N, 128, d_l1.data_ptr(), _stream()) == EINVAL
    assert lib.bl_group_row_l1(d_q.data_ptr(), N, 100, d_l1.data_ptr(), _stream()) == EINVAL
    assert lib.bl_group_row_l1(d_q.data_ptr(), N, 576, d_l1.data_ptr(), _stream()) == ERANGE
    assert lib.bl_group_labels(None, N, d_l1.data_ptr(), _stream()) == EINVAL and lib.bl_group_labels(parent.data_ptr(), -1, d_l1.data_ptr(), _stream()) == EINVAL
    assert lib.bl_group_labels(parent.data_ptr(), (1 << 19) + 1, d_l1.data_ptr(), _stream()) == ERANGE
    torch.cuda.synchronize()  # nothing was launched: the outputs are as they were
    assert parent.cpu().tolist() == list(range(N)) and not degree.any() and not counters.any()
    assert link() == 0 and lib.bl_group_link(None, None, None, None, D, None, 0, D, 128, s2, K, 1, None, None, counters.data_ptr(), _stream()) == 0
    with pytest.raises(ValueError, match="similarity"):
        hip_ops.group_link(d_c, d_q, d_sumsq, d_r, d_l1, 1.5)
    with pytest.raises(ValueError, match="slices"):
        hip_ops.group_link(d_c, d_q, d_sumsq, d_r, d_l1, 0.9, slices=65)
    with pytest.raises(ValueError, match="rounded up"):
        hip_ops.group_link(d_c[:, :60], d_q, d_sumsq, d_r, d_l1, 0.9)


# ------------------------------------------------------------------------------------------------ end to end
@pytest.fixture(scope="module")
def untrained(tmp_path_factory):
    """family -> (model, module, data, checkpoint path, folder of the data): seeded weights, no training; 48 synthetic samples"""
    from buglab.data.synthetic import make_report_dataset
    from buglab.models.modelregistry import load_model
    from buglab.runtime.neuralmodel import AbstractNeuralModel
    from buglab.utils.msgpackutils import save_msgpack_l_gz

    out = {}
    for family, spec in SPECS.items():
        data = make_report_dataset(48, seed=17, kind="seq" if family.startswith("seq") else "graph")
        folder = tmp_path_factory.mktemp("group_" + family.replace("-", "_"))
        path = folder / "detector.pkl.gz"
        model = load_model(dict(spec), path)[0]
        model.compute_metadata(copy.deepcopy(data))
        torch.manual_seed(5)
        model.save(path, model.build_neural_module())
        (folder / "data").mkdir()
        save_msgpack_l_gz(data, folder / "data" / "x.msgpack.l.gz")
        out[family] = AbstractNeuralModel.restore_model(Path(path), torch.device(DEV)) + (data, path, folder / "data")
    return out


def _edge_components(rows, mean, S):
    """the definition, recomputed on the host from the rows: fp64 dots in the stated order on every pair, a naive union-find"""
    from buglab.models._explain import node_scores_host
    from buglab.models._similar import quantize_host

    c, q, sumsq, r = quantize_host(rows, mean)
    ii, jj = np.triu_indices(rows.shape[0], 1)
    live = (r[ii] > 0) & (r[jj] > 0)
    ii, jj = ii[live], jj[live]
    dot = node_scores_host(c[ii], c[jj])
    edge = (dot > 0.0) & (dot * dot >= np.float64(S) * np.float64(S) * (sumsq[ii] * sumsq[jj]))
    parent = list(range(rows.shape[0]))

    def find(x):
        while parent[x] != x:
            x = parent[x]
        return x

    for a, b in zip(ii[edge].tolist(), jj[edge].tolist()):
        a, b = find(a), find(b)
        if a != b:
            parent[max(a, b)] = min(a, b)
    return np.asarray([find(x) for x in range(rows.shape[0])], np.int32), list(zip(ii[edge].tolist(), jj[edge].tolist()))


def _similarity_with_groups(rows):
    """a threshold at which these rows have both links and strangers: the median of the best cosine of every row (centred)"""
    from buglab.models._similar import centre, column_mean

    c = centre(rows, column_mean(rows)).astype(np.float64)
    c = c[(np.abs(c).sum(axis=1) > 0)]
    cos = (c @ c.T) / np.sqrt((c * c).sum(1)[:, None] * (c * c).sum(1)[None, :])
    np.fill_diagonal(cos, -1.0)
    return float(np.clip(np.round(np.median(cos.max(axis=1)), 3), 0.05, 0.999))


@pytest.mark.parametrize("family", list(SPECS))
def test_groups_on_the_device_equal_the_host_path_and_are_closed(family, untrained):
    from buglab.models import group as T
    from buglab.models import similar

    model, nn_, data, _, _ = untrained[family]
    with _deterministic():
        sites = similar.embed_sites(model, nn_, data, torch.device(DEV), "predicted", assume_buggy=True, parallelize=False)
        assert sites.rows.shape == (48, 32)
        S = _similarity_with_groups(sites.rows)
        for options in (dict(), dict(center=False), dict(min_confidence=float(np.exp(np.median(sites.logprobs)))), dict(min_group_size=2)):
            a = T.group_sites(sites, S, device=DEV, **options)
            b = T.group_sites(sites, S, host=True, **options)
            assert json.dumps([g.record() for g in a.groups], sort_keys=True) == json.dumps([g.record() for g in b.groups], sort_keys=True)
            assert a.summary == b.summary, options
        everything = T.group_sites(sites, S, device=DEV)
        s = everything.summary
        assert s["num_warnings"] == 48 == sum(g.size for g in everything.groups) and s["num_groups"] == len(everything.groups)
        assert 1 < s["num_groups"] < 48 and s["num_edges"] > 0, (S, s)  # links and strangers: the threshold was chosen for that
        sizes = [g.size for g in everything.groups]
        assert sizes == sorted(sizes, reverse=True) and [g.id for g in everything.groups] == list(range(len(sizes)))
        for g in everything.groups:
            positions = [m["position"] for m in g.members]
            assert positions == sorted(positions) and g.representative["position"] in positions and len(positions) == g.size
            assert all(-1.0 <= m["similarity"] <= 1.0 for m in g.members)
            assert [m["similarity"] for m in g.members if m["position"] == g.representative["position"]] == [1.0]
        # --min-confidence and --min-group-size filter what they say
        cut = float(np.exp(np.median(sites.logprobs)))
        kept = int((np.exp(sites.logprobs.astype(np.float64)) >= cut).sum())
        confident = T.group_sites(sites, S, device=DEV, min_confidence=cut)
        assert 0 < kept < 48 and confident.summary["num_warnings"] == kept and confident.summary["num_below_confidence"] == 48 - kept
        assert all(m["position"] in set(sites.positions[np.exp(sites.logprobs.astype(np.float64)) >= cut].tolist())
                   for g in confident.groups for m in g.members)
        big = T.group_sites(sites, S, device=DEV, min_group_size=2)
        assert [g.record() for g in big.groups] == [g.record() for g in everything.groups if g.size >= 2]
        assert big.summary["num_groups"] == s["num_groups"] and big.summary["num_groups_listed"] == len(big.groups) < s["num_groups"]

        # every group is closed under the definition, and no group is larger than the definition makes it
        found = T.group_embeddings(torch.from_numpy(sites.rows).to(DEV), S)
        label, edges = _edge_components(sites.rows, found.mean, S)
        assert all(found.label[i] == found.label[j] for i, j in edges) and len(edges) == found.num_edges
        C.assert_equal_bits([found.label], [label], "components of the definition")


def test_command_line_group(untrained, tmp_path, capsys):
    from buglab.models import group as T
    from buglab.models import similar
    from buglab.models._similar import SiteIndex

    model, nn_, data, path, data_dir = untrained["gnn-mlp"]
    with _deterministic():
        sites = similar.embed_sites(model, nn_, data, torch.device(DEV), "predicted", assume_buggy=True, parallelize=False)
        S = _similarity_with_groups(sites.rows)
        index = similar.build_site_index(model, nn_, data[:30], DEV, "truth", "known-bug", parallelize=False)
        index.save(tmp_path / "bugs.npz")
        outs = {}
        for name, extra in (("device", []), ("host", ["--host"])):
            out, report = tmp_path / f"{name}.jsonl.gz", tmp_path / f"{name}.json"
            args = [str(path), str(data_dir), str(out), "--similarity", str(S), "--assume-buggy", "--index", str(tmp_path / "bugs.npz"),
                    "--report-json", str(report), "--sequential"] + extra
            assert T.run(T.parse_args(args)) == 0
            assert "group: 48 warnings of 48 samples" in capsys.readouterr().out
            with gzip.open(out, "rb") as f:
                outs[name] = (f.read(), report.read_bytes())
        assert outs["device"] == outs["host"]  # OUT and --report-json, byte for byte
        records = [json.loads(line) for line in outs["device"][0].decode("utf-8").splitlines()]
        blob = json.loads(outs["device"][1])
        assert len(records) == blob["num_groups"] == blob["num_groups_listed"] and sum(r["size"] for r in records) == 48
        for r in records:
            assert set(r) == {"id", "size", "position", "node", "label", "filename", "package", "logprob", "members", "resembles"}
            assert r["resembles"]["tag"] == "known-bug" and -1.0 <= r["resembles"]["similarity"] <= 1.0 and len(r["members"]) == r["size"]
        want = T.group_sites(sites, S, index=SiteIndex.load(tmp_path / "bugs.npz"), device=DEV)
        assert records == json.loads(json.dumps([g.record() for g in want.groups]))
        # an index of embeddings of another size: status 2, nothing written
        wrong = index._replace(embeddings=np.zeros((index.size, 48), np.float32), mean=np.zeros(48, np.float32), dim=48)
        wrong.save(tmp_path / "wrong.npz")
        other = tmp_path / "other.jsonl"
        status = T.run(T.parse_args([str(path), str(data_dir), str(other), "--index", str(tmp_path / "wrong.npz"), "--sequential"]))
        assert status == T.EXIT_DIMENSION_MISMATCH == 2 and not other.exists() and "size 48" in capsys.readouterr().err
        # the filters, through the command line
        small = tmp_path / "small.jsonl"
        assert T.run(T.parse_args([str(path), str(data_dir), str(small), "--similarity", str(S), "--assume-buggy", "--min-group-size", "2",
                                   "--sequential"])) == 0
        lines = [json.loads(line) for line in small.read_text(encoding="utf-8").splitlines()]
        assert [(r["size"], r["position"]) for r in lines] == [(r["size"], r["position"]) for r in records if r["size"] >= 2]
        assert all("resembles" not in r for r in lines)

"""CPU: warning tracking without a GPU -- the NumPy twin of csrc/bl_track.hip (buglab/models/_track.py) against the restatement
in Python integers and Fractions (tests/track_cases.py) bit for bit; the sequential matching against the rounds of mutual best
inside the restatement, on random cases full of ties; stability; the edge inputs; the command line on the host path with its
three exit statuses, --hide-tag, --write-index and --within; and the argument errors of the wrappers and of the C entry points.

No tolerance anywhere: every output is an integer or one IEEE quotient of two exact integers."""
import collections
import json

import numpy as np
import pytest

from tests import track_cases as TC
from tests.similar_cases import assert_equal_bits
from tests.test_triage_host import _DrawnSites

FLOORS = (0.25, 0.81, 1.0)


def _keys(kind, L, N):
    return (None, None) if kind == "no keys" else (TC.keys3(L), TC.keys3(N, 1))


# ------------------------------------------------------------------------------------------------ 1. the twin against the restatement
@pytest.mark.parametrize("D", [1, 100, 128, 512])
def test_best_host_equals_the_restatement(D):
    from buglab.models import _track as T

    q_x, n_x, q_y, n_y, aff = TC.best_case(D)
    X, Y = 150, 37
    assert not n_x[[1, 4, 7]].any() and not n_y[[1, 4, 7]].any()
    aff_t = TC.transposed(aff, X, Y)
    open_x, open_y = TC.every_third_closed(X), TC.every_third_closed(Y, 1)
    for kind in ("no keys", "keys"):
        kx, ky = _keys(kind, X, Y)
        for floor in (0.25, 0.81):
            for ox, oy in ((None, None), (open_x, open_y)):
                want = TC.best_ref(aff, X, Y, floor, kx, ky, ox, oy)
                assert_equal_bits(T.best_host(q_x, n_x, q_y, n_y, floor, kx, ky, ox, oy), want, (D, kind, floor, "x -> y"))
                back = TC.best_ref(aff_t, Y, X, floor, ky, kx, oy, ox)
                assert_equal_bits(T.best_host(q_y, n_y, q_x, n_x, floor, ky, kx, oy, ox), back, (D, kind, floor, "y -> x"))
                assert (want[1][[1, 4, 7]] == -1).all() and (ox is None or (want[1][ox == 0] == -1).all())
                assert oy is None or oy[want[1][want[1] >= 0]].all()
    # a floor that some row's best pair misses, and one that it passes
    low, high = TC.best_ref(aff, X, Y, 0.25), TC.best_ref(aff, X, Y, 0.81)
    assert D == 1 or ((low[1] >= 0) & (high[1] < 0)).any()
    assert ((high[1] >= 0) & (high[0] >= 0.81)).any() and (low[0][high[1] >= 0] == high[0][high[1] >= 0]).all()


@pytest.mark.parametrize("kind", ["no keys", "keys"])
@pytest.mark.parametrize("floor", [0.25, 0.81])
def test_match_host_equals_the_restatement(floor, kind):
    from buglab.models import _track as T

    q_old, n_old, q_new, n_new, aff = TC.match_case()
    L, N = 150, 131
    ko, kn = _keys(kind, L, N)
    want = TC.match_ref(aff, L, N, floor, ko, kn)
    state, status, per_round = TC.rounds_ref(aff, L, N, floor, ko, kn)
    assert_equal_bits(state, want, "the rounds equal the sequential matching")
    got = T.match_host(q_old, n_old, q_new, n_new, floor, ko, kn)
    assert_equal_bits(got[:3], want, (floor, kind))
    assert got[3] == status[0] == len(per_round) >= 2 and status[1] == (want[1] >= 0).sum() > 20 and status[2] == 1
    assert (want[0][[1, 4, 7]] == -1).all() and (want[1][[2, 5]] == -1).all()
    assert TC.blocking_pairs(aff, L, N, floor, want[0], want[1], ko, kn) == []
    # the twin of bl_track_match, call for call: the state and the status after every call
    for max_rounds in (1, 2, 64):
        ours = theirs = None
        while True:
            ours, st = T.rounds_host(q_old, n_old, q_new, n_new, floor, ours, max_rounds, ko, kn)
            theirs, st_ref, _ = TC.rounds_ref(aff, L, N, floor, ko, kn, theirs, max_rounds)
            assert_equal_bits([*ours, st], [*theirs, st_ref], (floor, kind, max_rounds))
            if st[2]:
                break
        assert_equal_bits(ours, want, "the end")


def test_the_floor_decides_in_the_match_case():
    q_old, n_old, q_new, n_new, aff = TC.match_case()
    low, high = TC.match_ref(aff, 150, 131, 0.25), TC.match_ref(aff, 150, 131, 0.81)
    assert (high[1] >= 0).sum() < (low[1] >= 0).sum() and (high[2][high[1] >= 0] >= 0.81).all()


# ------------------------------------------------------------------------------------------------ 2. sequential against rounds
@pytest.mark.parametrize("floor", FLOORS)
@pytest.mark.parametrize("kind", ["no keys", "keys"])
def test_sequential_matching_equals_the_rounds_on_random_cases_with_ties(kind, floor):
    from buglab.models import _track as T

    tied = 0
    for seed in range(25):
        L, N = 8 + seed % 9, 6 + (3 * seed) % 11
        q_old, n_old, q_new, n_new, aff = TC.prototype_case(seed, L, N, invalid=seed % 2 == 0)
        ko, kn = _keys(kind, L, N)
        literal = TC.match_literal_ref(aff, L, N, floor, ko, kn)
        assert_equal_bits(TC.match_ref(aff, L, N, floor, ko, kn), literal, ("ordered pairs", seed))
        state, status, per_round = TC.rounds_ref(aff, L, N, floor, ko, kn)
        assert_equal_bits(state, literal, ("rounds", seed))
        assert status[0] == len(per_round) and status[1] == sum(per_round) == (literal[1] >= 0).sum() and status[2] == 1
        assert TC.blocking_pairs(aff, L, N, floor, literal[0], literal[1], ko, kn) == [], seed
        got = T.match_host(q_old, n_old, q_new, n_new, floor, ko, kn)
        assert_equal_bits(got[:3], literal, ("twin", seed))
        assert got[3] == status[0]
        values = [a for row in aff for a in row if a is not None and a >= floor]
        tied += len(values) - len(set(values))
        # a matching is one-to-one, and each side points at the other
        j = np.flatnonzero(literal[1] >= 0)
        assert len(set(literal[1][j].tolist())) == j.shape[0] and (literal[0][literal[1][j]] == j).all()
    assert tied > 100, "the cases are meant to tie"


def test_a_chain_needs_one_round_per_pair():
    from buglab.models import _track as T

    k = 7
    q_old, n_old, q_new, n_new, aff = TC.chain_case(k)
    state, status, per_round = TC.rounds_ref(aff, k, k, 0.25)
    assert per_round == [1] * k and status.tolist() == [k, k, 1, 0]
    assert state[0].tolist() == list(range(k))  # o_i with n_i, the last pair first
    assert_equal_bits(state, TC.match_ref(aff, k, k, 0.25), "chain")
    assert T.match_host(q_old, n_old, q_new, n_new, 0.25)[3] == k


# ------------------------------------------------------------------------------------------------ 3. edge inputs
def test_edge_inputs():
    from buglab.models import _track as T
    from buglab.models import track

    q_old, n_old, q_new, n_new, aff = TC.prototype_case(3)
    none = np.zeros((0, 64), np.int8), np.zeros(0, np.int32)
    for (qo, no), (qn, nn) in ((none, (q_new, n_new)), ((q_old, n_old), none), (none, none)):
        m_old, m_new, m_aff, rounds = T.match_host(qo, no, qn, nn, 0.25)
        assert (m_old == -1).all() and (m_new == -1).all() and not m_aff.any() and rounds == 0
        state, status = T.rounds_host(qo, no, qn, nn, 0.25, None, 3)
        assert status.tolist() == [0, 0, 1, len(nn)]
        best, arg = T.best_host(qo, no, qn, nn, 0.25)
        assert (best == -2.0).all() and (arg == -1).all() and best.shape == (len(no),)
    zero = np.zeros_like(q_old), np.zeros_like(n_old)
    m_old, m_new, m_aff, rounds = T.match_host(*zero, q_new, n_new, 0.25)
    assert (m_old == -1).all() and (m_new == -1).all() and rounds == 0
    with pytest.raises(ValueError, match="floor"):
        T.match_host(q_old, n_old, q_new, n_new, 0.0)
    with pytest.raises(ValueError, match="come together"):
        T.best_host(q_old, n_old, q_new, n_new, 0.5, keyx=np.zeros(len(n_old), np.int32))
    with pytest.raises(ValueError, match="max_rounds"):
        T.rounds_host(q_old, n_old, q_new, n_new, 0.5, None, 0)
    # the same through the public function, on rows
    rng = np.random.default_rng(0)
    x = rng.standard_normal((9, 6)).astype(np.float32)
    for old, new in ((x[:0], x), (x, x[:0]), (np.zeros((4, 6), np.float32), x), (x, np.full((3, 6), np.nan, np.float32))):
        m = track.match_embeddings(old, new, host=True)
        assert m.num_matched == 0 and m.rounds == 0 and m.match_old.shape == (len(old),) and m.match_new.shape == (len(new),)
        assert not m.similarity.any() and m.valid_new.shape == (len(new),)
    same = track.match_embeddings(x, x[::-1].copy(), host=True, min_similarity=1.0)
    assert same.match_new.tolist() == list(range(8, -1, -1)) and (same.similarity == 1.0).all() and same.rounds == 1
    for bad in (0.0, 1.5, float("nan")):
        with pytest.raises(ValueError, match="min-similarity"):
            track.match_embeddings(x, x, host=True, min_similarity=bad)
    with pytest.raises(ValueError):
        track.match_embeddings(x, np.zeros((3, 513), np.float32), host=True)
    from buglab.models._similar import DimensionMismatch

    with pytest.raises(DimensionMismatch, match="size 6"):
        track.match_embeddings(x, x[:, :4].copy(), host=True)


# ------------------------------------------------------------------------------------------------ 4. the command line
@pytest.fixture(scope="module", params=["gnn-mlp", "seq-great"])
def detector(request, tmp_path_factory):
    """an untrained model of either family saved as a checkpoint, and the synthetic data it was set up with"""
    import torch

    from buglab.data.synthetic import make_report_dataset
    from tests.test_visualize_host import _model

    family = request.param
    data = make_report_dataset(60, seed=35, kind="seq" if family.startswith("seq") else "graph")
    model = _model(family, data)
    torch.manual_seed(1)
    path = tmp_path_factory.mktemp("track_host_" + family.replace("-", "_")) / "detector.pkl.gz"
    model.save(path, model.build_neural_module())
    return path, data


def _lines(path):
    return [json.loads(line) for line in path.read_text().splitlines()]


def test_command_line_on_the_host(detector, tmp_path, monkeypatch, capsys):
    from buglab.models import _similar as S
    from buglab.models import track as T

    path, data = detector
    old, scan = data[:40], data[10:]
    real_open = T._open_model
    monkeypatch.setattr(T, "_open_model", lambda p: real_open(p)[:3] + (True,))  # the untrained model itself; the GPU is not asked for
    monkeypatch.setattr(T, "_read_data", lambda p, limit: {"scan": scan}[p][:limit])
    monkeypatch.setattr(T, "_embed_sites", _DrawnSites.embed)
    model, nn, _, _ = real_open(str(path))
    sites = _DrawnSites.embed(None, None, old, "cpu", "predicted")
    index = S.make_index(sites, "seen", True, type(model).__name__, S.model_fingerprint(nn))
    index = index._replace(tags=S._text(["dismissed" if i % 2 == 0 else "accepted" for i in range(index.size)]))
    index.save(tmp_path / "old.npz")
    # the stub's embedding depends on a sample's path alone: a sample of both scans is an exact copy, samples of one path are
    # copies of each other, and drawn rows of 32 columns are nowhere near a cosine of 0.9 otherwise
    paths = lambda points: collections.Counter(p["graph"]["path"] for p in points)
    expected = sum(min(c, paths(scan)[p]) for p, c in paths(old).items())
    assert 30 <= expected < 40

    out, report, new_index = tmp_path / "tracked.jsonl", tmp_path / "tracked.json", tmp_path / "new.npz"
    args = [str(path), str(tmp_path / "old.npz"), "scan", str(out), "--host", "--report-json", str(report), "--sequential"]
    status = T.run(T.parse_args(args + ["--write-index", str(new_index), "--tag", "fresh"]))
    assert status == T.EXIT_NEW_WARNINGS == 1 and f"track: {50 - expected} new, {expected} persisting" in capsys.readouterr().out
    records, s = _lines(out), json.loads(report.read_text())
    assert [r["status"] for r in records] == [r["status"] for r in records[:50]] + ["gone"] * (40 - expected)
    assert [r["position"] for r in records[:50]] == list(range(50)) and set(r["status"] for r in records[:50]) == {"new", "persisting"}
    assert (s["num_new"], s["num_persisting"], s["num_gone"], s["num_hidden"]) == (50 - expected, expected, 40 - expected, 0)
    assert s["rounds"] >= 1 and s["within"] == "none" and s["min_similarity"] == 0.9 and s["other_weights"] is False
    assert s["num_samples"] == 50 and s["num_old"] == 40 and s["lowest_listed_similarity"] >= 0.9
    kept = [r for r in records if r["status"] == "persisting"]
    assert set(kept[0]) == {"status", "position", "node", "label", "filename", "package", "logprob", "previous"}
    assert all(r["previous"]["filename"] == r["filename"] and r["previous"]["similarity"] == 1.0 for r in kept)
    assert len({r["previous"]["entry"] for r in kept}) == expected  # one-to-one
    assert all("previous" not in r for r in records if r["status"] == "new")
    gone = [r for r in records if r["status"] == "gone"]
    assert {r["entry"] for r in gone} | {r["previous"]["entry"] for r in kept} == set(range(40)) and all(r["tag"] in ("accepted", "dismissed") for r in gone)
    by_tag = s["by_tag"]
    assert by_tag["fresh"]["new"] == 50 - expected and by_tag["accepted"]["persisting"] + by_tag["dismissed"]["persisting"] == expected
    # the bytes of OUT are stable
    first = out.read_bytes()
    assert T.run(T.parse_args(args)) == 1 and out.read_bytes() == first
    capsys.readouterr()
    # --hide-tag leaves the dismissed ones out and counts them
    hidden_out = tmp_path / "hidden.jsonl"
    assert T.run(T.parse_args(args[:3] + [str(hidden_out)] + args[4:] + ["--hide-tag", "dismissed"])) == 1
    h, listed = json.loads(report.read_text()), _lines(hidden_out)
    dismissed = sum(1 for r in kept if r["previous"]["tag"] == "dismissed")
    assert 0 < dismissed == h["num_hidden"] == h["by_tag"]["dismissed"]["hidden"] and h["num_persisting"] == expected - dismissed
    assert all(r["previous"]["tag"] == "accepted" for r in listed if r["status"] == "persisting") and len(listed) == len(records) - dismissed
    # --write-index: tags are inherited, a new warning gets --tag, and the file has its own mean
    written = S.SiteIndex.load(new_index)
    assert written.size == 50 and written.positions.tolist() == list(range(50))
    assert written.tags.tolist() == [r["previous"]["tag"] if r["status"] == "persisting" else "fresh" for r in records[:50]]
    assert written.mean.tobytes() != index.mean.tobytes() and written.fingerprint == index.fingerprint
    # a second run against the written index: everything persists, nothing is new, nothing is gone -> status 0
    again = tmp_path / "again.jsonl"
    assert T.run(T.parse_args([str(path), str(new_index), "scan", str(again), "--host", "--report-json", str(report)])) == 0
    a = json.loads(report.read_text())
    assert (a["num_new"], a["num_persisting"], a["num_gone"]) == (0, 50, 0) and all(r["status"] == "persisting" for r in _lines(again))
    assert [r["previous"]["tag"] for r in _lines(again)] == written.tags.tolist()
    capsys.readouterr()
    # --within file never matches across files, where the floor alone would
    loose, fenced = tmp_path / "loose.jsonl", tmp_path / "fenced.jsonl"
    assert T.run(T.parse_args([str(path), str(tmp_path / "old.npz"), "scan", str(loose), "--host", "--min-similarity", "0.05"])) in (0, 1)
    assert T.run(T.parse_args([str(path), str(tmp_path / "old.npz"), "scan", str(fenced), "--host", "--min-similarity", "0.05", "--within",
                               "file", "--report-json", str(report)])) == 1
    crossing = lambda p: [r for r in _lines(p) if r["status"] == "persisting" and r["previous"]["filename"] != r["filename"]]
    assert crossing(loose) and not crossing(fenced) and json.loads(report.read_text())["within"] == "file"
    assert sum(r["status"] == "persisting" for r in _lines(fenced)) == expected
    capsys.readouterr()
    # other weights: a warning, and said in the report
    index._replace(fingerprint="ab" * 20).save(tmp_path / "other.npz")
    assert T.run(T.parse_args([str(path), str(tmp_path / "other.npz"), "scan", str(again), "--host", "--report-json", str(report)])) == 1
    assert json.loads(report.read_text())["other_weights"] is True
    # an index of another embedding size: status 2 before any data is read, nothing written
    wrong = index._replace(embeddings=np.zeros((index.size, 48), np.float32), mean=np.zeros(48, np.float32), dim=48)
    wrong.save(tmp_path / "wrong.npz")
    nothing = tmp_path / "nothing.jsonl"
    assert T.run(T.parse_args([str(path), str(tmp_path / "wrong.npz"), "nowhere", str(nothing)])) == T.EXIT_DIMENSION_MISMATCH == 2
    assert "size 48" in capsys.readouterr().err and not nothing.exists()
    for bad in (["--tag", "x"], ["--max-rounds", "0"], ["--within", "line"]):
        with pytest.raises(SystemExit):
            T.parse_args(["m", "i", "d", "o"] + bad)
    with pytest.raises(ValueError, match="min-similarity"):
        T.run(T.parse_args(["m", "i", "d", "o", "--min-similarity", "1.5"]))
    assert "BEYOND THE REFERENCE" in T.__doc__ and "an old warning with an embedding this close was still free" in T.__doc__


def test_refusals():
    from buglab.models import track as T
    from buglab.models._similar import make_index
    from buglab.models.ensemble.wrapper import EnsembleWrapper
    from buglab.models.greatreimplementation import GreatVarMisuse

    sites = _DrawnSites.embed(None, None, [], "cpu", "predicted")
    index = make_index(sites, None, True, "GnnBugLabModel", "ab" * 20)
    great = GreatVarMisuse({"num_layers": 2, "num_heads": 4, "intermediate_dimension": 96, "dropout_rate": 0.0}, vocab_size=64, embedding_dim=64)
    for model, word in ((EnsembleWrapper.__new__(EnsembleWrapper), "ensembles"), (great, "GreatVarMisuse")):
        with pytest.raises(TypeError, match=word):
            T.track_warnings(model, None, index, [], "cpu")
    with pytest.raises(ValueError, match="within"):
        T.track_sites(sites, index, within="line", host=True)
    # a scan without a single site: every old entry is gone, and the index it writes keeps the embedding size
    from buglab.data.synthetic import make_report_dataset

    old = make_index(_DrawnSites.embed(None, None, make_report_dataset(5, seed=2), "cpu", "predicted"), "seen", True, "GnnBugLabModel", "ab" * 20)
    scan = T.track_sites(sites, old, host=True)
    assert [w.status for w in scan.warnings] == ["gone"] * 5 and scan.index.size == 0 and scan.index.dim == old.dim == 32
    assert (scan.summary["num_new"], scan.summary["num_gone"], scan.summary["rounds"]) == (0, 5, 0)


# ------------------------------------------------------------------------------------------------ 5. the ABI
def test_entry_points_check_before_any_hip_call():
    """host-side argument checks of the hip_ops wrappers (plain ValueErrors, no GPU needed) and of the C entry points: a bad call
    never reaches a kernel"""
    import ctypes

    import torch

    from buglab.models import hip_ops

    lib = hip_ops.load_library()
    buf = (ctypes.c_int8 * 4096)()
    ptr = (ctypes.addressof(buf) + 15) // 16 * 16
    EINVAL, ERANGE = -1, -2
    assert lib.bl_track_match_workspace_bytes(10, 7, 3) == 64 + 17 * (8 + 24) + 17 * (4 + 12 + 8)
    assert lib.bl_track_best_workspace_bytes(10, 7, 3) == 64 + 10 * 3 * 8 + (4 * (30 + 17) + 7) // 8 * 8
    assert lib.bl_track_match_workspace_bytes((1 << 20) + 1, 7, 3) == -1 and lib.bl_track_match_workspace_bytes(10, -1, 3) == -1
    assert lib.bl_track_match_workspace_bytes(10, 7, 65) == -1 and lib.bl_track_best_workspace_bytes(10, 7, 0) == -1

    def match(q_old=ptr, ld=64, L=4, N=4, Dp=64, floor=0.5, rounds=2, slices=1, ws=ptr, ws_bytes=1 << 20, m_old=ptr, m_aff=ptr, status=ptr,
              key_old=None, key_new=None):
        return lib.bl_track_match(q_old, ld, ptr, key_old, L, ptr, 64, ptr, key_new, N, Dp, floor, rounds, slices, ws, ws_bytes, m_old, ptr,
                                  m_aff, status, None)

    assert match(q_old=None) == EINVAL and match(m_old=None) == EINVAL and match(status=None) == EINVAL and b"null" in lib.bl_last_error()
    assert match(L=-1) == EINVAL and match(Dp=96) == EINVAL and b"multiple of 64" in lib.bl_last_error()
    assert match(ld=72) == EINVAL and match(ld=48) == EINVAL and match(q_old=ptr + 4) == EINVAL and b"16-byte aligned" in lib.bl_last_error()
    for bad in (0.0, -0.5, 1.0000001, float("nan")):
        assert match(floor=bad) == EINVAL and b"floor" in lib.bl_last_error()
    assert match(rounds=0) == EINVAL and match(rounds=-3) == EINVAL and b"max_rounds" in lib.bl_last_error()
    assert match(rounds=4097) == ERANGE and b"BL_TRACK_MAX_ROUNDS" in lib.bl_last_error()
    assert match(slices=0) == EINVAL and match(slices=65) == EINVAL and b"slices" in lib.bl_last_error()
    assert match(key_old=ptr) == EINVAL and match(key_new=ptr) == EINVAL and b"come together" in lib.bl_last_error()
    assert match(ws=None) == EINVAL and match(ws_bytes=100) == EINVAL and b"workspace" in lib.bl_last_error()
    assert match(m_aff=ptr + 4) == EINVAL and b"8-byte aligned" in lib.bl_last_error()
    assert match(L=(1 << 20) + 1) == ERANGE and b"BL_REVIEW_MAX_ROWS" in lib.bl_last_error()
    assert match(Dp=576, ld=576) == ERANGE and b"BL_SIM_MAX_D" in lib.bl_last_error()

    def best(q_old=ptr, L=4, N=4, Dp=64, floor=0.5, slices=1, ws=ptr, ws_bytes=1 << 20, out=ptr, arg=ptr, key_old=None):
        return lib.bl_track_best_i8(q_old, 64, ptr, key_old, None, L, ptr, 64, ptr, None, None, N, Dp, floor, slices, ws, ws_bytes, out, arg, None)

    assert best(q_old=None) == EINVAL and best(out=None) == EINVAL and best(arg=None) == EINVAL and best(ws=None) == EINVAL
    assert best(floor=0.0) == EINVAL and best(floor=float("nan")) == EINVAL and best(slices=65) == EINVAL and best(key_old=ptr) == EINVAL
    assert best(out=ptr + 4) == EINVAL and best(ws_bytes=10) == EINVAL and best(Dp=32) == EINVAL and best(N=-1) == EINVAL
    assert best(N=(1 << 20) + 1) == ERANGE and best(Dp=576) == ERANGE
    assert best(L=0, q_old=None, out=None, arg=None, ws=None) == 0  # nothing to choose for: nothing launched

    q = torch.zeros((4, 64), dtype=torch.int8)
    n = torch.zeros(4, dtype=torch.int32)
    state = torch.zeros(4, dtype=torch.int32), torch.zeros(4, dtype=torch.int32), torch.zeros(4, dtype=torch.float64)
    with pytest.raises(hip_ops.HipOpsUnavailable):
        hip_ops.track_best(q, n, q, n, 0.5)
    with pytest.raises(hip_ops.HipOpsUnavailable):
        hip_ops.track_match(q, n, q, n, 0.5, *state)
    for bad in (0.0, 1.5, float("nan")):
        with pytest.raises(ValueError, match="floor"):
            hip_ops.track_best(q, n, q, n, bad)
        with pytest.raises(ValueError, match="floor"):
            hip_ops.track_match(q, n, q, n, bad, *state)
    with pytest.raises(ValueError, match="max_rounds"):
        hip_ops.track_match(q, n, q, n, 0.5, *state, max_rounds=0)
    with pytest.raises(ValueError, match="slices"):
        hip_ops.track_best(q, n, q, n, 0.5, slices=65)
    with pytest.raises(ValueError, match="come together"):
        hip_ops.track_match(q, n, q, n, 0.5, *state, key_old=n)
    with pytest.raises(ValueError, match="multiple of 64"):
        hip_ops.track_best(q[:, :60], n, q[:, :60], n, 0.5)
    with pytest.raises(ValueError, match="must be"):
        hip_ops.track_best(q, n[:3], q, n, 0.5)
    with pytest.raises(ValueError, match="open_old"):
        hip_ops.track_best(q, n, q, n, 0.5, open_old=torch.zeros(3, dtype=torch.uint8))
    assert [hip_ops.track_slices(X, Y) for X, Y in ((100, 100), (100, 5000), (100000, 100000), (16, 1 << 20))] == [1, 4, 1, 64]

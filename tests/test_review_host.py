"""CPU: review queues without a GPU -- the NumPy twin of csrc/bl_review.hip (buglab/models/_review.py) against the restatement
in Python integers (tests/review_cases.py) bit for bit, what farthest-point selection promises (monotone pick affinities, the
cover of what is left, twice the optimal radius at most), the cold start, the uncertainty band, the reasons a queue ends, the
command line on the host path with its exit statuses, and the C entry points' argument errors."""
import itertools
import json

import numpy as np
import pytest

from tests import review_cases as RC
from tests.similar_cases import assert_equal_bits, drawn_rows
from tests.test_triage_host import _DrawnSites, _fitted, checkpoint  # noqa: F401  (checkpoint is a fixture)


# ------------------------------------------------------------------------------------------------ 1. the twin against the restatement
@pytest.mark.parametrize("D", [1, 100, 128, 512])
def test_norms_and_cover_equal_the_restatement(D):
    from buglab.models import _review as R

    q, n, qc, nc, best, near = RC.cover_case(D)
    assert_equal_bits([R.norms_host(q)], [n], "norms")
    assert not n[[1, 4, 7]].any() and (np.delete(n, [1, 4, 7]) >= 16129).all() and n.max() <= 512 * 127 * 127
    assert any((qc[j] == qc[:j]).all(axis=1).any() for j in range(1, len(qc)) if nc[j] > 0)  # a centre that is a copy: ties
    assert_equal_bits(R.cover_host(q, n, qc, nc), [best, near], "cover")
    valid = n > 0
    assert (near[valid] >= 0).all() and (near[~valid] == -1).all() and (best[~valid] == -2.0).all()
    assert (best[:37][valid[:37]] == 1.0).all()  # a centre covers itself -- or an earlier copy of it does
    assert (near[:37][valid[:37]] <= np.arange(37)[valid[:37]]).all()
    # two calls over the two halves of the centres equal one call, in either order
    h = 18
    first = R.cover_host(q, n, qc[:h], nc[:h])
    assert_equal_bits(R.cover_host(q, n, qc[h:], nc[h:], *first, first_id=h), [best, near], "two halves")
    second = R.cover_host(q, n, qc[h:], nc[h:], first_id=h)
    assert_equal_bits(R.cover_host(q, n, qc[:h], nc[:h], *second), [best, near], "two halves, the later first")
    # ... and the restatement agrees that the state is combined in the same order
    assert_equal_bits(RC.cover_ref(q, n, qc[h:], nc[h:], *RC.cover_ref(q, n, qc[:h], nc[:h]), first_id=h), [best, near], "restated halves")


@pytest.mark.parametrize("kind", ["mixed", "heavy"])
def test_greedy_equals_the_restatement_and_keeps_its_promises(kind):
    from buglab.models import _review as R

    q, n, eligible, best0, near0, want = RC.greedy_case(kind)
    got = R.greedy_host(q, n, best0, near0, 40, eligible, 1.0)
    assert_equal_bits(got, want, kind)
    picks, aff, pnear, best, near = got
    assert (picks >= 20).all() and len(set(picks.tolist())) == 40 and eligible[picks].all() and (n[picks] > 0).all()
    assert (np.diff(aff) >= 0).all(), "pick affinities are non-decreasing"
    left = (eligible != 0) & (n > 0)
    left[picks] = False
    assert left.any() and (best[left] >= aff[-1]).all(), "every unpicked eligible row is covered at least as well as the last pick was"
    assert (best[picks] == 1.0).all() and (near[picks] == picks).all()
    assert (pnear < 20).sum() > 0 and all(p in picks[:k].tolist() for k, p in enumerate(pnear.tolist()) if p >= 20)
    assert best0.tobytes() == RC.greedy_case(kind)[3].tobytes()  # the state that came in was not written


def test_greedy_ends_where_the_definition_says():
    from buglab.models import _review as R

    q, n = RC.images_of(RC.repeated_rows(), center=False)
    fresh = (np.full(50, -2.0), np.full(50, -1, np.int32))
    want = RC.greedy_ref(q, n, *fresh, 20)
    # the ten distinct rows, each at its first copy (the lowest index among equals), in farthest-first order; then nothing
    assert want[0][0] == 0 and sorted(want[0][:10].tolist()) == list(range(10)) and (want[0][10:] == -1).all()
    assert not want[1][10:].any() and want[1][0] == -2.0 and (want[3] == 1.0).all() and (want[4] == np.arange(50) % 10).all()
    assert_equal_bits(R.greedy_host(q, n, *fresh, 20), want, "10 distinct rows five times")
    early = RC.greedy_ref(q, n, *fresh, 20, None, 0.9 * 0.9)
    assert_equal_bits(R.greedy_host(q, n, *fresh, 20, None, 0.9 * 0.9), early, "stop = 0.9^2")
    assert 1 <= (early[0] >= 0).sum() <= 10 and (early[3][early[0][early[0] >= 0]] == 1.0).all()
    none = R.greedy_host(q, n, *fresh, 5, np.zeros(50, np.uint8))
    assert (none[0] == -1).all() and none[3].tobytes() == fresh[0].tobytes() and none[4].tobytes() == fresh[1].tobytes()
    assert_equal_bits(none, RC.greedy_ref(q, n, *fresh, 5, np.zeros(50, np.uint8)), "nobody eligible")
    one = R.greedy_host(q[:1], n[:1], fresh[0][:1], fresh[1][:1], 3)
    assert one[0].tolist() == [0, -1, -1] and one[3].tolist() == [1.0] and one[4].tolist() == [0]
    e = np.zeros(50, np.uint8)
    e[[17, 33]] = 1
    assert R.greedy_host(q, n, *fresh, 1, e)[0].tolist() == [17]  # no centres: the lowest eligible index
    with pytest.raises(ValueError):
        R.greedy_host(q, n, *fresh, 5, None, 0.0)
    with pytest.raises(ValueError):
        R.greedy_host(q, n, *fresh, R.MAX_BUDGET + 1)
    with pytest.raises(ValueError, match="max-similarity"):
        R.stop_of(float("nan"))


def test_greedy_radius_is_at_most_twice_the_optimum_by_enumeration():
    """M = 12, B = 3: the radius of a choice is the greatest angle (of the images) from a row to its nearest chosen row.  Angles
    are a metric, the affinity is monotone in the angle, so Gonzalez' bound holds: greedy <= 2 optimum, the optimum by
    enumerating all 220 choices.  1e-9 covers the rounding of arccos."""
    from buglab.models import _review as R

    for seed in range(6):
        q, n = RC.images_of(RC.clustered_rows(12, 8, 4, seed)[0])
        assert (n > 0).all()
        g = q.astype(np.int64) @ q.astype(np.int64).T
        angle = np.arccos(np.clip(g / np.sqrt(np.outer(n.astype(np.int64), n.astype(np.int64)).astype(np.float64)), -1.0, 1.0))
        radius = lambda chosen: angle[:, list(chosen)].min(axis=1).max()
        optimum = min(radius(c) for c in itertools.combinations(range(12), 3))
        picks = R.greedy_host(q, n, np.full(12, -2.0), np.full(12, -1, np.int32), 3)[0]
        assert len(set(picks.tolist())) == 3 and radius(picks.tolist()) <= 2.0 * optimum + 1e-9, (seed, radius(picks.tolist()), optimum)


def test_the_exact_selection_agrees_where_the_images_decide_nothing():
    """well-separated clusters: fp64 on the rows and integers on the images pick the same clusters in the same order"""
    from buglab.models import _review as R
    from buglab.models._similar import column_mean, quantize_host

    x, member = RC.clustered_rows(200, 32, 6, seed=4, noise=0.05)
    c, q, sumsq, r = quantize_host(x, column_mean(x))
    n = R.norms_host(q)
    picks = R.greedy_host(q, n, np.full(200, -2.0), np.full(200, -1, np.int32), len(set(member.tolist())))[0]
    exact, best, valid = R.greedy_exact_host(c, 0, len(picks))
    assert valid.all() and sorted(member[picks].tolist()) == sorted(set(member.tolist())) == sorted(member[exact].tolist())
    assert member[picks].tolist() == member[exact].tolist() and np.allclose(best[exact], 1.0, rtol=0, atol=1e-12)


# ------------------------------------------------------------------------------------------------ 2. the queue
def _sites(rows, logprobs):
    from buglab.models._similar import SiteEmbeddings

    N = rows.shape[0]
    return SiteEmbeddings(rows, np.arange(100, 100 + N, dtype=np.int64), np.arange(N, dtype=np.int32), logprobs.astype(np.float32),
                          [f"n{i}" for i in range(N)], [f"f{i}.py" for i in range(N)], ["pkg"] * N, [""] * N, N + 3, 1, 2)


def test_cold_start_band_and_end_reasons():
    from buglab.models import _review as R
    from buglab.models import _triage as TR
    from buglab.models import review as T
    from buglab.models._similar import DimensionMismatch, make_index

    x, member = RC.clustered_rows(120, 5, 5, seed=2)
    rng = np.random.default_rng(0)
    lp = np.log(rng.uniform(0.05, 1.0, size=120))
    x[3] = 0.0  # an embedding that centres to something, and one that is not finite
    x[11, 2] = np.nan
    lp[11] = 0.0  # the most probable of all is invalid: never the first pick
    # cold start: no reviewed rows -> the most probable valid eligible warning first, with nothing nearer
    sel = T.queue_embeddings(x, 8, lp, host=True)
    order = np.argsort(-lp, kind="stable")
    assert sel.picks[0] == order[1] != 11 == order[0] and sel.pick_affinity[0] == -2.0 and sel.pick_near[0] == -1
    assert sel.picks.shape == (8,) and sel.end == R.END_BUDGET and not sel.valid[11] and (np.diff(sel.pick_affinity) >= 0).all()
    assert all(0 <= p < k for k, p in enumerate([sel.picks.tolist().index(v) for v in sel.pick_near[1:].tolist()], 1))
    assert (np.abs(sel.pick_similarity[1:]) <= 1.0).all() and sel.pick_similarity[0] == 0.0 and sel.stands_for.sum() == sel.open.sum() == 119
    # the int8 affinity and the re-scored cosine tell the same story
    assert np.allclose(R.cosine_of(sel.pick_affinity[1:]), sel.pick_similarity[1:], atol=0.05)
    # the queue is eligible rows only, and with fewer eligible rows than budget it ends with nothing left
    mask = np.zeros(120, bool)
    mask[[5, 11, 40, 77]] = True
    few = T.queue_embeddings(x, 8, lp, eligible=mask, host=True)
    assert sorted(few.picks.tolist()) == [5, 40, 77] and few.end == R.END_NOTHING_LEFT and few.picks[0] == max((5, 40, 77), key=lambda i: lp[i])
    # --max-similarity ends it early, and says so
    early = T.queue_embeddings(x, 100, lp, max_similarity=0.5, host=True)
    assert 1 <= early.picks.shape[0] < 100 and early.end == R.END_MAX_SIMILARITY and early.worst >= 0.25
    assert (early.best[early.open] >= 0.25).all()
    # reviewed rows come first in the row space, are never picked, and nearest items point at them
    sites = _sites(x, lp)
    index = make_index(_sites(x[:30].copy(), lp[:30]), "seen", True, "GnnBugLabModel", "ab" * 20)
    keep = np.r_[0:3, 4:11, 12:30]
    index = index._replace(**{f: getattr(index, f)[keep] for f in ("embeddings", "positions", "nodes", "labels", "paths", "packages", "scouts", "tags")})
    after = T.review_sites(_sites(x[30:].copy(), lp[30:]), 6, reviewed=index, host=True)
    assert [w.rank for w in after.warnings] == list(range(6)) and after.summary["num_reviewed"] == 28 and after.summary["end"] == "budget"
    assert after.warnings[0].nearest["reviewed"]["tag"] == "seen" and -1.0 <= after.warnings[0].nearest["similarity"] <= 1.0
    assert all(("reviewed" in w.nearest) != ("rank" in w.nearest) for w in after.warnings)
    assert all(w.nearest["rank"] < w.rank for w in after.warnings if "rank" in w.nearest)
    curve = after.summary["coverage"]
    assert [p["picks"] for p in curve] == [1, 2, 4, 6] and curve[-1]["worst_similarity"] == after.summary["worst_similarity"]
    assert all(a["worst_similarity"] <= b["worst_similarity"] for a, b in zip(curve, curve[1:]))
    assert after.summary["beats_most_confident"] in (True, False) and after.summary["most_confident_worst_similarity"] is not None
    with pytest.raises(DimensionMismatch, match="size 5"):
        T.review_sites(_sites(drawn_rows(4, 7, 1), lp[:4]), 2, reviewed=index, host=True)
    # the band: only warnings the re-ranker is unsure about are queued, and the rest are counted
    triage = _fitted(D=5)
    z, p = TR.score_host(x, lp.astype(np.float32), triage.shift, triage.scale, triage.w)
    unsure = (p >= 0.3) & (p <= 0.7)
    assert 3 < unsure.sum() < 110
    banded = T.review_sites(sites, 200, triage=triage, band=(0.3, 0.7), host=True)
    assert sorted(w.position - 100 for w in banded.warnings) == np.flatnonzero(unsure & (np.arange(120) != 11)).tolist()
    assert all(0.3 <= w.triage_probability <= 0.7 for w in banded.warnings) and banded.summary["end"] == "nothing-left"
    assert banded.summary["num_outside_band"] == 120 - unsure.sum() and banded.summary["uncertainty_band"] == [0.3, 0.7]
    assert banded.summary["num_eligible"] == len(banded.warnings) and "triage_probability" in banded.warnings[0].record()
    with pytest.raises(ValueError, match="band"):
        T.review_sites(sites, 5, triage=triage, band=(0.8, 0.2), host=True)
    # --min-confidence filters before anything else
    cut = float(np.exp(np.median(lp)))
    confident = T.review_sites(sites, 5, min_confidence=cut, host=True)
    kept = np.exp(lp.astype(np.float32).astype(np.float64)) >= cut
    assert confident.summary["num_below_confidence"] == 120 - kept.sum() and all(kept[w.position - 100] for w in confident.warnings)
    # nothing to queue
    empty = T.review_sites(_sites(np.zeros((0, 5), np.float32), np.zeros(0)), 5, host=True)
    assert empty.warnings == [] and empty.summary["end"] == "nothing-left" and empty.summary["worst_similarity"] is None


def test_the_queue_covers_better_than_the_most_confident_on_clustered_warnings():
    """one big confident cluster and a few small ones: "most confident first" reviews the big one B times"""
    from buglab.models import review as T

    x, member = RC.clustered_rows(400, 16, 8, seed=6, noise=0.2)
    lp = np.where(member == 0, -0.05, -1.5) + 0.01 * np.random.default_rng(1).standard_normal(400)
    sel = T.queue_embeddings(x, 8, lp, host=True)
    assert set(member[sel.picks].tolist()) == set(member.tolist()) and sel.worst > sel.confident_worst
    assert sel.stands_for.sum() == 400 and sel.stands_for[0] >= (member == 0).sum() * 0.9


# ------------------------------------------------------------------------------------------------ 3. the command line
def test_command_line_on_the_host(checkpoint, tmp_path, monkeypatch, capsys):
    from buglab.models import review as T
    from buglab.models._similar import make_index

    path, data = checkpoint
    seen, scan = data[:40], data[40:]
    real_open = T._open_model
    monkeypatch.setattr(T, "_open_model", lambda p: real_open(p)[:3] + (True,))  # the untrained model itself; the GPU is not asked for
    monkeypatch.setattr(T, "_read_data", lambda p, limit: {"scan": scan}[p][:limit])
    monkeypatch.setattr(T, "_embed_sites", _DrawnSites.embed)
    index = make_index(_DrawnSites.embed(None, None, seen, "cpu", "predicted"), "seen", True, "GnnBugLabModel", "ab" * 20)
    index.save(tmp_path / "reviewed.npz")
    _fitted(D=32).save(tmp_path / "triage.npz")

    out, report = tmp_path / "queue.jsonl", tmp_path / "queue.json"
    status = T.run(T.parse_args([str(path), "scan", str(out), "--budget", "12", "--reviewed", str(tmp_path / "reviewed.npz"), "--host",
                                 "--report-json", str(report), "--sequential"]))
    assert status == 0 and "review: 12 of 80 eligible warnings" in capsys.readouterr().out
    records = [json.loads(line) for line in out.read_text().splitlines()]
    s = json.loads(report.read_text())
    assert len(records) == 12 == s["num_picked"] and s["end"] == "budget" and s["num_reviewed"] == 40 and s["num_warnings"] == 80
    assert [r["rank"] for r in records] == list(range(12)) and len({r["position"] for r in records}) == 12
    assert s["picked_positions"] == [r["position"] for r in records]
    assert set(records[0]) == {"rank", "position", "node", "label", "filename", "package", "logprob", "nearest", "stands_for"}
    assert records[0]["nearest"]["reviewed"]["tag"] == "seen" and sum(r["stands_for"] for r in records) <= 80
    assert s["coverage"][0]["picks"] == 1 and s["coverage"][-1]["picks"] == 12 and s["beats_most_confident"] is True
    # with a re-ranker: only the band is queued
    banded = tmp_path / "banded.jsonl"
    assert T.run(T.parse_args([str(path), "scan", str(banded), "--budget", "80", "--triage", str(tmp_path / "triage.npz"), "--host",
                               "--uncertainty-band", "0.1", "0.9", "--report-json", str(report)])) == 0
    lines = [json.loads(line) for line in banded.read_text().splitlines()]
    s = json.loads(report.read_text())
    # (the stub's embedding depends on a sample's path alone, so some warnings are copies: they are never queued twice)
    assert 0 < len(lines) <= s["num_eligible"] == 80 - s["num_outside_band"] < 80 and s["num_reviewed"] == 0
    # at the default S = 1 what is left are exact copies: that is "nothing-left", and the copies are counted
    assert (s["end"], s["worst_similarity"]) == ("nothing-left", 1.0) and s["num_left_as_copies"] == s["num_eligible"] - len(lines)
    assert len({r["filename"] for r in lines}) == len(lines)
    assert all(0.1 <= r["triage_probability"] <= 0.9 for r in lines) and lines[0]["nearest"] is None and lines[1]["nearest"]["rank"] == 0
    assert lines[0]["logprob"] == max(r["logprob"] for r in lines)  # the cold start
    capsys.readouterr()
    # files of another embedding size: status 2 before any data is read, nothing written
    wrong = index._replace(embeddings=np.zeros((index.size, 48), np.float32), mean=np.zeros(48, np.float32), dim=48)
    wrong.save(tmp_path / "wrong.npz")
    other = tmp_path / "other.jsonl"
    assert T.run(T.parse_args([str(path), "nowhere", str(other), "--budget", "5", "--reviewed", str(tmp_path / "wrong.npz")])) == 2
    assert "size 48" in capsys.readouterr().err and not other.exists()
    _fitted(D=5).save(tmp_path / "small.npz")
    assert T.run(T.parse_args([str(path), "nowhere", str(other), "--budget", "5", "--triage", str(tmp_path / "small.npz")])) == T.EXIT_DIMENSION_MISMATCH
    assert "size 5" in capsys.readouterr().err and not other.exists()
    for bad in (["--budget", "-1"], ["--budget", "5", "--uncertainty-band", "0.2", "0.8"], []):
        with pytest.raises(SystemExit):
            T.parse_args(["m", "d", "o"] + bad)
    with pytest.raises(ValueError, match="max-similarity"):
        T.run(T.parse_args(["m", "d", "o", "--budget", "5", "--max-similarity", "1.5"]))
    assert "BEYOND THE REFERENCE" in T.__doc__


def test_refusals():
    from buglab.models import review as T
    from buglab.models.ensemble.wrapper import EnsembleWrapper

    with pytest.raises(TypeError, match="ensembles"):
        T.review_queue(EnsembleWrapper.__new__(EnsembleWrapper), None, [], "cpu", 5)
    with pytest.raises(ValueError, match="budget"):
        T.queue_embeddings(np.zeros((3, 4), np.float32), 1 << 20, host=True)
    with pytest.raises(ValueError):
        T.queue_embeddings(np.zeros((3, 513), np.float32), 2, host=True)


# ------------------------------------------------------------------------------------------------ 4. the ABI
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
    assert [hip_ops.review_blocks(M) for M in (0, 1, 64, 65, 133, 65536, 65537, 1 << 20)] == [1, 1, 1, 2, 3, 1024, 1024, 1024]
    assert [lib.bl_review_blocks(M) for M in (0, 1, 64, 65, 133, 65536, 65537, 1 << 20)] == [1, 1, 1, 2, 3, 1024, 1024, 1024]
    assert lib.bl_review_workspace_bytes(100) == hip_ops.review_workspace_bytes(100) == 16 + 2 * 1024 * 12
    assert lib.bl_review_workspace_bytes((1 << 20) + 1) == -1 and lib.bl_review_cover_workspace_bytes(10, 3) == 360
    assert lib.bl_review_cover_workspace_bytes(10, 65) == -1
    assert lib.bl_review_norms(None, 64, 4, 64, ptr, None) == EINVAL and b"null" in lib.bl_last_error()
    assert lib.bl_review_norms(ptr + 4, 64, 4, 64, ptr, None) == EINVAL and b"16-byte aligned" in lib.bl_last_error()
    assert lib.bl_review_norms(ptr, 64, 4, 100, ptr, None) == EINVAL and b"multiple of 64" in lib.bl_last_error()
    assert lib.bl_review_norms(ptr, 72, 4, 64, ptr, None) == EINVAL and lib.bl_review_norms(ptr, 48, 4, 64, ptr, None) == EINVAL
    assert lib.bl_review_norms(ptr, 576, 4, 576, ptr, None) == ERANGE and b"BL_SIM_MAX_D" in lib.bl_last_error()
    assert lib.bl_review_norms(ptr, 64, (1 << 20) + 1, 64, ptr, None) == ERANGE and b"BL_REVIEW_MAX_ROWS" in lib.bl_last_error()
    assert lib.bl_review_norms(None, 64, 0, 64, None, None) == 0

    def greedy(q=ptr, ld=64, M=4, Dp=64, B=2, stop=1.0, blocks=0, ws=ptr, ws_bytes=1 << 20, best=ptr, picks=ptr, aff=ptr):
        return lib.bl_review_greedy(q, ld, ptr, None, M, Dp, B, stop, blocks, ws, ws_bytes, best, ptr, picks, aff, ptr, None)

    assert greedy(q=None) == EINVAL and greedy(best=None) == EINVAL and greedy(picks=None) == EINVAL and b"null" in lib.bl_last_error()
    assert greedy(B=-1) == EINVAL and greedy(M=-1) == EINVAL and greedy(Dp=96) == EINVAL and greedy(ld=80 - 8) == EINVAL
    assert greedy(B=16385) == ERANGE and b"BL_REVIEW_MAX_BUDGET" in lib.bl_last_error()
    assert greedy(M=(1 << 20) + 1) == ERANGE and greedy(Dp=576, ld=576) == ERANGE
    for bad in (0.0, -0.5, 1.0000001, float("nan")):
        assert greedy(stop=bad) == EINVAL and b"stop" in lib.bl_last_error()
    assert greedy(blocks=-1) == EINVAL and greedy(blocks=1025) == EINVAL and b"blocks" in lib.bl_last_error()
    assert greedy(ws=None) == EINVAL and greedy(ws_bytes=100) == EINVAL and b"workspace" in lib.bl_last_error()
    assert greedy(best=ptr + 4) == EINVAL and greedy(aff=ptr + 4) == EINVAL and b"8-byte aligned" in lib.bl_last_error()
    assert greedy(B=0, q=None, ws=None, picks=None) == 0  # nothing to pick: nothing launched

    def cover(q=ptr, qc=ptr, M=4, L=4, first=0, Dp=64, slices=1, ws=ptr, ws_bytes=1 << 20, best=ptr):
        return lib.bl_review_cover_i8(q, 64, ptr, M, qc, 64, ptr, L, first, Dp, slices, ws, ws_bytes, best, ptr, None)

    assert cover(q=None) == EINVAL and cover(qc=None) == EINVAL and cover(best=None) == EINVAL
    assert cover(slices=0) == EINVAL and cover(slices=65) == EINVAL and cover(first=-1) == EINVAL and cover(first=0x7FFFFFFF) == EINVAL
    assert cover(Dp=32) == EINVAL and cover(ws_bytes=47) == EINVAL and cover(L=(1 << 20) + 1) == ERANGE
    assert cover(L=0, qc=None, ws=None) == 0 and cover(M=0, q=None, best=None, ws=None) == 0  # nothing to do: nothing launched

    q = torch.zeros((4, 64), dtype=torch.int8)
    n, best, near = torch.zeros(4, dtype=torch.int32), torch.zeros(4, dtype=torch.float64), torch.zeros(4, dtype=torch.int32)
    with pytest.raises(hip_ops.HipOpsUnavailable):
        hip_ops.review_norms(q)
    with pytest.raises(ValueError, match="multiple of 64"):
        hip_ops.review_norms(q[:, :60])
    with pytest.raises(ValueError, match="budget"):
        hip_ops.review_greedy(q, n, best, near, 16385)
    with pytest.raises(ValueError, match="stop"):
        hip_ops.review_greedy(q, n, best, near, 2, stop=0.0)
    with pytest.raises(ValueError, match="blocks"):
        hip_ops.review_greedy(q, n, best, near, 2, blocks=0)
    with pytest.raises(ValueError, match="slices"):
        hip_ops.review_cover(q, n, q, n, slices=65)
    with pytest.raises(ValueError, match="leave int32"):
        hip_ops.review_cover(q, n, q, n, first_id=-1)

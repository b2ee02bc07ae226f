"""GPU: review queues on the MI355X -- the kernels of csrc/bl_review.hip against the restatement in Python integers
(tests/review_cases.py, which tests/test_review_host.py also pins the NumPy twin to) bit for bit: norms; the cover for every
shape that reaches another branch of the GEMM, for every number of slices and for two calls instead of one; the greedy chain
for every number of workgroups, with the winner in another workgroup than most rows, and at every way a queue ends; strided
images and outputs inside poisoned guard bands, argument errors; and `review` end to end on two tiny untrained models, the
device path against `--host`.

No tolerance anywhere: every output is an integer or one IEEE quotient of two exact integers."""
import json

import numpy as np
import pytest
import torch

from tests import review_cases as RC
from tests import similar_cases as C
from tests.guard_bands import guarded
from tests.test_group_gpu import untrained  # noqa: F401  (a fixture)
from tests.test_similar_gpu import DEV, SPECS, _deterministic, _dev, _stream
from tests.test_triage_host import _fitted

pytestmark = pytest.mark.gpu



def _host(*tensors):
    return [t.cpu().numpy() for t in tensors]


# ------------------------------------------------------------------------------------------------ bl_review_norms
@pytest.mark.parametrize("D", [1, 100, 512])
def test_norms_equal_the_restatement(D):
    from buglab.models import hip_ops

    for M in (1, 5, 67):
        q, n = RC.images_of(RC.mixed_rows(M, D, seed=M + D, noise=1.0), center=False)
        assert M < 5 or n[4] == 0
        C.assert_equal_bits(_host(hip_ops.review_norms(_dev(q))), [n], (D, M))
    full = np.full((3, (D + 63) // 64 * 64), -127, np.int8)  # the largest norm a row of this width can have
    C.assert_equal_bits(_host(hip_ops.review_norms(_dev(full))), [np.full(3, full.shape[1] * 16129, np.int32)], (D, "all -127"))


# ------------------------------------------------------------------------------------------------ bl_review_cover_i8
@pytest.mark.parametrize("D", [1, 100, 128, 512])  # one column; padding columns; two whole k-chunks; eight
def test_cover_equals_the_restatement_for_every_cut(D):
    from buglab.models import hip_ops

    q, n, qc, nc, best, near = RC.cover_case(D)  # 150 rows, 37 centres with copies among them, rows 1, 4, 7 invalid
    d_q, d_n, d_qc, d_nc = (_dev(a) for a in (q, n, qc, nc))
    for slices in (None, 1, 3):
        C.assert_equal_bits(_host(*hip_ops.review_cover(d_q, d_n, d_qc, d_nc, slices=slices)), [best, near], (D, slices))
    h = 18  # two calls over the two halves equal one call: the lower-indexed centres first, and the other way round
    state = hip_ops.review_cover(d_q, d_n, d_qc[:h], d_nc[:h], slices=3)
    again = hip_ops.review_cover(d_q, d_n, d_qc[h:], d_nc[h:], *state, first_id=h)
    assert again[0].data_ptr() == state[0].data_ptr()  # updated in place
    C.assert_equal_bits(_host(*again), [best, near], (D, "two halves"))
    state = hip_ops.review_cover(d_q, d_n, d_qc[h:], d_nc[h:], first_id=h)
    C.assert_equal_bits(_host(*hip_ops.review_cover(d_q, d_n, d_qc[:h], d_nc[:h], *state, slices=3)), [best, near], (D, "the later half first"))
    first = hip_ops.review_cover(d_q, d_n, d_qc, d_nc)
    assert all(a.tobytes() == b.tobytes() for a, b in zip(_host(*first), _host(*hip_ops.review_cover(d_q, d_n, d_qc, d_nc))))


def test_cover_with_more_centres_than_a_slice_and_rows_that_are_no_multiple_of_the_tile():
    """1100 centres: slices of at least two tiles per wave, a ragged last tile, the default cut; the twin as the reference, which
    tests/test_review_host.py pins to the restatement"""
    from buglab.models import hip_ops
    from buglab.models._review import cover_host

    q, n = RC.images_of(RC.heavy_tailed_rows(1100, 100, seed=4))
    rows = slice(1000, 1077)
    want = cover_host(q[rows], n[rows], q, n, first_id=5)
    d_q, d_n = _dev(q), _dev(n)
    for slices in (None, 1, 7, 64):
        C.assert_equal_bits(_host(*hip_ops.review_cover(d_q[rows], d_n[rows], d_q, d_n, first_id=5, slices=slices)), want, slices)
    assert (want[1] == np.arange(1000, 1077) + 5).all() and (want[0] == 1.0).all()  # every row finds itself among the centres


# ------------------------------------------------------------------------------------------------ bl_review_greedy
def _greedy(q, n, best0, near0, B, eligible=None, stop=1.0, blocks=None):
    from buglab.models import hip_ops

    best, near = _dev(best0), _dev(near0)
    lists = hip_ops.review_greedy(_dev(q), _dev(n), best, near, B, eligible=None if eligible is None else _dev(eligible), stop=stop,
                                  blocks=blocks)
    return _host(*lists, best, near)


@pytest.mark.parametrize("kind", ["mixed", "heavy"])
def test_greedy_equals_the_restatement_for_every_number_of_workgroups(kind):
    from buglab.models import hip_ops

    q, n, eligible, best0, near0, want = RC.greedy_case(kind)  # M = 300, D = 100, B = 40, 20 reviewed rows, every third row left out
    assert hip_ops.review_blocks(300) == 5
    for blocks in (1, 3, None):
        C.assert_equal_bits(_greedy(q, n, best0, near0, 40, eligible, blocks=blocks), want, (kind, blocks))
    again = _greedy(q, n, best0, near0, 40, eligible)
    assert all(a.tobytes() == b.tobytes() for a, b in zip(again, _greedy(q, n, best0, near0, 40, eligible)))


def test_the_winner_lies_in_another_workgroup_than_most_rows():
    from buglab.models import hip_ops

    M = 2 * hip_ops.REVIEW_ROWS_PER_BLOCK + 5
    q, n = RC.images_of(RC.drawn_rows(M, 64, seed=12))
    fresh = (np.full(M, -2.0), np.full(M, -1, np.int32))
    want = RC.greedy_ref(q, n, *fresh, 8)
    per = -(-M // 3)
    assert hip_ops.review_blocks(M) == 3 and len({int(p) // per for p in want[0]}) == 3  # picks in all three workgroups
    for blocks in (None, 2, 133, 1024):
        C.assert_equal_bits(_greedy(q, n, *fresh, 8, blocks=blocks), want, blocks)


def test_every_way_a_queue_ends():
    q, n = RC.images_of(RC.repeated_rows(), center=False)  # 10 distinct rows, five times
    fresh = (np.full(50, -2.0), np.full(50, -1, np.int32))
    want = RC.greedy_ref(q, n, *fresh, 20)
    assert (want[0][:10] >= 0).all() and (want[0][10:] == -1).all()
    C.assert_equal_bits(_greedy(q, n, *fresh, 20), want, "10 picks, then -1")
    early = RC.greedy_ref(q, n, *fresh, 20, None, 0.9 * 0.9)
    assert (early[0] >= 0).sum() <= 10
    C.assert_equal_bits(_greedy(q, n, *fresh, 20, stop=0.9 * 0.9), early, "stop = 0.9^2")
    nobody = _greedy(q, n, *fresh, 6, np.zeros(50, np.uint8))
    C.assert_equal_bits(nobody, [np.full(6, -1, np.int32), np.zeros(6), np.full(6, -1, np.int32), *fresh], "nobody eligible")
    C.assert_equal_bits(_greedy(q[:1], n[:1], fresh[0][:1], fresh[1][:1], 3), RC.greedy_ref(q[:1], n[:1], fresh[0][:1], fresh[1][:1], 3), "M = 1")
    C.assert_equal_bits(_greedy(q, n, *fresh, 1), RC.greedy_ref(q, n, *fresh, 1), "B = 1")
    e = np.zeros(50, np.uint8)
    e[[17, 33]] = 1
    lowest = _greedy(q, n, *fresh, 1, e)
    assert lowest[0].tolist() == [17] and lowest[1].tolist() == [-2.0] and lowest[2].tolist() == [-1]  # no centres: the lowest eligible index
    C.assert_equal_bits(lowest, RC.greedy_ref(q, n, *fresh, 1, e), "no centres")
    invalid = q.copy()
    invalid[:] = 0
    C.assert_equal_bits(_greedy(invalid, np.zeros(50, np.int32), *fresh, 2), [np.full(2, -1, np.int32), np.zeros(2), np.full(2, -1, np.int32), *fresh],
                        "no valid row")


# ------------------------------------------------------------------------------------------------ the ABI
def _f64_guard(rows):
    g = guarded(rows, 2, ld=2, dtype=torch.int32, device=DEV, lead=6, any_width=True)  # doubles as int32 pairs, 8-byte aligned
    assert g.data_ptr() % 8 == 0
    return g


def _f64_of(g):
    return g.view.contiguous().cpu().numpy().view(np.float64)[:, 0]


def test_strided_images_and_outputs_inside_guard_bands():
    from buglab.models import hip_ops

    q, n, eligible, best0, near0, want = RC.greedy_case("mixed")
    M, Dp, L, B = 300, 128, 20, 40
    lib = hip_ops.load_library()
    g_q = guarded(M, Dp, ld=Dp + 16, dtype=torch.int8, device=DEV)  # the padding columns of every row hold the pattern
    g_q.view.copy_(_dev(q))
    assert g_q.data_ptr() % 16 == 0
    # the wrapper takes the strided view as it is
    C.assert_equal_bits(_host(hip_ops.review_norms(g_q.view)), [n], "strided norms")
    g_n = guarded(M, 1, ld=1, dtype=torch.int32, device=DEV, any_width=True)
    g_near = guarded(M, 1, ld=1, dtype=torch.int32, device=DEV, any_width=True)
    g_best = _f64_guard(M)
    g_picks, g_pnear = (guarded(B, 1, ld=1, dtype=torch.int32, device=DEV, any_width=True) for _ in range(2))
    g_aff = _f64_guard(B)
    g_near.view.fill_(-1)
    g_best.view.copy_(torch.full((M,), -2.0, dtype=torch.float64, device=DEV).view(torch.int32).view(M, 2))
    need_c, need_g = lib.bl_review_cover_workspace_bytes(M, 3), lib.bl_review_workspace_bytes(M)
    g_wc, g_wg = _f64_guard(need_c // 8), _f64_guard(need_g // 8)
    d_e = _dev(eligible)
    assert lib.bl_review_norms(g_q.data_ptr(), Dp + 16, M, Dp, g_n.data_ptr(), _stream()) == 0, lib.bl_last_error()
    rc = lib.bl_review_cover_i8(g_q.data_ptr(), Dp + 16, g_n.data_ptr(), M, g_q.data_ptr(), Dp + 16, g_n.data_ptr(), L, 0, Dp, 3, g_wc.data_ptr(),
                                need_c, g_best.data_ptr(), g_near.data_ptr(), _stream())
    assert rc == 0, lib.bl_last_error()
    C.assert_equal_bits([_f64_of(g_best), g_near.view[:, 0].cpu().numpy()], [best0, near0], "cover in guard bands")
    rc = lib.bl_review_greedy(g_q.data_ptr(), Dp + 16, g_n.data_ptr(), d_e.data_ptr(), M, Dp, B, 1.0, 3, g_wg.data_ptr(), need_g,
                              g_best.data_ptr(), g_near.data_ptr(), g_picks.data_ptr(), g_aff.data_ptr(), g_pnear.data_ptr(), _stream())
    assert rc == 0, lib.bl_last_error()
    for g, name in ((g_q, "q"), (g_n, "n"), (g_near, "near"), (g_best, "best"), (g_picks, "picks"), (g_pnear, "pick_near"), (g_aff, "pick_aff"),
                    (g_wc, "cover workspace"), (g_wg, "greedy workspace")):
        g.assert_untouched(name)
    C.assert_equal_bits([g_n.view[:, 0].cpu().numpy()], [n], "norms in guard bands")
    got = [g_picks.view[:, 0].cpu().numpy(), _f64_of(g_aff), g_pnear.view[:, 0].cpu().numpy(), _f64_of(g_best), g_near.view[:, 0].cpu().numpy()]
    C.assert_equal_bits(got, want, "greedy in guard bands")
    # the strided view through the wrappers, all the way
    d_n = hip_ops.review_norms(g_q.view)
    state = hip_ops.review_cover(g_q.view, d_n, g_q.view[:L], d_n[:L], slices=3)
    lists = hip_ops.review_greedy(g_q.view, d_n, *state, B, eligible=d_e)
    C.assert_equal_bits(_host(*lists, *state), want, "strided, through the wrappers")
    g_q.assert_untouched("q")


def test_argument_errors_are_returned_without_a_launch():
    from buglab.models import hip_ops

    q, n, eligible, best0, near0, _ = RC.greedy_case("mixed")
    M, Dp = 300, 128
    d_q, d_n, d_e = _dev(q), _dev(n), _dev(eligible)
    best, near = _dev(best0), _dev(near0)
    picks, pnear = torch.full((4,), 7, dtype=torch.int32, device=DEV), torch.full((4,), 7, dtype=torch.int32, device=DEV)
    aff = torch.full((4,), 7.0, dtype=torch.float64, device=DEV)
    ws = torch.zeros(1 << 14, dtype=torch.float64, device=DEV)
    lib = hip_ops.load_library()
    EINVAL, ERANGE = -1, -2

    def greedy(q_ptr=d_q.data_ptr(), ld=Dp, m=M, dp=Dp, b=4, stop=1.0, blocks=0, ws_ptr=ws.data_ptr(), ws_bytes=ws.numel() * 8,
               best_ptr=best.data_ptr(), picks_ptr=picks.data_ptr()):
        return lib.bl_review_greedy(q_ptr, ld, d_n.data_ptr(), d_e.data_ptr(), m, dp, b, stop, blocks, ws_ptr, ws_bytes, best_ptr, near.data_ptr(),
                                    picks_ptr, aff.data_ptr(), pnear.data_ptr(), _stream())

    def cover(q_ptr=d_q.data_ptr(), ld=Dp, m=M, l=20, first=0, dp=Dp, slices=1, ws_bytes=ws.numel() * 8, best_ptr=best.data_ptr()):
        return lib.bl_review_cover_i8(q_ptr, ld, d_n.data_ptr(), m, d_q.data_ptr(), Dp, d_n.data_ptr(), l, first, dp, slices, ws.data_ptr(),
                                      ws_bytes, best_ptr, near.data_ptr(), _stream())

    assert greedy(q_ptr=None) == EINVAL and b"null" in lib.bl_last_error()
    assert greedy(best_ptr=None) == EINVAL and greedy(picks_ptr=None) == EINVAL and greedy(ws_ptr=None) == EINVAL
    assert greedy(q_ptr=d_q.data_ptr() + 4) == EINVAL and b"16-byte aligned" in lib.bl_last_error()
    assert greedy(best_ptr=best.data_ptr() + 4) == EINVAL and b"8-byte aligned" in lib.bl_last_error()
    assert greedy(ld=Dp - 16) == EINVAL and greedy(ld=Dp + 8) == EINVAL and greedy(dp=100) == EINVAL and b"multiple of 64" in lib.bl_last_error()
    assert greedy(dp=576, ld=576) == ERANGE and b"BL_SIM_MAX_D" in lib.bl_last_error()
    assert greedy(m=-1) == EINVAL and greedy(b=-1) == EINVAL and greedy(m=(1 << 20) + 1) == ERANGE and greedy(b=16385) == ERANGE
    for bad in (0.0, -1.0, 1.5, float("nan")):
        assert greedy(stop=bad) == EINVAL and b"stop" in lib.bl_last_error()
    assert greedy(blocks=-1) == EINVAL and greedy(blocks=1025) == EINVAL and greedy(ws_bytes=64) == EINVAL and b"workspace" in lib.bl_last_error()
    assert cover(q_ptr=None) == EINVAL and cover(best_ptr=None) == EINVAL and cover(slices=0) == EINVAL and cover(slices=65) == EINVAL
    assert cover(first=-1) == EINVAL and cover(dp=96) == EINVAL and cover(ld=Dp + 4) == EINVAL and cover(ws_bytes=300 * 12 - 1) == EINVAL
    assert cover(l=(1 << 20) + 1) == ERANGE and cover(m=(1 << 20) + 1) == ERANGE and b"BL_REVIEW_MAX_ROWS" in lib.bl_last_error()
    assert lib.bl_review_norms(None, Dp, M, Dp, d_n.data_ptr(), _stream()) == EINVAL
    assert lib.bl_review_norms(d_q.data_ptr(), Dp, M, 96, d_n.data_ptr(), _stream()) == EINVAL
    torch.cuda.synchronize()  # nothing was launched: the outputs and the state are as they were
    assert picks.cpu().tolist() == [7] * 4 and pnear.cpu().tolist() == [7] * 4 and aff.cpu().tolist() == [7.0] * 4 and not ws.any()
    C.assert_equal_bits(_host(best, near, d_n), [best0, near0, n], "untouched state")
    assert greedy(b=0) == 0 and cover(l=0) == 0 and greedy() == 0 and cover() == 0
    with pytest.raises(ValueError, match="come together"):
        hip_ops.review_cover(d_q, d_n, d_q[:5], d_n[:5], best=best)
    with pytest.raises(ValueError, match="unit column stride"):
        hip_ops.review_norms(d_q[:, ::2][:, :64])
    with pytest.raises(ValueError, match="multiple of 16"):
        hip_ops.review_norms(torch.zeros((4, 72), dtype=torch.int8, device=DEV)[:, :64])
    with pytest.raises(TypeError):
        hip_ops.review_greedy(d_q, d_n, best.float(), near, 3)


# ------------------------------------------------------------------------------------------------ end to end
def _records(queue):
    return json.dumps([w.record() for w in queue.warnings], sort_keys=True)


@pytest.mark.parametrize("family", list(SPECS))
def test_queue_on_the_device_equals_the_host_path(family, untrained):
    from buglab.models import review as T
    from buglab.models import similar
    from buglab.models._review import greedy_host, norms_host
    from buglab.models._similar import quantize_host

    model, nn_, data, _, _ = untrained[family]
    with _deterministic():
        a = T.review_queue(model, nn_, data, torch.device(DEV), 10, assume_buggy=True, parallelize=False)
        b = T.review_queue(model, nn_, data, torch.device(DEV), 10, assume_buggy=True, parallelize=False, host=True)
        assert _records(a) == _records(b) and a.summary == b.summary and len(a.warnings) == 10 and a.summary["end"] == "budget"
        sites = similar.embed_sites(model, nn_, data, torch.device(DEV), "predicted", assume_buggy=True, parallelize=False)
        assert sites.rows.shape == (48, 32)
        index = similar.build_site_index(model, nn_, data[:20], DEV, "predicted", "seen", assume_buggy=True, parallelize=False)
        later = sites._replace(**{f: getattr(sites, f)[20:] for f in ("rows", "positions", "nodes", "logprobs", "labels", "paths", "packages", "scouts")})
        cut = float(np.exp(np.median(sites.logprobs)))
        for options in (dict(), dict(center=False), dict(reviewed=index), dict(reviewed=index, max_similarity=0.9), dict(min_confidence=cut),
                        dict(max_similarity=0.5)):
            which = later if "reviewed" in options else sites
            a = T.review_sites(which, 12, device=DEV, **options)
            b = T.review_sites(which, 12, host=True, **options)
            assert _records(a) == _records(b) and a.summary == b.summary, options
            assert a.summary["num_picked"] == len(a.warnings) <= 12 and a.summary["end"] in ("budget", "max-similarity", "nothing-left")
        # the first pick is the most probable warning, every later one is the least covered when it is taken
        cold = T.review_sites(sites, 12, device=DEV)
        assert cold.warnings[0].logprob == float(sites.logprobs.max()) and cold.warnings[0].nearest is None
        assert all(w.nearest["rank"] < w.rank for w in cold.warnings[1:])
        sel = T.queue_embeddings(torch.from_numpy(sites.rows).to(DEV), 12, sites.logprobs)
        c, q, sumsq, r = quantize_host(sites.rows, sel.mean)
        assert (np.diff(sel.pick_affinity) >= 0).all() and sel.valid.tolist() == (norms_host(q) > 0).tolist()
        # a re-ranker: only the band is queued (the probabilities are the device's own)
        triage = _fitted(D=32)
        banded = T.review_sites(sites, 48, triage=triage, band=(0.25, 0.75), device=DEV)
        assert all(0.25 <= w.triage_probability <= 0.75 for w in banded.warnings)
        assert len(banded.warnings) <= banded.summary["num_eligible"] == 48 - banded.summary["num_outside_band"]


def test_command_line_review(untrained, tmp_path, capsys):
    from buglab.models import review as T
    from buglab.models import similar

    model, nn_, data, path, data_dir = untrained["gnn-mlp"]
    with _deterministic():
        index = similar.build_site_index(model, nn_, data[:16], DEV, "predicted", "seen", assume_buggy=True, parallelize=False)
        index.save(tmp_path / "reviewed.npz")
        outs = {}
        for name, extra in (("device", []), ("host", ["--host"])):
            out, report = tmp_path / f"{name}.jsonl", tmp_path / f"{name}.json"
            args = [str(path), str(data_dir), str(out), "--budget", "9", "--assume-buggy", "--reviewed", str(tmp_path / "reviewed.npz"),
                    "--report-json", str(report), "--sequential"] + extra
            assert T.run(T.parse_args(args)) == 0
            assert "review: 9 of 48 eligible warnings" in capsys.readouterr().out
            outs[name] = (out.read_bytes(), report.read_bytes())
        assert outs["device"] == outs["host"]  # OUT and --report-json, byte for byte
        records = [json.loads(line) for line in outs["device"][0].decode("utf-8").splitlines()]
        blob = json.loads(outs["device"][1])
        assert len(records) == 9 == blob["num_picked"] and blob["num_reviewed"] == index.size and blob["end"] == "budget"
        assert [r["rank"] for r in records] == list(range(9)) and records[0]["nearest"]["reviewed"]["tag"] == "seen"
        # an index of another size: status 2, nothing written
        wrong = index._replace(embeddings=np.zeros((index.size, 48), np.float32), mean=np.zeros(48, np.float32), dim=48)
        wrong.save(tmp_path / "wrong.npz")
        other = tmp_path / "other.jsonl"
        status = T.run(T.parse_args([str(path), str(data_dir), str(other), "--budget", "9", "--reviewed", str(tmp_path / "wrong.npz"), "--sequential"]))
        assert status == T.EXIT_DIMENSION_MISMATCH == 2 and not other.exists() and "size 48" in capsys.readouterr().err

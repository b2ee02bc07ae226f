"""GPU: warning tracking on the MI355X -- the kernels of csrc/bl_track.hip against the restatement in Python integers and
Fractions (tests/track_cases.py, which tests/test_track_host.py also pins the NumPy twin to) bit for bit: the directional best
for every shape that reaches another branch of the GEMM, with closed rows, keys and floors, for every number of slices and in
both directions; the rounds for every `max_rounds`, the state and the status after every call; a chain that needs one round
per pair, resumed every two rounds; every way the matching ends, exact copies, ragged tiles; strided images and outputs inside
poisoned guard bands; and `track` end to end on two tiny untrained models, the device path against `--host`.

No tolerance anywhere: every output is an integer or one IEEE quotient of two exact integers."""
import json

import numpy as np
import pytest
import torch

from tests import similar_cases as C
from tests import track_cases as TC
from tests.guard_bands import guarded
from tests.test_group_gpu import untrained  # noqa: F401  (a fixture)
from tests.test_similar_gpu import DEV, SPECS, _deterministic, _dev, _stream

pytestmark = pytest.mark.gpu


def _host(*tensors):
    return [t.cpu().numpy() for t in tensors]


def _opt(a):
    return None if a is None else _dev(a)


# ------------------------------------------------------------------------------------------------ bl_track_best_i8
@pytest.mark.parametrize("D", [1, 100, 128, 512])  # one column; padding columns; two whole k-chunks; eight
def test_best_equals_the_restatement_in_both_directions(D):
    from buglab.models import hip_ops

    q_x, n_x, q_y, n_y, aff = TC.best_case(D)  # 150 x 37, copies among the rows, rows 1, 4, 7 of both sides invalid
    X, Y = 150, 37
    aff_t = TC.transposed(aff, X, Y)
    d = [_dev(a) for a in (q_x, n_x, q_y, n_y)]
    open_x, open_y = TC.every_third_closed(X), TC.every_third_closed(Y, 1)
    for kx, ky in ((None, None), (TC.keys3(X), TC.keys3(Y, 1))):
        for floor in (0.25, 0.81):  # 0.81 is a floor that some row's best pair misses (tests/test_track_host.py asserts it)
            for ox, oy in ((None, None), (open_x, open_y)):
                want = TC.best_ref(aff, X, Y, floor, kx, ky, ox, oy)
                back = TC.best_ref(aff_t, Y, X, floor, ky, kx, oy, ox)
                for slices in (None, 1, 3):
                    what = (D, kx is not None, floor, ox is not None, slices)
                    got = hip_ops.track_best(d[0], d[1], d[2], d[3], floor, key_old=_opt(kx), key_new=_opt(ky), open_old=_opt(ox),
                                             open_new=_opt(oy), slices=slices)
                    C.assert_equal_bits(_host(*got), want, what + ("x -> y",))
                    got = hip_ops.track_best(d[2], d[3], d[0], d[1], floor, key_old=_opt(ky), key_new=_opt(kx), open_old=_opt(oy),
                                             open_new=_opt(ox), slices=slices)
                    C.assert_equal_bits(_host(*got), back, what + ("y -> x",))


# ------------------------------------------------------------------------------------------------ bl_track_match
def _fresh(L, N):
    return (torch.full((L,), -1, dtype=torch.int32, device=DEV), torch.full((N,), -1, dtype=torch.int32, device=DEV),
            torch.zeros(N, dtype=torch.float64, device=DEV))


def _run(case, L, N, floor, ko=None, kn=None, max_rounds=64, slices=None):
    """the matching on the device call by call, every call checked against the restatement's -> (state, rounds, calls made)"""
    from buglab.models import hip_ops

    q_old, n_old, q_new, n_new, aff = case
    d = [_dev(a) for a in (q_old, n_old, q_new, n_new)]
    state, ref = _fresh(L, N), None
    rounds = made = 0
    while True:
        status = hip_ops.track_match(*d, floor, *state, max_rounds=max_rounds, key_old=_opt(ko), key_new=_opt(kn), slices=slices)
        ref, st_ref, _ = TC.rounds_ref(aff, L, N, floor, ko, kn, ref, max_rounds)
        C.assert_equal_bits(_host(*state, status), [*ref, st_ref], (floor, ko is not None, max_rounds, slices, made))
        rounds, made = rounds + int(st_ref[0]), made + 1
        if st_ref[2]:
            break
    return _host(*state), rounds, made


@pytest.mark.parametrize("keys", ["no keys", "keys"])
@pytest.mark.parametrize("floor", [0.25, 0.81])
def test_match_equals_the_restatement_after_every_call(floor, keys):
    case = TC.match_case()  # 150 old rows, 131 new ones: copies, noisy copies and fresh rows, invalid rows on both sides
    L, N = 150, 131
    ko, kn = (None, None) if keys == "no keys" else (TC.keys3(L), TC.keys3(N, 1))
    want = TC.match_ref(case[4], L, N, floor, ko, kn)
    total = int(TC.rounds_ref(case[4], L, N, floor, ko, kn)[1][0])
    for max_rounds in (1, 2, 64):
        state, rounds, made = _run(case, L, N, floor, ko, kn, max_rounds)
        C.assert_equal_bits(state, want, (floor, keys, max_rounds))
        assert rounds == total and made == total // max_rounds + 1
    again = _run(case, L, N, floor, ko, kn, 64, slices=3)[0]
    assert all(a.tobytes() == b.tobytes() for a, b in zip(again, _run(case, L, N, floor, ko, kn, 64)[0]))  # the same bytes again


def test_a_chain_of_one_pair_per_round_resumed_every_two_rounds():
    k = 7
    case = TC.chain_case(k)
    ref, status, per_round = TC.rounds_ref(case[4], k, k, 0.25)
    assert per_round == [1] * k and status.tolist() == [k, k, 1, 0]
    state, rounds, made = _run(case, k, k, 0.25, max_rounds=2)  # the resumption and the ended word: 4 calls of 2 rounds
    C.assert_equal_bits(state, ref, "chain, two rounds a call")
    assert rounds == k and made == k // 2 + 1
    state, rounds, made = _run(case, k, k, 0.25, max_rounds=64)  # 64 - 8 launches of every kind read the word and return
    C.assert_equal_bits(state, ref, "chain, one call")
    assert rounds == k and made == 1


def test_every_way_of_ending_and_exact_copies():
    from buglab.models import hip_ops

    # nothing admissible at all: the first round ends it, the state stays
    q_old, n_old, q_new, n_new, aff = TC.chain_case(7)
    state, rounds, made = _run((q_old, n_old, q_new, n_new, aff), 7, 7, 1.0)
    assert rounds == 0 and made == 1 and (state[0] == -1).all() and (state[1] == -1).all() and not state[2].any()
    # one side exhausted: 3 old rows against 7 new ones
    small = (q_old[:3], n_old[:3], q_new, n_new, [row for row in aff[:3]])
    state, rounds, made = _run(small, 3, 7, 0.25)
    assert (state[0] >= 0).all() and (state[1] >= 0).sum() == 3
    # every row invalid
    dead = (np.zeros_like(q_old), np.zeros_like(n_old), q_new, n_new, [[None] * 7 for _ in range(7)])
    assert _run(dead, 7, 7, 0.25)[1] == 0
    # a side without rows: nothing is read, one empty round ends it
    none_q, none_n = torch.zeros((0, 64), dtype=torch.int8, device=DEV), torch.zeros(0, dtype=torch.int32, device=DEV)
    st = _fresh(0, 7)
    status = hip_ops.track_match(none_q, none_n, _dev(q_new), _dev(n_new), 0.25, *st)
    assert status.cpu().tolist() == [0, 0, 1, 7] and (st[1].cpu() == -1).all()
    st = _fresh(7, 0)
    assert hip_ops.track_match(_dev(q_old), _dev(n_old), none_q, none_n, 0.25, *st).cpu().tolist() == [0, 0, 1, 0]
    best, arg = hip_ops.track_best(_dev(q_old), _dev(n_old), none_q, none_n, 0.25)
    assert (best.cpu() == -2.0).all() and (arg.cpu() == -1).all() and hip_ops.track_best(none_q, none_n, _dev(q_new), _dev(n_new), 0.25)[0].shape == (0,)
    # exact copies: 10 distinct rows five times on both sides, every affinity of a pattern with itself is 1.0 -- the index order decides
    copies = TC.copies_case()
    want = TC.match_ref(copies[4], 50, 50, 1.0)
    assert want[0].tolist() == list(range(50)) and (want[2] == 1.0).all()
    state, rounds, made = _run(copies, 50, 50, 1.0)
    C.assert_equal_bits(state, want, "copies")
    assert rounds == 5  # a round matches the lowest open copy of every pattern
    C.assert_equal_bits(_run(copies, 50, 50, 1.0, TC.keys3(50), TC.keys3(50, 1))[0], TC.match_ref(copies[4], 50, 50, 1.0, TC.keys3(50), TC.keys3(50, 1)),
                        "copies with keys")


def test_more_than_one_row_tile_with_a_ragged_last_tile():
    from buglab.models import hip_ops

    case = TC.ragged_case()  # 1100 x 77
    q_old, n_old, q_new, n_new, aff = case
    L, N = 1100, 77
    d = [_dev(a) for a in (q_old, n_old, q_new, n_new)]
    want, back = TC.best_ref(aff, L, N, 0.25), TC.best_ref(TC.transposed(aff, L, N), N, L, 0.25)
    assert (back[1] == np.arange(1000, 1077)).all() and (back[0] == 1.0).all()  # every new row finds itself among the old ones
    for slices in (None, 1, 7, 64):
        C.assert_equal_bits(_host(*hip_ops.track_best(*d, 0.25, slices=slices)), want, ("old -> new", slices))
        C.assert_equal_bits(_host(*hip_ops.track_best(d[2], d[3], d[0], d[1], 0.25, slices=slices)), back, ("new -> old", slices))
    for slices in (None, 5):
        state, rounds, made = _run(case, L, N, 0.25, slices=slices)
        C.assert_equal_bits(state, TC.match_ref(aff, L, N, 0.25), ("match", slices))
        assert (state[1] == np.arange(1000, 1077)).all()


# ------------------------------------------------------------------------------------------------ the ABI
def _f64_guard(rows):
    g = guarded(rows, 2, ld=2, dtype=torch.int32, device=DEV, lead=6, any_width=True)  # doubles as int32 pairs, 8-byte aligned
    assert g.data_ptr() % 8 == 0
    return g


def _f64_of(g):
    return g.view.contiguous().cpu().numpy().view(np.float64)[:, 0]


def _i32_guard(rows, value=None):
    g = guarded(rows, 1, ld=1, dtype=torch.int32, device=DEV, any_width=True)
    if value is not None:
        g.view.fill_(value)
    return g


def test_strided_images_and_outputs_inside_guard_bands():
    from buglab.models import hip_ops

    q_old, n_old, q_new, n_new, aff = TC.match_case()
    L, N, Dp, S, floor = 150, 131, 128, 3, 0.81
    ko, kn = TC.keys3(L), TC.keys3(N, 1)
    lib = hip_ops.load_library()
    g_qo = guarded(L, Dp, ld=Dp + 16, dtype=torch.int8, device=DEV)  # the padding columns of every row hold the pattern
    g_qn = guarded(N, Dp, ld=Dp + 32, dtype=torch.int8, device=DEV)
    g_qo.view.copy_(_dev(q_old)), g_qn.view.copy_(_dev(q_new))
    assert g_qo.data_ptr() % 16 == 0 and g_qn.data_ptr() % 16 == 0
    g_no, g_nn, g_ko, g_kn = _i32_guard(L), _i32_guard(N), _i32_guard(L), _i32_guard(N)
    for g, a in ((g_no, n_old), (g_nn, n_new), (g_ko, ko), (g_kn, kn)):
        g.view[:, 0].copy_(_dev(a))
    # the directional best
    g_best, g_arg = _f64_guard(L), _i32_guard(L)
    need = lib.bl_track_best_workspace_bytes(L, N, S)
    g_ws = _f64_guard(need // 8)
    rc = lib.bl_track_best_i8(g_qo.data_ptr(), Dp + 16, g_no.data_ptr(), g_ko.data_ptr(), None, L, g_qn.data_ptr(), Dp + 32, g_nn.data_ptr(),
                              g_kn.data_ptr(), None, N, Dp, floor, S, g_ws.data_ptr(), need, g_best.data_ptr(), g_arg.data_ptr(), _stream())
    assert rc == 0, lib.bl_last_error()
    C.assert_equal_bits([_f64_of(g_best), g_arg.view[:, 0].cpu().numpy()], TC.best_ref(aff, L, N, floor, ko, kn), "best in guard bands")
    # the rounds
    g_mo, g_mn, g_aff, g_status = _i32_guard(L, -1), _i32_guard(N, -1), _f64_guard(N), _i32_guard(4)
    g_aff.view.fill_(0)
    need_m = lib.bl_track_match_workspace_bytes(L, N, S)
    g_wm = _f64_guard(need_m // 8)
    rc = lib.bl_track_match(g_qo.data_ptr(), Dp + 16, g_no.data_ptr(), g_ko.data_ptr(), L, g_qn.data_ptr(), Dp + 32, g_nn.data_ptr(),
                            g_kn.data_ptr(), N, Dp, floor, 64, S, g_wm.data_ptr(), need_m, g_mo.data_ptr(), g_mn.data_ptr(), g_aff.data_ptr(),
                            g_status.data_ptr(), _stream())
    assert rc == 0, lib.bl_last_error()
    for g, name in ((g_qo, "q_old"), (g_qn, "q_new"), (g_no, "n_old"), (g_nn, "n_new"), (g_ko, "key_old"), (g_kn, "key_new"), (g_best, "best"),
                    (g_arg, "arg"), (g_ws, "best workspace"), (g_mo, "match_old"), (g_mn, "match_new"), (g_aff, "match_aff"),
                    (g_status, "status"), (g_wm, "match workspace")):
        g.assert_untouched(name)
    ref, st_ref, _ = TC.rounds_ref(aff, L, N, floor, ko, kn, None, 64)
    got = [g_mo.view[:, 0].cpu().numpy(), g_mn.view[:, 0].cpu().numpy(), _f64_of(g_aff), g_status.view[:, 0].cpu().numpy()]
    C.assert_equal_bits(got, [*ref, st_ref], "match in guard bands")
    # the strided views through the wrappers
    d_no, d_nn = hip_ops.review_norms(g_qo.view), hip_ops.review_norms(g_qn.view)
    C.assert_equal_bits(_host(*hip_ops.track_best(g_qn.view, d_nn, g_qo.view, d_no, floor, key_old=_dev(kn), key_new=_dev(ko))),
                        TC.best_ref(TC.transposed(aff, L, N), N, L, floor, kn, ko), "strided, through the wrapper")
    state = _fresh(L, N)
    status = hip_ops.track_match(g_qo.view, d_no, g_qn.view, d_nn, floor, *state, max_rounds=64, key_old=_dev(ko), key_new=_dev(kn))
    C.assert_equal_bits(_host(*state, status), [*ref, st_ref], "strided match, through the wrapper")
    g_qo.assert_untouched("q_old"), g_qn.assert_untouched("q_new")


def test_argument_errors_are_returned_without_a_launch():
    from buglab.models import hip_ops

    q_old, n_old, q_new, n_new, _ = TC.match_case()
    L, N, Dp = 150, 131, 128
    d_qo, d_no, d_qn, d_nn = (_dev(a) for a in (q_old, n_old, q_new, n_new))
    state = _fresh(L, N)
    status = torch.full((4,), 7, dtype=torch.int32, device=DEV)
    ws = torch.zeros(1 << 14, dtype=torch.float64, device=DEV)
    lib = hip_ops.load_library()
    EINVAL, ERANGE = -1, -2

    def match(q_ptr=d_qo.data_ptr(), ld=Dp, l=L, dp=Dp, floor=0.5, rounds=4, slices=1, ws_ptr=ws.data_ptr(), ws_bytes=ws.numel() * 8,
              aff_ptr=state[2].data_ptr(), key=None):
        return lib.bl_track_match(q_ptr, ld, d_no.data_ptr(), key, l, d_qn.data_ptr(), Dp, d_nn.data_ptr(), None, N, dp, floor, rounds, slices,
                                  ws_ptr, ws_bytes, state[0].data_ptr(), state[1].data_ptr(), aff_ptr, status.data_ptr(), _stream())

    assert match(q_ptr=None) == EINVAL and b"null" in lib.bl_last_error()
    assert match(q_ptr=d_qo.data_ptr() + 4) == EINVAL and b"16-byte aligned" in lib.bl_last_error()
    assert match(aff_ptr=state[2].data_ptr() + 4) == EINVAL and b"8-byte aligned" in lib.bl_last_error()
    assert match(ld=Dp - 16) == EINVAL and match(ld=Dp + 8) == EINVAL and match(dp=100) == EINVAL and b"multiple of 64" in lib.bl_last_error()
    assert match(l=-1) == EINVAL and match(l=(1 << 20) + 1) == ERANGE and match(rounds=0) == EINVAL and match(rounds=4097) == ERANGE
    for bad in (0.0, -1.0, 1.5, float("nan")):
        assert match(floor=bad) == EINVAL and b"floor" in lib.bl_last_error()
    assert match(slices=0) == EINVAL and match(slices=65) == EINVAL and match(key=d_no.data_ptr()) == EINVAL
    assert match(ws_ptr=None) == EINVAL and match(ws_bytes=64) == EINVAL and b"workspace" in lib.bl_last_error()
    torch.cuda.synchronize()  # nothing was launched: the state, the status and the workspace are as they were
    assert status.cpu().tolist() == [7] * 4 and not ws.any() and (state[0].cpu() == -1).all() and (state[1].cpu() == -1).all()
    assert match() == 0
    with pytest.raises(ValueError, match="unit column stride"):
        hip_ops.track_best(d_qo[:, ::2][:, :64], d_no, d_qn[:, ::2][:, :64], d_nn, 0.5)
    with pytest.raises(TypeError):
        hip_ops.track_match(d_qo, d_no, d_qn, d_nn, 0.5, state[0], state[1], state[2].float())
    with pytest.raises(ValueError, match="state"):
        hip_ops.track_match(d_qo, d_no, d_qn, d_nn, 0.5, state[1], state[0], state[2])


# ------------------------------------------------------------------------------------------------ end to end
def _records(scan):
    return json.dumps([w.record() for w in scan.warnings + scan.hidden], sort_keys=True)


@pytest.mark.parametrize("family", list(SPECS))
def test_track_on_the_device_equals_the_host_path(family, untrained, tmp_path, monkeypatch):
    from buglab.models import similar
    from buglab.models import track as T

    model, nn_, data, path, data_dir = untrained[family]
    if family != "gnn-mlp":  # the fixture's file is read back for the graph model only (as the other tools' tests do): the samples themselves
        monkeypatch.setattr(T, "_read_data", lambda p, limit: data[:limit])
    with _deterministic():
        index = similar.build_site_index(model, nn_, data[:30], DEV, "predicted", "seen", assume_buggy=True, parallelize=False)
        index = index._replace(tags=np.asarray(["dismissed" if i % 3 == 0 else "accepted" for i in range(index.size)]))
        for options in (dict(), dict(min_similarity=0.5), dict(within="file"), dict(min_similarity=0.99, hide_tags=["dismissed"], tag="fresh"),
                        dict(max_rounds=1)):
            a = T.track_warnings(model, nn_, index, data[10:], torch.device(DEV), assume_buggy=True, parallelize=False, **options)
            b = T.track_warnings(model, nn_, index, data[10:], torch.device(DEV), assume_buggy=True, parallelize=False, host=True, **options)
            assert _records(a) == _records(b) and a.summary == b.summary, options
            assert all(x.tobytes() == y.tobytes() if isinstance(x, np.ndarray) else x == y for x, y in zip(a.index, b.index)), options
            s = a.summary
            assert s["num_warnings"] == 38 and s["num_new"] + s["num_persisting"] + s["num_hidden"] == 38 and s["num_old"] == 30
            assert s["num_persisting"] + s["num_hidden"] + s["num_gone"] == 30 and s["other_weights"] is False
        # samples 10 .. 29 are in both scans with the same embedding: at a floor this high only such pairs match
        a = T.track_warnings(model, nn_, index, data[10:], torch.device(DEV), assume_buggy=True, parallelize=False, min_similarity=0.999)
        assert a.summary["num_persisting"] > 0 and all(w.previous["similarity"] >= 0.99 for w in a.warnings if w.status == "persisting")
        # the command line: both paths write the same bytes, and the exit status says whether there are new warnings
        index.save(tmp_path / "old.npz")
        outs = {}
        for name, extra in (("device", []), ("host", ["--host"])):
            out, report, written = tmp_path / f"{name}.jsonl", tmp_path / f"{name}.json", tmp_path / f"{name}.npz"
            args = [str(path), str(tmp_path / "old.npz"), str(data_dir), str(out), "--assume-buggy", "--report-json", str(report), "--sequential",
                    "--write-index", str(written), "--tag", "fresh", "--min-similarity", "0.999"] + extra
            status = T.run(T.parse_args(args))
            blob = json.loads(report.read_text())
            assert status == (1 if blob["num_new"] else 0) and blob["num_warnings"] == 48
            outs[name] = (out.read_bytes(), report.read_bytes())
        assert outs["device"] == outs["host"]  # OUT and --report-json, byte for byte
        from buglab.models._similar import SiteIndex

        one, other = SiteIndex.load(tmp_path / "device.npz"), SiteIndex.load(tmp_path / "host.npz")
        assert all(x.tobytes() == y.tobytes() if isinstance(x, np.ndarray) else x == y for x, y in zip(one, other)) and one.size == 48
        assert set(one.tags.tolist()) <= {"accepted", "dismissed", "fresh"}
        # against the index it wrote itself everything persists
        again = tmp_path / "again.jsonl"
        assert T.run(T.parse_args([str(path), str(tmp_path / "device.npz"), str(data_dir), str(again), "--assume-buggy", "--sequential",
                                   "--min-similarity", "0.999"])) == 0
        assert all(json.loads(line)["status"] == "persisting" for line in again.read_text().splitlines())

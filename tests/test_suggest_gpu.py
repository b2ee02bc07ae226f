"""GPU: ranked suggestions on the MI355X -- the kernel of csrc/bl_suggest.hip against its NumPy twin
(buglab/models/_suggest.py::rank_host, which tests/test_suggest_host.py pins to a literal restatement of the contract) bit for
bit on the handmade minibatch of tests/suggest_cases.py, its offset writes into run-long buffers between poisoned guard
regions, its agreement with bl_eval_judge where the two must agree, run-to-run determinism, and the two public paths end to end
on two tiny untrained models: `suggest` on the device against `suggest(host=True)`, `evaluate --on-device --top-k` against the
host path's text.

No tolerance anywhere: every output is an integer, a selected fp64 sum of two fp32 values, or a count."""
import copy
import gzip
import json
from pathlib import Path

import numpy as np
import pytest
import torch

from tests import suggest_cases as C

pytestmark = pytest.mark.gpu

DEV = "cuda"
SPECS = {"gnn-mlp": {"modelName": "gnn-mlp", "hidden_state_size": 32, "num_layers": 4, "dropout_rate": 0.1},
         "seq-great": {"modelName": "seq-great", "hidden_state_size": 64, "num_layers": 2, "num_heads": 4, "intermediate_dimension_size": 96,
                       "dropout_rate": 0.1}}


def _on_device(ix):
    from buglab.controllers._batching import to_device_i32
    from buglab.models import hip_ops

    return dict(zip(hip_ops.SUGGEST_INDEX_FIELDS, to_device_i32([getattr(ix, f) for f in hip_ops.SUGGEST_INDEX_FIELDS], DEV)))


def _buffers(capacity, k):
    return (torch.full((2, capacity), 77, dtype=torch.int32, device=DEV), torch.full((capacity, k), 77, dtype=torch.int32, device=DEV),
            torch.full((capacity, k), 123.0, dtype=torch.float64, device=DEV))


def _rank(src, ix, k, skip_nobug=False, into=None, offset=0):
    from buglab.models import hip_ops

    out = into if into is not None else _buffers(ix["tgt_rw"].shape[0], k)
    hip_ops.rank_suggestions(src, ix, *out, offset, k=k, skip_nobug=skip_nobug)
    return out


def _host(out):
    return tuple(t.cpu().numpy() for t in out)


@pytest.fixture(scope="module")
def crafted():
    src, ix, at = C.handcrafted()
    lengths = np.diff(ix.rw_off).tolist()
    for n in (0, 63, 64, 65, 257, C.STAGE - 1, C.STAGE, C.STAGE + 1):  # NO_BUG adds an entry: STAGE rewrites are STAGE + 1 entries
        assert n in lengths, n
    return src, ix, at, torch.from_numpy(src).to(DEV), _on_device(ix)


@pytest.mark.parametrize("skip_nobug", [False, True])
@pytest.mark.parametrize("k", [1, 5, 32])
def test_device_equals_the_twin_bit_for_bit(crafted, k, skip_nobug):
    from buglab.models._suggest import rank_host

    src, ix, at, d_src, d_ix = crafted
    want = rank_host(src, ix, k, skip_nobug)
    got = _host(_rank(d_src, d_ix, k, skip_nobug))
    C.assert_equal_bits(got, want, (k, skip_nobug))
    # the shapes the minibatch is there for did what they are there for (the numbers: tests/test_suggest_host.py)
    rank, entry, _ = got
    listed = (entry >= 0).sum(axis=1)
    assert listed[at["nobug_only"]] == (0 if skip_nobug else 1) and listed[at["few_rankable"]] == min(k, 1 if skip_nobug else 2)
    assert rank[0, at["truth_not_rankable"]] == -1 and rank[0, at["target_without_key"]] == -1 and rank[1, at["target_without_key"]] == -1
    assert rank[0, at["tie_waves"]] == 1 and rank[0, at["no_bug"]] == (-1 if skip_nobug else 0)
    assert entry[at["tie_waves"], 0] == 63 and (k < 5 or entry[at["tie_waves"], :3].tolist() == [63, 64, 256])


def test_drawn_minibatch_and_determinism():
    from buglab.models._suggest import rank_host

    src, ix = C.drawn(3, B=50)
    d_src, d_ix = torch.from_numpy(src).to(DEV), _on_device(ix)
    first = _host(_rank(d_src, d_ix, 32))
    C.assert_equal_bits(first, rank_host(src, ix, 32))
    again = _host(_rank(d_src, d_ix, 32))
    assert all(a.tobytes() == b.tobytes() for a, b in zip(first, again))  # the same launch twice: identical bytes


def test_offsets_and_guard_regions(crafted):
    """two launches at offsets 0 and B fill one buffer; what lies before and after it keeps its poison"""
    from buglab.models import hip_ops
    from buglab.models._suggest import rank_host

    src, ix, _, d_src, d_ix = crafted
    src2, ix2 = C.drawn(4, B=ix.tgt_rw.shape[0])
    B, k, guard = ix.tgt_rw.shape[0], 5, 512
    N = 2 * B
    flats = (torch.full((2 * guard + 2 * N,), 77, dtype=torch.int32, device=DEV), torch.full((2 * guard + N * k,), 77, dtype=torch.int32, device=DEV),
             torch.full((2 * guard + N * k,), 123.0, dtype=torch.float64, device=DEV))
    out = (flats[0][guard:guard + 2 * N].view(2, N), flats[1][guard:guard + N * k].view(N, k), flats[2][guard:guard + N * k].view(N, k))
    _rank(d_src, d_ix, k, into=out, offset=0)
    _rank(torch.from_numpy(src2).to(DEV), _on_device(ix2), k, skip_nobug=True, into=out, offset=B)
    rank, entry, logprob = _host(out)
    C.assert_equal_bits((rank[:, :B], entry[:B], logprob[:B]), rank_host(src, ix, k), "offset 0")
    C.assert_equal_bits((rank[:, B:], entry[B:], logprob[B:]), rank_host(src2, ix2, k, skip_nobug=True), "offset B")
    for flat, size, poison in zip(flats, (2 * N, N * k, N * k), (77, 77, 123.0)):
        host = flat.cpu().numpy()
        assert (host[:guard] == poison).all() and (host[guard + size:] == poison).all()
    # what does not fit is refused before anything is launched
    before = [t.clone() for t in out]
    with pytest.raises(ValueError, match="do not fit"):
        _rank(d_src, d_ix, k, into=out, offset=B + 1)
    with pytest.raises(ValueError, match="k must be"):
        hip_ops.rank_suggestions(d_src, d_ix, *out, 0, k=33)
    with pytest.raises(ValueError, match="inconsistent shapes"):
        hip_ops.rank_suggestions(d_src, dict(d_ix, rw_loc_idx=torch.zeros(1, dtype=torch.int32, device=DEV)), *out, 0, k=k)
    assert all(torch.equal(a, b) for a, b in zip(before, out))


def test_agrees_with_the_judge_where_the_two_must_agree():
    """NaN-free, finite values on a grid of halves (every sum exact), every node keyed: the location rank is 0 exactly where
    bl_eval_judge says location_correct; where the joint rank is 0 and the truth is a rewrite at the first-maximum node, the
    sample is repaired"""
    from buglab.models import hip_ops

    reached = 0
    for seed in (-1, -2, -3, -4):
        src, ix = C.drawn(seed, B=50)
        assert np.isfinite(src).all() and (ix.rw_loc_idx >= 0).all()
        d_src, d_ix = torch.from_numpy(src).to(DEV), _on_device(ix)
        B = ix.tgt_rw.shape[0]
        conf, verdict = torch.empty(B, dtype=torch.float64, device=DEV), torch.empty((4, B), dtype=torch.int32, device=DEV)
        hip_ops.eval_judge(d_src, d_ix, conf, verdict, 0)
        rank = _host(_rank(d_src, d_ix, 5))[0]
        verdict = verdict.cpu().numpy()
        assert ((rank[1] == 0) == (verdict[1] == 1)).all() and 0 < int((rank[1] == 0).sum()) < B, seed
        both = (ix.tgt_rw >= 0) & (rank[0] == 0) & (rank[1] == 0)
        assert (verdict[3][both] == 1).all(), seed
        reached += int(both.sum())
    assert reached >= 3  # the draws reach the second statement


# ------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def untrained(tmp_path_factory):
    """family -> (model, module, data): seeded weights, no training; 60 synthetic samples = two predict minibatches"""
    from buglab.data.synthetic import make_report_dataset
    from buglab.models.modelregistry import load_model
    from buglab.runtime.neuralmodel import AbstractNeuralModel

    out = {}
    for family, spec in SPECS.items():
        data = make_report_dataset(60, seed=17, kind="seq" if family.startswith("seq") else "graph")
        path = tmp_path_factory.mktemp(family.replace("-", "_")) / "detector.pkl.gz"
        model = load_model(dict(spec), path)[0]
        model.compute_metadata(copy.deepcopy(data))
        torch.manual_seed(5)
        model.save(path, model.build_neural_module())
        out[family] = AbstractNeuralModel.restore_model(Path(path), torch.device(DEV)) + (data, path)
    return out


@pytest.mark.parametrize("assume_buggy", [False, True])
@pytest.mark.parametrize("family", list(SPECS))
def test_suggest_on_the_device_equals_the_host_path(family, assume_buggy, untrained, monkeypatch):
    from buglab.models import _suggest as S
    from buglab.models.suggest import suggest
    from tests.test_visualize_host import bits

    model, nn_, data, _ = untrained[family]
    mappings = []
    builder = S.suggest_indices
    monkeypatch.setattr(S, "suggest_indices", lambda layout, points, node_mappings=None: (mappings.append(node_mappings),
                                                                                          builder(layout, points, node_mappings))[1])
    device = torch.device(DEV)
    on_device = list(suggest(model, nn_, data, device, 5, assume_buggy=assume_buggy, parallelize=False))
    on_host = list(suggest(model, nn_, data, device, 5, host=True, assume_buggy=assume_buggy, parallelize=False))
    assert len(on_device) == len(on_host) == 60 and [s.position for s in on_device] == list(range(60)) == [s.position for s in on_host]
    assert len(mappings) == 2 and all((m is not None) == family.startswith("seq") for m in mappings)  # through extend_sees_minibatch
    for a, b in zip(on_device, on_host):
        assert a.datapoint is b.datapoint and a.ranked.entries == b.ranked.entries, a.position
        assert [bits(x) for x in a.ranked.logprobs] == [bits(x) for x in b.ranked.logprobs], a.position
        assert (a.ranked.truth_rank, a.ranked.truth_location_rank) == (b.ranked.truth_rank, b.ranked.truth_location_rank), a.position
        assert a.record() == b.record()
    masses = [s.record()["mass"] for s in on_device]
    # the heads' fp32 log-softmaxes: 1e-5 as in tests/test_suggest_host.py::test_mass_is_a_probability_when_the_values_are
    # (without NO_BUG the rest is not renormalised, and is below 1 all the more)
    assert max(masses) <= 1.0 + 1e-5
    # a stream of unknown length, collated in worker threads: the buffers grow on the device
    streamed = list(suggest(model, nn_, iter(data), device, 5, assume_buggy=assume_buggy, parallelize=True, capacity=1))
    assert [s.ranked for s in streamed] == [s.ranked for s in on_device]


@pytest.mark.parametrize("family", list(SPECS))
def test_evaluate_on_device_with_top_k_prints_the_host_text(family, untrained):
    from buglab.models.evaluate import evaluate_on_device, evaluate_predictions, report_to_json

    model, nn_, data, _ = untrained[family]
    device = torch.device(DEV)
    host = evaluate_predictions(model.predict(iter(data), nn_, device, False), top_k=3)
    report = evaluate_on_device(model, nn_, data, device, parallelize=False, top_k=3)
    same = lambda a, b: json.dumps(a, sort_keys=True) == json.dumps(b, sort_keys=True)  # (a NaN equals a NaN there)
    assert same(report.top_k, host.top_k) and report.top_k["num_samples"]["all"] == 60 and 0 < report.top_k["num_samples"]["buggy"] < 60
    assert report.format() + report.format_top_k() == host.format() + host.format_top_k()
    assert same(json.loads(report_to_json(report))["top_k"], json.loads(report_to_json(host))["top_k"])
    # without top_k: today's report, and nothing of the ranking in it
    plain = evaluate_on_device(model, nn_, data, device, parallelize=False)
    assert plain.top_k is None and plain.format() == report.format() and "top_k" not in json.loads(report_to_json(plain))
    # --eval-only-no-bug, and a stream of unknown length
    clean = evaluate_on_device(model, nn_, iter(data), device, eval_only_no_bug=True, top_k=2, capacity=1)
    assert same(clean.top_k, evaluate_predictions(model.predict(iter(data), nn_, device, False), eval_only_no_bug=True, top_k=2).top_k)
    assert clean.top_k["num_samples"] == {"all": 30, "buggy": 0, "correct": 30}


def test_command_line_writes_the_records(untrained, tmp_path, capsys):
    from buglab.models import suggest as T
    from buglab.utils.msgpackutils import load_all_msgpack_l_gz, save_msgpack_l_gz

    model, nn_, data, path = untrained["gnn-mlp"]
    folder = tmp_path / "shard"
    folder.mkdir()
    save_msgpack_l_gz(data, folder / "x.msgpack.l.gz")
    out = tmp_path / "suggestions.jsonl.gz"
    arguments = {"MODEL_FILENAME": str(path), "DATA_PATH": str(folder), "OUT_PATH": str(out), "--top-k": 3, "--limit-num-elements": None,
                 "--sequential": True, "--host": False, "--assume-buggy": False, "--min-probability": None}
    assert T.run(arguments) == 60
    assert "60 samples ranked, 0 rejected" in capsys.readouterr().err
    with gzip.open(out, "rt", encoding="utf-8") as f:
        records = [json.loads(line) for line in f]
    read_back = list(load_all_msgpack_l_gz(folder))  # the samples as the tool reads them
    want = [s.record() for s in T.suggest(model, nn_, read_back, DEV, 3, parallelize=False)]
    assert records == json.loads(json.dumps(want)) and [r["position"] for r in records] == list(range(60))
    assert all(len(r["suggestions"]) <= 3 and "truth_rank" in r for r in records)

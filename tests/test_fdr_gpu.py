"""GPU: FDR-controlled warnings on the MI355X -- the kernels of csrc/bl_fdr.hip against their NumPy twin (buglab/models/_fdr.py,
which tests/test_fdr_host.py pins to plain loops) bit for bit, offset writes into run-long buffers inside guard bands, a poisoned
workspace, run-to-run determinism, and `fit` / `scan` end to end on two tiny untrained models: the device path against `--host`
record for record.

No tolerance anywhere: every output is a selected fp32 value, an integer count, a flag, or an fp64 quotient of two integers."""
import copy
import gzip
import json
from pathlib import Path

import numpy as np
import pytest
import torch

from tests import fdr_cases as C
from tests.guard_bands import guarded

pytestmark = pytest.mark.gpu

DEV = "cuda"
SPECS = {"gnn-mlp": {"modelName": "gnn-mlp", "hidden_state_size": 32, "num_layers": 4, "dropout_rate": 0.1},
         "seq-great": {"modelName": "seq-great", "hidden_state_size": 64, "num_layers": 2, "num_heads": 4, "intermediate_dimension_size": 96,
                       "dropout_rate": 0.1}}


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


# ------------------------------------------------------------------------------------------------ bl_fdr_counts
@pytest.mark.parametrize("n_ref", [1, 2, 63, 64, 65, 4096, 4097, 70001])
@pytest.mark.parametrize("B", [1, 50, 257])
def test_counts_equal_the_twin_bit_for_bit(B, n_ref):
    from buglab.models import hip_ops
    from buglab.models._fdr import counts_host

    src, idx, ref = C.counts_case(B, n_ref, seed=1)
    if B >= 16:  # ties with reference entries, NaN, both infinities, and indices -1 and n_src are all in the case
        assert (idx == -1).any() and (idx == src.shape[0]).any() and np.isnan(src[idx[(idx >= 0) & (idx < src.shape[0])]]).any()
        assert np.isin(src[idx[(idx >= 0) & (idx < src.shape[0])]], ref).any()
    score = torch.full((B,), 123.0, dtype=torch.float32, device=DEV)
    count = torch.full((B,), 77, dtype=torch.int32, device=DEV)
    hip_ops.fdr_counts(_dev(src), _dev(idx), _dev(ref), score, count, 0)
    C.assert_equal_bits((score.cpu().numpy(), count.cpu().numpy()), counts_host(src, idx, ref), (B, n_ref))


def test_counts_offsets_guard_bands_and_refusals():
    """two launches at offsets 3 and 3 + B fill part of one buffer; every element around the written samples keeps its pattern"""
    from buglab.models import hip_ops
    from buglab.models._fdr import counts_host

    (src, idx, ref), (src2, idx2, ref2) = C.counts_case(257, 4097, seed=2), C.counts_case(50, 4097, seed=3)
    capacity, first = 400, 3
    g_score = guarded(capacity, 1, ld=1, dtype=torch.float32, device=DEV, any_width=True)
    g_count = guarded(capacity, 1, ld=1, dtype=torch.int32, device=DEV, any_width=True)
    score, count = g_score.view[:, 0], g_count.view[:, 0]
    assert score.is_contiguous() and count.is_contiguous()
    hip_ops.fdr_counts(_dev(src), _dev(idx), _dev(ref), score, count, first)
    hip_ops.fdr_counts(_dev(src2), _dev(idx2), _dev(ref2), score, count, first + 257)
    g_score.assert_untouched("out_score"), g_count.assert_untouched("out_count")
    got_s, got_c = score.cpu().numpy(), count.cpu().numpy()
    C.assert_equal_bits((got_s[first:first + 257], got_c[first:first + 257]), counts_host(src, idx, ref), "offset 3")
    C.assert_equal_bits((got_s[first + 257:first + 307], got_c[first + 257:first + 307]), counts_host(src2, idx2, ref2), "offset 260")
    outside = np.r_[0:first, first + 307:capacity]  # samples no launch owns: still the pattern
    assert (got_s[outside].view(np.uint32) == g_score.pattern).all() and (got_c[outside].view(np.uint32) == g_count.pattern).all()
    # what does not fit is refused before anything is launched: by the launcher, and by the entry point itself
    before = (score.clone(), count.clone())
    with pytest.raises(ValueError, match="do not fit"):
        hip_ops.fdr_counts(_dev(src), _dev(idx), _dev(ref), score, count, capacity - 256)
    d_src, d_idx, d_ref = _dev(src), _dev(idx), _dev(ref)
    lib = hip_ops.load_library()
    rc = lib.bl_fdr_counts(d_src.data_ptr(), d_src.numel(), d_idx.data_ptr(), 257, d_ref.data_ptr(), 4097, score.data_ptr(), count.data_ptr(),
                           capacity - 256, capacity, torch.cuda.current_stream().cuda_stream)
    assert rc == -1 and b"do not fit" in lib.bl_last_error()  # BL_EINVAL
    torch.cuda.synchronize()
    assert torch.equal(before[0].view(torch.int32), score.view(torch.int32)) and torch.equal(before[1], count)
    g_score.assert_untouched("out_score"), g_count.assert_untouched("out_count")


# ------------------------------------------------------------------------------------------------ bl_fdr_bh
def _bh(count, n_ref, q, workspace=None):
    from buglab.models import hip_ops

    cutoff, flag, qv, R = hip_ops.fdr_bh(count, n_ref, q, workspace)
    return cutoff.cpu().numpy(), flag.cpu().numpy(), qv.cpu().numpy(), R.cpu().numpy()


# 2, 1024, 1025 and 65537 bins: one chunk, its last full and first overfull size, 17 chunks; 16000 and 16001 bins: the largest
# histogram kept in LDS and the smallest one in global memory
@pytest.mark.parametrize("n_ref", [1, 1023, 1024, 15999, 16000, 65536])
@pytest.mark.parametrize("N", [1, 255, 256, 257, 10000])
def test_bh_equals_the_twin_bit_for_bit(N, n_ref):
    from buglab.models import hip_ops
    from buglab.models._fdr import bh_host

    workspace = torch.empty(hip_ops.fdr_bh_workspace_bytes(n_ref) + 64, dtype=torch.uint8, device=DEV)
    for kind in ("mixed", "equal", "top"):
        count = C.bh_counts(N, n_ref, kind, seed=4)
        d_count = _dev(count)
        for q in (0.01, 0.1, 1.0):
            want = bh_host(count, n_ref, q)
            workspace.fill_(0x7F)  # the kernel zeroes what it counts in
            got = _bh(d_count, n_ref, q, workspace)
            C.assert_equal_bits(got, want, (N, n_ref, kind, q))
            assert (workspace[-64:] == 0x7F).all()  # and stays inside the bytes it asked for
            again = _bh(d_count, n_ref, q, workspace)  # on the workspace the first call left behind
            assert all(a.tobytes() == b.tobytes() for a, b in zip(got, again)), (N, n_ref, kind, q)
            if kind == "top":
                assert got[0].tolist() == ([n_ref, N] if q == 1.0 else [-1, 0])
    fresh = _bh(d_count, n_ref, 1.0)  # the launcher's own allocation
    C.assert_equal_bits(fresh, want, "fresh workspace")


def test_bh_outputs_sit_inside_guard_bands():
    from buglab.models import hip_ops
    from buglab.models._fdr import bh_host

    N, n_ref, q = 1000, 4097, 0.1
    count = C.bh_counts(N, n_ref, "mixed", seed=5)
    d_count = _dev(count)
    g_flag = guarded(N, 1, ld=1, dtype=torch.int32, device=DEV, any_width=True)
    g_cut = guarded(2, 1, ld=1, dtype=torch.int32, device=DEV, any_width=True)
    g_q = guarded(N, 2, ld=2, dtype=torch.int32, device=DEV, lead=6, any_width=True)  # N doubles, 8-byte aligned
    g_ws = guarded(hip_ops.fdr_bh_workspace_bytes(n_ref) // 4, 1, ld=1, dtype=torch.int32, device=DEV, lead=6, any_width=True)
    assert g_q.data_ptr() % 8 == 0 and g_ws.data_ptr() % 8 == 0 and hip_ops.fdr_bh_workspace_bytes(n_ref) % 8 == 0
    lib = hip_ops.load_library()
    rc = lib.bl_fdr_bh(d_count.data_ptr(), N, n_ref, q, g_ws.data_ptr(), g_cut.data_ptr(), g_flag.data_ptr(), g_q.data_ptr(),
                       torch.cuda.current_stream().cuda_stream)
    assert rc == 0, lib.bl_last_error()
    for g, name in ((g_flag, "out_flag"), (g_cut, "out_cutoff"), (g_q, "out_q"), (g_ws, "workspace")):
        g.assert_untouched(name)
    got = (g_cut.view[:, 0].cpu().numpy(), g_flag.view[:, 0].cpu().numpy(), g_q.view.contiguous().cpu().numpy().view(np.float64)[:, 0],
           g_ws.view[:n_ref + 1, 0].cpu().numpy())
    C.assert_equal_bits(got, bh_host(count, n_ref, q))


# ------------------------------------------------------------------------------------------------ end to end
@pytest.fixture(scope="module")
def untrained(tmp_path_factory):
    """family -> (model, module, clean pool, scanned data, checkpoint path): seeded weights, no training; 60 + 60 synthetic
    samples, about half of each with a bug"""
    from buglab.data.synthetic import make_report_dataset
    from buglab.models.modelregistry import load_model
    from buglab.runtime.neuralmodel import AbstractNeuralModel

    out = {}
    for family, spec in SPECS.items():
        kind = "seq" if family.startswith("seq") else "graph"
        pool, data = make_report_dataset(60, seed=18, kind=kind), make_report_dataset(60, seed=17, kind=kind)
        path = tmp_path_factory.mktemp("fdr_" + family.replace("-", "_")) / "detector.pkl.gz"
        model = load_model(dict(spec), path)[0]
        model.compute_metadata(copy.deepcopy(pool + data))
        torch.manual_seed(5)
        model.save(path, model.build_neural_module())
        out[family] = AbstractNeuralModel.restore_model(Path(path), torch.device(DEV)) + (pool, data, path)
    return out


def _same_records(a, b):
    return json.dumps(a, sort_keys=True) == json.dumps(b, sort_keys=True)  # (bit-equal floats print alike; a NaN equals a NaN)


@pytest.mark.parametrize("family", list(SPECS))
def test_fit_then_scan_on_the_device_equals_the_host_path(family, untrained):
    from buglab.models import _fdr as F
    from buglab.models import fdr as T
    from buglab.models import visualize as V

    model, nn_, pool, data, _ = untrained[family]
    device = torch.device(DEV)
    model.null_reference = None
    num_clean = sum(p["target_fix_action_idx"] is None for p in pool)
    on_host = T.fit_null_reference(model, nn_, pool, device, host=True, parallelize=False)
    ref = T.fit_null_reference(model, nn_, pool, device, parallelize=False)
    assert model.null_reference is ref and ref.scores.tobytes() == on_host.scores.tobytes() and ref[1:] == on_host[1:]
    assert (ref.num_kept, ref.num_dropped_nan, ref.num_skipped_buggy, ref.calibration) == (num_clean, 0, 60 - num_clean, None)
    assert 10 < num_clean < 60 and np.unique(ref.scores).shape[0] > 5  # the model tells samples apart
    for q in (0.5, 1.0):
        a = T.scan_with_fdr(model, nn_, data, device, q, top_k=3, parallelize=False)
        b = T.scan_with_fdr(model, nn_, data, device, q, top_k=3, host=True, parallelize=False)
        assert a.positions == b.positions == list(range(60)) and a.labels == b.labels
        C.assert_equal_bits((a.score, a.count, a.p_value, a.q_value, a.flagged), (b.score, b.count, b.p_value, b.q_value, b.flagged), (family, q))
        assert (a.cutoff, a.num_flagged, a.q_effective) == (b.cutoff, b.num_flagged, b.q_effective) and _same_records(a.summary, b.summary)
        assert _same_records(a.records(), b.records()) and len(a.records()) == 60
    assert a.num_flagged == 60 and a.cutoff == ref.num_kept  # at q = 1 everything is flagged
    # a stream of unknown length, collated in worker threads: the buffers grow on the device
    grown = T._scores_on_device(model, nn_, ((p, i) for i, p in enumerate(data)), device, True, ref.scores, lambda tag: None, 1)
    assert grown.positions == list(range(60))
    C.assert_equal_bits((grown.score.cpu().numpy(), grown.count.cpu().numpy()), (a.score, a.count))

    # a reference that puts a third of the scan below every one of its scores: some, not all, samples are flagged whatever the
    # untrained model thinks
    bar = np.sort(a.score)[20]
    model.null_reference = F.make_null_reference(a.score[a.score >= bar], 60, 0, None)
    n_ref = model.null_reference.num_kept
    some = T.scan_with_fdr(model, nn_, data, device, 0.2, top_k=3, html=True, parallelize=False)
    host = T.scan_with_fdr(model, nn_, data, device, 0.2, top_k=3, html=True, host=True, parallelize=False)
    below = int((a.score < bar).sum())
    assert 0 < below <= 20 and 60 <= 0.2 * (n_ref + 1) * below  # count 0 qualifies: (0 + 1) N <= q (n + 1) R[0]
    assert below <= some.num_flagged < 60 and (some.count[some.flagged] <= some.cutoff).all() and (some.count[~some.flagged] > some.cutoff).all()
    assert _same_records(some.records(), host.records()) and _same_records(some.summary, host.summary)
    records = some.records()
    flagged_positions = [r["position"] for r in records if r["flagged"]]
    assert [("suggestions" in r) for r in records] == [r["flagged"] for r in records] and len(flagged_positions) == some.num_flagged
    assert all(1 <= len(r["suggestions"]) <= 3 and all(s["kind"] == "rewrite" for s in r["suggestions"]) for r in records if r["flagged"])
    # the page holds exactly the flagged samples: it is the report of a scan over them and nothing else
    subset = [data[i] for i in flagged_positions]
    assert some.html == V.report_to_html(V.scan(model, nn_, subset, device).snippets)
    assert some.html.count('<section class="snippet') == some.num_flagged == host.html.count('<section class="snippet')
    lab = some.summary["labelled"]
    buggy = np.array([p["target_fix_action_idx"] is not None for p in data])
    assert lab["num_buggy"] == int(buggy.sum()) and lab["false_alarms"] == int((some.flagged & ~buggy).sum())
    assert lab["false_discovery_proportion"] == lab["false_alarms"] / some.num_flagged
    assert lab["power"] == int((some.flagged & buggy).sum()) / int(buggy.sum())
    model.null_reference = None


def test_command_line_fit_then_scan(untrained, tmp_path, capsys):
    from buglab.models import fdr as T
    from buglab.runtime.neuralmodel import AbstractNeuralModel
    from buglab.utils.msgpackutils import load_all_msgpack_l_gz, save_msgpack_l_gz

    _, _, pool, data, path = untrained["gnn-mlp"]
    clean_dir, scan_dir = tmp_path / "clean", tmp_path / "scan"
    clean_dir.mkdir(), scan_dir.mkdir()
    save_msgpack_l_gz(pool, clean_dir / "x.msgpack.l.gz"), save_msgpack_l_gz(data, scan_dir / "x.msgpack.l.gz")
    out_model, out, page, report = tmp_path / "with_reference.pkl.gz", tmp_path / "scan.jsonl.gz", tmp_path / "page.html", tmp_path / "report.json"
    # a checkpoint without the field: status 2, nothing written
    assert T.run(T.parse_args(["scan", str(path), str(scan_dir), str(out), "--fdr", "0.5", "--sequential"])) == 2 and not out.exists()
    capsys.readouterr()
    assert T.run(T.parse_args(["fit", str(path), str(clean_dir), str(out_model), "--max-reference", "20", "--sequential"])) == 0
    assert "kept 20 clean scores" in capsys.readouterr().out
    model, nn_ = AbstractNeuralModel.restore_model(out_model, torch.device(DEV))
    assert model.null_reference.num_kept == 20 and AbstractNeuralModel.restore_model(path, torch.device(DEV))[0].null_reference is None
    args = ["scan", str(out_model), str(scan_dir), str(out), "--fdr", "1.0", "--top-k", "2", "--html", str(page), "--report-json", str(report),
            "--sequential"]
    assert T.run(T.parse_args(args)) == 0
    text = capsys.readouterr().out
    with gzip.open(out, "rt", encoding="utf-8") as f:
        records = [json.loads(line) for line in f]
    read_back = list(load_all_msgpack_l_gz(scan_dir))  # the samples as the tool reads them
    want = T.scan_with_fdr(model, nn_, read_back, DEV, 1.0, top_k=2, parallelize=False)
    assert records == json.loads(json.dumps(want.records())) and [r["position"] for r in records] == list(range(60))
    assert all(r["flagged"] and len(r["suggestions"]) <= 2 for r in records)
    assert page.read_text(encoding="utf-8").count('<section class="snippet') == 60
    blob = json.loads(report.read_text(encoding="utf-8"))
    assert blob == json.loads(json.dumps(want.summary)) and blob["num_flagged"] == 60 and blob["num_reference"] == 20
    lab = blob["labelled"]
    assert lab["false_discovery_proportion"] == lab["false_alarms"] / 60 and lab["power"] == 1.0 and 0 < lab["num_buggy"] < 60
    assert "Flagged 60 samples" in text and "realised false discovery proportion" in text

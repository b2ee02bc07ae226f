"""GPU: prediction and evaluation with the GREAT var-misuse model.
  * the forward-only head (hip_ops.varmisuse_predict, csrc/bl_varmisuse_predict.hip): logits bit-equal to the training head's, the
    per-sample records against the NumPy twin (buglab/models/_great_predict.py) fed those logits, bit-identical reruns, appending
    into run-long buffers;
  * `evaluate_great` against the counters of a validation pass over the same minibatches, on the device against the host judge;
  * `GreatVarMisuse.predict` per sample, and the command line of buglab/models/evaluategreat.py."""
import json
import math

import numpy as np
import pytest
import torch

from tests.test_great_varmisuse_gpu import _head_case, _small_factory

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from buglab.models import hip_ops

    hip_ops.load_library()


def _case(name):
    if name == "odd_L_full_length":      # L not a multiple of 4, one sample with length == L
        return _head_case(D=64, B=3, L=23, seed=0, full_lengths=True)
    if name == "no_bug_no_candidates":   # no buggy sample, and one sample without candidates
        t = _head_case(D=128, B=4, L=37, seed=1, no_bug=True)
        t[7][1] = False
        return t
    if name == "ties":                   # two equal largest logits in each column of sample 0: the first index wins
        t = _head_case(D=512, B=5, L=64, seed=2, ties=True)  # localization: rows 3 and 7
        x, ln_g, W, cand = t[0], t[1], t[3], t[7]
        x[5] = W[:, 1] * ln_g                               # pointer: rows 5 and 9
        x[9] = x[5]
        cand[0, 5] = cand[0, 9] = True
        return t
    if name == "widest":                 # the widest row the head takes
        return _head_case(D=1024, B=2, L=8, seed=5)
    if name == "longer_than_a_workgroup":  # 257 positions: thread 0 takes two, every wave and the block reductions are live
        return _head_case(D=64, B=2, L=257, seed=7, full_lengths=True)
    raise KeyError(name)


def _device(tensors):
    x, ln_g, ln_b, W, bias, lens_att, err, cand, tgt = tensors
    f = lambda t: t.float().cuda()
    return [f(x), f(ln_g), f(ln_b), f(W), f(bias), lens_att.cuda(), err.cuda(), cand.cuda(), tgt.cuda()]


def _predict(dev, out_d, out_i, offset):
    from buglab.models import hip_ops

    return hip_ops.varmisuse_predict(*dev, out_d, out_i, offset)


def _buffers(n, fill_d=-7.25, fill_i=-77):
    return (torch.full((7, n), fill_d, dtype=torch.float64, device="cuda"), torch.full((4, n), fill_i, dtype=torch.int32, device="cuda"))


def _assert_records(got_d, got_i, want_d, want_i):
    """Integer rows equal; -inf and NaN exactly where the twin has them; the rest within 1e-12 absolute (sums of at most 512 fp64
    terms: a few hundred ulp, far below this)."""
    assert np.array_equal(got_i, want_i)
    assert np.array_equal(np.isnan(got_d), np.isnan(want_d))
    assert np.array_equal(np.isneginf(got_d), np.isneginf(want_d)) and not np.isposinf(got_d).any()
    fin = np.isfinite(want_d)
    worst = float(np.abs(got_d[fin] - want_d[fin]).max())
    print("max |device - twin| over the fp64 rows:", worst)
    assert worst <= 1e-12


def _twin(logits, tensors):
    from buglab.models._great_predict import judge_great_host

    lens_att, err, tgt = tensors[5], tensors[6], tensors[8]
    B = lens_att.shape[0]
    return judge_great_host(logits.cpu().numpy(), logits.shape[0] // B, lens_att.numpy(), err.numpy(), tgt.numpy())


@pytest.mark.parametrize("name", ["odd_L_full_length", "no_bug_no_candidates", "ties", "widest", "longer_than_a_workgroup"])
def test_kernel_matches_training_logits_and_twin(name):
    from buglab.models import hip_ops

    tensors = _case(name)
    dev = _device(tensors)
    B = tensors[5].shape[0]
    stats = torch.zeros(hip_ops.VARMISUSE_STATS, dtype=torch.float64, device="cuda")
    _, train_logits, _ = hip_ops.varmisuse_head(*dev, stats)
    out_d, out_i = _buffers(B)
    logits = _predict(dev, out_d, out_i, 0)
    assert logits.dtype == torch.float32 and logits.shape == train_logits.shape
    assert torch.equal(logits.view(torch.int32), train_logits.view(torch.int32))  # bit-equal, -inf included
    want_d, want_i = _twin(logits, tensors)
    got_d, got_i = out_d.cpu().numpy(), out_i.cpu().numpy()
    _assert_records(got_d, got_i, want_d, want_i)
    if name == "ties":
        lg = logits.cpu().reshape(B, -1, 2)[0]
        assert lg[3, 0] == lg[7, 0] == lg[:, 0].max() and lg[5, 1] == lg[9, 1] == lg[:, 1].max()  # (the case is what it says)
        assert got_i[0, 0] == 3 and got_i[1, 0] == 5
    if name == "no_bug_no_candidates":
        assert got_i[1, 1] == -1 and math.isnan(got_d[5, 1]) and got_d[1, 1] == -math.inf and (got_d[6] == -math.inf).all()
    if name == "odd_L_full_length":
        assert int(tensors[5][0]) == 23
    if name == "longer_than_a_workgroup":
        assert int(tensors[5][0]) == 257
    again_d, again_i = _buffers(B, 1.5, 5)
    again = _predict(dev, again_d, again_i, 0)
    assert torch.equal(again.view(torch.int32), logits.view(torch.int32))
    assert torch.equal(again_d.view(torch.int64), out_d.view(torch.int64)) and torch.equal(again_i, out_i)  # bit-identical rerun


def test_records_append_at_the_offset():
    first, second = _head_case(D=64, B=3, L=23, seed=0, full_lengths=True), _head_case(D=64, B=3, L=18, seed=9)
    B = 3
    N = 2 * B + 3
    out_d, out_i = _buffers(N)
    parts = []
    for k, tensors in enumerate((first, second)):
        logits = _predict(_device(tensors), out_d, out_i, k * B)
        parts.append(_twin(logits, tensors))
    got_d, got_i = out_d.cpu().numpy(), out_i.cpu().numpy()
    _assert_records(got_d[:, : 2 * B], got_i[:, : 2 * B], np.concatenate([p[0] for p in parts], 1), np.concatenate([p[1] for p in parts], 1))
    assert (got_d[:, 2 * B:] == -7.25).all() and (got_i[:, 2 * B:] == -77).all()
    with pytest.raises(ValueError, match="do not fit"):
        _predict(_device(first), out_d, out_i, N - B + 1)


# ---- the model -----------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def trained():
    """(model, module on the device, 48 synthetic records): random weights -- what is compared does not depend on training."""
    from buglab.data.synthetic_great import make_great_records

    model = _small_factory()
    recs = make_great_records(48, seed=21)
    model.compute_metadata(recs)
    torch.manual_seed(3)
    return model, model.build_neural_module().cuda(), recs


def test_evaluate_great_matches_a_validation_pass(trained):
    from buglab.models.evaluategreat import evaluate_great

    model, nn, recs = trained
    nn.eval()
    nn.reset_metrics()
    with torch.no_grad():
        for mb, _ in model.minibatch_iterator(model.tensorize_dataset(recs), "cuda", 16):
            nn(**mb)
    valid = dict(zip(("samples", "localization_hits", "buggy_localization_hits", "buggy_samples", "repair_hits", "localization_loss_sum",
                      "repair_loss_sum"), nn.metric_stats.cpu().tolist()))
    nn.train()  # prediction reads no training flag ...
    nn.reset_metrics()
    step = nn._dropout_step
    ev = evaluate_great(model, nn, recs, "cuda", minibatch_size=16, parallelize=False)
    assert nn.training and nn._dropout_step == step and not nn.metric_stats.any()  # ... and changes none of these
    counts = ev.counts()
    assert valid["samples"] == 48 and 0 < valid["buggy_samples"] < 48 and ev.skipped == 0
    for k in ("samples", "localization_hits", "buggy_localization_hits", "buggy_samples", "repair_hits"):
        assert counts[k] == valid[k], k
    for total, n in (("localization_loss_sum", "samples"), ("repair_loss_sum", "buggy_samples")):
        a, b = counts[total] / counts[n], valid[total] / valid[n]
        print(total, "mean: records", a, "validation", b)
        assert abs(a - b) <= 1e-5 * abs(b), total
    assert ev.metrics()["Num samples"] == 48


def test_predict_leaves_the_module_alone_and_yields_per_sample(trained):
    model, nn, recs = trained
    recs = [dict(r) for r in recs[:20]]
    strings = [k for k, r in enumerate(recs) if r["error_location"] == 0][:2]
    for k in strings:
        recs[k]["repair_candidates"] = ["value_1", "count_0"]  # the GREAT data's no-bug records: no integer candidate
    long = dict(recs[0], source_tokens=recs[0]["source_tokens"] * 12)
    assert len(long["source_tokens"]) > 256
    data = recs[:5] + [long] + recs[5:]
    nn.train()
    nn.reset_metrics()
    nn.metric_stats[0] = 5.0
    step = nn._dropout_step
    out = list(model.predict(data, nn, "cuda", parallelize=True, minibatch_size=8))
    assert nn.training and nn._dropout_step == step and nn.metric_stats.tolist() == [5.0] + [0.0] * 7
    assert [r for r, _ in out] == recs  # one prediction per accepted record, in order
    lengths = [len(r["source_tokens"]) for r in recs]
    for k, (r, p) in enumerate(out):
        group = lengths[k // 8 * 8 : k // 8 * 8 + 8]
        la = min(lengths[k] + 1, max(group))
        assert p.localization_logprobs.dtype == np.float64 and p.localization_logprobs.shape == (la,)
        assert abs(np.exp(p.localization_logprobs).sum() - 1) < 1e-9
        assert 0 <= p.predicted_location < la and p.location_logprob == p.localization_logprobs[p.predicted_location]
        assert p.no_bug_logprob == p.localization_logprobs[0] and p.location_logprob == p.localization_logprobs.max()
        assert (p.predicted_repair is None) == (k in strings)
        if k in strings:
            assert p.repair_logprob is None and p.repair_logprobs == {}
        else:
            assert sorted(p.repair_logprobs) == sorted(c for c in r["repair_candidates"] if c < la)
            assert p.repair_logprobs[p.predicted_repair] == p.repair_logprob == max(p.repair_logprobs.values())
            assert abs(sum(math.exp(v) for v in p.repair_logprobs.values()) - 1) < 1e-9


def test_evaluate_great_on_device_equals_host_judge(trained):
    from buglab.models.evaluategreat import evaluate_great

    model, nn, recs = trained
    dev = evaluate_great(model, nn, iter(recs), "cuda", minibatch_size=16, parallelize=True, capacity=1)  # (a stream: no len(); it grows)
    host = evaluate_great(model, nn, recs, "cuda", minibatch_size=16, parallelize=False, on_device=False)
    assert np.array_equal(dev.out_i, host.out_i) and dev.kinds == host.kinds and np.array_equal(dev.error_location, host.error_location)
    _assert_records(dev.out_d, dev.out_i, host.out_d, host.out_i)
    a, b = dev.report(), host.report()
    sa, sb = a.summary(), b.summary()
    assert {k: v for k, v in sa.items() if k.startswith("num_")} == {k: v for k, v in sb.items() if k.startswith("num_")}
    assert a.per_scout() == b.per_scout() and dev.counts()["repair_hits"] == host.counts()["repair_hits"]
    ca, cb = a.curves(), b.curves()
    for k in ca:
        assert np.allclose(ca[k], cb[k], rtol=0, atol=1e-9, equal_nan=True), k


def test_buffer_grows_for_a_stream(trained):
    """A stream longer than the first buffer: the records already written survive the doubling."""
    from buglab.models import evaluategreat

    model, nn, recs = trained
    whole = evaluategreat.evaluate_great(model, nn, recs, "cuda", minibatch_size=16, parallelize=False)

    class Tiny(list):  # reports a length shorter than the stream it yields
        def __len__(self):
            return 5

    grown = evaluategreat.evaluate_great(model, nn, Tiny(recs), "cuda", minibatch_size=16, parallelize=False)
    assert np.array_equal(grown.out_i, whole.out_i) and np.array_equal(grown.out_d, whole.out_d)


def test_command_line(trained, tmp_path, capsys):
    from buglab.data.synthetic_great import write_great_dir
    from buglab.models import evaluategreat

    model, nn, recs = trained
    bad = dict(recs[1], error_location=recs[1]["repair_candidates"][0], repair_targets=[0], has_bug=True)  # no candidate is a target
    data = recs + [bad]
    write_great_dir(str(tmp_path / "test"), data, per_file=20)
    model.save(tmp_path / "great.pkl.gz", nn)
    args = evaluategreat.parse_args([str(tmp_path / "great.pkl.gz"), str(tmp_path / "test"), "--minibatch-size", "16", "--report-json",
                                     str(tmp_path / "report.json"), "--predictions-out", str(tmp_path / "pred.jsonl")])
    result = evaluategreat.run(args)
    text = capsys.readouterr().out
    report = json.loads((tmp_path / "report.json").read_text())
    lines = [json.loads(line) for line in (tmp_path / "pred.jsonl").read_text().splitlines()]
    assert report["skipped"] == 1 and report["summary"]["num_samples"] + report["skipped"] == len(data)
    assert len(lines) == report["summary"]["num_samples"] == result.out_i.shape[1]
    assert "Localization Accuracy" in text and "Skipped records: 1" in text and "Accuracy (Localization & Repair)" in text
    assert [line["predicted_location"] for line in lines] == result.out_i[0].tolist()

"""GPU: weight averaging -- the EMA kept inside the fused clip + Adam pass (bl_adam_clip_step_ema / _dp_ema), the buffer exchange
(bl_swap_f32), FlatAdam's averaging and its checkpoint round trip, stale weight packs around `averaged_parameters()`, the
trainer end to end and the command line.

The bound on the average is derived, not measured: with the DEVICE's own p_new and previous ema, the kernel's
fma(omd, p_new - ema, ema) has one rounding in the subtraction (<= 2^-24 |p_new - ema| <= 2 * 2^-24 M, M = max(|p_new|, |ema|),
scaled by omd <= 1) and one in the fma (<= 2^-24 M): 3 units of 2^-24 M; the fourth is slack for the fp64 comparison."""
import copy
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests.conftest import PKG
from tests.guard_bands import guarded

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
SIZES = [1, 3, 255, 256, 257, 2048 * 256 + 261]  # the last: the capped grid goes round its stride loop twice, with a ragged end
HYPER = dict(lr=1e-2, beta1=0.9, beta2=0.999, eps=1e-8)
SPEC = {"hidden_state_size": 64, "num_layers": 4}  # the tiny gnn-mlp of tests/test_train_cli_gpu.py


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")


def _bits(t):
    return t.detach().contiguous().view(torch.int32)


def _same_bits(a, b):
    return a.shape == b.shape and bool(torch.equal(_bits(a), _bits(b)))


def _inputs(n, seed):
    """p, g, m, v, ema on the device; g is large enough for a 0.5 clip to bite at every size but the smallest"""
    gen = torch.Generator().manual_seed(seed)
    p = torch.randn(n, generator=gen)
    g = torch.randn(n, generator=gen)
    m = 0.1 * torch.randn(n, generator=gen)
    v = 0.01 * torch.rand(n, generator=gen)
    ema = p + 0.05 * torch.randn(n, generator=gen)
    return [t.to(DEV) for t in (p, g, m, v, ema)]


def _assert_ema_within_bound(ema_gpu, ema_old, p_new, omd, what):
    from buglab.runtime._averaging import ema_update_twin

    e_old, pn = ema_old.double().cpu().numpy(), p_new.double().cpu().numpy()
    twin = ema_update_twin(e_old, pn, float(np.float32(omd)))
    bound = 4.0 * 2.0 ** -24 * np.maximum(np.abs(pn), np.abs(e_old))
    err = np.abs(ema_gpu.double().cpu().numpy() - twin)
    worst = float((err / np.maximum(bound, 1e-300)).max())
    print(f"{what}: worst |ema - twin| / bound = {worst:.3f}")
    assert (err <= bound).all(), (what, worst)


def _run_pair(form, n, clip, step, omd, seed):
    """the existing entry point and the _ema one on copies of the same inputs -> (plain buffers, ema-form buffers, ema before)"""
    from buglab.models import hip_ops

    base = _inputs(n, seed)
    sqn = torch.zeros(1, device=DEV)
    hip_ops.sqnorm(base[1], sqn)
    bt = torch.tensor([3.0], device=DEV)
    a = [t.clone() for t in base]
    b = [t.clone() for t in base]
    if form == "plain":
        hip_ops.adam_clip_step(a[0], a[1], a[2], a[3], sqn, prescale=0.5, clip=clip, step=step, **HYPER)
        hip_ops.adam_clip_step_ema(b[0], b[1], b[2], b[3], b[4], sqn, one_minus_decay=omd, prescale=0.5, clip=clip, step=step, **HYPER)
    else:
        hip_ops.adam_clip_step_dp(a[0], a[1], a[2], a[3], sqn, bt, clip=clip, step=step, **HYPER)
        hip_ops.adam_clip_step_dp_ema(b[0], b[1], b[2], b[3], b[4], sqn, bt, one_minus_decay=omd, clip=clip, step=step, **HYPER)
    torch.cuda.synchronize()
    return base, a, b


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("form", ["plain", "dp"])
def test_kernel_parameters_bit_identical_and_average_within_bound(form, n):
    case = 0
    for clip in (0.5, 0.0):
        for step in (1, 7):
            omd = float(np.float32(1.0 - 0.9)) if step == 7 else float(np.float32(9.0 / 11.0))
            case += 1
            base, a, b = _run_pair(form, n, clip, step, omd, seed=100 * case + n % 97)
            for name, x, y in zip("pmv", (a[0], a[2], a[3]), (b[0], b[2], b[3])):
                assert _same_bits(x, y), (name, form, n, clip, step)
            assert _same_bits(b[1], base[1])                   # the gradient is read only
            assert not _same_bits(b[0], base[0]) or n == 0     # (the step did move the parameters)
            _assert_ema_within_bound(b[4], base[4], b[0], omd, f"{form} n={n} clip={clip} step={step}")


@pytest.mark.parametrize("n", [257, SIZES[-1]])
@pytest.mark.parametrize("form", ["plain", "dp"])
def test_kernel_five_chained_steps(form, n):
    """each step's twin starts from the DEVICE's previous average: the per-step bound needs no compounding"""
    from buglab.models import hip_ops
    from buglab.runtime._averaging import one_minus_decay_f32

    p, g, m, v, ema = _inputs(n, seed=5)
    q, _, qm, qv, _ = [t.clone() for t in (p, g, m, v, ema)]
    sqn = torch.zeros(1, device=DEV)
    bt = torch.tensor([2.0], device=DEV)
    gen = torch.Generator().manual_seed(6)
    for k in range(1, 6):
        g.copy_(torch.randn(n, generator=gen))
        hip_ops.sqnorm(g, sqn)
        omd = one_minus_decay_f32(k, 0.9)
        before = ema.clone()
        if form == "plain":
            hip_ops.adam_clip_step_ema(p, g, m, v, ema, sqn, one_minus_decay=omd, clip=0.5, step=k, **HYPER)
            hip_ops.adam_clip_step(q, g, qm, qv, sqn, clip=0.5, step=k, **HYPER)
        else:
            hip_ops.adam_clip_step_dp_ema(p, g, m, v, ema, sqn, bt, one_minus_decay=omd, clip=0.5, step=k, **HYPER)
            hip_ops.adam_clip_step_dp(q, g, qm, qv, sqn, bt, clip=0.5, step=k, **HYPER)
        assert _same_bits(p, q) and _same_bits(m, qm) and _same_bits(v, qv), k
        _assert_ema_within_bound(ema, before, p, omd, f"{form} n={n} chained step {k}")


@pytest.mark.parametrize("n", SIZES)
def test_idle_data_parallel_step_leaves_all_five_buffers_untouched(n):
    from buglab.models import hip_ops

    base = _inputs(n, seed=9)
    work = [t.clone() for t in base]
    sqn = torch.zeros(1, device=DEV)
    hip_ops.sqnorm(work[1], sqn)
    for total in (0.0, -1.0):
        bt = torch.tensor([total], device=DEV)
        hip_ops.adam_clip_step_dp_ema(work[0], work[1], work[2], work[3], work[4], sqn, bt, one_minus_decay=0.25, clip=0.5, step=3, **HYPER)
        for name, x, y in zip(("p", "g", "m", "v", "ema"), work, base):
            assert _same_bits(x, y), (name, n, total)


def _guarded_vector(n, values, lead=4):
    G = guarded(1, n, ld=(n + 3) // 4 * 4, dtype=torch.float32, device=DEV, lead=lead, guard_rows=256 if n <= 257 else 1)
    G.fill(values.view(1, n))
    return G, G.view[0]


@pytest.mark.parametrize("n", SIZES)
def test_guard_bands_around_parameters_and_average(n):
    """`param` and `ema` inside pattern-filled allocations (16- but not 32-byte aligned): both kernels and the swap store
    nothing outside [0, n)"""
    from buglab.models import hip_ops

    p0, g, m, v, e0 = _inputs(n, seed=13)
    P, p = _guarded_vector(n, p0)
    E, e = _guarded_vector(n, e0)
    assert p.data_ptr() % 32 == 16 and p.is_contiguous() and p.shape == (n,)
    sqn = torch.zeros(1, device=DEV)
    hip_ops.sqnorm(g, sqn)
    q, qm, qv = p0.clone(), m.clone(), v.clone()
    hip_ops.adam_clip_step_ema(p, g, m, v, e, sqn, one_minus_decay=0.5, clip=0.5, step=1, **HYPER)
    hip_ops.adam_clip_step(q, g, qm, qv, sqn, clip=0.5, step=1, **HYPER)
    assert _same_bits(p, q)
    _assert_ema_within_bound(e, e0, p, 0.5, f"guarded n={n}")
    hip_ops.adam_clip_step_dp_ema(p, g, m, v, e, sqn, torch.tensor([2.0], device=DEV), one_minus_decay=0.5, clip=0.5, step=2, **HYPER)
    P.assert_untouched("param after the two fused steps")
    E.assert_untouched("ema after the two fused steps")
    assert bool(torch.isfinite(p).all()) and bool(torch.isfinite(e).all())
    was_p, was_e = p.clone(), e.clone()
    hip_ops.swap_buffers(p, e)
    assert _same_bits(p, was_e) and _same_bits(e, was_p)
    P.assert_untouched("param after the swap")
    E.assert_untouched("ema after the swap")


@pytest.mark.parametrize("n", SIZES)
def test_swap_is_bit_exact_also_off_the_16_byte_grid_and_is_its_own_inverse(n):
    from buglab.models import hip_ops

    gen = torch.Generator().manual_seed(n % 1000)
    # bit patterns, not numbers: NaN payloads, infinities and denormals must cross unchanged
    a0 = torch.randint(-2 ** 31, 2 ** 31 - 1, (n,), generator=gen, dtype=torch.int64).to(torch.int32).view(torch.float32).to(DEV)
    b0 = torch.randint(-2 ** 31, 2 ** 31 - 1, (n,), generator=gen, dtype=torch.int64).to(torch.int32).view(torch.float32).to(DEV)
    for lead_a, lead_b in ((4, 4), (5, 4), (5, 7)):
        A, a = _guarded_vector(n, a0, lead=lead_a)
        B, b = _guarded_vector(n, b0, lead=lead_b)
        assert a.data_ptr() % 16 == 4 * (lead_a % 4) and b.data_ptr() % 16 == 4 * (lead_b % 4)
        hip_ops.swap_buffers(a, b)
        assert _same_bits(a, b0) and _same_bits(b, a0), (n, lead_a, lead_b)
        hip_ops.swap_buffers(a, b)
        assert _same_bits(a, a0) and _same_bits(b, b0), (n, lead_a, lead_b)
        A.assert_untouched(f"a (lead {lead_a})")
        B.assert_untouched(f"b (lead {lead_b})")


def test_swap_refuses_overlap_and_accepts_nothing():
    from buglab.models import hip_ops

    lib = hip_ops.load_library()
    buf = torch.arange(64, dtype=torch.float32, device=DEV)
    was = buf.clone()
    stream = torch.cuda.current_stream().cuda_stream
    for off_a, off_b, n in ((0, 4, 8), (4, 0, 8), (0, 0, 1), (3, 10, 8)):
        rc = lib.bl_swap_f32(buf.data_ptr() + 4 * off_a, buf.data_ptr() + 4 * off_b, n, stream)
        assert rc != 0 and b"overlap" in lib.bl_last_error(), (off_a, off_b, n)
    assert lib.bl_swap_f32(buf.data_ptr(), buf.data_ptr() + 16, 0, stream) == 0  # BL_OK: n == 0 is a no-op
    with pytest.raises(RuntimeError, match="overlap"):
        hip_ops.swap_buffers(buf[0:8], buf[4:12])
    hip_ops.swap_buffers(buf[0:0], buf[0:0])
    assert _same_bits(buf, was)
    hip_ops.swap_buffers(buf[0:8], buf[8:16])  # adjacent, not overlapping
    assert _same_bits(buf[0:8], was[8:16]) and _same_bits(buf[8:16], was[0:8]) and _same_bits(buf[16:], was[16:])


# ---- FlatAdam with manufactured gradients: no model involved ------------------------------------------------------------------
SHAPES = [(37, 5), (13,), (64, 3)]


def _fresh_params(seed=21):
    gen = torch.Generator().manual_seed(seed)
    return [torch.nn.Parameter(torch.randn(*s, generator=gen).to(DEV)) for s in SHAPES]


def _gradients(numel, steps, seed=22):
    gen = torch.Generator().manual_seed(seed)
    return [torch.randn(numel, generator=gen).to(DEV) for _ in range(steps)]


def _flat_adam(params, **kw):
    from buglab.runtime.optim import FlatAdam

    return FlatAdam(params, lr=1e-2, clip_gradient_norm=0.5, num_warmup_steps=0, **kw)


def _steps(opt, grads):
    for g in grads:
        opt.flat_grad.copy_(g)
        opt.step()


def test_flat_adam_average_follows_the_twin_and_parameters_do_not_notice():
    from buglab.runtime._averaging import one_minus_decay_f32

    plain = _flat_adam(_fresh_params())
    opt = _flat_adam(_fresh_params(), ema_decay=0.9)
    assert plain.ema is None and _same_bits(opt.ema, opt.flat_param) and _same_bits(opt.flat_param, plain.flat_param)
    grads = _gradients(opt.numel, 6)
    ptr = (opt.flat_param.data_ptr(), opt.ema.data_ptr())
    for k, g in enumerate(grads, start=1):
        before = opt.ema.clone()
        _steps(opt, [g])
        _steps(plain, [g])
        assert _same_bits(opt.flat_param, plain.flat_param) and _same_bits(opt.m, plain.m) and _same_bits(opt.v, plain.v), k
        _assert_ema_within_bound(opt.ema, before, opt.flat_param, one_minus_decay_f32(k, 0.9), f"FlatAdam step {k}")
    assert not _same_bits(opt.ema, opt.flat_param)
    assert ptr == (opt.flat_param.data_ptr(), opt.ema.data_ptr())

    # averaged_parameters(): contents trade places, views stay; no step and no nesting inside; restored when the body raises
    raw, avg = opt.flat_param.clone(), opt.ema.clone()
    views = [(p.data.data_ptr(), p.grad.data_ptr()) for p in opt.params]
    with opt.averaged_parameters():
        assert _same_bits(opt.flat_param, avg) and _same_bits(opt.ema, raw)
        off, _ = opt._span[id(opt.params[1])]
        assert _same_bits(opt.params[1].data, avg[off:off + 13])
        with pytest.raises(RuntimeError):
            opt.step()
        with pytest.raises(RuntimeError):
            with opt.averaged_parameters():
                pass
        with pytest.raises(RuntimeError):
            opt.state_dict()
    assert _same_bits(opt.flat_param, raw) and _same_bits(opt.ema, avg)
    with pytest.raises(KeyError):
        with opt.averaged_parameters():
            raise KeyError("the body raises")
    assert _same_bits(opt.flat_param, raw) and _same_bits(opt.ema, avg)
    assert views == [(p.data.data_ptr(), p.grad.data_ptr()) for p in opt.params]
    assert ptr == (opt.flat_param.data_ptr(), opt.ema.data_ptr())
    with plain.averaged_parameters():  # averaging off: a no-op context
        assert _same_bits(plain.flat_param, raw)


def test_flat_adam_continued_run_is_the_same_run():
    """3 steps, state_dict, a fresh FlatAdam on parameters holding the AVERAGE (what the checkpoint holds), enable_averaging,
    load_state_dict, 3 more steps == 6 steps straight, bit for bit"""
    straight = _flat_adam(_fresh_params(), ema_decay=0.9)
    grads = _gradients(straight.numel, 6)
    _steps(straight, grads)

    first = _flat_adam(_fresh_params(), ema_decay=0.9)
    _steps(first, grads[:3])
    sd = {k: (v.detach().cpu().clone() if isinstance(v, torch.Tensor) else v) for k, v in first.state_dict().items()}
    assert set(sd) == {"m", "v", "step", "param", "ema", "ema_decay", "ema_start_step"} and sd["step"] == 3
    resumed_params = _fresh_params(seed=99)
    for old, new in zip(first.params, resumed_params):
        off, _ = first._span[id(old)]
        new.data.copy_(first.ema[off:off + old.numel()].view(old.shape))
    second = _flat_adam(resumed_params)
    second.enable_averaging(0.9)
    second.load_state_dict({k: (v.to(DEV) if isinstance(v, torch.Tensor) else v) for k, v in sd.items()})
    assert second.step_count - second.ema_start_step == 3
    _steps(second, grads[3:])
    for name in ("flat_param", "m", "v", "ema"):
        assert _same_bits(getattr(second, name), getattr(straight, name)), name
    assert second.step_count == straight.step_count == 6


# ---- a real model: stale packs, the trainer, the command line ---------------------------------------------------------------
def stale_pack_losses(optimizer_class):
    """-> (loss before entering, loss inside averaged_parameters(), loss of a second module filled from the average, loss after
    leaving), each a Python float of an fp32.  Module-level so that the effect of the invalidate_weight_packs() calls can be
    checked from outside with an optimiser class that leaves them out."""
    from pathlib import Path

    from buglab.data.collate import to_device
    from buglab.data.synthetic import make_buglab_dataset
    from buglab.models import hip_ops
    from buglab.models.modelregistry import load_model

    was = hip_ops.deterministic()
    hip_ops.set_deterministic(True)  # before collating: the collator lays the minibatch out for the ordered kernels
    try:
        data = make_buglab_dataset(8, seed=4)
        model = load_model(dict(SPEC, modelName="gnn-mlp"), Path("/tmp/_bl_averaging_stale.pkl.gz"))[0]
        model.compute_metadata(copy.deepcopy(data))
        samples = [s for s in (model.tensorize(copy.deepcopy(d)) for d in data) if s is not None]
        mb = to_device(model.collate_minibatch({"samples": samples}), DEV)
        torch.manual_seed(0)
        nn_ = model.build_neural_module().to(DEV).train()
        opt = optimizer_class(nn_.parameters(), lr=1e-2, num_warmup_steps=0, ema_decay=0.5)
        for step in range(3):
            opt.zero_grad()
            nn_(**mb, dropout_seed=step).backward()
            opt.step()
        nn_.eval()
        other = model.build_neural_module().to(DEV).eval()
        for p, q in zip(nn_.parameters(), other.parameters()):
            off, _ = opt._span[id(p)]
            q.data.copy_(opt.ema[off:off + p.numel()].view(p.shape))
        hip_ops.invalidate_weight_packs()
        with torch.no_grad():
            reference = float(other(**mb))
            before = float(nn_(**mb))  # packs the RAW weights: what a missing invalidation would leave in use
            with opt.averaged_parameters():
                inside = float(nn_(**mb))
            after = float(nn_(**mb))
    finally:
        hip_ops.set_deterministic(was)
    return before, inside, reference, after


def test_no_stale_weight_packs_around_averaged_parameters():
    from buglab.runtime.optim import FlatAdam

    before, inside, reference, after = stale_pack_losses(FlatAdam)
    print(f"loss raw {before!r}, averaged {inside!r}, reference module {reference!r}, raw again {after!r}")
    assert inside == reference  # bit-equal: both are floats of fp32 values
    assert after == before
    assert before != reference  # (the average is not the iterate: the two comparisons above can tell them apart)


@pytest.fixture(scope="module")
def shards(tmp_path_factory):
    from buglab.data.synthetic import make_buglab_dataset
    from buglab.utils.msgpackutils import save_msgpack_l_gz

    root = tmp_path_factory.mktemp("averaging")
    data = make_buglab_dataset(64, seed=5)
    (root / "train").mkdir()
    (root / "valid").mkdir()
    save_msgpack_l_gz(data[:48], root / "train" / "a.msgpack.l.gz")
    save_msgpack_l_gz(data[48:], root / "valid" / "v.msgpack.l.gz")
    return root


def _train(shards, path, ema_decay):
    """-> (trainer, optimiser, per-epoch snapshots taken by a validation-epoch-end hook)"""
    from buglab.models import train
    from buglab.models.modelregistry import load_model
    from buglab.runtime.optim import FlatAdam
    from buglab.runtime.richpath import RichPath
    from buglab.runtime.shardloader import ShardDataset
    from buglab.runtime.trainer import LazyDataIterable, ModelTrainer

    box, snapshots = {}, []

    def creator(params):
        box["opt"] = FlatAdam(params, lr=1e-3, num_warmup_steps=0)
        return box["opt"]

    def at_validation_end(model, nn_, epoch, metrics):
        # runs inside averaged_parameters(): with averaging, flat_param holds the average and `ema` the raw iterate
        opt = box["opt"]
        snapshots.append({"step": opt.step_count, "in_place": opt.flat_param.clone(), "aside": None if opt.ema is None else opt.ema.clone()})

    model = load_model(dict(SPEC, modelName="gnn-mlp"), path)[0]
    trainer = ModelTrainer(model, path, max_num_epochs=2, minibatch_size=16, optimizer_creator=creator, clip_gradient_norm=0.5,
                           ema_decay=ema_decay)
    trainer.register_validation_epoch_end_hook(at_validation_end)
    torch.manual_seed(0)
    np.random.seed(0)
    trainer.load_metadata_and_create_network(
        LazyDataIterable(train.construct_data_loading_callable(RichPath.create(str(shards / "train")))), False, False)
    trainer.train(ShardDataset(str(shards / "train"), shuffle=True), ShardDataset(str(shards / "valid")), show_progress_bar=False,
                  initialize_metadata=False, parallelize=False, patience=100)
    torch.cuda.synchronize()
    return trainer, box["opt"], snapshots


def test_trainer_checkpoint_holds_the_average_and_the_live_module_the_iterate(shards, tmp_path):
    from buglab.runtime.neuralmodel import AbstractNeuralModel

    path = tmp_path / "averaged.pkl.gz"
    trainer, opt, snapshots = _train(shards, path, 0.5)
    assert len(snapshots) == 2 and 0 < snapshots[0]["step"] < snapshots[1]["step"] == opt.step_count
    sidecar = torch.load(str(path) + ".optim", map_location=DEV, weights_only=False)
    assert set(sidecar) == {"m", "v", "step", "param", "ema", "ema_decay", "ema_start_step"}
    assert sidecar["ema_decay"] == 0.5 and sidecar["ema_start_step"] == 0
    saved = next(s for s in snapshots if s["step"] == sidecar["step"])  # the epoch whose validation improved last
    average, raw = saved["in_place"], saved["aside"]
    assert not _same_bits(average, raw)
    assert _same_bits(sidecar["ema"], average) and _same_bits(sidecar["param"], raw)

    _, restored = AbstractNeuralModel.restore_model(path, torch.device(DEV))
    live = list(trainer.neural_module.parameters())
    loaded = list(restored.parameters())
    assert len(loaded) == len(live) == len(opt.params)
    differs = 0
    for p, q in zip(live, loaded):
        off, _ = opt._span[id(p)]
        assert _same_bits(q.data, average[off:off + p.numel()].view(p.shape))      # the checkpoint holds the average ...
        differs += not _same_bits(q.data, raw[off:off + p.numel()].view(p.shape))  # ... which is not the raw iterate
        # the live module is still a set of views into flat_param
        assert p.data.data_ptr() == opt.flat_param.data_ptr() + 4 * off
    assert differs > 0
    # after train() the live module holds the raw iterate again (of the LAST epoch, saved or not)
    assert _same_bits(opt.flat_param, snapshots[-1]["aside"]) and _same_bits(opt.ema, snapshots[-1]["in_place"])
    assert not opt._averaged_in_place


def test_trainer_without_averaging_writes_the_sidecar_it_always_wrote(shards, tmp_path):
    path = tmp_path / "plain.pkl.gz"
    _, opt, snapshots = _train(shards, path, None)
    assert opt.ema is None and all(s["aside"] is None for s in snapshots)
    sidecar = torch.load(str(path) + ".optim", map_location="cpu", weights_only=False)
    assert set(sidecar) == {"m", "v", "step"}


def test_command_line_flag(shards, tmp_path):
    """train.py ... --ema-decay 0.9 in a fresh process: exits 0 and says that it averages; without the flag it does not say so"""
    env = {k: v for k, v in os.environ.items() if not k.startswith(("BL_", "BUGLAB_"))}
    script = os.path.join(PKG, "buglab", "models", "train.py")
    for flag, expected in ((["--ema-decay", "0.9"], True), ([], False)):
        out = tmp_path / f"cli{int(expected)}.pkl.gz"
        r = subprocess.run([sys.executable, script, "gnn-mlp", str(shards / "train"), str(shards / "valid"), str(out), "--max-num-epochs", "1",
                            "--minibatch-size", "16", "--quiet", "--sequential", "--model-spec", '{"hidden_state_size": 64, "num_layers": 4}']
                           + flag, capture_output=True, text=True, timeout=300, env=env)
        log = r.stdout + r.stderr
        assert r.returncode == 0, log[-3000:]
        assert out.exists()
        assert ("Weight averaging" in log) == expected, log[-3000:]
        sidecar = torch.load(str(out) + ".optim", map_location="cpu", weights_only=False)
        assert ("ema" in sidecar) == expected

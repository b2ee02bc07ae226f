"""CPU: weight averaging on the host side -- the decay schedule and the fp64 twin (buglab.runtime._averaging), FlatAdam's
bookkeeping (enable_averaging, the four load_state_dict combinations, the update index across an idle data-parallel step),
the command lines and the declarations of the three entry points.  No GPU: every device call here must refuse."""
import logging
import os
import re

import numpy as np
import pytest
import torch

from tests.conftest import ROOT

HEADER = os.path.join(ROOT, "include", "buglab_hip.h")


def _params(seed=0):
    g = torch.Generator().manual_seed(seed)
    return [torch.nn.Parameter(torch.randn(5, 3, generator=g)), torch.nn.Parameter(torch.randn(7, generator=g))]


# ---- the schedule and the twin --------------------------------------------------------------------------------------------
def test_ema_decay_at_first_values_by_hand():
    from buglab.runtime._averaging import ema_decay_at

    assert ema_decay_at(1, 0.999) == 2.0 / 11.0
    assert ema_decay_at(2, 0.999) == 3.0 / 12.0
    assert ema_decay_at(3, 0.999) == 4.0 / 13.0
    assert ema_decay_at(1, 0.1) == 0.1  # a decay below the warm-up value holds from the first update
    with pytest.raises(ValueError):
        ema_decay_at(0, 0.9)


def test_ema_decay_at_is_monotone_reaches_the_decay_and_stays():
    from buglab.runtime._averaging import ema_decay_at

    decay = 0.9
    d = [ema_decay_at(k, decay) for k in range(1, 400)]
    assert all(a <= b for a, b in zip(d, d[1:]))
    # (1 + k) / (10 + k) >= 0.9  <=>  k >= 80
    assert d[78] < decay and d[79] == decay and all(x == decay for x in d[79:])
    assert ema_decay_at(10 ** 9, 0.9999) == 0.9999


def test_one_minus_decay_is_rounded_to_fp32_once():
    from buglab.runtime._averaging import ema_decay_at, one_minus_decay_f32

    for k in (1, 2, 7, 100):
        omd = one_minus_decay_f32(k, 0.999)
        assert omd == float(np.float32(1.0 - ema_decay_at(k, 0.999))) and float(np.float32(omd)) == omd
    assert 0.0 < one_minus_decay_f32(10 ** 6, 0.999) <= 1.0


def test_ema_update_twin():
    from buglab.runtime._averaging import ema_update_twin

    rng = np.random.default_rng(0)
    ema, p = rng.standard_normal(33).astype(np.float32), rng.standard_normal(33).astype(np.float32)
    out = ema_update_twin(ema, p, 1.0)
    assert out.dtype == np.float64 and np.array_equal(out, p.astype(np.float64))  # omd = 1: the average IS the new value
    assert np.array_equal(ema_update_twin(p, p, 0.3), p.astype(np.float64))         # ema == p_new is a fixed point
    assert np.array_equal(ema_update_twin(ema, p, 0.25), ema.astype(np.float64) + 0.25 * (p.astype(np.float64) - ema.astype(np.float64)))


# ---- FlatAdam ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bad", [0, 0.0, 1, 1.0, -0.5, 1.5, float("nan")])
def test_enable_averaging_rejects_decays_outside_the_open_interval(bad):
    from buglab.runtime.optim import FlatAdam

    opt = FlatAdam(_params())
    with pytest.raises(ValueError):
        opt.enable_averaging(bad)
    assert opt.ema is None
    if bad != 0:  # 0 is the constructor's "off"
        with pytest.raises(ValueError):
            FlatAdam(_params(), ema_decay=bad)


def test_enable_averaging_allocates_a_copy_and_state_dict_carries_it():
    from buglab.runtime.optim import FlatAdam

    plain = FlatAdam(_params())
    assert plain.ema is None and set(plain.state_dict()) == {"m", "v", "step"}
    with plain.averaged_parameters():  # a no-op context without averaging
        pass

    for opt in (FlatAdam(_params(), ema_decay=0.99), FlatAdam(_params())):
        if opt.ema is None:
            opt.step_count = 5
            opt.enable_averaging(0.99)
            assert opt.ema_start_step == 5
        else:
            assert opt.ema_start_step == 0
        assert opt.ema.shape == opt.flat_param.shape and opt.ema.dtype == torch.float32
        assert opt.ema.data_ptr() != opt.flat_param.data_ptr() and torch.equal(opt.ema, opt.flat_param)
        sd = opt.state_dict()
        assert set(sd) == {"m", "v", "step", "param", "ema", "ema_decay", "ema_start_step"}
        assert sd["param"] is opt.flat_param and sd["ema"] is opt.ema and sd["ema_decay"] == 0.99


def _state(opt, averaged: bool, step=11, start=4):
    g = torch.Generator().manual_seed(7)
    sd = {"m": torch.randn(opt.numel, generator=g), "v": torch.rand(opt.numel, generator=g), "step": step}
    if averaged:
        sd.update(param=torch.randn(opt.numel, generator=g), ema=torch.randn(opt.numel, generator=g), ema_decay=0.9, ema_start_step=start)
    return sd


def test_load_state_dict_averaging_on_keys_present():
    from buglab.runtime.optim import FlatAdam

    opt = FlatAdam(_params(), ema_decay=0.9)
    sd = _state(opt, True)
    opt.load_state_dict(sd)
    assert torch.equal(opt.flat_param, sd["param"]) and torch.equal(opt.ema, sd["ema"])
    assert torch.equal(opt.m, sd["m"]) and torch.equal(opt.v, sd["v"])
    assert opt.step_count == 11 and opt.ema_start_step == 4 and opt.step_count - opt.ema_start_step == 7
    assert torch.equal(opt.params[0].data.flatten(), sd["param"][:15])  # the views still look into flat_param


def test_load_state_dict_averaging_on_keys_absent(caplog):
    from buglab.runtime.optim import FlatAdam

    opt = FlatAdam(_params(), ema_decay=0.9)
    opt.ema.fill_(123.0)
    before = opt.flat_param.clone()
    with caplog.at_level(logging.INFO, logger="buglab.runtime.optim"):
        opt.load_state_dict(_state(opt, False))
    assert torch.equal(opt.flat_param, before) and torch.equal(opt.ema, before)
    assert opt.step_count == 11 and opt.step_count - opt.ema_start_step == 0
    assert len([r for r in caplog.records if "average" in r.getMessage()]) == 1


def test_load_state_dict_averaging_off_keys_present(caplog):
    from buglab.runtime.optim import FlatAdam

    opt = FlatAdam(_params())
    before = opt.flat_param.clone()
    sd = _state(opt, True)
    with caplog.at_level(logging.INFO, logger="buglab.runtime.optim"):
        opt.load_state_dict(sd)
    assert opt.ema is None and torch.equal(opt.flat_param, before)  # what the checkpoint holds (the average) stays
    assert torch.equal(opt.m, sd["m"]) and torch.equal(opt.v, sd["v"]) and opt.step_count == 11
    assert len([r for r in caplog.records if "average" in r.getMessage()]) == 1


def test_load_state_dict_averaging_off_keys_absent(caplog):
    from buglab.runtime.optim import FlatAdam

    opt = FlatAdam(_params())
    before = opt.flat_param.clone()
    sd = _state(opt, False)
    with caplog.at_level(logging.INFO, logger="buglab.runtime.optim"):
        opt.load_state_dict(sd)
    assert opt.ema is None and torch.equal(opt.flat_param, before) and torch.equal(opt.m, sd["m"]) and opt.step_count == 11
    assert not caplog.records


def test_update_index_follows_the_step_counter_across_an_idle_data_parallel_step():
    """The idle step `previous_step_was_idle` takes back from step_count is taken back from k = step_count - start as well;
    the one_minus_decay handed to the kernel is that of k."""
    from buglab.runtime._averaging import one_minus_decay_f32
    from buglab.runtime.optim import FlatAdam

    class CpuFlatAdam(FlatAdam):
        def _apply_update_data_parallel(self):
            self.seen.append((self.step_count - self.ema_start_step, self._ema_one_minus_decay(), float(self.tail[0])))

    opt = CpuFlatAdam(_params())
    opt.seen = []
    opt.step_count = 3
    opt.enable_averaging(0.99)
    k = lambda: opt.step_count - opt.ema_start_step
    assert k() == 0
    opt.zero_grad()
    opt.step_data_parallel(4)
    assert k() == 1 and not opt.previous_step_was_idle() and k() == 1
    before = k()
    opt.zero_grad()
    opt.step_data_parallel(0)  # nobody had a minibatch: the kernel leaves everything untouched
    assert k() == before + 1
    assert opt.previous_step_was_idle() and k() == before
    assert opt.previous_step_was_idle() and k() == before  # taken back once
    opt.zero_grad()
    opt.step_data_parallel(2)
    assert [(i, b) for i, _, b in opt.seen] == [(1, 4.0), (2, 0.0), (2, 2.0)]  # the next real update is the 2nd, not the 3rd
    assert [o for _, o, _ in opt.seen] == [one_minus_decay_f32(1, 0.99), one_minus_decay_f32(2, 0.99), one_minus_decay_f32(2, 0.99)]


def test_device_paths_refuse_cpu_tensors():
    from buglab.models import hip_ops
    from buglab.runtime.optim import FlatAdam

    t = [torch.zeros(8) for _ in range(5)]
    with pytest.raises(hip_ops.HipOpsUnavailable):
        hip_ops.adam_clip_step_ema(*t, torch.zeros(1), one_minus_decay=0.5)
    with pytest.raises(hip_ops.HipOpsUnavailable):
        hip_ops.adam_clip_step_dp_ema(*t, torch.zeros(1), torch.ones(1), one_minus_decay=0.5)
    with pytest.raises(hip_ops.HipOpsUnavailable):
        hip_ops.swap_buffers(t[0], t[1])
    opt = FlatAdam(_params(), ema_decay=0.9)
    with pytest.raises(hip_ops.HipOpsUnavailable):
        opt.step()
    with pytest.raises(hip_ops.HipOpsUnavailable):
        with opt.averaged_parameters():
            pass
    assert not opt._averaged_in_place


# ---- interfaces ------------------------------------------------------------------------------------------------------------------
def test_command_lines_parse_ema_decay():
    from buglab.models import train, traingreat

    args = train.parse_args(["gnn-mlp", "tr", "va", "m.pkl.gz", "--ema-decay", "0.999"])
    assert float(args["--ema-decay"]) == 0.999
    assert float(train.parse_args(["gnn-mlp", "tr", "va", "m.pkl.gz"])["--ema-decay"]) == 0.0
    args = traingreat.parse_args(["tr", "va", "m.pkl.gz", "--ema-decay=0.99"])
    assert float(args["--ema-decay"]) == 0.99
    assert float(traingreat.parse_args(["tr", "va", "m.pkl.gz"])["--ema-decay"]) == 0.0
    assert "--ema-decay=<d>" in train.__doc__ and "--ema-decay=<d>" in traingreat.__doc__


def test_optimizer_factory_takes_ema_decay():
    from buglab.models.utils import optimizer

    assert optimizer(_params()).ema is None
    opt = optimizer(_params(), 1e-4, ema_decay=0.9)
    assert opt.ema is not None and opt.ema_decay == 0.9


@pytest.mark.parametrize("bad", [1.5, 0.0, 1.0, -1.0, float("nan")])
def test_trainer_rejects_a_bad_decay(tmp_path, bad):
    from buglab.runtime.trainer import ModelTrainer

    with pytest.raises(ValueError):
        ModelTrainer(object(), tmp_path / "m.pkl.gz", ema_decay=bad)
    assert ModelTrainer(object(), tmp_path / "m.pkl.gz")._ema_decay is None
    assert ModelTrainer(object(), tmp_path / "m.pkl.gz", ema_decay=0.5)._ema_decay == 0.5


def test_entry_points_are_declared_in_the_header():
    """(tests/test_cabi.py then checks that the library exports them and that the ctypes table lists them)"""
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    for name in ("bl_adam_clip_step_ema", "bl_adam_clip_step_dp_ema", "bl_swap_f32"):
        assert re.search(rf"\bint {name}\s*\(", src), name
    from buglab.models import hip_ops

    assert {"bl_adam_clip_step_ema", "bl_adam_clip_step_dp_ema", "bl_swap_f32"} <= set(hip_ops.EXPORTED_SYMBOLS)
    assert all(hasattr(hip_ops, n) for n in ("adam_clip_step_ema", "adam_clip_step_dp_ema", "swap_buffers"))


def test_argument_errors_come_before_any_device_call():
    """null / overlapping / out-of-range arguments: BL_EINVAL and a message, on a machine without a GPU"""
    import ctypes

    from buglab.models import hip_ops

    lib = hip_ops.load_library()
    buf = (ctypes.c_float * 64)()
    base = ctypes.addressof(buf)
    at = lambda i: ctypes.c_void_p(base + 4 * i)
    # (param, grad, m, v, ema, n, sqnorm, prescale | batch_total, clip, lr, beta1, beta2, eps, step, omd, stream)
    ok_tail = (0.0, 1e-4, 0.9, 0.999, 1e-8, 1)
    assert lib.bl_adam_clip_step_ema(at(0), at(8), at(16), at(24), None, 8, None, 1.0, *ok_tail, 0.5, None) != 0
    assert b"null" in lib.bl_last_error()
    assert lib.bl_adam_clip_step_ema(at(0), at(8), at(16), at(24), at(4), 8, None, 1.0, *ok_tail, 0.5, None) != 0
    assert b"overlap" in lib.bl_last_error()
    for omd in (0.0, -0.1, 1.5, float("nan")):
        assert lib.bl_adam_clip_step_ema(at(0), at(8), at(16), at(24), at(32), 8, None, 1.0, *ok_tail, omd, None) != 0
        assert b"ema_one_minus_decay" in lib.bl_last_error()
        assert lib.bl_adam_clip_step_dp_ema(at(0), at(8), at(16), at(24), at(32), 8, None, at(40), *ok_tail, omd, None) != 0
        assert b"ema_one_minus_decay" in lib.bl_last_error()
    assert lib.bl_adam_clip_step_dp_ema(at(0), at(8), at(16), at(24), at(7), 8, None, at(40), *ok_tail, 0.5, None) != 0
    assert b"overlap" in lib.bl_last_error()
    assert lib.bl_adam_clip_step_dp_ema(at(0), at(8), at(16), at(24), at(32), 8, None, None, *ok_tail, 0.5, None) != 0
    assert lib.bl_adam_clip_step_ema(at(0), at(8), at(16), at(24), at(32), 8, None, 1.0, 0.5, 1e-4, 0.9, 0.999, 1e-8, 1, 0.5, None) != 0
    assert b"grad_sqnorm" in lib.bl_last_error()  # clipping without a norm
    assert lib.bl_swap_f32(at(0), at(4), 8, None) != 0 and b"overlap" in lib.bl_last_error()
    assert lib.bl_swap_f32(at(4), at(0), 5, None) != 0 and b"overlap" in lib.bl_last_error()
    assert lib.bl_swap_f32(None, at(0), 4, None) != 0
    assert lib.bl_swap_f32(ctypes.c_void_p(base + 2), at(8), 4, None) != 0 and b"aligned" in lib.bl_last_error()
    assert lib.bl_swap_f32(at(0), at(4), 0, None) == 0  # n == 0: nothing to do, nothing to refuse
    assert lib.bl_swap_f32(None, None, 0, None) == 0

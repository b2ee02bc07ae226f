"""GPU: the ORDER of the work a training step spreads over its streams (step / caller's stream, side stream of the weight-gradient
GEMMs, the trainer's upload stream), one test per cross-stream edge (E1 .. E11, DESIGN.md "Stream ordering").

The arithmetic of the kernels is covered against fp64 elsewhere; a missing wait passes all of that, because at test shapes the other
stream has always finished by the time anybody looks.  Here one stream is STALLED (tests/stream_stall.py: a bounded busy kernel) right
before the call under test, so that a consumer that does not wait for it runs first, and every block the allocator considers free is
filled with NaN first, so that what it then reads is not a plausible number.  A test only counts if the stall was still running when
the host call returned (asserted; the stall is 10 x the call's unstalled host time, 50 ms at least, doubled once, 1 s at most).

Reference of every gradient comparison: the same module state (one state_dict), minibatch and dropout seed with
`hip_ops.USE_SIDE_STREAM = False` and no stall -- one stream, no order to get wrong.  Only quantities LINEAR in the gradient are
compared (gradients, Adam's first moment, the squared norm), never parameters after Adam (lr * g / (|g| + eps) flips sign on
last-bit differences of near-zero entries).  Bound: the project's parity bound, |d| <= 1e-4 * max|g_ref| + 1e-6 per tensor
(BASELINE.json, tests/test_hip_parity.py) -- x (1 - beta1) x clip scale for the first moment, 1e-4 relative for the squared norm.  A
missed wait drops a whole GEMM or lets NaN in (error ~ max|g_ref|); the order of the fp32 atomics moves ~1e-6 of it.  Integer data
(E8 - E10) and the zeroed buffer (E6 b) are compared exactly.

Every test prints its worst |d| / bound and the realised stall (HIP events).  Measured on the MI355X (4 hardware queues per process):
control: the clone overtakes the stall in both directions (reads 0; stalls 49.9 / 50.0 ms realised for 50 requested).  Every call
under test returned after 0.7 - 2.9 ms of host time (use_step_stream: 0.1 ms once the stream exists, 7 ms when it creates it), so
every stall was the 50 ms minimum and was still running at return; realised 50 - 51 ms.  Worst |d| / bound over several runs:
0.003 - 0.006 for the gnn-mlp gradient tests (E1 - E4, E6, E7), 0.001 - 0.002 for ggnn (E4) and seq-great (E5), 0 exactly for E6
zero_grad; E8 - E11 exact.  Poisoning alone (no stall) moved nothing: no read-before-write of a workspace.  Nothing was found open.
With one wait deleted at a time (scratch builds) the tests of its row failed with |d| ~ max|g_ref| or NaN; the one exception is
`fork2` at its early place (DESIGN.md "Stream ordering").

The gnn-mlp cases have 4 layers, not fewer: the stack is built in blocks of [3 x (H, H, H), concat, (2H, 2H, H)] and refuses anything
else.  ensemble/wrapper.py's staging upload is not driven (E10): it needs the member layouts of trained models.
"""
import copy
import tempfile
import time
from pathlib import Path

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import buglab_oracle as O
from tests import helpers as Hh
from tests import stream_stall as S

SEED = 11  # dropout seed of every gnn run
RTOL, ATOL = 1e-4, 1e-6  # the project's gradient parity bound (tests/test_hip_parity.py)


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from buglab.models import hip_ops

    hip_ops.load_library()
    torch.cuda.synchronize()
    torch.cuda.empty_cache()  # (what earlier test modules left cached would all be poisoned, again and again)


@pytest.fixture(autouse=True)
def _leave_nothing_behind(_gpu):
    """Nothing is left stalled and nothing is left changed: switches, message GEMM split, the thread's current stream."""
    from buglab.models import hip_ops

    side, fused, mode, stream = hip_ops.USE_SIDE_STREAM, hip_ops.FUSED_LAYER, hip_ops.msg_gemm_mode(), torch.cuda.current_stream()
    try:
        yield
    finally:
        torch.cuda.synchronize()
        hip_ops.USE_SIDE_STREAM, hip_ops.FUSED_LAYER = side, fused
        hip_ops.set_msg_gemm_mode(mode)
        torch.cuda.set_stream(stream)
        hip_ops.join_side_stream()
        torch.cuda.synchronize()


def _main():
    return torch.cuda.current_stream()


def _side():
    from buglab.models.hip_ops import _streams

    st = _streams.side_stream_for_current_device()
    assert st is not None, "the side stream is switched off"
    return st


def _poison():
    del_me = S.poison_free_blocks()
    del del_me
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------------------------------------
# the tools themselves
def test_a_stall_opens_a_window():
    """Power control: work on one of the library's two streams that does NOT wait for the other, stalled one overtakes it.  x is zero,
    `x.fill_(1)` is queued behind a stall, a clone on the other stream without a wait reads 0.  Both directions.  Reads only memory this
    test owns.  A clone of 1 means the two streams are serialised here (they share a hardware queue): no other test of this file would
    prove anything then."""
    main, side = _main(), _side()
    assert main.cuda_stream != side.cuda_stream
    for name, stalled, other in (("current stream stalled", main, side), ("side stream stalled", side, main)):
        with torch.cuda.stream(stalled):
            x = torch.zeros(4096, device="cuda")
        torch.cuda.synchronize()
        try:
            ev = S.stall(stalled, S.MIN_STALL_MS)
            with torch.cuda.stream(stalled):
                x.fill_(1)
            with torch.cuda.stream(other):
                y = x.clone()
            assert not ev.query(), f"{name}: the stall was over before the racing clone was queued"
        finally:
            torch.cuda.synchronize()
        print(f"control, {name}: clone read {float(y.max()):.0f} (0 = overtook the stall), stall {S.realised_ms(ev):.1f} ms")
        assert float(x.min()) == 1.0
        assert float(y.max()) == 0.0, (f"{name}: a clone on the other stream with no wait saw the value queued BEHIND the stall -- the two streams "
                                       "are serialised on this machine (hardware-queue sharing); no test of this file proves anything here")
        assert 0.2 * S.MIN_STALL_MS <= S.realised_ms(ev) <= 1.5 * S.MAX_STALL_MS, S.realised_ms(ev)  # (calibration: a stall is bounded)


def test_poison_reaches_a_block_that_was_just_freed():
    scratch = torch.empty(3 * 1024 * 1024 + 512, dtype=torch.uint8, device="cuda")
    small = torch.empty(1000, dtype=torch.float32, device="cuda")
    p_big, p_small = scratch.data_ptr(), small.data_ptr()
    del scratch, small
    held = S.poison_free_blocks()
    try:
        assert S.holds(held, p_big) and S.holds(held, p_small)
        assert all(bool((t == 0xFF).all()) for t in held[:8])
    finally:
        torch.cuda.synchronize()
    del held
    again = torch.empty(1000, dtype=torch.float32, device="cuda")  # the re-cached block: NaN until somebody writes it
    if again.data_ptr() == p_small:
        assert bool(torch.isnan(again).all())


# ------------------------------------------------------------------------------------------------------------------------------
# cases, references, comparison
_GNN_CASES = {
    # (4 layers: the smallest stack gnn-mlp can be built with -- one block [3 x (H, H, H), concat, (2H, 2H, H)])
    "h128": dict(B=3, n=150, E=800, T=4, H=128, layers=4, C=8, dropout=0.1),   # fused layer, early fork (Dout < 256)
    "h256": dict(B=2, n=120, E=600, T=3, H=256, layers=4, dropout=0.1),        # fused layer, late fork (Dout >= 256)
    "ggnn": dict(B=2, n=60, E=300, T=3, H=64, layers=4, model="ggnn", dropout=0.1),
}


class _GnnCase:
    def __init__(self, name):
        from buglab.data.collate import to_device

        self.name = name
        self.cfg, _, mb_np = Hh.make_case(**_GNN_CASES[name])
        self.mb = to_device(mb_np, "cuda")
        self.num_graphs = int(mb_np["graph_data"]["num_graphs"])
        self.state = {k: v.clone() for k, v in Hh.build_module_like(self.cfg, O.init_params(self.cfg, seed=0)).state_dict().items()}
        torch.cuda.synchronize()

    def module(self):
        m = Hh.build_module_like(self.cfg)
        m.load_state_dict(self.state)
        return m.train()

    def loss(self, m):
        return m(**self.mb, dropout_seed=SEED)


class _SeqGreatCase:
    """seq-great through the registry as in tests/test_seq_great_gpu.py: hidden 64, 2 heads (dk = 32), 2 layers."""

    def __init__(self):
        from buglab.data.collate import to_device
        from buglab.data.synthetic import make_buglab_seq_dataset
        from buglab.models.modelregistry import load_model

        self.name = "seq-great"
        data = make_buglab_seq_dataset(6, seed=5)
        self.model = load_model({"modelName": "seq-great", "hidden_state_size": 64, "num_layers": 2, "num_heads": 2, "intermediate_dimension_size": 96,
                                 "dropout_rate": 0.0}, Path(tempfile.gettempdir()) / "_bl_stream_order.pkl.gz")[0]
        self.model.compute_metadata(copy.deepcopy(data))
        samples = [self.model.tensorize(copy.deepcopy(d)) for d in data]
        assert all(s is not None for s in samples)
        mb_np = self.model.collate_minibatch({"samples": samples})
        self.shape = (int(mb_np["graph_data"]["seq_batch"]), int(mb_np["graph_data"]["seq_len"]))
        self.mb = to_device(mb_np, "cuda")
        torch.manual_seed(0)
        self.state = {k: v.clone() for k, v in self.model.build_neural_module().cuda().state_dict().items()}
        torch.cuda.synchronize()

    def module(self):
        m = self.model.build_neural_module().cuda()
        m.load_state_dict(self.state)
        return m.train()

    def loss(self, m):
        return m(**self.mb)


_cases, _references = {}, {}


def _case(name):
    if name not in _cases:
        _cases[name] = _SeqGreatCase() if name == "seq-great" else _GnnCase(name)
    return _cases[name]


def _grads(module):
    return {k: (p.grad.detach().clone() if p.grad is not None else torch.zeros_like(p)) for k, p in module.named_parameters()}


def _reference(name, fused=True, mode="f16x3"):
    """Gradients of the case on ONE stream (computed once per (case, layer form, message GEMM split), never changed)."""
    from buglab.models import hip_ops

    key = (name, fused, mode)
    if key not in _references:
        case = _case(name)
        prev = hip_ops.USE_SIDE_STREAM, hip_ops.FUSED_LAYER, hip_ops.set_msg_gemm_mode(mode)
        hip_ops.USE_SIDE_STREAM, hip_ops.FUSED_LAYER = False, fused
        try:
            m = case.module()
            case.loss(m).backward()
            torch.cuda.synchronize()
            _references[key] = _grads(m)
        finally:
            hip_ops.USE_SIDE_STREAM, hip_ops.FUSED_LAYER = prev[:2]
            hip_ops.set_msg_gemm_mode(prev[2])
    return _references[key]


def _worst_ratio(got, ref, what, scale=1.0):
    """max over tensors of |got - ref| / (scale * (RTOL * max|ref| + ATOL)); asserts it is <= 1 (a NaN anywhere fails)."""
    worst = 0.0
    for k, r in ref.items():
        bound = scale * (RTOL * float(r.abs().max()) + ATOL)
        d = float((got[k].double() - r.double()).abs().max()) if r.numel() else 0.0
        assert d <= bound, f"{what}: {k}: |d| = {d:.3e} > {bound:.3e} (max|g_ref| = {float(r.abs().max()):.3e})"
        worst = max(worst, d / bound)
    return worst


def _bind(module, how):
    """all: every .grad bound to a zeroed buffer and opted in to direct accumulation (what FlatAdam does); alternate: every other
    parameter (tests/test_hip_parity.py::_run_hip); none: plain parameters without a .grad."""
    for i, p in enumerate(module.parameters()):
        if how == "all" or (how == "alternate" and i % 2 == 0):
            if p.grad is None:
                p.grad = torch.zeros_like(p)
            else:
                p.grad.zero_()
            p._bl_direct_grad = True
        else:
            p.grad = None
            p._bl_direct_grad = False


def _backward_under_stall(case, bind, which, fused=True, mode="f16x3", after=None, expect_free_running=None, host_s=None):
    """loss.backward() of `case` with the stream `which()` stalled right before it, every free block poisoned first.
    after(module) runs right after backward() returned (before any join); if it returns gradients, those are compared instead of
    the ones read after the join.  The unstalled (poison-only) run that sizes the stall is compared with the reference as well.
    -> (StalledRun with value = the gradients compared, worst ratio)."""
    from buglab.models import hip_ops
    from buglab.models.hip_ops import _streams

    ref = _reference(case.name, fused, mode)
    hip_ops.USE_SIDE_STREAM, hip_ops.FUSED_LAYER = True, fused
    hip_ops.set_msg_gemm_mode(mode)
    module = case.module()

    def prepare():
        hip_ops.join_side_stream()
        torch.cuda.synchronize()
        _bind(module, bind)
        loss = case.loss(module)
        torch.cuda.synchronize()
        _poison()
        return loss

    def finish(loss, stalled):
        try:
            free_running = _streams._free_running
            read_early = after(module) if after is not None else None
            hip_ops.join_side_stream()
        finally:
            torch.cuda.synchronize()
        if expect_free_running is not None:
            assert free_running == expect_free_running, f"free-running side stream: {free_running}, the test is about {expect_free_running}"
        return read_early if read_early is not None else _grads(module)

    run, plain = S.run_stalled(which, prepare, lambda loss: loss.backward(), finish, unstalled_host_s=host_s)
    worst = _worst_ratio(run.value, ref, f"{case.name}, {which.__name__[1:]} stream stalled")
    if plain is not None:
        # poisoning alone (no stall) must not move anything either: that would be a read-before-write of a workspace
        worst = max(worst, _worst_ratio(plain, ref, f"{case.name}, poison only"))
    return run, worst


def _report(what, worst, *runs):
    print(f"{what}: worst |d| / bound = {worst:.3g}; " + ", ".join(f"stall {r.realised_ms:.0f} ms (call returned after {r.host_s * 1e3:.1f} ms)" for r in runs))


# ------------------------------------------------------------------------------------------------------------------------------
# E1 / E2: the side stream waits for the main stream inside bl_mp_layer_bwd
def test_e1_dense_weight_gradient_waits_for_the_main_chain():
    """fork1: the dense weight gradient reads g_z, which the first kernel of the call writes on the main stream."""
    run, worst = _backward_under_stall(_case("h128"), "all", _main, expect_free_running=True)
    _report("E1 h128 f16x3", worst, run)


@pytest.mark.parametrize("name,mode", [("h128", "f16x3"), ("h128", "bf16x6"), ("h256", "f16x3")])
def test_e2_routed_weight_gradient_waits_for_the_main_chain(name, mode):
    """fork2 at its early place (Dout < 256), its late place (Dout >= 256), and on the f16x3 path, whose GEMM also reads the
    device-side amax and the packed gradient operand written just before the fork."""
    from buglab.models import hip_ops

    hip_ops.set_msg_gemm_mode(mode)
    assert hip_ops.msg_gemm_mode() == mode
    run, worst = _backward_under_stall(_case(name), "all", _main, mode=mode, expect_free_running=True)
    _report(f"E2 {name} {mode}", worst, run)


# E3: parameters that did not opt in: the call itself joins the side stream
@pytest.mark.parametrize("bind", ["none", "alternate"])
@pytest.mark.parametrize("fused", [True, False], ids=["one-call", "kernel-by-kernel"])
def test_e3_backward_joins_the_side_stream_itself_when_parameters_did_not_opt_in(fused, bind):
    """`join_side = 1` (bl_mp_layer_bwd) / `_on_side_stream.join()`: gradients handed back through autograd are complete in the
    main stream's order when backward() returns -- read there WITHOUT join_side_stream(), with the side stream stalled."""

    run, worst = _backward_under_stall(_case("h128"), bind, _side, fused=fused, after=_grads, expect_free_running=False)
    _report(f"E3 {'one-call' if fused else 'kernel-by-kernel'} {bind}", worst, run)


# E4: the kernel-by-kernel layers
@pytest.mark.parametrize("name", ["h128", "ggnn"])
def test_e4_kernel_by_kernel_layers(name):
    """_MpLayer (FUSED_LAYER off): side1 / side2 wait for the main stream when entered and are left running (detach); _GatedMpLayer:
    `with side:` entered twice, the second time it must wait for the gq the main stream computed in between; joined in the call."""
    case = _case(name)
    free = name == "h128"  # (the gated layer hands its gradients back through autograd: always joined)
    a, w1 = _backward_under_stall(case, "all", _main, fused=False, expect_free_running=free)
    b, w2 = _backward_under_stall(case, "all", _side, fused=False, expect_free_running=free, host_s=a.unstalled_host_s)
    _report(f"E4 {name}", max(w1, w2), a, b)


# E5: the one-call relational transformer layer
def test_e5_great_layer_forks_and_join():
    case = _case("seq-great")
    layers = [m for m in case.module().modules() if hasattr(m, "fused_call_ok")]
    assert len(layers) == 2 and all(l.fused_call_ok(*case.shape) for l in layers), "the one-call layer (great_layer_ok) is not taken"
    a, w1 = _backward_under_stall(case, "all", _main)
    b, w2 = _backward_under_stall(case, "all", _side, host_s=a.unstalled_host_s)
    _report("E5 seq-great", max(w1, w2), a, b)


# E7: what the free-running GEMMs read is held until the join
@pytest.mark.parametrize("fused", [True, False], ids=["one-call", "kernel-by-kernel"])
def test_e7_what_the_free_running_gemms_read_is_held_until_the_join(fused):
    """backward() has returned, its Python references are gone, the side stream has not started: every block the allocator would
    hand out now is overwritten (and kept) before the join.  `saved` / `ws` / the detached tensors must not be among them."""
    keep = []

    def overwrite_what_is_free(module):
        keep.append(S.poison_free_blocks())

    try:
        run, worst = _backward_under_stall(_case("h128"), "all", _side, fused=fused, after=overwrite_what_is_free, expect_free_running=True)
    finally:
        torch.cuda.synchronize()
        keep.clear()
    _report(f"E7 {'one-call' if fused else 'kernel-by-kernel'}", worst, run)


# ------------------------------------------------------------------------------------------------------------------------------
# E6: FlatAdam's consumers of free-running gradients
_ADAM = dict(lr=1e-3, clip_gradient_norm=0.5, num_warmup_steps=0)


def _consume(case, module, opt, consumer):
    """-> {flat_grad, m, sqnorm} after the consumer (device idle)."""
    if consumer == "step":
        opt.step()
    elif consumer == "zero_grad":
        opt.zero_grad()
    elif consumer == "step_data_parallel":
        opt.step_data_parallel(case.num_graphs)
    elif consumer == "two_backwards":
        case.loss(module).backward()
        opt.step()
    torch.cuda.synchronize()
    return {"flat_grad": opt._grad_and_tail.clone(), "m": opt.m.clone(), "sqnorm": opt.sqnorm.clone()}


def _adam_reference(consumer):
    from buglab.models import hip_ops
    from buglab.runtime.optim import FlatAdam

    key = ("adam", consumer)
    if key not in _references:
        case = _case("h128")
        prev = hip_ops.USE_SIDE_STREAM
        hip_ops.USE_SIDE_STREAM = False
        try:
            m = case.module()
            opt = FlatAdam(m.parameters(), **_ADAM)
            opt.zero_grad()
            case.loss(m).backward()
            _references[key] = _consume(case, m, opt, consumer)
        finally:
            hip_ops.USE_SIDE_STREAM = prev
    return _references[key]


@pytest.mark.parametrize("consumer", ["step", "zero_grad", "step_data_parallel", "two_backwards"])
def test_e6_flat_adam_consumers_wait_for_the_free_running_gradients(consumer):
    """FlatAdam binds every .grad, so the weight-gradient GEMMs of the fused layers are left running on the (stalled) side stream
    when backward() returns; each consumer must join them before it reads or clears the flat gradient buffer.
    step / step_data_parallel / two backwards + step: flat gradient, first moment and squared norm equal the one-stream run's;
    zero_grad: the buffer is EXACTLY zero afterwards (a late GEMM adding into the zeroed buffer leaves it non-zero)."""
    from buglab.models import hip_ops
    from buglab.models.hip_ops import _streams
    from buglab.runtime.optim import FlatAdam

    case = _case("h128")
    ref = _adam_reference(consumer)
    hip_ops.USE_SIDE_STREAM = True

    def prepare():
        hip_ops.join_side_stream()
        torch.cuda.synchronize()
        module = case.module()
        opt = FlatAdam(module.parameters(), **_ADAM)
        opt.zero_grad()
        loss = case.loss(module)
        torch.cuda.synchronize()
        _poison()
        return module, opt, loss

    def finish(state, stalled):
        module, opt, _ = state
        try:
            free_running = _streams._free_running
            out = _consume(case, module, opt, consumer)
        finally:
            torch.cuda.synchronize()
        assert free_running, "no weight-gradient GEMM was left running when backward() returned: this test would not test what it claims"
        out["spans"] = [(k, opt._span[id(p)][0], p.numel()) for k, p in module.named_parameters() if id(p) in opt._span]
        return out

    run, plain = S.run_stalled(_side, prepare, lambda state: state[2].backward(), finish)
    worst = 0.0
    for what, got in (("side stream stalled", run.value), ("poison only", plain)):
        if consumer == "zero_grad":
            assert int(torch.count_nonzero(got["flat_grad"])) == 0 and not bool(torch.isnan(got["flat_grad"]).any()), \
                f"{what}: the flat gradient buffer is not zero after zero_grad(): a weight-gradient GEMM added into it afterwards"
            continue
        # step_data_parallel scaled the buffer by the graph count (the kernel divides by the count it finds in the tail)
        count = float(case.num_graphs) if consumer == "step_data_parallel" else 1.0
        cut = lambda flat: {k: flat[o:o + size] for k, o, size in got["spans"]}
        g_ref = {k: v / count for k, v in cut(ref["flat_grad"]).items()}
        worst = max(worst, _worst_ratio({k: v / count for k, v in cut(got["flat_grad"]).items()}, g_ref, f"{what}: flat_grad"))
        # first step: m = (1 - beta1) * g * min(1, clip / (|g| + 1e-6))  (csrc/bl_head_ops.hip adam_clip_kernel)
        norm = float(ref["sqnorm"].sqrt()) / count
        m_scale = (1.0 - 0.9) * min(1.0, _ADAM["clip_gradient_norm"] / (norm + 1e-6))
        m_ref, m_got = cut(ref["m"]), cut(got["m"])
        for k, g in g_ref.items():
            bound = m_scale * (RTOL * float(g.abs().max()) + ATOL)
            d = float((m_got[k].double() - m_ref[k].double()).abs().max())
            assert d <= bound, f"{what}: m of {k}: |d| = {d:.3e} > {bound:.3e}"
            worst = max(worst, d / bound)
        sq, sq_ref = float(got["sqnorm"]), float(ref["sqnorm"])
        assert abs(sq - sq_ref) <= RTOL * sq_ref, f"{what}: squared gradient norm {sq:.9e} vs {sq_ref:.9e}"
        worst = max(worst, abs(sq - sq_ref) / (RTOL * sq_ref))
    _report(f"E6 {consumer}", worst, run)


# ------------------------------------------------------------------------------------------------------------------------------
# E8: use_step_stream
def test_e8_use_step_stream_waits_for_the_previous_current_stream(monkeypatch):
    """`x.fill_(1)` is queued behind a stall of the current stream; after `use_step_stream()` a clone on the (new) current stream
    reads 1.  The unstalled run that sizes the stall also creates the step stream; the stalled call re-selects it, and waits.  (On
    purpose: when the high-priority stream was CREATED while the busy kernel ran, the stall was over early in 3 of 13 runs on the
    MI355X -- its event had completed within the 7 ms the creation took.  Create streams before a stall, never during one.)"""
    from buglab.models import hip_ops

    monkeypatch.delenv("BUGLAB_STEP_STREAM_PRIORITY", raising=False)
    entry = torch.cuda.current_stream()  # (in a whole-suite run an earlier trainer test has left the step stream selected)
    old = torch.cuda.default_stream()

    def prepare():
        torch.cuda.set_stream(old)
        x = torch.zeros(4096, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        return [x]

    def call(state):
        state.append(hip_ops.use_step_stream())

    def finish(state, stalled):
        try:
            x, st = state
            assert st is not None and torch.cuda.current_stream() == st and st != old
            y = x.clone()  # on the step stream
        finally:
            torch.cuda.synchronize()
            torch.cuda.set_stream(old)
        return y

    try:
        run, plain = S.run_stalled(lambda: old, prepare, call, finish, behind=lambda state: state[0].fill_(1))
    finally:
        torch.cuda.synchronize()
        torch.cuda.set_stream(entry)
    assert bool((plain == 1).all())
    assert bool((run.value == 1).all()), "work queued on the previous current stream was not waited for"
    print(f"E8: stall {run.realised_ms:.0f} ms, use_step_stream returned after {run.host_s * 1e3:.2f} ms")


# ------------------------------------------------------------------------------------------------------------------------------
# E9: the trainer's upload stream hands a minibatch to the training stream
@pytest.fixture(scope="module")
def shard_dir(tmp_path_factory):
    """(built like tests/test_averaging_gpu.py::shards)"""
    from buglab.data.synthetic import make_buglab_dataset
    from buglab.utils.msgpackutils import save_msgpack_l_gz

    root = tmp_path_factory.mktemp("stream_order")
    data = make_buglab_dataset(64, seed=5)
    (root / "train").mkdir()
    save_msgpack_l_gz(data[:48], root / "train" / "a.msgpack.l.gz")
    return root, data[:48]


_E9_KEYS = ("msg_src", "msg_tgt", "tgt_ptr", "token_ids")


def test_e9_upload_stream_hands_minibatches_to_the_training_stream(shard_dir, monkeypatch):
    """`_iter_minibatches` with loader processes: `receive_packed` runs on the upload stream in a prefetch thread, the consumer's
    stream waits for `_upload_ready` and marks the blob as in use there (`record_stream`).  The upload stream is stalled in front of
    every upload: sums of a few int arrays taken on the consumer's stream must equal the host's.  Each minibatch is dropped right
    after use, with the consumer's stream held up, and NaN-filled tensors of the blob's size are allocated on the upload stream:
    without `record_stream` they would be the blob's block, rewritten while the sums have not run."""
    from buglab.models.modelregistry import load_model
    from buglab.runtime import shardloader
    from buglab.runtime.shardloader import ShardDataset
    from buglab.runtime.trainer import ModelTrainer

    root, points = shard_dir
    monkeypatch.setenv("BUGLAB_LOADER_WORKERS", "2")
    model = load_model({"modelName": "gnn-mlp", "hidden_state_size": 64}, root / "m.pkl.gz")[0]
    for x in copy.deepcopy(points):
        model.update_metadata_from(x)
    model.finalize_metadata()
    trainer = ModelTrainer(model, root / "m.pkl.gz", minibatch_size=16, clip_gradient_norm=0.5)
    trainer._use_multiprocessing = True
    ds = ShardDataset(str(root / "train"))
    device = torch.device("cuda", torch.cuda.current_device())
    original = shardloader.receive_packed
    log = []  # per minibatch: [stall event, still running when receive_packed returned, host sums]
    stall_ms = [0.0]

    def host_sums(item):
        from multiprocessing import shared_memory

        _, name, meta = item
        shm = shared_memory.SharedMemory(name=name)
        try:
            blob = np.ndarray((int(meta["total"]),), dtype=np.int32, buffer=shm.buf)
            return {k: int(blob[o:o + int(np.prod(shape, dtype=np.int64))].astype(np.int64).sum())
                    for where, k, shape, o in meta["layout"] if where == "gd" and k in _E9_KEYS}
        finally:
            shm.close()

    def stalled_receive(item, dev):
        sums = host_sums(item)
        ev = S.stall(torch.cuda.current_stream(), stall_ms[0]) if stall_ms[0] else None  # (the upload stream is current in this thread)
        mb = original(item, dev)
        log.append([ev, ev is not None and not ev.query(), sums])
        return mb

    monkeypatch.setattr(shardloader, "receive_packed", stalled_receive)

    def consume(stalled):
        del log[:]
        results, junk, consumed_early = [], [], 0
        try:
            for i, mb in enumerate(trainer._iter_minibatches(ds, device, True)):
                if i:  # the previous minibatch is gone by now: whatever the allocator considers free is overwritten, on its own stream
                    junk.append(S.poison_free_blocks())
                ev = log[i][0]
                if stalled:
                    consumed_early += int(not ev.query())
                    S.stall(torch.cuda.current_stream(), S.MIN_STALL_MS)  # the consumer is busy: its reads of the blob come late
                gd = mb["graph_data"]
                results.append({k: gd[k].sum(dtype=torch.int64) for k in _E9_KEYS})
                n = gd["_blob"].numel()
                del gd, mb
                with torch.cuda.stream(trainer._upload_stream):
                    junk.append(torch.full((n,), float("nan"), device=device))
            junk.append(S.poison_free_blocks())
        finally:
            torch.cuda.synchronize()
        return [{k: int(v) for k, v in r.items()} for r in results], consumed_early

    plain, _ = consume(False)  # unstalled: the host-side duration of one upload
    assert len(plain) >= 2 and plain == [row[2] for row in log]
    per_upload_s = trainer.last_input_timing["upload_s"] / max(1, trainer.last_input_timing["minibatches"])
    stall_ms[0] = max(S.MIN_STALL_MS, 10.0 * 1e3 * per_upload_s)
    for attempt in range(2):
        got, consumed_early = consume(True)
        if all(row[1] for row in log):
            break
        stall_ms[0] *= 2.0
    assert all(row[1] for row in log), f"a stall of {stall_ms[0] / 2:.0f} ms on the upload stream was over when receive_packed returned"
    assert consumed_early >= 1, "no minibatch reached the consumer while its upload was still behind the stall"
    assert len(got) == len(plain) and got == [row[2] for row in log], (got, [row[2] for row in log])
    print(f"E9: {len(got)} minibatches, {consumed_early} consumed while their upload was stalled; stalls "
          + ", ".join(f"{S.realised_ms(row[0]):.0f} ms" for row in log))


# ------------------------------------------------------------------------------------------------------------------------------
# E10: pinned staging buffers are dropped at return while their copy is still queued
def _same_bin_blobs(n, dtype=np.int32):
    rng = np.random.default_rng(3)
    return [rng.integers(1, 1 << 20, size=n).astype(dtype) for _ in range(3)]


def _upload_three(upload, blob_of):
    """Three uploads back to back behind a stall of the current stream.  -> [(device blob, host blob)] (device idle)."""

    def once(ms):
        try:
            ev = S.stall(torch.cuda.current_stream(), ms) if ms else None
            t0 = time.perf_counter()
            ups = [upload(k) for k in range(3)]
            host_s = time.perf_counter() - t0
            running = ev is not None and not ev.query()
        finally:
            torch.cuda.synchronize()
        return ups, host_s, running, ev

    _, host_s, _, _ = once(0.0)
    ms = max(S.MIN_STALL_MS, 10.0 * 1e3 * host_s)
    ups, _, running, ev = once(ms)
    if not running:
        ups, _, running, ev = once(2.0 * ms)
    assert running, "the stall was over when the third upload returned"
    for k, up in enumerate(ups):
        dev_blob, host_blob = blob_of(up, k)
        assert torch.equal(dev_blob.cpu().reshape(-1), torch.from_numpy(host_blob).reshape(-1)), f"upload {k} does not hold its own data"
    return S.realised_ms(ev)


def test_e10_pinned_staging_is_not_reused_while_its_copy_is_queued():
    """`torch.empty(pin_memory=True)` -> `.to(non_blocking=True)` -> the staging buffer dies at return: the host allocator must not hand
    it to the next call (same size: same bin) before the copy has run.  collate.upload_packed and its siblings
    greatreimplementation.upload_great and controllers._batching.to_device_i32 (ensemble/wrapper.py `_finalize` needs member layouts
    of trained models: not driven here)."""
    from buglab.controllers._batching import to_device_i32
    from buglab.data import collate
    from buglab.models.greatreimplementation import _UPLOAD_ORDER, upload_great

    _, _, mb_np = Hh.make_case(B=3, n=150, E=800, T=4, H=128, layers=4, C=8)
    blob, meta = collate.pack_minibatch(mb_np)
    blobs = [blob, (blob + 7919).astype(np.int32), (blob[::-1] * 3 + 1).astype(np.int32)]
    ms1 = _upload_three(lambda k: collate.upload_packed(blobs[k], meta, "cuda"), lambda up, k: (up["graph_data"]["_blob"], blobs[k]))

    rows = _same_bin_blobs(3 * 4096)
    great = [{key: (r[i * 1024:(i + 1) * 1024] if key != "has_bug" else (r[:1024] % 2).astype(np.uint8)) for i, key in enumerate(_UPLOAD_ORDER)}
             for r in rows]
    ms2 = _upload_three(lambda k: upload_great(great[k], "cuda"),
                        lambda up, k: (torch.cat([up[key].reshape(-1) for key in _UPLOAD_ORDER[:-1]]),
                                       np.concatenate([great[k][key] for key in _UPLOAD_ORDER[:-1]])))

    parts = [[r[:5000], r[5000:5003], r[5003:]] for r in rows]
    ms3 = _upload_three(lambda k: to_device_i32(parts[k], "cuda"), lambda up, k: (torch.cat(up), rows[k]))
    print(f"E10: stalls {ms1:.0f} / {ms2:.0f} / {ms3:.0f} ms (upload_packed / upload_great / to_device_i32)")


# ------------------------------------------------------------------------------------------------------------------------------
# E11: the pinned tail of a data-parallel step is read only after its event
def test_e11_previous_step_was_idle_reads_the_tail_after_its_event():
    """The flag travels device -> pinned memory asynchronously; both pinned slots are first filled with the OPPOSITE answer, so a read
    that does not wait for the copy (still behind the stall) returns the wrong one."""
    from buglab.runtime.optim import FlatAdam

    p = torch.nn.Parameter(torch.zeros(64, device="cuda"))
    opt = FlatAdam([p], lr=1e-3, num_warmup_steps=0)

    def step(graphs):
        opt.zero_grad()
        if graphs:
            p.grad.fill_(0.01)
        opt.step_data_parallel(graphs)

    stalls = []
    for graphs, expect_idle in ((0, True), (3, False)):
        try:
            for _ in range(2):  # both pinned slots hold the other answer
                step(0 if graphs else 3)
                torch.cuda.synchronize()
                assert opt.previous_step_was_idle() == (not expect_idle)
            opt.zero_grad()
            if graphs:
                p.grad.fill_(0.01)
            torch.cuda.synchronize()
            ev = S.stall(torch.cuda.current_stream(), S.MIN_STALL_MS)
            opt.step_data_parallel(graphs)
            assert not ev.query(), "the stall was over when step_data_parallel returned"
            idle = opt.previous_step_was_idle()
        finally:
            torch.cuda.synchronize()
        assert idle == expect_idle, f"a step with {graphs} graphs was reported as {'idle' if idle else 'not idle'}"
        stalls.append(S.realised_ms(ev))
    print("E11: stalls " + ", ".join(f"{ms:.0f} ms" for ms in stalls))

"""The hip_ops package is a facade over its domain modules.  Host-only (no GPU, no library): pins what a split can break
without any A/B test noticing -- a switch assigned on the package that no longer reaches the code that reads it, state that
exists twice, and names callers use on the package."""
import ast
import importlib
import importlib.util
import os
import re
import types

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "neurips21-self-supervised-bug-detection-and-repair_amd")

# dir(hip_ops) of the commit before the split, without dunders, stdlib / typing / torch imports and sub-modules.
PARENT_SURFACE = (
    "ACT_GELU", "ACT_GELU_AGG", "ACT_NONE", "ACT_RELU", "ACT_SIGMOID", "ACT_TANH", "AGGREGATIONS", "BUG_LOSS_STATS", "BugLossIndex",
    "DEDUP_EMPTY_SLOT", "DEDUP_MAX_PERM", "DENSE_X6", "DGRAD_VEC", "Dropout", "ENSEMBLE_KINDS", "ENSEMBLE_MAX_MEMBERS",
    "EXPORTED_SYMBOLS", "FUSED_ATTENTION", "FUSED_GREAT_LAYER", "FUSED_LAYER", "FUSED_LOSS", "GEMM_MODE", "GRAD_READY_CALLBACK",
    "GraphIndex", "H3_ROW_SCALE", "H3_W_SCALE", "HipOpsUnavailable", "INFERENCE_MODE", "KernelTimer", "LIB_NAME", "LINEAR_X6",
    "LINEAR_X6_MIN_ROWS", "NO_DROPOUT", "POOLINGS", "REPORT_INDEX_FIELDS", "REPORT_MAX_SAMPLES", "RelEdges", "RowSource",
    "SELECTOR_MAX_K", "VARMISUSE_STATS", "WGRAD_X6", "WINNER_SINK", "_ACTS", "_AddLayerNorm", "_BugLoss", "_DropoutFn",
    "_EmbedSubtokenMax", "_FORWARDED", "_GatedMpLayer", "_GatherLinear", "_GatherRows", "_GreatLayer", "_GruScan", "_HipOpsModule",
    "_KIND", "_LocalizationScores", "_MSG_GEMM_MODES", "_MlpScore", "_MpLayer", "_MpLayerFeat", "_MpLayerFused", "_RelAttention",
    "_RowDot", "_SIGNATURES", "_SQNORM_SCRATCH", "_SegmentLogSoftmax", "_SegmentMaxPool", "_VarMisuseHead", "_WeightCopies",
    "_as_groups", "_bug_loss_desc", "_byte_mask", "_check", "_direct_grad_target", "_direct_small", "_f32", "_f64", "_grad_target",
    "_great_desc", "_group_ptr_cache", "_i32", "_i64", "_layer_desc", "_note_use", "_notify_backward_launched", "_on_side_stream",
    "_opted_in_for_direct_grad", "_p", "_packed_layer_weights", "_packed_message_weights", "_pending_uses", "_req", "_rows",
    "_rows_packed", "_stream", "_take_saved", "_timed", "_transposed_layer_weights", "_uniform_group_ptr", "_use_vector_dgrad",
    "_varmisuse_desc", "_varmisuse_workspace", "_weight_copies", "act_bwd", "act_bwd_packed", "adam_clip_step", "adam_clip_step_dp",
    "add_layernorm", "amax", "bl_bug_loss_t", "bl_dropout_t", "bl_great_layer_grads_t", "bl_great_layer_t", "bl_head_view_t",
    "bl_mp_layer_t", "bl_pack_job_t", "bl_packed_head_view_t", "bl_rows_packed_t", "bl_rows_t", "bl_varmisuse_head_t", "bl_x6_epi_t",
    "bug_loss", "dedup_lsh_insert_query", "dedup_minhash", "dedup_sha1_u32", "deterministic", "dropout_rows", "embed_subtoken_max",
    "ensemble_combine", "fused_layer_ok", "gated_mp_layer", "gather_linear", "gather_rows", "gemm_rows", "gemm_rows_h3",
    "gemm_rows_routed", "gemm_rows_x6", "gemm_wgrad", "gemm_wgrad_h3", "gemm_wgrad_routed", "gemm_wgrad_routed_x6", "gemm_wgrad_x6",
    "great_layer", "great_layer_ok", "gru_scan", "h3_saturation_events", "invalidate_weight_packs", "join_side_stream", "layernorm_bwd",
    "load_library", "localization_scores", "message_activation_code", "mlp_score", "mp_layer", "mp_layer_with_edge_features",
    "msg_gemm_mode", "node_update_bwd", "pack_bf16x3", "pack_f16x2", "pack_weights_h3", "pack_weights_x6", "pack_weights_x6w",
    "rel_attention", "report_order", "report_summarize", "routed_dgrad_nodes", "routed_dgrad_vec", "rowdot", "rows_x6w_ok",
    "scatter_add_rows", "score_targets", "segment_log_softmax", "segment_max", "segment_max_bwd", "segment_max_pool", "selector_sample",
    "set_deterministic", "set_fused_node_bwd", "set_grad_ready_callback", "set_msg_gemm_mode", "set_wgrad_kchunk_cap", "set_wgrad_tile",
    "side_stream_if_any", "sqnorm", "use_step_stream", "varmisuse_head", "x6_ok")
# Three names of that listing are gone on purpose, and must stay gone:
DROPPED = {
    "_name": "loop variable of the removed globals().pop loop",
    "_rows_packed_h": "folded into the one packed-rows helper, _rows_packed",
    "_weights_epoch": "an int: a copy on the package would go stale -- its one copy is weights._weights_epoch",
}


def _submodules(hip_ops):
    names = sorted(f[:-3] for f in os.listdir(os.path.dirname(hip_ops.__file__)) if f.endswith(".py") and f != "__init__.py")
    assert {"_cabi", "_switches", "_streams", "gemm", "weights", "graph"} <= set(names)
    return {n: importlib.import_module(f"{hip_ops.__name__}.{n}") for n in names}


def _forwarded_names():
    from buglab.models.hip_ops import _cabi, _switches

    switches = [n for n in vars(_switches) if n.isupper() and not n.startswith("_")]
    assert sorted(switches) == sorted(_switches.__all__) and len(switches) == 16
    return [(n, _switches) for n in switches] + [(n, _cabi) for n in ("CALL_COUNT", "_lib", "LIB_PATH")]


@pytest.mark.parametrize("name", [n for n, _ in _forwarded_names()])
def test_assignment_on_the_package_reaches_the_one_owner(name):
    from buglab.models import hip_ops

    owner = dict(_forwarded_names())[name]
    before = getattr(owner, name)
    try:
        a, b = object(), object()
        setattr(hip_ops, name, a)
        assert getattr(owner, name) is a and getattr(hip_ops, name) is a
        setattr(owner, name, b)
        assert getattr(hip_ops, name) is b
        assert name not in vars(hip_ops)
        for sub_name, sub in _submodules(hip_ops).items():
            if sub is not owner:
                assert name not in vars(sub), f"{sub_name} holds its own copy of {name}"
    finally:
        setattr(owner, name, before)
    assert getattr(hip_ops, name) is before


def test_every_name_of_the_parent_surface_resolves():
    from buglab.models import hip_ops

    missing = [n for n in PARENT_SURFACE if not hasattr(hip_ops, n)]
    assert not missing, missing
    for n in DROPPED:
        assert n not in PARENT_SURFACE and n not in vars(hip_ops), n
    # the NamedTuples are the package's: what was pickled as buglab.models.hip_ops.<Name> still loads
    for n in ("GraphIndex", "RelEdges", "BugLossIndex", "Dropout"):
        assert isinstance(getattr(hip_ops, n), type) and issubclass(getattr(hip_ops, n), tuple)


def _python_files():
    for top in ("bench.py", "__graft_entry__.py"):
        yield os.path.join(ROOT, top)
    for top in (os.path.join(PKG, "buglab"), os.path.join(ROOT, "tests"), os.path.join(ROOT, "tools")):
        for d, _, files in os.walk(top):
            for f in files:
                if f.endswith(".py"):
                    yield os.path.join(d, f)


def test_every_name_used_on_the_package_resolves():
    from buglab.models import hip_ops

    used = {}
    for path in _python_files():
        text = open(path, encoding="utf-8").read()
        found = re.findall(r"\bhip_ops\.([A-Za-z_]\w*)(?![\w*])", text)
        if re.search(r"\bhip_ops as ops\b", text):
            found += re.findall(r"\bops\.([A-Za-z_]\w*)(?![\w*])", text)
        for names in re.findall(r"from buglab\.models\.hip_ops import ([\w, ]+)", text):
            found += [n.split(" as ")[0].strip() for n in names.split(",") if n.strip()]
        for n in found:
            used.setdefault(n, os.path.relpath(path, ROOT))
    assert len(used) > 100  # (the scan found the call sites)
    bad = {n: where for n, where in used.items()
           if not hasattr(hip_ops, n) and importlib.util.find_spec(f"{hip_ops.__name__}.{n}") is None and n not in DROPPED}
    assert not bad, bad


def test_state_exists_once():
    import torch

    from buglab.models import hip_ops
    from buglab.models.hip_ops import weights

    W = torch.zeros(1)
    ent = {"version": W._version, "epoch": weights._weights_epoch}
    assert weights._weight_copies._fresh(ent, W)
    hip_ops.invalidate_weight_packs()
    assert not weights._weight_copies._fresh(ent, W) and weights._weights_epoch == ent["epoch"] + 1
    assert hip_ops._weight_copies is weights._weight_copies

    f = lambda params: None
    try:
        hip_ops.set_grad_ready_callback(f)
        assert hip_ops.GRAD_READY_CALLBACK is f
        hip_ops._note_use([W])
        assert hip_ops._pending_uses == {id(W): 1}
    finally:
        hip_ops.set_grad_ready_callback(None)
    assert hip_ops.GRAD_READY_CALLBACK is None and not hip_ops._pending_uses


def test_cabi_module_and_library_handle_do_not_collide():
    import ctypes

    import buglab.models.hip_ops._cabi as by_path
    from buglab.models import hip_ops
    from buglab.models.hip_ops import _cabi

    assert isinstance(by_path, types.ModuleType) and by_path is _cabi and hip_ops._cabi is _cabi
    assert hip_ops._lib is None or isinstance(hip_ops._lib, ctypes.CDLL)
    assert hip_ops._lib is _cabi._lib


def test_package_file_is_a_facade():
    src = open(os.path.join(PKG, "buglab", "models", "hip_ops", "__init__.py"), encoding="utf-8").read()
    assert src.count("\n") < 150
    assert not [n for n in ast.parse(src).body if isinstance(n, (ast.FunctionDef, ast.AsyncFunctionDef))]

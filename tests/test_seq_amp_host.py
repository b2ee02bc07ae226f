"""CPU: the sequence GEMM mode switch (hip_ops.set_seq_gemm_mode / seq_gemm_mode, bl_set_seq_gemm_mode / bl_seq_gemm_mode) -- names,
round trip, facade export, ctypes prototypes against the header.  No kernel runs here: the library loads without a GPU."""
import ctypes
import os
import re

import pytest

from tests.conftest import PKG, ROOT

HEADER = os.path.join(ROOT, "include", "buglab_hip.h")
LIB = os.path.join(PKG, "buglab", "models", "hip_ops", "libbuglab_hip.so")


@pytest.fixture(scope="module")
def ops():
    if not os.path.exists(LIB):
        import __graft_entry__ as g

        g.build()
    from buglab.models import hip_ops

    hip_ops.load_library()
    return hip_ops


def test_unknown_mode_names_are_rejected(ops):
    before = ops.seq_gemm_mode()
    for bad in ("f16x1", "bf16x3", "amp", "", None, 1):
        with pytest.raises(ValueError, match="bf16x6"):
            ops.set_seq_gemm_mode(bad)
    assert ops.seq_gemm_mode() == before
    lib = ops.load_library()
    for code in (2, -1, 7):  # the C entry point: BL_EINVAL, mode unchanged, a message for bl_last_error
        assert lib.bl_set_seq_gemm_mode(code) == -1 and b"bl_set_seq_gemm_mode" in lib.bl_last_error()
    assert ops.seq_gemm_mode() == before


def test_mode_round_trips_and_its_names_live_in_switches(ops):
    from buglab.models.hip_ops import _switches, runtime

    assert _switches._SEQ_GEMM_MODES == ("bf16x6", "bf16x1")  # index = bl_set_seq_gemm_mode's code
    assert "BL_SEQ_GEMM" not in os.environ and ops.seq_gemm_mode() == "bf16x6"  # the default
    lib = ops.load_library()
    try:
        assert ops.set_seq_gemm_mode("bf16x1") == "bf16x6"
        assert ops.seq_gemm_mode() == "bf16x1" and lib.bl_seq_gemm_mode() == 1
        assert ops.set_seq_gemm_mode("bf16x1") == "bf16x1"
        assert ops.set_seq_gemm_mode("bf16x6") == "bf16x1"
        assert ops.seq_gemm_mode() == "bf16x6" and lib.bl_seq_gemm_mode() == 0
        for name in _switches._SEQ_GEMM_MODES:
            ops.set_seq_gemm_mode(name)
            assert ops.seq_gemm_mode() == name
    finally:
        lib.bl_set_seq_gemm_mode(0)
    # one owner: the functions are runtime's, the package only forwards them; the message switch is untouched by this one
    assert ops.set_seq_gemm_mode is runtime.set_seq_gemm_mode and ops.seq_gemm_mode is runtime.seq_gemm_mode
    was = ops.msg_gemm_mode()
    ops.set_seq_gemm_mode(ops.set_seq_gemm_mode("bf16x1"))
    assert ops.msg_gemm_mode() == was


def test_autograd_scope_restores_the_callers_mode(ops):
    """what the Functions' backward passes use: run in the forward's mode, leave the switch where the caller put it"""
    from buglab.models.hip_ops import _autograd

    assert _autograd._seq_gemm_mode_code() == 0
    with _autograd._in_seq_gemm_mode(1):
        assert ops.seq_gemm_mode() == "bf16x1"
        with _autograd._in_seq_gemm_mode(1):
            assert ops.seq_gemm_mode() == "bf16x1"
        with pytest.raises(KeyError):
            with _autograd._in_seq_gemm_mode(0):
                assert ops.seq_gemm_mode() == "bf16x6"
                raise KeyError("x")
        assert ops.seq_gemm_mode() == "bf16x1"
    assert ops.seq_gemm_mode() == "bf16x6"


def test_facade_exports_and_ctypes_table_match_the_header(ops):
    assert {"set_seq_gemm_mode", "seq_gemm_mode"} <= set(dir(ops))
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    assert re.search(r"\bint32_t\s+bl_set_seq_gemm_mode\s*\(\s*int32_t\s+mode\s*\)\s*;", src)
    assert re.search(r"\bint32_t\s+bl_seq_gemm_mode\s*\(\s*void\s*\)\s*;", src)
    assert ops._SIGNATURES["bl_set_seq_gemm_mode"] == ([ctypes.c_int32], ctypes.c_int32)
    assert ops._SIGNATURES["bl_seq_gemm_mode"] == ([], ctypes.c_int32)
    assert {"bl_set_seq_gemm_mode", "bl_seq_gemm_mode"} <= set(ops.EXPORTED_SYMBOLS)
    lib = ops.load_library()
    assert lib.bl_set_seq_gemm_mode.argtypes == [ctypes.c_int32] and lib.bl_set_seq_gemm_mode.restype is ctypes.c_int32
    assert lib.bl_seq_gemm_mode.argtypes == [] and lib.bl_seq_gemm_mode.restype is ctypes.c_int32


def test_amp_help_text_names_what_is_reduced():
    from buglab.models import train, trainandeval

    for mod in (train, trainandeval):
        line = re.search(r"--amp .*\n.*\n", mod.__doc__).group(0)
        assert "gnn-mlp message GEMMs" in line and "seq-* projections" in line and "ggnn" in line, line

"""CPU: the streaming relational attention's host side -- which shapes bl_rel_attn_stream_ok takes, the argument checks of the
two launchers (BL_EINVAL and a message before any HIP call: this file runs without a GPU), hip_ops.attention_path over the switch
values and modes, and the agreement of header, exports and ctypes table on the three prototypes."""
import ctypes
import os
import re

import pytest

from tests.conftest import ROOT

HEADER = os.path.join(ROOT, "include", "buglab_hip.h")
NAMES = ("bl_rel_attn_stream_ok", "bl_rel_attn_stream_fwd", "bl_rel_attn_stream_bwd")


@pytest.fixture(scope="module")
def ops():
    from buglab.models import hip_ops

    hip_ops.load_library()
    return hip_ops


def test_which_shapes_the_streaming_kernels_take(ops):
    ok = ops.load_library().bl_rel_attn_stream_ok
    for L in (4, 64, 68, 1024, 1028, 1540, 4096, 5000, 1 << 20):  # no upper bound from LDS
        assert ok(L, 32, 8) == 1, L
    for L in (0, -4, 1, 2, 3, 66, 1030, 4097):
        assert ok(L, 32, 8) == 0, L
    for dk in (0, 8, 16, 24, 48, 64, 128):  # one head dimension
        assert ok(1028, dk, 8) == 0, dk
    # the edge-bias gradient table of a workgroup: 2 T dk <= 1024
    assert [ok(1028, 32, T) for T in (0, 1, 8, 16, 17, 64)] == [0, 1, 1, 1, 0, 0]
    # ... and the one-call layer does not claim what its stored-probability kernels cannot hold: the op-by-op path runs beyond 1024
    lib = ops.load_library()
    assert lib.bl_great_layer_ok(1, 512, 2, 32, 4, 96) == 1 and lib.bl_great_layer_ok(1, 1028, 2, 32, 4, 96) == 0
    assert lib.bl_rel_attn_probs_ok(1028, 32, 4) == 0 and lib.bl_attn_mm32_ok(2048, 32) == 0


def _views(ops, n):
    """n valid head views (16-byte aligned base, strides multiples of 4) over host buffers: only ever seen by the argument checks"""
    bufs = [(ctypes.c_float * 256)() for _ in range(n)]
    views = []
    for b in bufs:
        addr = (ctypes.addressof(b) + 15) & ~15
        views.append(ops.bl_head_view_t(addr, 4 * 2 * 3 * 32, 3 * 32, 2 * 3 * 32))
    return bufs, views


def test_argument_errors_without_a_gpu(ops):
    lib = ops.load_library()
    keep, (q, k, v, o, go, gq, gk, gv) = _views(ops, 8)
    f = (ctypes.c_float * 64)()
    i = (ctypes.c_int32 * 64)()
    fp, ip = ctypes.cast(f, ctypes.c_void_p), ctypes.cast(i, ctypes.c_void_p)
    drop, ref = ops.Dropout(0.1, 1, 2).c(), ctypes.byref

    def fwd(q=q, k=k, v=v, csr=(None, None, None), B=1, L=4, H=2, dk=32, T=1, bf=fp, br=fp, lens=ip, drop=drop, o=o, lse=fp):
        r = lambda x: ref(x) if x is not None else None
        return lib.bl_rel_attn_stream_fwd(r(q), 0.25, r(k), r(v), *csr, B, L, H, dk, T, bf, br, lens, drop, r(o), lse, None)

    def bwd(go=go, lse=fp, q=q, k=k, v=v, csr=(None, None, None), B=1, L=4, H=2, dk=32, T=1, bf=fp, br=fp, lens=ip, drop=drop, delta=fp, gq=gq,
            gk=gk, gv=gv, gbf=fp, gbr=fp):
        r = lambda x: ref(x) if x is not None else None
        return lib.bl_rel_attn_stream_bwd(r(go), lse, r(q), 0.25, r(k), r(v), *csr, B, L, H, dk, T, bf, br, lens, drop, delta, r(gq), r(gk), r(gv),
                                          gbf, gbr, None)

    def refused(rc, *words):
        msg = lib.bl_last_error()
        assert rc != 0, "accepted"
        for w in words:
            assert w in msg, (w, msg)

    for call, name in ((fwd, b"bl_rel_attn_stream_fwd"), (bwd, b"bl_rel_attn_stream_bwd")):
        refused(call(q=None), name, b"null")
        refused(call(v=None), name, b"null")
        refused(call(lse=None), name, b"null")
        refused(call(lens=None), name, b"null")
        refused(call(bf=None), name, b"null")
        refused(call(csr=(ip, None, ip)), name, b"partial edge CSR")
        refused(call(csr=(ip, ip, None)), name, b"partial edge CSR")
        refused(call(csr=(None, ip, None)), name, b"partial edge CSR")
        refused(call(L=6), name, b"unsupported shape", b"L=6")
        refused(call(dk=16), name, b"unsupported shape", b"dk=16")
        refused(call(T=17), name, b"unsupported shape", b"T=17")
        refused(call(H=0), name, b"bad shape")
        refused(call(B=-1), name, b"bad shape")
        refused(call(B=16, L=8192, H=8), name, b"2^32")  # with dropout the mask index row * L + key is 32 bits
        refused(call(drop=ops.Dropout(1.5, 1, 2).c()), name, b"dropout")
        odd = ops.bl_head_view_t(q.p + 4, q.sb, q.sh, q.sl)
        refused(call(q=odd), name, b"16-byte aligned")
        odd = ops.bl_head_view_t(q.p, q.sb, q.sh + 2, q.sl)
        refused(call(k=odd), name, b"multiples of 4")
    refused(fwd(o=None), b"null")
    refused(bwd(go=None), b"null")
    refused(bwd(gk=None), b"null")
    refused(bwd(delta=None), b"null")
    refused(bwd(csr=(ip, ip, ip), gbf=None), b"g_bias_f")
    # B == 0 is an empty minibatch, not an error -- and launches nothing
    assert fwd(B=0) == 0 and bwd(B=0) == 0
    del keep


def test_attention_path_over_switches_and_modes(ops):
    path = ops.attention_path
    was, was_fused = ops.STREAMING_ATTENTION, ops.FUSED_ATTENTION
    try:
        ops.STREAMING_ATTENTION = "auto"
        assert path(512, 32, 8) == "fused" and path(1024, 32, 8) == "rowwise"  # no run that works today changes kernels
        assert path(96, 16, 5) == "fused" and path(40, 64, 2) == "fused"
        assert path(512, 32, 8, scalar_bias=True) == "rowwise" and path(512, 32, 8, value_biases=True) == "fused"
        assert path(512, 64, 12) == "rowwise" and path(768, 32, 8) == "rowwise"  # (ceil(L / 256) = 3: K^T does not tile)
        assert path(1028, 32, 8) == "stream" and path(4096, 32, 8) == "stream" and path(2048, 32, 1) == "stream"
        ops.FUSED_ATTENTION = False
        assert path(512, 32, 8) == "rowwise" and path(1028, 32, 8) == "stream"
        ops.FUSED_ATTENTION = True
        for kw, why in ((dict(value_biases=True), "value biases"), (dict(scalar_bias=True), "scalar"), (dict(dk=64), "dk=64"),
                        (dict(dk=16), "dk=16"), (dict(T=17), "T=17"), (dict(L=1030), "L=1030")):
            args = dict(L=1540, dk=32, T=8)
            args.update(kw)
            with pytest.raises(ValueError) as ei:
                path(**args)
            msg = str(ei.value)
            assert f"L={args['L']}" in msg and "1024" in msg and why in msg, msg
        ops.STREAMING_ATTENTION = "1"
        assert path(512, 32, 8) == "stream" and path(64, 32, 3) == "stream" and path(1028, 32, 8) == "stream"
        assert path(96, 16, 5) == "fused" and path(512, 64, 12) == "rowwise"  # where streaming cannot: the stored paths, as before
        assert path(512, 32, 8, scalar_bias=True) == "rowwise" and path(512, 32, 8, value_biases=True) == "fused"
        with pytest.raises(ValueError):
            path(1540, 32, 8, value_biases=True)
        ops.STREAMING_ATTENTION = "0"
        assert path(512, 32, 8) == "fused" and path(1024, 32, 8) == "rowwise"
        with pytest.raises(ValueError) as ei:
            path(1028, 32, 8)
        assert "switched off" in str(ei.value) and "L=1028" in str(ei.value) and "1024" in str(ei.value)
        for v, want in ((True, "stream"), (False, "fused"), (" AUTO ", "fused"), (1, "stream"), (0, "fused")):
            ops.STREAMING_ATTENTION = v
            assert path(512, 32, 8) == want, v
        ops.STREAMING_ATTENTION = "sometimes"
        with pytest.raises(ValueError):
            path(512, 32, 8)
    finally:
        ops.STREAMING_ATTENTION, ops.FUSED_ATTENTION = was, was_fused


def test_the_switch_has_one_owner(ops):
    """Assigned on the package, read by seq.py: one copy (the rule of hip_ops/_switches.py), environment variable BL_STREAMING_ATTENTION."""
    import subprocess
    import sys

    from buglab.models.hip_ops import _switches, seq

    was = ops.STREAMING_ATTENTION
    try:
        marker = "1"
        ops.STREAMING_ATTENTION = marker
        assert seq.STREAMING_ATTENTION is marker and "STREAMING_ATTENTION" not in vars(ops) and "STREAMING_ATTENTION" not in vars(_switches)
        seq.STREAMING_ATTENTION = "0"
        assert ops.STREAMING_ATTENTION == "0"
    finally:
        ops.STREAMING_ATTENTION = was
    assert "STREAMING_ATTENTION" not in seq.__all__ and "attention_path" in seq.__all__
    code = "from buglab.models import hip_ops; print(hip_ops.STREAMING_ATTENTION)"
    for value, want in (("0", "0"), ("1", "1"), (None, "auto")):
        env = {k: v for k, v in os.environ.items() if k != "BL_STREAMING_ATTENTION"}
        if value is not None:
            env["BL_STREAMING_ATTENTION"] = value
        env["PYTHONPATH"] = os.pathsep.join(p for p in sys.path if p)
        out = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, check=True).stdout.strip()
        assert out == want, (value, out)


def _declared(name):
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    m = re.search(r"\b(int32_t|int)\s+" + name + r"\s*\(([^;]*?)\)\s*;", src, flags=re.S)
    assert m, name
    return m.group(1), [" ".join(a.split()) for a in m.group(2).split(",")]


def test_header_exports_and_ctypes_agree_on_the_three_prototypes(ops):
    import subprocess

    from buglab.models.hip_ops import _cabi

    nm = subprocess.run(["nm", "-D", "--defined-only", _cabi.LIB_PATH], capture_output=True, text=True, check=True).stdout
    full = open(HEADER).read()
    for name in NAMES:
        assert re.search(r" T " + name + r"\b", nm), name
        assert name in ops.EXPORTED_SYMBOLS
        ret, args = _declared(name)
        argtypes, restype = _cabi._SIGNATURES[name]
        assert restype is (ctypes.c_int32 if ret == "int32_t" else ctypes.c_int)
        want = []
        for a in args:
            if "bl_head_view_t*" in a:
                want.append(ctypes.POINTER(_cabi.bl_head_view_t))
            elif "*" in a:
                want.append(ctypes.c_void_p)
            elif a.startswith("bl_dropout_t"):
                want.append(_cabi.bl_dropout_t)
            elif a.startswith("float"):
                want.append(ctypes.c_float)
            else:
                assert a.startswith("int32_t"), a
                want.append(ctypes.c_int32)
        assert list(argtypes) == want, name
        assert getattr(ops.load_library(), name).argtypes == argtypes
    # the header comment of the three cites the reference code they replace
    at = full.index("int32_t bl_rel_attn_stream_ok")
    comment = full[full.rindex("/*", 0, at):at]
    assert "multihead_attention.py:46-80" in comment and "relational_multihead_attention.py:72-178" in comment
    assert [a.split()[-1] for a in _declared("bl_rel_attn_stream_ok")[1]] == ["L", "dk", "T"]
    assert _declared("bl_rel_attn_stream_fwd")[1][-1] == "void* stream" and _declared("bl_rel_attn_stream_bwd")[1][-1] == "void* stream"


def test_max_seq_size_beyond_the_positional_table_fails_at_construction():
    from pathlib import Path

    from buglab.models.modelregistry import load_model
    from buglab.models.seqmodel import MAX_POSITIONS

    spec = {"hidden_state_size": 64, "num_heads": 2, "num_layers": 1, "intermediate_dimension_size": 96}
    for name in ("seq-great", "seq-rat", "seq-transformer"):
        with pytest.raises(ValueError) as ei:
            load_model(dict(spec, modelName=name, max_seq_size=MAX_POSITIONS + 1), Path("/tmp/_bl_stream_host.pkl.gz"))
        assert str(MAX_POSITIONS) in str(ei.value) and "max_seq_size" in str(ei.value)
        model = load_model(dict(spec, modelName=name, max_seq_size=MAX_POSITIONS), Path("/tmp/_bl_stream_host.pkl.gz"))[0]
        assert model._max_seq_size == MAX_POSITIONS
    load_model(dict(spec, modelName="seq-gru", max_seq_size=MAX_POSITIONS + 1), Path("/tmp/_bl_stream_host.pkl.gz"))  # (reads no positions)

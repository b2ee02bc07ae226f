"""CPU: the GREAT var-misuse model's host side (buglab/models/greatreimplementation.py, buglab/models/traingreat.py) and the C ABI
of its HIP head (csrc/bl_varmisuse_head.hip) -- reading, metadata, tensorisation, collation, the position table, exported
symbols, structure layout and argument errors.  Nothing here touches a GPU."""
import ctypes
import gzip
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from tests.conftest import PKG, ROOT

HEADER = os.path.join(ROOT, "include", "buglab_hip.h")
LIB = os.path.join(PKG, "buglab", "models", "hip_ops", "libbuglab_hip.so")
NEW_SYMBOLS = ("bl_varmisuse_head_workspace_bytes", "bl_varmisuse_head_fwd", "bl_varmisuse_head_bwd")
SMALL = {"num_layers": 2, "num_heads": 4, "intermediate_dimension": 96, "dropout_rate": 0.0}


@pytest.fixture(scope="module")
def built_lib():
    if not os.path.exists(LIB):
        import __graft_entry__ as g

        g.build()
    return LIB


def _write(path, records):
    with gzip.open(path, "wt") as f:
        for r in records:
            f.write(json.dumps(r) + "\n")


def _rec(tokens, edges=(), err=0, cands=(), targets=()):
    return {"source_tokens": list(tokens), "edges": [list(e) for e in edges], "error_location": err, "repair_candidates": list(cands),
            "repair_targets": list(targets), "has_bug": err > 0, "bug_kind": 1, "bug_kind_name": "VARIABLE_MISUSE", "provenances": []}


def test_jsonl_reader_sorted_files_and_limit_plus_one(tmp_path):
    from buglab.models.traingreat import load_all_json_l_gz

    _write(tmp_path / "b.jsonl.gz", [{"i": 3}, {"i": 4}])
    _write(tmp_path / "a.jsonl.gz", [{"i": 0}, {"i": 1}, {"i": 2}])
    _write(tmp_path / "c.jsonl.gz", [{"i": 5}])
    (tmp_path / "ignored.json").write_text("{}")
    assert [r["i"] for r in load_all_json_l_gz(str(tmp_path))] == [0, 1, 2, 3, 4, 5]
    # the reference stops once MORE than `limit` records were yielded: limit + 1 of them
    assert [r["i"] for r in load_all_json_l_gz(str(tmp_path), limit_num_yielded_elements=3)] == [0, 1, 2, 3]
    assert [r["i"] for r in load_all_json_l_gz(str(tmp_path), take_only_first_n_files=2)] == [0, 1, 2, 3, 4]
    shuffled = sorted(r["i"] for r in load_all_json_l_gz(str(tmp_path), shuffle=True))
    assert shuffled == [0, 1, 2, 3, 4, 5]


def _model(**kw):
    from buglab.models.greatreimplementation import GreatVarMisuse

    return GreatVarMisuse(dict(SMALL), vocab_size=64, embedding_dim=64, **kw)


def test_edge_ids_map_to_ascending_order():
    m = _model()
    m.compute_metadata([_rec(["a", "b", "c"], edges=[(0, 1, 9, "x"), (1, 2, 2, "y")]), _rec(["a", "b"], edges=[(1, 0, 5, "z")])])
    assert m.edge_id_to_edge == {2: 0, 5: 1, 9: 2}
    assert m.build_neural_module().seq_layers[0].num_edge_types == 6


def test_tensorize_rejections():
    m = _model(max_length=5)
    m.compute_metadata([_rec(["a"] * 6, edges=[(0, 1, 1, "x")])])
    assert m.tensorize(_rec(["a"] * 6)) is None                                  # longer than max_length
    assert m.tensorize(_rec(["a"] * 5, err=1, cands=[2, 3], targets=[4])) is None  # no candidate is a target
    t = m.tensorize(_rec(["a"] * 5, err=1, cands=[2, 3], targets=[3, 4]))
    assert t is not None and t.repair_candidates_mask.dtype == bool
    assert t.repair_candidates_mask.tolist() == [False, False, True, True, False]
    assert m.tensorize(_rec(["a"] * 5, err=0, cands=["x"])).repair_candidates_mask is None  # NO_BUG: masks unused


def test_collated_two_sample_batch():
    from buglab.data.seqcollate import edge_csr

    m = _model()
    recs = [_rec(["fooBar", "x", "y", "x", "z"], edges=[(0, 1, 7, "a"), (3, 2, 4, "b")], err=3, cands=[1, 3], targets=[1, 4]),
            _rec(["y", "x", "q"], edges=[(2, 0, 7, "a")], err=0)]
    m.compute_metadata(recs * 5)  # (min_freq_threshold 5: every subtoken in the vocabulary)
    mb = m.collate_samples([m.tensorize(r) for r in recs])
    B, L, S = mb["token_ids"].shape
    assert (B, L) == (2, 8)  # longest 5, padded to a multiple of 4
    assert (mb["token_ids"][1, 3:] == 0).all() and (mb["token_ids"][0, 5:] == 0).all()
    assert (mb["token_lens"][1, 3:] == 1).all() and (mb["token_lens"][0, 5:] == 1).all()
    assert mb["token_lens"][0, 0] == 2  # fooBar -> foo, bar
    assert mb["seq_lens"].tolist() == [5, 3]
    assert mb["lens_att"].tolist() == [5, 4]  # min(length + 1, longest)
    assert mb["has_bug"].astype(bool).tolist() == [True, False]
    assert mb["error_locations"].tolist() == [3, 0]
    assert mb["candidate_mask"][0].tolist() == [0, 1, 0, 1, 0, 0, 0, 0] and not mb["candidate_mask"][1].any()
    assert mb["target_mask"][0].tolist() == [0, 1, 0, 0, 1, 0, 0, 0]
    # edges + reversal with types shifted by n = 2 (ids 4 -> 0, 7 -> 1)
    e = np.array([[0, 0, 1], [0, 3, 2], [1, 2, 0], [0, 1, 0], [0, 2, 3], [1, 0, 2]])
    t = np.array([1, 0, 1, 3, 2, 3])
    rp, key, code = edge_csr(e, t, B, L)
    assert (mb["edge_row_ptr"] == rp).all() and (mb["edge_key"] == key).all() and (mb["edge_code"] == code).all()
    # query row (0, 0): forward of edge 0 (key 1, code 2) and reverse of its reversal (key 1, code 2 * 3 + 1)
    r0 = slice(rp[0], rp[1])
    assert sorted(zip(key[r0].tolist(), code[r0].tolist())) == [(1, 2), (1, 7)]


def test_positional_table_matches_float64_formula():
    import torch

    from buglab.models.greatreimplementation import positional_table

    D = 48
    P = positional_table(D)
    assert P.shape == (5000, D) and P.dtype == torch.float32
    pos = np.arange(5000, dtype=np.float64)[:, None]
    ref = np.empty((5000, D))
    for i in range(D):
        a = pos[:, 0] / 10000.0 ** (2 * i / D)  # exponent 2 i / D for every i
        ref[:, i] = np.sin(a) if i % 2 == 0 else np.cos(a)
    assert np.abs(P.numpy() - ref.astype(np.float32)).max() == 0.0
    m = _model()
    m.compute_metadata([_rec(["a"], edges=[(0, 0, 1, "x")])])
    nn = m.build_neural_module()
    assert "positional_encodings" in dict(nn.named_buffers()) and all(p is not nn.positional_encodings for p in nn.parameters())


def test_save_restore_round_trip(tmp_path):
    import torch

    from buglab.runtime.neuralmodel import AbstractNeuralModel

    m = _model()
    recs = [_rec(["a", "b", "c"], edges=[(0, 1, 3, "x")], err=1, cands=[1, 2], targets=[2])]
    m.compute_metadata(recs)
    nn = m.build_neural_module()
    m.save(tmp_path / "m.pkl.gz", nn)
    m2, nn2 = AbstractNeuralModel.restore_model(tmp_path / "m.pkl.gz")
    assert m2.edge_id_to_edge == m.edge_id_to_edge
    for (k, a), (_, b) in zip(nn.state_dict().items(), nn2.state_dict().items()):
        assert torch.equal(a, b), k
    t1, t2 = m.tensorize(recs[0]), m2.tensorize(recs[0])
    assert (t1.token_ids == t2.token_ids).all()


def _header_symbols():
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    return set(re.findall(r"\b(bl_[a-z0-9_]+)\s*\(", src))


def test_new_symbols_in_header_exports_and_ctypes_table(built_lib):
    from buglab.models import hip_ops

    nm = subprocess.run(["nm", "-D", "--defined-only", built_lib], capture_output=True, text=True, check=True).stdout
    exported = set(re.findall(r" T (bl_[a-z0-9_]+)", nm))
    for s in NEW_SYMBOLS:
        assert s in _header_symbols() and s in exported and s in hip_ops.EXPORTED_SYMBOLS, s
    assert "greatreimplementation.py" in open(HEADER).read()


def test_descriptor_layout_matches_ctypes_mirror(tmp_path):
    from buglab.models.hip_ops import _cabi as L
    cls = L.bl_varmisuse_head_t
    lines = ["#include <stdio.h>", "#include <stddef.h>", f'#include "{HEADER}"', "int main(void) {",
             '  printf("%zu %d", sizeof(bl_varmisuse_head_t), BL_VARMISUSE_STATS);']
    lines += [f'  printf(" %zu", offsetof(bl_varmisuse_head_t, {f}));' for f, _ in cls._fields_]
    lines += ['  printf("\\n");', "  return 0;", "}"]
    src = tmp_path / "layout.c"
    src.write_text("\n".join(lines))
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-std=c11", "-o", str(exe), str(src)], check=True, capture_output=True, text=True)
    size, nstats, *offs = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()
    assert ctypes.sizeof(cls) == int(size)
    assert int(nstats) == L.VARMISUSE_STATS
    assert [getattr(cls, f).offset for f, _ in cls._fields_] == [int(o) for o in offs]


def test_argument_errors_without_gpu(built_lib):
    from buglab.models import hip_ops

    lib = hip_ops.load_library()
    buf = (ctypes.c_float * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p).value
    d = hip_ops.bl_varmisuse_head_t()
    d.B, d.L, d.D, d.ln_eps = 2, 5, 64, 1e-5
    d.x = d.ln_g = d.ln_b = d.W = d.bias = d.lens_att = d.error_location = d.candidate_mask = d.target_mask = p
    rc = lib.bl_varmisuse_head_fwd(None, p, p, p, p, p, p, p, None)
    assert rc == -1 and b"null descriptor" in lib.bl_last_error()
    d.D = 66
    rc = lib.bl_varmisuse_head_fwd(ctypes.byref(d), p, p, p, p, p, p, p, None)
    assert rc == -1 and b"multiple of 4" in lib.bl_last_error()
    d.D = 2048
    assert lib.bl_varmisuse_head_fwd(ctypes.byref(d), p, p, p, p, p, p, p, None) == -1
    assert lib.bl_varmisuse_head_workspace_bytes(2, 5, 2048) == -1
    d.D, d.x = 64, None
    rc = lib.bl_varmisuse_head_bwd(ctypes.byref(d), p, p, p, p, p, p, p, p, p, p, p, p, None)
    assert rc == -1 and b"null" in lib.bl_last_error()
    d.x, d.B = p, 0
    rc = lib.bl_varmisuse_head_fwd(ctypes.byref(d), p, p, p, p, p, p, p, None)
    assert rc == -1 and b"B (0)" in lib.bl_last_error()
    d.B = 2
    rc = lib.bl_varmisuse_head_fwd(ctypes.byref(d), None, p, p, p, p, p, p, None)
    assert rc == -1 and b"null output" in lib.bl_last_error()
    assert lib.bl_varmisuse_head_workspace_bytes(30, 512, 512) > 0


def _cli(*args):
    env = dict(os.environ, PYTHONPATH=os.pathsep.join([PKG, ROOT]))
    return subprocess.run([sys.executable, os.path.join(PKG, "buglab", "models", "traingreat.py"), *args], capture_output=True,
                          text=True, env=env, timeout=120)


def test_traingreat_help_and_amp_refused(tmp_path):
    r = _cli("--help")
    assert r.returncode == 0 and "TRAIN_DATA_PATH" in r.stdout and "--minibatch-size" in r.stdout
    r = _cli(str(tmp_path), str(tmp_path), str(tmp_path / "m.pkl.gz"), "--amp")
    assert r.returncode != 0 and "--amp" in r.stderr and "gnn-mlp" in r.stderr
    env = dict(os.environ, PYTHONPATH=os.pathsep.join([PKG, ROOT]))
    r = subprocess.run([sys.executable, "-m", "buglab.models.traingreat", "--help"], capture_output=True, text=True, env=env, cwd=PKG,
                       timeout=120)
    assert r.returncode == 0 and "MODEL_FILENAME" in r.stdout
    from buglab.models.traingreat import DEFAULT_TRANSFORMER_CONFIG, parse_args

    a = parse_args(["t", "v", "m"])
    assert (a["--max-num-epochs"], a["--minibatch-size"], a["--validate-after"]) == ("100", "30", "1000000")
    assert DEFAULT_TRANSFORMER_CONFIG["num_layers"] == 10 and DEFAULT_TRANSFORMER_CONFIG["normalization_mode"] == "prenorm"


def test_synthetic_great_records_are_valid(tmp_path):
    from buglab.data.synthetic_great import make_great_records, write_great_dir
    from buglab.models.traingreat import load_all_json_l_gz

    recs = make_great_records(20, seed=3)
    write_great_dir(str(tmp_path), recs, per_file=8)
    back = list(load_all_json_l_gz(str(tmp_path)))
    assert back == json.loads(json.dumps(recs))
    m = _model()
    m.compute_metadata(back)
    ts = [m.tensorize(r) for r in back]
    assert all(t is not None for t in ts) and any(r["error_location"] > 0 for r in back) and any(r["error_location"] == 0 for r in back)

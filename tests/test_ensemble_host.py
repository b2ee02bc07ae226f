"""CPU: model ensembles (buglab.models.ensemble; reference buglab/models/ensemble/) -- the CLI and the file it writes, argument
checks, the un-batching gather layout every model shares (basemodel.prediction_layout) against the dict-based un-batching of
reference basemodel.py:240-346, the ensemble's host-side gather indices, and the C entry point's argument errors."""
import copy
import ctypes
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

from tests import ensemble_ref as R
from tests.conftest import PKG

SEQ_SPEC = {"hidden_state_size": 32, "num_layers": 1, "num_heads": 4, "intermediate_dimension_size": 48, "dropout_rate": 0.1}


def _spec(family, **extra):
    if family.startswith("seq"):
        return dict(SEQ_SPEC, modelName=family, **extra)
    return dict({"modelName": family, "hidden_state_size": 32, "dropout_rate": 0.1}, **extra)


def _data(family, n=10, seed=3):
    from buglab.data.synthetic import make_buglab_dataset, make_buglab_seq_dataset

    return make_buglab_seq_dataset(n, seed=seed) if family.startswith("seq") else make_buglab_dataset(n, seed=seed)


def _make_checkpoint(path, family, data, seed, **extra):
    from buglab.models.modelregistry import load_model

    model = load_model(_spec(family, **extra), path)[0]
    model.compute_metadata(copy.deepcopy(data))
    torch.manual_seed(seed)
    nn_ = model.build_neural_module()
    model.save(path, nn_)
    return model, nn_


def test_cli_builds_an_ensemble_file_that_restores_with_every_member(tmp_path):
    from buglab.data.synthetic import make_buglab_seq_dataset
    from buglab.models.ensemble.wrapper import EnsembleModuleWrapper, EnsembleWrapper
    from buglab.runtime.neuralmodel import AbstractNeuralModel

    data = make_buglab_seq_dataset(8, seed=5)
    paths = [tmp_path / "g1.pkl.gz", tmp_path / "g2.pkl.gz", tmp_path / "s.pkl.gz"]
    srcs = [_make_checkpoint(paths[0], "gnn-mlp", data, 1)[1], _make_checkpoint(paths[1], "gnn-mlp", data, 2)[1],
            _make_checkpoint(paths[2], "seq-great", data, 3)[1]]
    out = tmp_path / "ens.pkl.gz"
    r = subprocess.run([sys.executable, "-m", "buglab.models.ensemble", str(out), "consensus"] + [str(p) for p in paths],
                       cwd=PKG, capture_output=True, text=True, env={"CUDA_VISIBLE_DEVICES": "", "HIP_VISIBLE_DEVICES": "",
                                                                    "PATH": "/usr/bin:/bin", "PYTHONPATH": PKG})
    assert r.returncode == 0, r.stderr
    assert "Loaded 3 models" in r.stdout and out.exists() and not Path(str(out) + ".tmp").exists()
    model, nn_ = AbstractNeuralModel.restore_model(out, "cpu")
    assert isinstance(model, EnsembleWrapper) and isinstance(nn_, EnsembleModuleWrapper)
    assert model.kind == "consensus" and [type(m).__name__ for m in model.models] == ["GnnBugLabModel", "GnnBugLabModel", "SeqBugLabModel"]
    members = list(nn_.nns)
    assert len(members) == 3
    for got, want in zip(members, srcs):
        sd_got, sd_want = got.state_dict(), want.state_dict()
        assert list(sd_got) == list(sd_want)
        assert all(torch.equal(sd_got[k], sd_want[k]) for k in sd_want)
    assert not torch.equal(next(iter(members[0].parameters())), next(iter(members[1].parameters())))  # two seeds
    # nn.to / .eval / .train reach every member (an nn.ModuleList, where the reference keeps a plain list)
    n_params = sum(p.numel() for m in members for p in m.parameters())
    assert sum(p.numel() for p in nn_.parameters()) == n_params
    nn_.train()
    assert all(m.training for m in nn_.nns)
    nn_.eval()
    assert not any(mod.training for m in nn_.nns for mod in m.modules())
    nn_.to(torch.float64)
    assert all(p.dtype == torch.float64 for m in nn_.nns for p in m.parameters())


def test_bad_kind_and_members_without_predict_are_rejected(tmp_path):
    from buglab.models.ensemble.wrapper import EnsembleWrapper
    from buglab.models.greatreimplementation import GreatVarMisuse

    model = _make_checkpoint(tmp_path / "g.pkl.gz", "gnn-mlp", _data("gnn-mlp", 4), 0)[0]
    with pytest.raises(ValueError, match="kind"):
        EnsembleWrapper([model], "majority")
    great = GreatVarMisuse.__new__(GreatVarMisuse)
    assert not hasattr(great, "predict")
    with pytest.raises(ValueError, match="predict"):
        EnsembleWrapper([model, great], "avg")
    with pytest.raises(ValueError):
        EnsembleWrapper([], "avg")
    from buglab.models.ensemble.__main__ import main

    with pytest.raises(SystemExit):
        main([str(tmp_path / "o.pkl.gz"), "median", str(tmp_path / "g.pkl.gz")])


def _collated(family, n=12, seed=3, **extra):
    from buglab.models.modelregistry import load_model

    data = _data(family, n, seed)
    model = load_model(_spec(family, **extra), Path("/nonexistent/m.pkl.gz"))[0]
    model.compute_metadata(copy.deepcopy(data))
    with model._tensorize_all_location_rewrites():
        pairs = [(t, d) for t, d in ((model.tensorize(d), d) for d in copy.deepcopy(data)) if t is not None]
    mb = model.collate_minibatch({"samples": [t for t, _ in pairs], "num_nodes": 0})
    return model, mb, [d for _, d in pairs], [t for t, _ in pairs]


def _fake_outputs(mb, offset=0.0):
    gd = mb["graph_data"]
    B = int(gd["num_graphs"])
    ids = np.concatenate([np.asarray(gd["reference_node_graph_idx"]["candidate_nodes"]), np.arange(B)]).astype(np.int64)
    sizes = [ids.shape[0]] + [int(np.asarray(mb[k]).shape[0]) for k in
                               ("rewrite_to_location_group", "candidate_symbol_to_location_group", "swapped_pair_to_call_location_group")]
    flat = (-0.5 - 0.001 * np.arange(sum(sizes)) - offset).astype(np.float32)  # distinct values
    loc, text, var, swap = np.split(flat, np.cumsum(sizes)[:-1])
    return ids, flat, loc, text, var, swap


@pytest.mark.parametrize("family", ["gnn-mlp", "ggnn", "seq-great", "seq-rat"])
def test_prediction_layout_reproduces_the_dict_unbatching(family):
    from buglab.models.basemodel import prediction_layout

    model, mb, points, samples = _collated(family)
    B = len(points)
    assert B >= 8
    ids, flat, loc, text, var, swap = _fake_outputs(mb)
    maps = mb.get("node_mappings")
    if family.startswith("seq"):  # the graph -> token map is not injective for some samples: candidates share a token
        assert sum(len(set(m[k] for k in np.unique(p["graph"]["reference_nodes"]))) < len(np.unique(p["graph"]["reference_nodes"]))
                   for m, p in zip(maps, points)) >= 1
    want = list(R.unbatch_dicts(mb, ids, loc, swap, B, points, text, var, node_mappings=maps))
    lay = prediction_layout(mb)
    assert lay.flat_size == flat.shape[0] and lay.num_samples == B
    assert lay.loc_idx.dtype == np.int32 and lay.rw_idx.dtype == np.int32
    for b, (point, wloc, wrw) in enumerate(want):
        nodes = np.unique(point["graph"]["reference_nodes"]).tolist()
        got_loc = flat[lay.loc_idx[lay.loc_off[b]:lay.loc_off[b + 1]]].tolist()
        got_rw = flat[lay.rw_idx[lay.rw_off[b]:lay.rw_off[b + 1]]].tolist()
        assert dict(zip(nodes + [-1], got_loc)) == wloc
        assert got_rw == wrw
    # the single model's un-batching, with the layout precomputed (predict) and without: values, key order and rewrites
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a))
    for with_layout in (True, False):
        mbx = dict(mb, prediction_layout=lay) if with_layout else mb
        got = list(model._iter_per_sample_results(mbx, t(ids), t(loc), t(swap), B, points, t(text), t(var), node_mappings=maps))
        assert len(got) == B
        for (p, gl, gr), (q, wl, wr) in zip(got, want):
            assert p is q and list(gl.items()) == list(wl.items()) and gr == wr


def _kernel_numpy(kind, src, loc_idx, loc_off, rw_idx, rw_off):
    """What bl_ensemble_combine computes, restated over the gather indices (float64)."""
    M = loc_idx.shape[0]
    out_loc, out_rw = np.zeros(loc_idx.shape[1]), np.zeros(rw_idx.shape[1])
    for b in range(loc_off.shape[0] - 1):
        ls, rs = slice(loc_off[b], loc_off[b + 1]), slice(rw_off[b], rw_off[b + 1])
        preds = [None if loc_idx[m, ls][0] < 0 else
                 (dict(enumerate(src[loc_idx[m, ls]].astype(np.float64).tolist())), src[rw_idx[m, rs]].astype(np.float64).tolist())
                 for m in range(M)]
        loc, rw = R.combine(kind, preds)
        out_loc[ls], out_rw[rs] = list(loc.values()), rw
    return out_loc, out_rw


@pytest.mark.parametrize("kind", ["avg", "consensus"])
def test_ensemble_gather_indices_on_the_host(kind):
    """The ensemble's host half on the CPU: tensorise with every member (a sequence member with a small `max_seq_size` drops
    out of some samples), group, collate, build the gather indices; fabricated member outputs combined through them equal the
    reference's combination of the members' own un-batched predictions."""
    from buglab.data.synthetic import make_buglab_seq_dataset
    from buglab.models.basemodel import prediction_layout
    from buglab.models.ensemble.wrapper import EnsembleWrapper
    from buglab.models.modelregistry import load_model

    data = make_buglab_seq_dataset(14, seed=8)
    members = [load_model(_spec(f, **x), Path("/nonexistent/m.pkl.gz"))[0]
               for f, x in (("gnn-mlp", {}), ("seq-great", {"max_seq_size": 40}), ("ggnn", {}))]
    for m in members:
        m.compute_metadata(copy.deepcopy(data))
    ens = EnsembleWrapper(members, kind)
    points = copy.deepcopy(data)
    for m in members:
        m._tensorize_only_at_target_location_rewrites = False
    try:
        batches = list(ens._gather(map(ens._tensorize_all, points)))
        assert len(batches) == 1
        emb = ens._finalize(batches[0], "cpu")
    finally:
        for m in members:
            m._tensorize_only_at_target_location_rewrites = True
    slots = np.array(batches[0][1])
    assert (slots[:, 1] < 0).any() and (slots[:, 1] >= 0).any() and (slots[:, 0] >= 0).all()
    M, total_loc, total_rw, B = emb.sizes
    ix = emb.index.numpy()
    a, c = M * total_loc, M * (total_loc + total_rw)
    loc_idx, rw_idx, loc_off, rw_off = ix[:a].reshape(M, -1), ix[a:c].reshape(M, -1), ix[c:c + B + 1], ix[c + B + 1:]
    flats, own = [], []
    for m, (model, mb) in enumerate(zip(members, emb.members)):
        host_mb = model.collate_minibatch(batches[0][0][m])
        ids, flat, loc, text, var, swap = _fake_outputs(host_mb, offset=0.3 * m)
        assert flat.shape[0] == prediction_layout(host_mb).flat_size
        flats.append(flat)
        mine = [p for p, s in zip(emb.originals, slots[:, m]) if s >= 0]
        res = R.unbatch_dicts(host_mb, ids, loc, swap, len(mine), mine, text, var, node_mappings=host_mb.get("node_mappings"))
        own.append({id(p): (l, r) for p, l, r in res})
    want = R.combine_predictions(kind, own, emb.originals)
    got_loc, got_rw = _kernel_numpy(kind, np.concatenate(flats), loc_idx, loc_off, rw_idx, rw_off)
    assert len(want) == B
    for b, (p, wl, wr) in enumerate(want):
        np.testing.assert_array_equal(got_loc[loc_off[b]:loc_off[b + 1]], np.array(list(wl.values())))
        np.testing.assert_array_equal(got_rw[rw_off[b]:rw_off[b + 1]], np.array(wr, dtype=np.float64))


def test_combine_argument_errors_are_reported_without_touching_the_gpu():
    """bl_ensemble_combine validates everything before its first HIP call: BL_EINVAL (-1) / BL_ERANGE (-2) and a message."""
    from buglab.models import hip_ops

    lib = hip_ops.load_library()
    buf = (ctypes.c_int32 * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    call = lambda M=2, B=1, kind=0, n_src=16, total_loc=4, total_rw=4, src=p, loc_idx=p, loc_off=p, rw_idx=p, rw_off=p, out_loc=p, out_rw=p: \
        lib.bl_ensemble_combine(src, n_src, loc_idx, loc_off, total_loc, rw_idx, rw_off, total_rw, M, B, kind, out_loc, out_rw, None)
    for kwargs, rc, text in (
        ({"M": 0}, -1, b"at least 1"),
        ({"kind": 7}, -1, b"unknown kind"),
        ({"total_loc": -3}, -1, b"negative size"),
        ({"B": -1}, -1, b"negative size"),
        ({"src": None}, -1, b"null"),
        ({"loc_off": None}, -1, b"null"),
        ({"rw_idx": None}, -1, b"null"),
        ({"M": 17}, -2, b"at most 16"),
        ({"M": 4, "total_loc": 1 << 30}, -2, b"int32"),
        ({"n_src": 1 << 31}, -2, b"int32"),
    ):
        assert call(**kwargs) == rc, kwargs
        assert text in lib.bl_last_error(), (kwargs, lib.bl_last_error())
    with pytest.raises(ValueError, match="kind"):
        hip_ops.ensemble_combine(None, None, None, None, None, "median")

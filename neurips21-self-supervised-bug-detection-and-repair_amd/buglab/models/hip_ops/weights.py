"""Operand copies of the weights (packed / transposed forms) of buglab.models.hip_ops, re-made once per parameter update."""
from __future__ import annotations

import torch

from ._cabi import bl_pack_job_t, _check, load_library, _stream

__all__ = ["invalidate_weight_packs", "_as_groups", "_KIND", "_WeightCopies", "_weight_copies", "_packed_layer_weights",
           "_packed_message_weights", "_transposed_layer_weights"]


_weights_epoch = 0          # bumped by whoever changes parameters behind autograd's back (FlatAdam's kernel)


def invalidate_weight_packs():
    """Parameters were updated in place by a kernel (no `_version` bump): packed copies are stale."""
    global _weights_epoch
    _weights_epoch += 1


def _as_groups(w: torch.Tensor) -> torch.Tensor:
    return w if w.dim() == 3 else w.unsqueeze(0)


# Operand copies of the weights (bf16x3-packed tiled forms for the bf16x6 GEMMs, fp32 transposes for the vector input
# gradient).  They are functions of the parameter values, so a training step re-makes all of them once after the optimiser
# step -- in ONE launch (bl_pack_weights_multi) over a table of every copy any layer has asked for so far, instead of one
# launch per layer and form.  Validity = (parameter object, its autograd version, the epoch bumped by whoever writes
# parameters behind autograd's back, its storage address).
# ..w: the wide row GEMM's image (bl_pack_weights_x6w); ..h: the f16x3 image (bl_pack_weights_h3, scale BL_H3_W_SCALE)
_KIND = {"nk": 0, "kn": 1, "t": 2, "nkw": 3, "knw": 4, "nkh": 5, "knh": 6}


class _WeightCopies:
    def __init__(self):
        self.entries = {}   # id(W) -> {"ref", "ptr", "shape", "forms": {name: tensor}, "version", "epoch"}
        self.plan = None    # (device job table, njobs, total_blocks, [entries in table order])

    def _fresh(self, ent, W) -> bool:
        return ent["version"] == W._version and ent["epoch"] == _weights_epoch

    def get(self, W: torch.Tensor, names):
        import weakref

        ent = self.entries.get(id(W))
        if ent is not None and (ent["ref"]() is not W or ent["ptr"] != W.data_ptr() or ent["shape"] != tuple(W.shape)):
            ent = None
        if ent is None:
            if len(self.entries) > 256:
                self.entries = {k: v for k, v in self.entries.items() if v["ref"]() is not None}
            ent = {"ref": weakref.ref(W), "ptr": W.data_ptr(), "shape": tuple(W.shape), "forms": {}, "version": -1, "epoch": -1}
            self.entries[id(W)] = ent
            self.plan = None
        G, K, N = _as_groups(W).shape  # the parameter is [G][K][N] (forward form: C = A . W[g])
        for nm in names:
            if nm not in ent["forms"]:
                if nm == "t":
                    ent["forms"][nm] = torch.empty((G, N, K), dtype=torch.float32, device=W.device)
                else:  # "kn": C = A . W (K x N) ; "nk": C = G . W^T, i.e. bl_pack_weights_x6 of [G][N'][K'] with N' = K, K' = N
                    n_out, k_in = (N, K) if nm.startswith("kn") else (K, N)
                    per = (int(load_library().bl_packed_weight_elems_x6w(1, k_in, n_out)) if nm.endswith("w")
                           else int(load_library().bl_packed_weight_elems_h3(1, k_in, n_out)) if nm.endswith("h")
                           else ((n_out + 127) // 128) * (k_in // 32) * 12288)
                    ent["forms"][nm] = torch.empty((G, per), dtype=torch.int16, device=W.device)
                ent["version"] = -1  # (a new form has to be filled)
                self.plan = None
        if not self._fresh(ent, W):
            self.refresh(W.device)
        return [ent["forms"][nm] for nm in names]

    def refresh(self, device) -> None:
        """Re-make every registered copy on `device` whose parameter changed: one launch."""
        lib = load_library()
        # (strong references for the duration: a parameter that is only kept alive by a reference cycle can be collected by
        # the cyclic GC at any allocation below)
        alive = [(e, e["ref"]()) for e in self.entries.values()]
        alive = [(e, W) for e, W in alive if W is not None and W.device == device]
        live = [e for e, _ in alive]
        if self.plan is None or self.plan[4] != device or len(self.plan[3]) != len(live) or any(a is not b for a, b in zip(self.plan[3], live)):
            jobs, blocks = [], 0
            for e, W in alive:
                G, K, N = _as_groups(W).shape
                for nm, out in e["forms"].items():
                    j = bl_pack_job_t()
                    j.w, j.out, j.kind = W.data_ptr(), out.data_ptr(), _KIND[nm]
                    # kind 1 (kn): w [G][K][N]; kind 0 (nk): bl_pack_weights_x6(w_is_kn = 0) reads w as [G][N'][K'] = [G][K][N]
                    # with output columns N' = K and contraction K' = N; kind 2: transpose of [G][K][N]
                    j.G, j.K, j.N = (G, K, N) if not nm.startswith("nk") else (G, N, K)
                    j.first_block = blocks
                    blocks += int(lib.bl_pack_job_blocks(j.kind, j.G, j.K, j.N))
                    jobs.append(j)
            raw = b"".join(bytes(j) for j in jobs)
            table = torch.frombuffer(bytearray(raw), dtype=torch.uint8).to(device) if jobs else None
            self.plan = (table, len(jobs), blocks, live, device)
        table, njobs, blocks, _, _ = self.plan
        if njobs:
            _check(lib.bl_pack_weights_multi(table.data_ptr(), njobs, blocks, _stream()), "bl_pack_weights_multi")
        for e, W in alive:
            e["version"], e["epoch"] = W._version, _weights_epoch


_weight_copies = _WeightCopies()


def _packed_layer_weights(W: torch.Tensor, need_bwd: bool):
    """bf16x3-packed, tiled copies of a layer's weights: the forward form (C = A . W[t]) and, when asked for, the form of the
    input-gradient GEMM (C = G . W[t]^T).  A 2-D weight (the dense node update's Wd [Dm, Dout]) is one group."""
    got = _weight_copies.get(W, ("kn", "nk") if need_bwd else ("kn",))
    return got[0], (got[1] if need_bwd else None)


def _packed_message_weights(W: torch.Tensor, Din: int, need_bwd: bool):
    """The per-type message weights W [T, 2 Din, Dm] in the images the fused layer calls expect (bl_mp_layer_weight_image): the wide
    row GEMM's image where that kernel takes the shape, the tiled one otherwise."""
    lib = load_library()
    Dm = W.shape[2]
    suffix = ("", "w", "h")  # bl_mp_layer_weight_image: 0 = 128 x 128 bf16x6 image, 1 = wide bf16x6 image, 2 = f16x3 image
    fwd = "kn" + suffix[int(lib.bl_mp_layer_weight_image(int(Din), int(Dm), 0))]
    if not need_bwd:
        return _weight_copies.get(W, (fwd,))[0], None
    bwd = "nk" + suffix[int(lib.bl_mp_layer_weight_image(int(Din), int(Dm), 1))]
    got = _weight_copies.get(W, (fwd, bwd))
    return got[0], got[1]


def _transposed_layer_weights(W: torch.Tensor) -> torch.Tensor:
    return _weight_copies.get(W, ("t",))[0]

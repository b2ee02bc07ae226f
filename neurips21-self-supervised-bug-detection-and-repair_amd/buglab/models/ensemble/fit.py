"""Fitting a `weighted` ensemble on held-out data -- BEYOND THE REFERENCE, which has no counterpart.

The validation data runs ONCE through the ensemble's own minibatches (`EnsembleWrapper._minibatches`, what `predict` forms);
every member's flat output is gathered into the canonical layout on the device (torch indexing: plumbing) and appended to a
device pool.  The fit (buglab/models/ensemble/_weights.py::fit_weights: projected BFGS, the same optimiser code whoever computes
the statistics) then costs one launch per head (hip_ops.ens_loc_stats / ens_rw_stats, csrc/bl_ensemble_fit.hip) and one copy of
1 + 2M (1 + M) doubles per objective evaluation.  The targets come from the datapoints as `_calibrate.calibration_indices`
and the evaluation path take them: the place of the target rewrite's reference node among np.unique(reference_nodes), NO_BUG's
place (the last) for a sample without a bug, and the target rewrite's original index."""
from __future__ import annotations

import logging
from contextlib import ExitStack
from typing import Any, Dict, Iterable, List, Optional

import numpy as np

from buglab.models.ensemble import _weights as W
from buglab.models.ensemble._weights import EnsembleWeights

LOGGER = logging.getLogger(__name__)


class CollectedEnsemblePool:
    """One pass of the validation data: the two device pools the fit reads."""

    def __init__(self, num_members: int, device):
        import torch

        self.device = torch.device(device)
        self.M = int(num_members)
        self._loc_vals, self._loc_present, self._rw_vals, self._rw_present = [], [], [], []
        self._loc_len: List[np.ndarray] = []
        self._loc_tgt: List[np.ndarray] = []
        self.loc = self.rw = None  # (vals, present, off, tgt) / (vals, present) on the device, after `close`
        self.num_samples = self.num_buggy = 0

    def add(self, src, emb) -> None:
        """`src`: the present members' flat outputs of the ensemble minibatch `emb`, concatenated."""
        import torch

        from buglab.controllers._batching import to_device_i32

        M, total_loc, total_rw, B = emb.sizes
        assert M == self.M
        ix = emb.index
        a, c = M * total_loc, M * total_loc + M * total_rw
        loc_idx, rw_idx = ix[:a].view(M, total_loc).long(), ix[a:c].view(M, total_rw).long()
        n_loc = np.diff(emb.loc_off)
        tgt_loc, tgt_rw = np.empty(B, np.int64), []
        for b, point in enumerate(emb.originals):
            target = point["target_fix_action_idx"]
            if target is None:
                tgt_loc[b] = n_loc[b] - 1
                continue
            nodes, place = np.unique(np.asarray(point["graph"]["reference_nodes"], dtype=np.int64), return_inverse=True)
            assert nodes.shape[0] + 1 == n_loc[b] and 0 <= int(target) < emb.rw_off[b + 1] - emb.rw_off[b]
            tgt_loc[b] = place[int(target)]
            tgt_rw.append((b, int(emb.rw_off[b]) + int(target)))
        i32 = lambda values: np.asarray(values, dtype=np.int32)
        first, buggy, rw_at = to_device_i32([i32(emb.loc_off[:-1]), i32([b for b, _ in tgt_rw]), i32([k for _, k in tgt_rw])], self.device)
        present = loc_idx[:, first.long()] >= 0  # [M, B]: a member's gather indices of a sample are all -1 or none
        self._loc_vals.append(src[loc_idx.clamp(min=0)])  # an absent member's entries are never read
        self._loc_present.append(present.to(torch.int32))
        self._loc_len.append(n_loc.astype(np.int32))
        self._loc_tgt.append(tgt_loc.astype(np.int32))
        if tgt_rw:
            self._rw_vals.append(src[rw_idx[:, rw_at.long()].clamp(min=0)])
            self._rw_present.append(present[:, buggy.long()].to(torch.int32))

    def close(self) -> None:
        import torch

        from buglab.controllers._batching import to_device_i32

        M, dev = self.M, self.device
        lens = np.concatenate(self._loc_len) if self._loc_len else np.zeros(0, np.int32)
        tgt = np.concatenate(self._loc_tgt) if self._loc_tgt else np.zeros(0, np.int32)
        off = np.zeros(lens.shape[0] + 1, np.int64)
        np.cumsum(lens, out=off[1:])
        if M * int(off[-1]) > np.iinfo(np.int32).max:
            raise ValueError(f"fit_ensemble_weights: a pool of {M} x {int(off[-1])} entries is beyond int32 offsets; use "
                             "--limit-num-elements")
        off_d, tgt_d = to_device_i32([off, tgt], dev)
        cat = lambda parts, dtype: (torch.cat(parts, dim=1) if parts else torch.zeros((M, 0), dtype=dtype, device=dev)).contiguous()
        self.loc = (cat(self._loc_vals, torch.float32), cat(self._loc_present, torch.int32), off_d.contiguous(), tgt_d.contiguous())
        self.rw = (cat(self._rw_vals, torch.float32), cat(self._rw_present, torch.int32))
        self.num_samples, self.num_buggy = int(lens.shape[0]), int(self.rw[0].shape[1])
        self._loc_vals = self._loc_present = self._rw_vals = self._rw_present = None

    def host_pools(self):
        """The two pools copied to the host, as the twin reads them."""
        to = lambda t: t.cpu().numpy()
        return W.LocPool(*(to(t) for t in self.loc)), W.RwPool(*(to(t) for t in self.rw))


def collect_ensemble_pool(ensemble, nn, data: Iterable[Any], device, *, parallelize: bool = True) -> CollectedEnsemblePool:
    """Runs the ensemble's own minibatches once over `data`; the pools hold the members' RAW log-probabilities."""
    import torch

    from buglab.runtime.neuralmodel import ordered_map

    nns = list(nn.nns)
    models = ensemble.models
    if len(nns) != len(models):
        raise ValueError(f"{len(models)} ensemble members but {len(nns)} modules")
    for n in nns:
        n.eval()
    collected = CollectedEnsemblePool(len(models), device)
    with torch.no_grad(), ExitStack() as stack:
        for m in models:
            stack.enter_context(m._tensorize_all_location_rewrites())
        tensorized = ordered_map(ensemble._tensorize_all, data, parallelize)
        for emb in ensemble._minibatches(tensorized, device, parallelize):
            flats = [ensemble._member_flat_output(nn_, mb) for nn_, mb in zip(nns, emb.members) if mb is not None]
            assert [int(f.shape[0]) for f in flats] == emb.flat_sizes
            collected.add((torch.cat(flats) if len(flats) > 1 else flats[0]).contiguous(), emb)
    collected.close()
    return collected


def fit_on_device(collected: CollectedEnsemblePool, *, fit_temperature: bool = True):
    """The fit with the device's statistics: per objective evaluation one launch per head and one small copy.
    -> (EnsembleWeights, details)."""
    from buglab.models import hip_ops

    loc_present = (collected.loc[1] != 0).any(dim=1).cpu().numpy()
    rw_present = (collected.rw[1] != 0).any(dim=1).cpu().numpy()
    loc_fn = lambda theta, beta: hip_ops.ens_loc_stats(*collected.loc, theta, beta).cpu().numpy()
    rw_fn = lambda phi: hip_ops.ens_rw_stats(*collected.rw, phi).cpu().numpy()
    return W.fit_weights(loc_fn, collected.num_samples, loc_present, rw_fn, collected.num_buggy, rw_present,
                         fit_temperature=fit_temperature)


def fit_ensemble_weights(ensemble, nn, data: Iterable[Any], device, *, fit_temperature: bool = True, parallelize: bool = True,
                         host_fit: bool = False, report: Optional[Dict[str, Any]] = None) -> EnsembleWeights:
    """Fits the `EnsembleWeights` of the `weighted` ensemble (ensemble, nn) on `data` and stores them on `ensemble`.  `host_fit`:
    the statistics of every optimiser step come from the NumPy twin on a host copy of the pool instead of from the device (the
    members' forward passes run on the device either way).  `report`, when given, is filled with the parameters and the fit's
    details."""
    if ensemble.kind != "weighted":
        raise ValueError(f"fit_ensemble_weights needs a `weighted` ensemble (got `{ensemble.kind}`).")
    collected = collect_ensemble_pool(ensemble, nn, data, device, parallelize=parallelize)
    if collected.num_samples == 0:
        raise ValueError("fit_ensemble_weights: no sample of the data could be tensorised by any member")
    if host_fit:
        weights, details = W.fit_host(*collected.host_pools(), fit_temperature=fit_temperature)
    else:
        weights, details = fit_on_device(collected, fit_temperature=fit_temperature)
    ensemble.ensemble_weights = weights
    if report is not None:
        w_loc, w_rw = weights.member_weights()
        report.update({"weights": {**weights._asdict(), "notes": list(weights.notes)}, "num_samples": collected.num_samples,
                       "num_buggy": collected.num_buggy, "host_fit": bool(host_fit), "location_weight": w_loc.tolist(),
                       "rewrite_weight": w_rw.tolist(), "fit": details})
    return weights


def format_report(report: Dict[str, Any]) -> str:
    w = report["weights"]
    lines = [f"Fitted on {report['num_samples']} samples ({report['num_buggy']} buggy)"
             f"{' with the statistics of the host twin' if report['host_fit'] else ''}."]
    for m, (wl, wr, beta) in enumerate(zip(report["location_weight"], report["rewrite_weight"], w["beta"])):
        lines.append(f"  member {m}: location weight {wl:.6f}, rewrite weight {wr:.6f}, temperature {1.0 / beta:.6g} (beta {beta:.6g})")
    lines += [f"  note: {note}" for note in w["notes"]]
    for title, k in (("localization NLL per sample", 0), ("rewrite NLL per buggy sample", 1)):
        lines.append(f"  {title}: avg {w['nll_before'][k]:.6f} -> weighted {w['nll_after'][k]:.6f}")
    return "\n".join(lines) + "\n"

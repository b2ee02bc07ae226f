#!/usr/bin/env python
"""
Usage:
    python -m buglab.models.calibrate MODEL_FILENAME VALID_DATA_PATH OUT_MODEL_FILENAME [--limit-num-elements N] [--sequential]
                                      [--no-bias] [--no-repair] [--num-bins 15] [--report-json FILE]

Confidence calibration of a trained detector on held-out data -- BEYOND THE REFERENCE, which has no counterpart.  The
confidence the reference's evaluate.py thresholds, its visualize.py ranks by, the detector scores of the self-supervision
records and the `avg` ensemble's probabilities are all exp() of the log-probabilities `predict` yields; nothing in training
makes a reported 0.9 mean "right nine times in ten", and the NO_BUG entry's balance against the candidate locations (the
false-positive rate) moves with `buggy_samples_weight_spec` and the bug-free share of the training data.  This fits, without
retraining, one inverse temperature and a NO_BUG bias for the localization distribution and one inverse temperature for the
repair groups (buglab/models/_calibrate.py has the arithmetic) and writes a checkpoint that carries them: `predict`,
`evaluate` (both paths), `visualize`, `bugselector` and `detectorscoring` then see calibrated values.

The validation data runs ONCE through the minibatches of the model's own `predict`; every minibatch's raw flat output stays on
the device and its location segments and target repair groups are appended to a device pool.  The fit is a damped Newton
iteration whose every step is one launch over the pool (hip_ops.conf_loc_stats / conf_group_stats, csrc/bl_confidence.hip) and
a copy of six (three) doubles.  Printed: the parameters, the negative log-likelihood per sample and the expected calibration
error before and after -- the ECE over equal-width bins of the confidence `evaluate` uses against `location_correct`, both
from hip_ops.eval_judge on the raw and on the calibrated outputs, binned on the host after one copy.
"""
from __future__ import annotations

import argparse
import logging
import sys
from pathlib import Path
from typing import Any, Dict, Iterable, List, NamedTuple, Optional

if __package__ in (None, ""):
    sys.path.insert(0, str(Path(__file__).resolve().parents[2]))

import numpy as np

from buglab.models import _calibrate as K
from buglab.models._calibrate import ConfidenceCalibration

LOGGER = logging.getLogger(__name__)


class _Minibatch(NamedTuple):
    flat: Any           # the raw flat output, float32, on the device
    eval_ix: Dict[str, Any]
    candidate_ptr: Any
    repair_group_ptr: Any
    repair_group_items: Any
    num_samples: int


class CollectedPool:
    """One pass of the validation data: the device pools the fit reads and what the before / after report needs."""

    def __init__(self, device):
        import torch

        self.device = torch.device(device)
        self.minibatches: List[_Minibatch] = []
        self._loc_vals, self._rw_vals = [], []
        self._loc_len: List[np.ndarray] = []
        self._loc_tgt: List[np.ndarray] = []
        self._rw_len: List[np.ndarray] = []
        self._rw_tgt: List[np.ndarray] = []
        self.loc = self.rw = None  # (vals, off, tgt) on the device, after `close`
        self.num_samples = self.num_bug_free = self.num_buggy = 0

    def add(self, flat, mb) -> None:
        ss = mb["selfsup"]
        ix: K.CalibrationIndices = ss["calibration"]
        self._loc_vals.append(flat[ss["loc_gather"].long()])
        self._rw_vals.append(flat[ss["rw_gather"].long()])
        self._loc_len.append(ix.loc_len), self._loc_tgt.append(ix.loc_tgt)
        self._rw_len.append(ix.rw_len), self._rw_tgt.append(ix.rw_tgt)
        self.minibatches.append(_Minibatch(flat, ss["ix"], mb["graph_data"]["candidate_ptr"], mb["repair_group_ptr"],
                                           mb["repair_group_items"], int(ix.loc_len.shape[0])))

    def close(self) -> None:
        import torch

        from buglab.controllers._batching import to_device_i32

        def pool(vals, lens, tgts):
            lens = np.concatenate(lens) if lens else np.zeros(0, np.int32)
            tgt = np.concatenate(tgts) if tgts else np.zeros(0, np.int32)
            off = np.zeros(lens.shape[0] + 1, np.int64)
            np.cumsum(lens, out=off[1:])
            if off[-1] > np.iinfo(np.int32).max:
                raise ValueError(f"calibrate: a pool of {int(off[-1])} entries is beyond int32 offsets; use --limit-num-elements")
            off_d, tgt_d = to_device_i32([off, tgt], self.device)
            v = torch.cat(vals) if vals else torch.zeros(0, dtype=torch.float32, device=self.device)
            return v.contiguous(), off_d.contiguous(), tgt_d.contiguous()

        self.loc = pool(self._loc_vals, self._loc_len, self._loc_tgt)
        self.rw = pool(self._rw_vals, self._rw_len, self._rw_tgt)
        lens = np.concatenate(self._loc_len) if self._loc_len else np.zeros(0, np.int32)
        tgt = np.concatenate(self._loc_tgt) if self._loc_tgt else np.zeros(0, np.int32)
        self.num_samples = int(lens.shape[0])
        self.num_bug_free = int(np.sum(tgt == lens - 1))
        self.num_buggy = int(sum(x.shape[0] for x in self._rw_len))
        self._loc_vals = self._rw_vals = None

    def host_pools(self):
        """The two pools copied to the host, as the twin reads them."""
        to = lambda t: t.cpu().numpy()
        return K.Pool(*(to(t) for t in self.loc)), K.Pool(*(to(t) for t in self.rw))


def collect_calibration_pool(model, nn, data: Iterable[Any], device, *, parallelize: bool = False) -> CollectedPool:
    """Runs `prediction_minibatches` once over `data` with the model's own calibration (if any) set aside: the pools hold RAW
    log-probabilities."""
    import torch

    from buglab.controllers import _batching as Bt
    from buglab.models import _evaluate as E
    from buglab.models import hip_ops

    Bt.require_single_model(model, "calibrate_model")
    device = torch.device(device)
    collected = CollectedPool(device)

    def extend(layout, points, dev, mb):
        ss = Bt.selfsup_indices(layout, points)
        ix = K.calibration_indices(layout, points, ss.tgt_loc)
        ev = E.eval_indices(layout, points, mb.get("node_mappings"))
        names = ("loc_gather", "rw_gather") + tuple(hip_ops.EVAL_INDEX_FIELDS)
        arrays = [ix.loc_gather, ix.rw_gather] + [getattr(ev, f) for f in hip_ops.EVAL_INDEX_FIELDS]
        dev_arrays = dict(zip(names, Bt.to_device_i32(arrays, dev)))
        return {"calibration": ix, "loc_gather": dev_arrays.pop("loc_gather"), "rw_gather": dev_arrays.pop("rw_gather"),
                "ix": dev_arrays}

    previous = model.confidence_calibration
    if previous is not None:
        LOGGER.info("The model's existing calibration %s is ignored while collecting and will be replaced.", previous)
    nn.eval()
    try:
        model.confidence_calibration = None
        with torch.no_grad(), model._tensorize_all_location_rewrites():
            for mb, _tags in Bt.prediction_minibatches(model, ((d, None) for d in data), device, parallelize, extend,
                                                       lambda tag: None, extend_sees_minibatch=True):
                collected.add(Bt.flat_prediction_output(nn, mb), mb)
    finally:
        model.confidence_calibration = previous
    collected.close()
    return collected


def fit_on_device(collected: CollectedPool, *, fit_bias: bool = True, fit_repair: bool = True):
    """The Newton fit with the device's stats: one launch and one copy of six (three) doubles per evaluation.
    -> (ConfidenceCalibration, details)."""
    from buglab.models import hip_ops

    loc_fn = lambda beta, bias: hip_ops.conf_loc_stats(*collected.loc, beta, bias).cpu().numpy()
    group_fn = lambda beta: hip_ops.conf_group_stats(*collected.rw, beta).cpu().numpy()
    return K.fit_calibration(loc_fn, collected.num_samples, collected.num_bug_free, group_fn, collected.num_buggy,
                             fit_bias=fit_bias, fit_repair=fit_repair)


def judged_confidence(collected: CollectedPool, cal: Optional[ConfidenceCalibration]):
    """(confidence = exp of what `evaluate` thresholds, location_correct) of every collected sample under `cal` (None: raw), from
    hip_ops.eval_judge; one copy back."""
    import torch

    from buglab.models import hip_ops

    n = collected.num_samples
    blob = torch.empty(3 * max(n, 1), dtype=torch.float64, device=collected.device)
    cap = max(n, 1)
    conf, verdict = blob[:cap], blob[cap:].view(torch.int32).view(4, cap)
    at = 0
    for mb in collected.minibatches:
        flat = mb.flat
        if cal is not None and not cal.is_identity:
            flat = flat.clone()
            hip_ops.conf_apply(flat, mb.candidate_ptr, mb.num_samples, mb.repair_group_ptr, mb.repair_group_items, beta=cal.beta,
                               no_bug_bias=cal.no_bug_bias, repair_beta=cal.repair_beta)
        hip_ops.eval_judge(flat, mb.eval_ix, conf, verdict, at)
        at += mb.num_samples
    host = blob.cpu()
    return np.exp(host[:cap][:n].numpy()), host[cap:].view(torch.int32).view(4, cap)[1, :n].numpy() != 0


def drop_operating_point(model) -> bool:
    """A warning operating point (buglab/models/operatingpoint.py) is a threshold on the confidences the model reported when
    it was fitted; a new calibration changes those, so the point is dropped, with one warning.  -> whether there was one."""
    point = getattr(model, "warning_operating_point", None)
    if point is None:
        return False
    LOGGER.warning("The model's warning operating point %s was fitted on other confidences and is dropped; fit it again on the "
                   "calibrated model (python -m buglab.models.operatingpoint).", point)
    model.warning_operating_point = None
    return True


def calibrate_model(model, nn, data: Iterable[Any], device, *, parallelize: bool = False, fit_bias: bool = True,
                    fit_repair: bool = True, num_bins: int = 15, report: Optional[Dict[str, Any]] = None) -> ConfidenceCalibration:
    """Fits a `ConfidenceCalibration` for (model, nn) on `data` on the device and stores it on `model` (replacing an earlier
    one).  `report`, when given, is filled with the parameters, the negative log-likelihood per sample and the expected
    calibration error before and after, and the fit's details."""
    from buglab.models import hip_ops

    collected = collect_calibration_pool(model, nn, data, device, parallelize=parallelize)
    if collected.num_samples == 0:
        raise ValueError("calibrate_model: no sample of the data could be tensorised")
    cal, details = fit_on_device(collected, fit_bias=fit_bias, fit_repair=fit_repair)
    model.confidence_calibration = cal
    drop_operating_point(model)
    if report is not None:
        n, nb = collected.num_samples, collected.num_buggy
        loss = lambda beta, bias: float(hip_ops.conf_loc_stats(*collected.loc, beta, bias)[0]) / n
        rloss = lambda beta: float(hip_ops.conf_group_stats(*collected.rw, beta)[0]) / nb if nb else float("nan")
        ece = {}
        for name, c in (("before", None), ("after", cal)):
            confidence, correct = judged_confidence(collected, c)
            ece[name], bins = K.expected_calibration_error(confidence, correct, num_bins)
            ece[name + "_bins"] = bins
        report.update({
            "calibration": {**cal._asdict(), "notes": list(cal.notes)}, "num_samples": n, "num_bug_free": collected.num_bug_free,
            "num_buggy": nb, "localization_nll": {"before": loss(1.0, 0.0), "after": loss(cal.beta, cal.no_bug_bias)},
            "repair_nll": {"before": rloss(1.0), "after": rloss(cal.repair_beta)},
            "ece": {"before": ece["before"], "after": ece["after"], "num_bins": num_bins},
            "reliability": {"before": ece["before_bins"], "after": ece["after_bins"]}, "fit": details})
    return cal


def format_report(report: Dict[str, Any]) -> str:
    c = report["calibration"]
    lines = [
        f"Calibrated on {report['num_samples']} samples ({report['num_bug_free']} bug-free, {report['num_buggy']} buggy).",
        f"  temperature {1.0 / c['beta']:.6g} (beta {c['beta']:.6g}), NO_BUG bias {c['no_bug_bias']:.6g}, "
        f"repair temperature {1.0 / c['repair_beta']:.6g} (beta {c['repair_beta']:.6g}), converged: {c['converged']}",
    ]
    lines += [f"  note: {note}" for note in c["notes"]]
    for title, key in (("localization NLL per sample", "localization_nll"), ("repair NLL per buggy sample", "repair_nll"),
                       (f"expected calibration error ({report['ece']['num_bins']} bins)", "ece")):
        lines.append(f"  {title}: {report[key]['before']:.6f} -> {report[key]['after']:.6f}")
    return "\n".join(lines) + "\n"


def parse_args(argv=None) -> argparse.Namespace:
    p = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    p.add_argument("MODEL_FILENAME", help="A trained detector checkpoint (`*.pkl.gz`).")
    p.add_argument("VALID_DATA_PATH", help="Held-out `*.msgpack.l.gz` data: a file or a folder.")
    p.add_argument("OUT_MODEL_FILENAME", help="Where to write the checkpoint that carries the calibration.")
    p.add_argument("--limit-num-elements", type=int, default=None, help="Fit on at most this many samples.")
    p.add_argument("--sequential", action="store_true", help="Do not parallelize data loading.")
    p.add_argument("--no-bias", action="store_true", help="Fit the temperature only; leave the NO_BUG bias at 0.")
    p.add_argument("--no-repair", action="store_true", help="Leave the repair log-probabilities as they are.")
    p.add_argument("--num-bins", type=int, default=15, help="Bins of the expected calibration error.")
    p.add_argument("--report-json", default=None, help="Also write the report as data.")
    return p.parse_args(argv)


def run(args: argparse.Namespace) -> ConfidenceCalibration:
    from buglab.models._cli import open_model, require_gpu, write_report_json
    from buglab.runtime.richpath import RichPath
    from buglab.utils.msgpackutils import load_all_msgpack_l_gz

    require_gpu(None, "calibrate")
    model, nn, device, _ = open_model(args.MODEL_FILENAME)
    data = load_all_msgpack_l_gz(RichPath.create(args.VALID_DATA_PATH), shuffle=True, limit_num_yielded_elements=args.limit_num_elements)
    report: Dict[str, Any] = {}
    cal = calibrate_model(model, nn, data, device, parallelize=not args.sequential, fit_bias=not args.no_bias,
                          fit_repair=not args.no_repair, num_bins=args.num_bins, report=report)
    model.save(Path(args.OUT_MODEL_FILENAME), nn)
    sys.stdout.write(format_report(report))
    write_report_json(args.report_json, report)
    return cal


if __name__ == "__main__":
    logging.basicConfig(level=logging.INFO)
    run(parse_args())

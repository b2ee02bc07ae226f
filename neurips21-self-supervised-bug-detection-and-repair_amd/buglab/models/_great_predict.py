"""NumPy twin of the GREAT prediction head's per-sample pass (csrc/bl_varmisuse_predict.hip::vm_predict_samples), in float64:
the contract of include/buglab_hip.h::bl_varmisuse_predict applied to masked logits that are already on the host.  Used by
`evaluate_great(..., on_device=False)` (buglab/models/evaluategreat.py) and by the tests; never on the hot path."""
from __future__ import annotations

from typing import Tuple

import numpy as np

RECORD_D, RECORD_I = 7, 4  # rows of out_d / out_i


def _first_max(v: np.ndarray) -> Tuple[float, int]:
    """(maximum, first index that holds it) over fp32 values; a NaN never wins.  (-inf, -1) if nothing is above -inf."""
    if v.shape[0] == 0:
        return -np.inf, -1
    w = np.where(np.isnan(v), np.float32(-np.inf), v)
    i = int(np.argmax(w))  # first maximum
    return (float(w[i]), i) if w[i] > -np.inf else (-np.inf, -1)


def _lse(v: np.ndarray, m: float) -> float:
    """max + log(sum exp(double(v) - double(max))); -inf where there is no maximum."""
    if m == -np.inf:
        return -np.inf
    with np.errstate(invalid="ignore", over="ignore"):
        return m + float(np.log(np.sum(np.exp(v.astype(np.float64) - m))))


def judge_great_host(logits, L: int, lens_att, error_location, target_mask) -> Tuple[np.ndarray, np.ndarray]:
    """logits fp32 [B * L, 2] (masked: -inf at positions >= lens_att, the pointer column also at non-candidates), lens_att /
    error_location int [B], target_mask [B * L] or [B, L] -> (out_d float64 [7, B], out_i int32 [4, B]), the record of
    bl_varmisuse_predict for every sample."""
    logits = np.asarray(logits, dtype=np.float32)
    L = int(L)
    lg = logits.reshape(-1, L, 2)
    B = lg.shape[0]
    lens_att = np.asarray(lens_att).reshape(B)
    error_location = np.asarray(error_location).reshape(B)
    target = np.asarray(target_mask).reshape(B, L) != 0
    out_d = np.empty((RECORD_D, B), dtype=np.float64)
    out_i = np.empty((RECORD_I, B), dtype=np.int32)
    with np.errstate(invalid="ignore"):  # -inf - -inf = NaN where the contract says so
        for b in range(B):
            la = min(max(int(lens_att[b]), 0), L)
            loc, ptr, tgt = lg[b, :la, 0], lg[b, :la, 1], target[b, :la]
            m0, i0 = _first_max(loc)
            m1, i1 = _first_max(ptr)
            cand = ptr != -np.inf  # what the pointer sums run over (a NaN among them makes them NaN, as on the device)
            m2, _ = _first_max(np.where(tgt, ptr, np.float32(-np.inf)))
            lse0, lse1, lse2 = _lse(loc, m0), _lse(ptr[cand], m1), _lse(ptr[cand & tgt], m2)
            pred = max(i0, 0)
            err = int(error_location[b])
            out_d[0, b], out_d[1, b] = lse0, lse1
            out_d[2, b] = np.float64(lg[b, pred, 0]) - lse0
            out_d[3, b] = np.float64(lg[b, 0, 0]) - lse0
            out_d[4, b] = np.float64(lg[b, err, 0]) - lse0 if 0 <= err < la else -np.inf
            out_d[5, b] = np.float64(lg[b, i1, 1]) - lse1 if i1 >= 0 else np.nan
            out_d[6, b] = lse2 - lse1 if m2 > -np.inf else -np.inf
            out_i[0, b], out_i[1, b] = pred, i1
            out_i[2, b] = int(pred == err)
            out_i[3, b] = int(i1 >= 0 and bool(target[b, i1]))
    return out_d, out_i

"""Weight averaging in NumPy fp64: the twin of the EMA half of csrc/bl_head_ops.hip's adam_clip_kernel<true>, and the one place
that says which decay an update runs with.  No GPU, no library.

The k-th update of the average (k = 1, 2, ...) runs with the decay
    d_k = min(decay, (1 + k) / (10 + k))
-- the usual warm-up: a freshly started average follows the parameters (d_1 = 2/11) instead of remembering the initial weights
for 1 / (1 - decay) steps; d_k grows monotonically and stays at `decay` once it gets there.  The host computes d_k in Python
floats, rounds 1 - d_k to fp32 ONCE and hands that one number to the kernel, which does
    ema = fma(omd, p_new - ema, ema)
per element: one rounding in the subtraction, one in the fma."""
from __future__ import annotations

import numpy as np


def validate_decay(decay) -> float:
    """-> float(decay) if 0 < decay < 1, ValueError otherwise (NaN included)."""
    d = float(decay)
    if not (0.0 < d < 1.0):
        raise ValueError(f"ema decay must lie strictly between 0 and 1 (got {decay!r})")
    return d


def ema_decay_at(k: int, decay: float) -> float:
    """The decay of the k-th update of the average, k = 1, 2, ..."""
    if k < 1:
        raise ValueError(f"ema_decay_at: updates are counted from 1 (got {k})")
    return min(float(decay), (1.0 + k) / (10.0 + k))


def one_minus_decay_f32(k: int, decay: float) -> float:
    """1 - d_k rounded to fp32 once (returned as the Python float of that fp32 value): what the kernel is given."""
    return float(np.float32(1.0 - ema_decay_at(k, decay)))


def ema_update_twin(ema, p_new, one_minus_decay) -> np.ndarray:
    """ema + omd * (p_new - ema) in fp64."""
    ema = np.asarray(ema, dtype=np.float64)
    p_new = np.asarray(p_new, dtype=np.float64)
    return ema + float(one_minus_decay) * (p_new - ema)

"""Library-wide modes of libbuglab_hip.so: thin setters / getters over the C ABI."""
from __future__ import annotations

import os

from . import _switches
from ._cabi import load_library

__all__ = ["set_deterministic", "_MSG_GEMM_MODES", "set_msg_gemm_mode", "msg_gemm_mode", "set_seq_gemm_mode", "seq_gemm_mode", "set_wgrad_tile",
           "set_wgrad_kchunk_cap", "set_fused_node_bwd", "set_run_rows", "set_live_backward", "live_backward", "set_live_forward", "live_forward",
           "deterministic"]


def set_deterministic(on: bool = True) -> None:
    """Bit-reproducible gradients (ordered flushes instead of free-running atomics; slower).  BL_DETERMINISTIC=1 in the
    environment does the same for this process AND the loader processes (the collator must keep every token's
    occurrences in one chunk); this call only reaches the collators of this process."""
    load_library().bl_set_deterministic(1 if on else 0)
    os.environ["BL_DETERMINISTIC"] = "1" if on else "0"


_MSG_GEMM_MODES = ("bf16x6", "f16x3", "f16x1")


def set_msg_gemm_mode(mode: str) -> str:
    """'f16x3' (default), 'bf16x6' or 'f16x1': the operand split of the message GEMMs inside the fused layer calls
    (bl_set_msg_gemm_mode).  'f16x1' is the reduced-precision mode of `train.py --amp` (reference train.py:8,106: autocast): the
    f16x3 images with the high-plane term only -- fp16 operands, fp32 accumulation, fp32 results; outside the 1e-4 parity bound
    by construction and never the benchmarked headline.  Returns the previous mode.  Not to be switched between a forward pass
    and its backward pass."""
    if mode not in _MSG_GEMM_MODES:
        raise ValueError(f"mode must be one of {_MSG_GEMM_MODES}")
    prev = load_library().bl_set_msg_gemm_mode(_MSG_GEMM_MODES.index(mode))
    return _MSG_GEMM_MODES[prev]


def msg_gemm_mode() -> str:
    return _MSG_GEMM_MODES[load_library().bl_get_msg_gemm_mode()]


def set_seq_gemm_mode(mode: str) -> str:
    """'bf16x6' (default) or 'bf16x1': the operand split of the packed-row GEMMs behind the sequence models' Linear layers (QKV,
    output, linear1 / linear2 and seq-gru's input projections; forward, input gradient, weight gradient; op by op and inside the
    one-call GREAT layer -- bl_set_seq_gemm_mode).  'bf16x1' is the reduced-precision mode of `train.py --amp` for those models
    (reference train.py:8,106: autocast): the bf16x3 images with the high planes only -- bf16 operands, fp32 accumulation, fp32
    results; attention, LayerNorm, heads, losses and the optimiser stay fp32.  Outside the 1e-4 parity bound by construction and
    never the benchmarked headline.  Returns the previous mode.  A backward pass runs in the mode of its forward pass whatever
    the switch says by then (the autograd Functions capture it)."""
    if mode not in _switches._SEQ_GEMM_MODES:
        raise ValueError(f"mode must be one of {_switches._SEQ_GEMM_MODES}")
    prev = load_library().bl_set_seq_gemm_mode(_switches._SEQ_GEMM_MODES.index(mode))
    return _switches._SEQ_GEMM_MODES[prev]


def seq_gemm_mode() -> str:
    return _switches._SEQ_GEMM_MODES[load_library().bl_seq_gemm_mode()]


def set_wgrad_tile(rows: int) -> int:
    """256 (default): wide weight-gradient tile where it applies; 128: the 128 x 128 tile everywhere.  -> previous value."""
    return int(load_library().bl_set_wgrad_tile(int(rows)))


def set_wgrad_kchunk_cap(rows: int) -> int:
    """Most rows a workgroup of the bf16x6 weight-gradient GEMMs reduces per output-tile flush.  -> previous value."""
    return int(load_library().bl_set_wgrad_kchunk_cap(int(rows)))


def set_fused_node_bwd(on: bool) -> bool:
    """A/B switch: the node update's backward chain of the fused layer call as one kernel (default) or three.  -> previous."""
    return bool(load_library().bl_set_fused_node_bwd(1 if on else 0))


def set_run_rows(on: bool) -> bool:
    """A/B switch (BL_RUN_ROWS=0 starts with it off): backward of the fused layer call computes the target halves of the routed
    f16x3 gradients once per run of messages (default) or once per message, on the same arrays.  -> previous."""
    return bool(load_library().bl_set_run_rows(1 if on else 0))


def set_live_backward(on: bool) -> bool:
    """A/B switch (BL_LIVE_BWD=0 starts with it off): backward of the fused layer call runs over the live rows of a descriptor that
    carries them (GraphIndex.live: the rows the heads' gather can reach) or over all rows.  Off, GnnBugLabModule does not hand the
    live arrays to the layers either and keeps its full output attached.  -> previous."""
    return bool(load_library().bl_set_live_backward(1 if on else 0))


def live_backward() -> bool:
    return bool(load_library().bl_get_live_backward())


def set_live_forward(on: bool) -> bool:
    """A/B switch (BL_LIVE_FWD=0 starts with it off): the last layers run their FORWARD over their live rows too, where the library's
    one predicate (bl_mp_layer_live_ok) says they can; it applies only where the live backward is on.  Off, every kernel and launch is
    as without it.  -> previous."""
    return bool(load_library().bl_set_live_forward(1 if on else 0))


def live_forward() -> bool:
    return bool(load_library().bl_get_live_forward())


def deterministic() -> bool:
    return bool(load_library().bl_get_deterministic())

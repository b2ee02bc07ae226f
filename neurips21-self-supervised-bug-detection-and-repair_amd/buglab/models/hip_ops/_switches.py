"""The Python-level A/B switches of buglab.models.hip_ops: ONE copy of each, here.

Tests, bench.py and the tools flip them on the package (`hip_ops.FUSED_LAYER = False`): the package forwards reads and
assignments of every name in `__all__` to this module (hip_ops/__init__.py::_HipOpsModule).  Every module of the package reads
`_switches.NAME` at call time -- never `from ._switches import NAME`, which would freeze a copy the assignment no longer reaches."""
from __future__ import annotations

import os
from typing import Optional

__all__ = ["WINNER_SINK", "GEMM_MODE", "WGRAD_X6", "FUSED_LAYER", "DENSE_X6", "DGRAD_VEC", "INFERENCE_MODE", "LINEAR_X6", "LINEAR_X6_MIN_ROWS",
           "FUSED_LOSS", "FUSED_ATTENTION", "FUSED_GREAT_LAYER", "GRAD_READY_CALLBACK", "USE_SIDE_STREAM", "DIRECT_PARAM_GRAD",
           "SIDE_STREAM_PRIORITY"]

# Debug tap for the parity tests: when set to a list, every message-passing layer's forward appends its
# winner table (int32 [N, Dm]: id of the message that won each channel's max at each node, -1 = none).
WINNER_SINK: Optional[list] = None

# fp32-accurate GEMM on the bf16 matrix cores (csrc/bl_gemm_x6.hip)
GEMM_MODE = os.environ.get("BL_GEMM_MODE", "bf16x6")  # "bf16x6" | "fp32"
WGRAD_X6 = os.environ.get("BL_WGRAD_X6", "1") != "0"   # bf16x6 weight gradient of the message layers

# Operand splits of the sequence models' projection GEMMs, in the order of bl_set_seq_gemm_mode's codes (the mode itself lives in
# the library: hip_ops.set_seq_gemm_mode / seq_gemm_mode in runtime.py; BL_SEQ_GEMM=bf16x1 sets the initial value there)
_SEQ_GEMM_MODES = ("bf16x6", "bf16x1")

# One C call per message-passing layer and direction (bl_mp_layer_fwd / bl_mp_layer_bwd).
FUSED_LAYER = os.environ.get("BL_FUSED_LAYER", "1") != "0"

# The dense node update (LayerNorm -> Linear -> tanh -> Dropout) as bf16x6 GEMMs too (forward, input gradient, weight
# gradient); BL_DENSE_X6=0: exact-fp32 MFMA GEMMs.
DENSE_X6 = os.environ.get("BL_DENSE_X6", "1") != "0"

# The routed input gradient of a message-passing layer from the NON-ZEROS of the message gradient, on the vector units, node
# sums fused in (csrc/bl_routed_dgrad.hip), instead of the matrix-core GEMM over all E x Dm entries + bl_mp_scatter_grad.
# BL_DGRAD_VEC=0: matrix cores.  Needs W transposed ([T, Dm, 2 Din]); cached per parameter value like the packed forms.
# Default (BL_DGRAD_VEC unset): vector units while the message GEMMs run as bf16x6 (0.404 vs 0.550 ms per hidden-128 layer), matrix
# cores when they run as f16x3 -- the routed f16x3 GEMM + segmented sums cost the same exclusive time as the vector kernel + its
# sums (4.24 vs 4.33 ms per c2 step) and overlap better with the free-running weight gradients (the vector kernel holds a CU's
# whole LDS with one 1024-thread workgroup): 13.12 vs 13.68 ms per step (profiles/r06h_bench*.json).
DGRAD_VEC = {"1": True, "0": False}.get(os.environ.get("BL_DGRAD_VEC", ""), None)

INFERENCE_MODE = True  # forward-only form of the fused layer call when no input needs a gradient (A/B switch for tests)

# Plain Linear layers with many rows (the sequence models' QKV / output / feed-forward projections) on the bf16x6 path:
# packed input, epilogue-fused bias / activation / dropout, packed g_z from the activation backward, bf16x6 input and weight
# gradients.  BL_LINEAR_X6=0: exact-fp32 MFMA GEMMs.
LINEAR_X6 = os.environ.get("BL_LINEAR_X6", "1") != "0"
LINEAR_X6_MIN_ROWS = 1024

# loss assembly (csrc/bl_loss.hip): everything between the scorers' logits and the scalar loss in one kernel per direction
FUSED_LOSS = os.environ.get("BL_FUSED_LOSS", "1") != "0"

FUSED_ATTENTION = os.environ.get("BL_FUSED_ATTENTION", "1") != "0"  # seq-great: scores -> probabilities in one kernel
# (the three-valued streaming-attention switch, hip_ops.STREAMING_ATTENTION / BL_STREAMING_ATTENTION = auto | 1 | 0, is owned by
# seq.py, next to attention_path() which interprets it; the package forwards it there exactly as it forwards the names above here)

# one relational transformer encoder layer per C call (csrc/bl_great_layer.hip)
FUSED_GREAT_LAYER = os.environ.get("BL_FUSED_GREAT_LAYER", "1") != "0"  # A/B switch: 0 = the op-by-op path

# "the backward of this layer has been launched" notifications (data-parallel gradient buckets, runtime/optim.py): set through
# hip_ops.set_grad_ready_callback (graph.py), which also resets the use counts
GRAD_READY_CALLBACK = None

# side stream: weight-gradient GEMMs run next to the input-gradient chain of the same layer (both
# only read the node gradient), so one kernel's prologue / epilogue / last-round tail is filled by
# the other kernel's workgroups.  BL_SIDE_STREAM=0 disables.
USE_SIDE_STREAM = os.environ.get("BL_SIDE_STREAM", "1") != "0"
# Weight gradients of the message-passing layers are accumulated (fp32 atomics in the kernel)
# straight into `param.grad` for parameters whose owner OPTED IN (`param._bl_direct_grad = True`, set by
# FlatAdam, which pre-binds every .grad to a view of its flat gradient buffer), on the side stream, WITHOUT
# joining at the end of the layer's backward: the side stream runs one weight-gradient GEMM after the other
# behind the main chain and is joined once, by `join_side_stream()`, before the gradients are consumed
# (FlatAdam.zero_grad / .step).  Parameters of any other optimiser get ordinary autograd gradients, complete
# when backward() returns (the side stream is joined inside the layer's backward).
DIRECT_PARAM_GRAD = os.environ.get("BL_DIRECT_GRAD", "1") != "0"

# Priority of the side stream that carries the weight-gradient GEMMs (lower number = higher priority; out-of-range values are
# mapped to the nearest valid one).  BL_SIDE_STREAM_PRIORITY: A/B knob.
SIDE_STREAM_PRIORITY = int(os.environ.get("BL_SIDE_STREAM_PRIORITY", "0"))

# Switches whose one copy lives in the LIBRARY (a C call consults them, so a Python copy could only go stale); runtime.py holds their
# setters / getters, the environment variable sets the initial value there:
#   BL_MSG_GEMM   hip_ops.set_msg_gemm_mode / msg_gemm_mode      operand split of the message GEMMs
#   BL_SEQ_GEMM   hip_ops.set_seq_gemm_mode / seq_gemm_mode      operand split of the sequence models' projections
#   BL_RUN_ROWS   hip_ops.set_run_rows                           target halves of the routed gradients once per run
#   BL_LIVE_BWD   hip_ops.set_live_backward / live_backward      backward of the last layers over the rows the heads can reach
#                                                                (gnn.py asks live_backward() before it hands the live arrays on)
#   BL_LIVE_FWD   hip_ops.set_live_forward / live_forward        forward of those layers over the same rows (only where BL_LIVE_BWD is
#                                                                on; GraphNeuralNetwork.forward asks the library layer by layer)

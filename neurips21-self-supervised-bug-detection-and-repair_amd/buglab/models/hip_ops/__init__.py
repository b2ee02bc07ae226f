"""ctypes binding of libbuglab_hip.so (C ABI in include/buglab_hip.h) + torch.autograd wrappers.

This is the ONLY place the HIP kernels are called from.  There is no CPU fallback: importing works
anywhere (so host-side code can be tested without a GPU), but the first call that needs a kernel
raises `HipOpsUnavailable` if the shared library is missing or the tensors are not on a ROCm device.

PyTorch is used for device memory, streams and autograd bookkeeping only; every FLOP of the
message-passing layers and of the scoring heads runs in the kernels under csrc/.

This file is a facade: the code lives in the modules below and callers keep using every name on the package.
  _cabi      structures, prototypes, loader, argument helpers; owns the library handle, LIB_PATH and CALL_COUNT
  _switches  every A/B switch that is assigned from outside (one copy each)
  _streams   side / step stream policy and live kernel timing
  _autograd  what all autograd Functions share
  gemm       raw GEMM and row-wise entry points        weights   packed / transposed weight copies
  graph      message-passing layers, notifications     linear    gathered Linear, row dot, dropout
  heads      scoring heads and losses                  seq       attention, GRU scan, one-call GREAT layer
  services   ensemble, self-supervision, reports, evaluation, suggestions, FDR, calibration, dedup, drift, grouping, triage,
             review queues, warning tracking
  optim      clip + Adam on flat buffers               runtime   library-wide modes
"""
from __future__ import annotations

import sys
import types

from . import _cabi, _switches, _streams, seq as _seq
from ._cabi import *  # noqa: F401,F403
from ._streams import *  # noqa: F401,F403
from ._autograd import *  # noqa: F401,F403
from .gemm import *  # noqa: F401,F403
from .weights import *  # noqa: F401,F403
from .runtime import *  # noqa: F401,F403
from .graph import *  # noqa: F401,F403
from .linear import *  # noqa: F401,F403
from .heads import *  # noqa: F401,F403
from .seq import *  # noqa: F401,F403
from .services import *  # noqa: F401,F403
from .optim import *  # noqa: F401,F403

# Names whose one copy lives in its owner module but that callers read / set on the package (bench.py, tests, tools): the
# switches (`hip_ops.USE_SIDE_STREAM = False`), and CALL_COUNT, LIB_PATH and `_lib` (the CDLL handle: tools point it at a tuning
# build) of the C-ABI module.  The package itself never holds them: no star import above carries one.
# STREAMING_ATTENTION is the one switch owned by a domain module (seq.py, next to attention_path, which reads it).
_FORWARDED = {**{name: _switches for name in _switches.__all__}, **{name: _cabi for name in _cabi.FORWARDED_BY_PACKAGE},
              "STREAMING_ATTENTION": _seq}


class _HipOpsModule(types.ModuleType):
    def __getattr__(self, name):
        owner = _FORWARDED.get(name)
        if owner is None:
            raise AttributeError(f"module {self.__name__!r} has no attribute {name!r}")
        return getattr(owner, name)

    def __setattr__(self, name, value):
        owner = _FORWARDED.get(name)
        if owner is not None:
            setattr(owner, name, value)
        else:
            super().__setattr__(name, value)


sys.modules[__name__].__class__ = _HipOpsModule

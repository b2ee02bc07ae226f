"""`AbstractNeuralModel` -- the host-side half of ptgnn's (model, nn.Module) pair, reduced to the
surface the reference uses: metadata pass, tensorize, minibatching,
`save` / `restore_model` (gzip-pickled `(model, nn)`, reference gnn.py:325, evaluate.py:44,
trainbugdetector.py:98, modelregistry.py:152-156)."""
from __future__ import annotations

import gzip
import io
import queue
import threading
from abc import ABC, abstractmethod
from collections import deque
from concurrent.futures import ThreadPoolExecutor
from pathlib import Path
from typing import Any, Dict, Generic, Iterable, Iterator, List, Optional, Tuple, TypeVar, Union

import torch

TRawDatapoint = TypeVar("TRawDatapoint")
TTensorizedDatapoint = TypeVar("TTensorizedDatapoint")
TNeuralModule = TypeVar("TNeuralModule")


COLLATE_WORKERS = 3  # minibatches collated concurrently by minibatch_iterator(parallelize=True)


def ordered_map(fn, iterable: Iterable, parallelize: bool = False, num_workers: int = 8) -> Iterator:
    """fn(x) for every x, in order; with `parallelize` in worker threads, at most 4 * num_workers results ahead."""
    if not parallelize:
        for x in iterable:
            yield fn(x)
        return
    with ThreadPoolExecutor(max_workers=num_workers) as pool:
        window: "deque" = deque()
        for x in iterable:
            window.append(pool.submit(fn, x))
            if len(window) >= 4 * num_workers:
                yield window.popleft().result()
        while window:
            yield window.popleft().result()


def write_checkpoint(path: Path, model, neural_module) -> None:
    """The checkpoint format: gzip-pickled `(model, neural_module)`.  Written to a temporary file and moved into place: a crash
    mid-write cannot corrupt the previous best checkpoint."""
    import os

    path = Path(path)
    tmp = path.with_name(path.name + ".tmp")
    with gzip.open(tmp, "wb") as f:
        torch.save((model, neural_module), f)
    os.replace(tmp, path)


class AbstractNeuralModel(ABC, Generic[TRawDatapoint, TTensorizedDatapoint, TNeuralModule]):
    def __init__(self):
        self.__metadata_initialized = False

    # ---- to be implemented by models ----------------------------------------------------------
    @abstractmethod
    def update_metadata_from(self, datapoint) -> None: ...

    def finalize_metadata(self) -> None:
        pass

    @abstractmethod
    def build_neural_module(self): ...

    @abstractmethod
    def tensorize(self, datapoint): ...

    @abstractmethod
    def initialize_minibatch(self) -> Dict[str, Any]: ...

    @abstractmethod
    def extend_minibatch_with(self, tensorized_datapoint, partial_minibatch) -> bool: ...

    @abstractmethod
    def finalize_minibatch(self, accumulated_minibatch_data, device) -> Dict[str, Any]: ...

    # ---- metadata -----------------------------------------------------------------------------
    def compute_metadata(self, dataset_iterator: Iterable, parallelize: bool = True, show_progress_bar: bool = False) -> None:
        assert not self.__metadata_initialized, "Metadata has already been initialized."
        for datapoint in dataset_iterator:
            if datapoint is not None:
                self.update_metadata_from(datapoint)
        self.finalize_metadata()
        self.__metadata_initialized = True

    # ---- tensorisation / minibatching ---------------------------------------------------------
    def tensorize_dataset(self, dataset_iterator: Iterable, return_input_data: bool = False, parallelize: bool = False,
                          num_workers: int = 8) -> Iterator:
        """Tensorise lazily; samples for which `tensorize` returns None are dropped (reference
        gnn.py:404-405).  `parallelize` tensorises in worker threads, preserving order."""
        for t, orig in ordered_map(lambda d: (self.tensorize(d), d), dataset_iterator, parallelize, num_workers):
            if t is not None:
                yield (t, orig) if return_input_data else t

    def minibatch_iterator(self, tensorized_data: Iterable, device: Union[str, torch.device], max_minibatch_size: int,
                           yield_partial_minibatches: bool = True, parallelize: bool = False, finalize=None) -> Iterator:
        """Yields `(minibatch dict, [original datapoints])`.  With `parallelize` the next minibatch
        is collated and copied (pinned, non-blocking) in a background thread while the device
        works on the current one.  `finalize(accumulated, device)`: replaces `finalize_minibatch` (predict adds its
        un-batching indices there, so they are built in the collate workers too)."""
        finalize = finalize or self.finalize_minibatch

        def gather():
            """Groups tensorised samples into un-collated minibatches (cheap: list appends)."""
            mb = self.initialize_minibatch()
            originals: List = []
            n = 0
            for item in tensorized_data:
                t, orig = item if isinstance(item, tuple) and len(item) == 2 and not hasattr(item, "_fields") else (item, None)
                keep = self.extend_minibatch_with(t, mb)
                originals.append(orig)
                n += 1
                if not keep or n >= max_minibatch_size:
                    yield mb, originals
                    mb, originals, n = self.initialize_minibatch(), [], 0
            if n > 0 and yield_partial_minibatches:
                yield mb, originals

        if not parallelize:
            for mb, originals in gather():
                yield finalize(mb, device), originals
            return
        # Collation (NumPy + the native counting sorts release the GIL) and the pinned host->device copy of the next
        # minibatches run in a few worker threads while the device works on the current one; order is preserved.
        # One c2 minibatch collates in ~40 ms against a ~21 ms device step, hence more than one worker.
        q: "queue.Queue" = queue.Queue(maxsize=COLLATE_WORKERS + 1)
        sentinel = object()

        def worker():
            try:
                with ThreadPoolExecutor(max_workers=COLLATE_WORKERS) as pool:
                    pending: "deque" = deque()
                    for mb, originals in gather():
                        pending.append((pool.submit(finalize, mb, device), originals))
                        while len(pending) > COLLATE_WORKERS:
                            fut, orig = pending.popleft()
                            q.put((fut.result(), orig))
                    while pending:
                        fut, orig = pending.popleft()
                        q.put((fut.result(), orig))
                q.put(sentinel)
            except BaseException as e:  # surface collate errors in the consumer
                q.put(e)

        threading.Thread(target=worker, daemon=True).start()
        while True:
            x = q.get()
            if x is sentinel:
                return
            if isinstance(x, BaseException):
                raise x
            yield x

    # ---- persistence --------------------------------------------------------------------------
    def save(self, path: Path, neural_module) -> None:
        write_checkpoint(path, self, neural_module)

    @classmethod
    def restore_model(cls, path: Path, device=None) -> Tuple["AbstractNeuralModel", Any]:
        with gzip.open(path, "rb") as f:
            buf = io.BytesIO(f.read())
        model, nn = torch.load(buf, map_location=device, weights_only=False)
        if device is not None:
            nn = nn.to(device)
        return model, nn

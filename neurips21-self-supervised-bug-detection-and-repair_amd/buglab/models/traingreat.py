#!/usr/bin/env python
"""
Usage:
    traingreat.py [options] TRAIN_DATA_PATH VALID_DATA_PATH MODEL_FILENAME

Options:
    --amp                         Refused: mixed precision exists only for the gnn-mlp message GEMMs.
    --max-num-epochs=<epochs>     The maximum number of epochs to run training for. [default: 100]
    --max-files-per-fold=<n>      The maximum number of files to include in each fold.
    --minibatch-size=<size>       The minibatch size. [default: 30]
    --validate-after=<n_samples>  Run the validation after seen n_samples. [default: 1000000]
    --restore-path=<path>         The path to previous model file for starting from previous checkpoint.
    --sequential                  Do not parallelize data loading. Makes debugging easier.
    --quiet                       Do not show progress bar.
    --ema-decay=<d>               Weight averaging: validate, select and save an exponential moving average of the parameters
                                  with decay d (0 < d < 1; warmed up from 2/11) instead of the last iterate. [default: 0]
    -h --help                     Show this screen.
    --debug                       Enable debug routines. [default: False]

Trains the GREAT var-misuse model (buglab.models.greatreimplementation) on directories of GREAT `*.jsonl.gz` files -- the
command line of reference buglab/models/traingreat.py (the Azure-only flags --aml / --azure-info are dropped: no network).
"""
import argparse
import gzip
import json
import logging
import random
import sys
from pathlib import Path
from typing import Callable, Iterator, Optional

if __package__ in (None, ""):  # executed as a script, like the reference
    sys.path.insert(0, str(Path(__file__).resolve().parents[2]))

from buglab.runtime.richpath import RichPath, run_and_debug

LOGGER = logging.getLogger(__name__)

DEFAULT_TRANSFORMER_CONFIG = {  # reference traingreat.py:125-136
    "num_layers": 10,
    "num_heads": 8,
    "intermediate_dimension": 2048,
    "dropout_rate": 0.1,
    "rezero_mode": "off",
    "normalization_mode": "prenorm",
}
DEFAULT_EMBEDDING_DIM = 512
DEFAULT_VOCAB_SIZE = 10240  # "Closest multiple of 64"


def load_all_json_l_gz(path, shuffle: bool = False, take_only_first_n_files: Optional[int] = None,
                       limit_num_yielded_elements: Optional[int] = None) -> Iterator:
    """The records of the `*.jsonl.gz` files of a directory (or one file), files in sorted order (shuffled when asked).  Stops
    once MORE than `limit_num_yielded_elements` records were yielded, i.e. after limit + 1 (reference traingreat.py:37-58).
    A file that fails to read is reported and skipped."""
    if not isinstance(path, RichPath):
        path = RichPath.create(str(path))
    files = sorted(path.iterate_filtered_files_in_dir("*.jsonl.gz"))
    if take_only_first_n_files is not None:
        files = files[:take_only_first_n_files]
    if shuffle:
        random.shuffle(files)
    yielded = 0
    for f in files:
        try:
            with gzip.open(f.to_local_path().path, "rt", encoding="utf-8") as lines:
                for line in lines:
                    if not line.strip():
                        continue
                    record = json.loads(line)
                    if record is not None:
                        yielded += 1
                        yield record
                    if limit_num_yielded_elements is not None and yielded > limit_num_yielded_elements:
                        return
        except (OSError, ValueError) as e:
            print(f"Error loading {f}: {e}.")


def construct_data_loading_callable(data_path, shuffle: bool = False, max_files_per_fold: Optional[int] = None,
                                    limit_num_yielded_elements: Optional[int] = None) -> Callable[[], Iterator]:
    return lambda: load_all_json_l_gz(data_path, shuffle=shuffle, take_only_first_n_files=max_files_per_fold,
                                      limit_num_yielded_elements=limit_num_yielded_elements)


def default_model(transformer_config=None, embedding_dim: int = DEFAULT_EMBEDDING_DIM, vocab_size: int = DEFAULT_VOCAB_SIZE, **kwargs):
    from buglab.models.greatreimplementation import GreatVarMisuse

    return GreatVarMisuse(dict(transformer_config or DEFAULT_TRANSFORMER_CONFIG), embedding_dim=embedding_dim, vocab_size=vocab_size,
                          **kwargs)


def run(arguments, model_factory: Callable = default_model):
    """reference traingreat.py:76-169.  `model_factory` builds the untrained model (tests pass a small configuration)."""
    import torch

    from buglab.models.utils import LinearWarmupScheduler, optimizer
    from buglab.runtime.neuralmodel import AbstractNeuralModel
    from buglab.runtime.trainer import LazyDataIterable, ModelTrainer

    logging.basicConfig(level=logging.INFO, format="%(asctime)s %(name)s %(levelname)s %(message)s")
    max_files_per_fold = arguments["--max-files-per-fold"]
    if max_files_per_fold is not None:
        max_files_per_fold = int(max_files_per_fold)
    training_data = LazyDataIterable(construct_data_loading_callable(
        RichPath.create(arguments["TRAIN_DATA_PATH"]), shuffle=True, max_files_per_fold=max_files_per_fold,
        limit_num_yielded_elements=int(arguments["--validate-after"])))
    validation_data = LazyDataIterable(construct_data_loading_callable(
        RichPath.create(arguments["VALID_DATA_PATH"]), max_files_per_fold=max_files_per_fold))
    model_path = Path(arguments["MODEL_FILENAME"])
    initialize_metadata = True
    restore = arguments.get("--restore-path", None)
    if restore is not None:
        LOGGER.info("Resuming training from %s.", restore)
        initialize_metadata = False
        model, nn = AbstractNeuralModel.restore_model(Path(restore), torch.device("cuda:0" if torch.cuda.is_available() else "cpu"))
    else:
        nn = None
        model = model_factory()
    ema_decay = float(arguments.get("--ema-decay") or 0)
    trainer = ModelTrainer(model, model_path, max_num_epochs=int(arguments["--max-num-epochs"]),
                           minibatch_size=int(arguments["--minibatch-size"]), optimizer_creator=optimizer,
                           clip_gradient_norm=0.25,  # as the original GREAT (reference traingreat.py:144)
                           scheduler_creator=lambda o: LinearWarmupScheduler(o),
                           ema_decay=ema_decay if ema_decay != 0 else None)
    if nn is not None:
        trainer.neural_module = nn
        trainer.restore_optimizer_state_from = Path(restore)  # Adam's moments, when this trainer wrote them
    trainer.register_train_epoch_end_hook(lambda model, nn, epoch, metrics: LOGGER.info("train epoch %s: %s", epoch, metrics))
    trainer.register_validation_epoch_end_hook(lambda model, nn, epoch, metrics: LOGGER.info("valid epoch %s: %s", epoch, metrics))
    return trainer.train(training_data, validation_data, show_progress_bar=not arguments["--quiet"], initialize_metadata=initialize_metadata,
                         parallelize=not arguments["--sequential"], patience=10)


def parse_args(argv=None):
    p = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    p.add_argument("TRAIN_DATA_PATH")
    p.add_argument("VALID_DATA_PATH")
    p.add_argument("MODEL_FILENAME")
    p.add_argument("--amp", action="store_true")
    p.add_argument("--max-num-epochs", default="100")
    p.add_argument("--max-files-per-fold", default=None)
    p.add_argument("--minibatch-size", default="30")
    p.add_argument("--validate-after", default="1000000")
    p.add_argument("--restore-path", default=None)
    p.add_argument("--sequential", action="store_true")
    p.add_argument("--quiet", action="store_true")
    p.add_argument("--ema-decay", default="0")
    p.add_argument("--debug", action="store_true")
    ns = p.parse_args(argv)
    if ns.amp:
        p.error("--amp is not supported for the GREAT model: fp16 operands exist only for the gnn-mlp message GEMMs, and this "
                "model would train in fp32 regardless")
    d = {"TRAIN_DATA_PATH": ns.TRAIN_DATA_PATH, "VALID_DATA_PATH": ns.VALID_DATA_PATH, "MODEL_FILENAME": ns.MODEL_FILENAME}
    for k, v in vars(ns).items():
        if not k.isupper():
            d["--" + k.replace("_", "-")] = v
    return d


if __name__ == "__main__":
    args = parse_args()
    run_and_debug(lambda: run(args), args.get("--debug", False))

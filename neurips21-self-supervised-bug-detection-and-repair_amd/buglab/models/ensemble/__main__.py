#!/usr/bin/env python
"""
Usage:
    python -m buglab.models.ensemble [--debug] OUT_MODEL_FILENAME ENSEMBLE_KIND MODEL_FILENAMES...

Builds an ensemble file from trained checkpoints (reference buglab/models/ensemble/__main__.py).  ENSEMBLE_KIND is `avg` or
`consensus`; the members may be of any of the registry's BugLab detector types.  Every member is restored on the CPU (no GPU
needed) and the pair (EnsembleWrapper, EnsembleModuleWrapper) is written in the checkpoint format of
AbstractNeuralModel.save, so that evaluate.py reads the file like any other model.
"""
import argparse
import sys
from pathlib import Path

if __package__ in (None, ""):
    sys.path.insert(0, str(Path(__file__).resolve().parents[3]))

from buglab.models.ensemble.wrapper import EnsembleModuleWrapper, EnsembleWrapper
from buglab.runtime.neuralmodel import AbstractNeuralModel, write_checkpoint


def run(arguments):
    models, nns = [], []
    for path in arguments["MODEL_FILENAMES"]:
        print(f"Loading {path}...")
        model, nn = AbstractNeuralModel.restore_model(Path(path), "cpu")
        models.append(model)
        nns.append(nn)
    print(f"Loaded {len(models)} models. Saving...")
    model = EnsembleWrapper(models, arguments["ENSEMBLE_KIND"])
    write_checkpoint(Path(arguments["OUT_MODEL_FILENAME"]), model, EnsembleModuleWrapper(nns))  # AbstractNeuralModel.save's format


def main(argv=None):
    p = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    p.add_argument("OUT_MODEL_FILENAME")
    p.add_argument("ENSEMBLE_KIND", choices=["avg", "consensus"])
    p.add_argument("MODEL_FILENAMES", nargs="+")
    p.add_argument("--debug", action="store_true", help="Enable debug routines (drop into pdb on an exception).")
    ns = p.parse_args(argv)
    args = {"OUT_MODEL_FILENAME": ns.OUT_MODEL_FILENAME, "ENSEMBLE_KIND": ns.ENSEMBLE_KIND, "MODEL_FILENAMES": ns.MODEL_FILENAMES}
    if not ns.debug:
        return run(args)
    try:
        return run(args)
    except Exception:
        import pdb
        import traceback

        traceback.print_exc()
        pdb.post_mortem()
        raise


if __name__ == "__main__":
    main()

#!/usr/bin/env python
"""
Usage:
    python -m buglab.models.ensemble [--debug] OUT_MODEL_FILENAME ENSEMBLE_KIND MODEL_FILENAMES...
    python -m buglab.models.ensemble [--debug] OUT_MODEL_FILENAME weighted MODEL_FILENAMES... --fit-on VALID_DATA_PATH
                                     [--no-temperature] [--limit-num-elements N] [--sequential] [--host-fit] [--report-json FILE]

Builds an ensemble file from trained checkpoints (reference buglab/models/ensemble/__main__.py).  ENSEMBLE_KIND is `avg` or
`consensus`; the members may be of any of the registry's BugLab detector types.  Every member is restored on the CPU (no GPU
needed) and the pair (EnsembleWrapper, EnsembleModuleWrapper) is written in the checkpoint format of
AbstractNeuralModel.save, so that evaluate.py reads the file like any other model.

Beyond the reference: the kind `weighted` fits one weight per member for each head and one temperature per member for the
location distribution on the held-out data of --fit-on (buglab/models/ensemble/fit.py; this needs the GPU, the members' forward
passes run there) and stores them in the file.  --no-temperature fits the weights alone; --host-fit takes the statistics of
every optimiser step from the NumPy twin instead of the device (for comparison).
"""
import argparse
import json
import sys
from pathlib import Path

if __package__ in (None, ""):
    sys.path.insert(0, str(Path(__file__).resolve().parents[3]))

from buglab.models.ensemble.wrapper import EnsembleModuleWrapper, EnsembleWrapper
from buglab.runtime.neuralmodel import AbstractNeuralModel, write_checkpoint

FIT_OPTIONS = ("--fit-on", "--no-temperature", "--limit-num-elements", "--sequential", "--host-fit", "--report-json")


def _fit(model, module, arguments):
    import torch

    from buglab.models.ensemble.fit import fit_ensemble_weights, format_report
    from buglab.runtime.richpath import RichPath
    from buglab.utils.msgpackutils import load_all_msgpack_l_gz

    if not torch.cuda.is_available():
        raise RuntimeError("ensemble: fitting a `weighted` ensemble needs a ROCm GPU; the BugLab hot path has no CPU fallback")
    device = torch.device("cuda")
    module.to(device)
    data = load_all_msgpack_l_gz(RichPath.create(arguments["--fit-on"]), shuffle=True,
                                 limit_num_yielded_elements=arguments["--limit-num-elements"])
    report = {}
    fit_ensemble_weights(model, module, data, device, fit_temperature=not arguments["--no-temperature"],
                         parallelize=not arguments["--sequential"], host_fit=arguments["--host-fit"], report=report)
    module.to("cpu")
    sys.stdout.write(format_report(report))
    if arguments["--report-json"] is not None:
        with open(arguments["--report-json"], "w", encoding="utf-8") as f:
            f.write(json.dumps(report, indent=1, sort_keys=True) + "\n")


def run(arguments):
    models, nns = [], []
    for path in arguments["MODEL_FILENAMES"]:
        print(f"Loading {path}...")
        model, nn = AbstractNeuralModel.restore_model(Path(path), "cpu")
        models.append(model)
        nns.append(nn)
    model = EnsembleWrapper(models, arguments["ENSEMBLE_KIND"])
    module = EnsembleModuleWrapper(nns)
    if arguments["ENSEMBLE_KIND"] == "weighted":
        print(f"Loaded {len(models)} models. Fitting...")
        _fit(model, module, arguments)
        print("Saving...")
    else:
        print(f"Loaded {len(models)} models. Saving...")
    write_checkpoint(Path(arguments["OUT_MODEL_FILENAME"]), model, module)  # AbstractNeuralModel.save's format


def main(argv=None):
    p = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    p.add_argument("OUT_MODEL_FILENAME")
    p.add_argument("ENSEMBLE_KIND", choices=["avg", "consensus", "weighted"])
    p.add_argument("MODEL_FILENAMES", nargs="+")
    p.add_argument("--debug", action="store_true", help="Enable debug routines (drop into pdb on an exception).")
    fit = p.add_argument_group("fitting (the `weighted` kind only)")
    fit.add_argument("--fit-on", default=None, metavar="VALID_DATA_PATH", help="Held-out `*.msgpack.l.gz` data: a file or a folder.")
    fit.add_argument("--no-temperature", action="store_true", help="Fit the weights only; leave every member's temperature at 1.")
    fit.add_argument("--limit-num-elements", type=int, default=None, help="Fit on at most this many samples.")
    fit.add_argument("--sequential", action="store_true", help="Do not parallelize data loading.")
    fit.add_argument("--host-fit", action="store_true", help="Take the optimiser's statistics from the NumPy twin, not the device.")
    fit.add_argument("--report-json", default=None, help="Also write the fit's report as data.")
    ns = p.parse_args(argv)
    args = {"OUT_MODEL_FILENAME": ns.OUT_MODEL_FILENAME, "ENSEMBLE_KIND": ns.ENSEMBLE_KIND, "MODEL_FILENAMES": ns.MODEL_FILENAMES,
            "--fit-on": ns.fit_on, "--no-temperature": ns.no_temperature, "--limit-num-elements": ns.limit_num_elements,
            "--sequential": ns.sequential, "--host-fit": ns.host_fit, "--report-json": ns.report_json}
    if ns.ENSEMBLE_KIND == "weighted":
        if ns.fit_on is None:
            p.error("the `weighted` kind is fitted on held-out data: --fit-on VALID_DATA_PATH is required")
    else:
        given = [o for o in FIT_OPTIONS if args[o] not in (None, False)]
        if given:
            p.error(f"{', '.join(given)}: only the `weighted` kind is fitted; `{ns.ENSEMBLE_KIND}` takes no such option")
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

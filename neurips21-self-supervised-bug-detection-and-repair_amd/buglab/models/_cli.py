"""What the command-line tools of buglab/models and buglab/controllers share before and after their own work: opening a
checkpoint, reading `*.msgpack.l.gz` data, insisting on a GPU, writing records and the `--report-json` file -- and the
pass-throughs to `similar` of the tools that embed sites.  Heavy imports are made when a function runs, not when a tool is
imported."""
import gzip
import json
from pathlib import Path
from typing import Any, Dict, Iterable, List, Optional, Tuple


def open_model(path) -> Tuple[Any, Any, Any, bool]:
    """-> (model, nn, device, have_gpu): the checkpoint on "cuda", or on "cpu" when no GPU is visible, so that a tool can check
    what the checkpoint carries (and exit with its own status) before it insists on a GPU."""
    import torch

    from buglab.runtime.neuralmodel import AbstractNeuralModel

    have_gpu = torch.cuda.is_available()
    device = torch.device("cuda" if have_gpu else "cpu")
    model, nn = AbstractNeuralModel.restore_model(Path(path), device)
    return model, nn, device, have_gpu


def read_data(path, limit: Optional[int]) -> List[Any]:
    from buglab.runtime.richpath import RichPath
    from buglab.utils.msgpackutils import load_all_msgpack_l_gz

    return list(load_all_msgpack_l_gz(RichPath.create(path), shuffle=False, limit_num_yielded_elements=limit))


def require_gpu(have_gpu: Optional[bool], tool: str, what: str = "the BugLab hot path") -> None:
    """RuntimeError without a GPU; `have_gpu` None: ask torch."""
    if have_gpu is None:
        import torch

        have_gpu = torch.cuda.is_available()
    if not have_gpu:
        raise RuntimeError(f"{tool}: no ROCm GPU visible; {what} has no CPU fallback")


def write_report_json(path, obj) -> None:
    """The `--report-json` file; nothing without a path."""
    if path is not None:
        with open(path, "w", encoding="utf-8") as f:
            f.write(json.dumps(obj, indent=1, sort_keys=True) + "\n")


def write_records(records: Iterable[Dict[str, Any]], out_path) -> int:
    """JSON lines, gzip when the name ends in .gz -> the number of records."""
    out_path = str(out_path)
    opened = gzip.open(out_path, "wt", encoding="utf-8") if out_path.endswith(".gz") else open(out_path, "w", encoding="utf-8")
    count = 0
    with opened as f:
        for record in records:
            f.write(json.dumps(record, sort_keys=True) + "\n")
            count += 1
    return count


def embedding_dim(nn) -> int:
    from buglab.models import similar

    return similar.embedding_dim(nn)


def embed_sites(model, nn, data, device, site: str, **options):
    from buglab.models import similar

    return similar.embed_sites(model, nn, data, device, site, **options)


def collect_sites(model, nn, data, device, site: str, assume_buggy: bool, host: bool, parallelize: bool):
    from buglab.models import similar

    return similar._collect_sites(model, nn, data, device, site, assume_buggy, host, parallelize)

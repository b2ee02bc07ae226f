"""python -m buglab.data.deduplication DATA_PATH OUT_DIR [--against PATH ...]: drop near-duplicate functions from
`*.msgpack.l.gz` shards of BugLabData.

The data-hygiene step the reference runs while it extracts data (buglab/data/deduplication/, used by
staticdatasetextractor.py:77 and buggydatacreation.py:228-240), as a filter over finished shards.  A DOCUMENT IS A FUNCTION, not a
datapoint: its key is (package_name, graph["path"], start of graph["code_range"]) and its text the graph["text"] of the key's first
datapoint -- a function's rewrites are near-copies of it by construction and must not count against it.  All datapoints of a key
are kept or dropped together.  `--against` indexes other data first (the test set) without writing it, so that training functions
close to test functions are dropped."""
import argparse
import json
import logging
import multiprocessing
import os
import sys
import time
from pathlib import Path
from typing import Callable, Dict, Iterator, List, Optional, Sequence, Tuple

from buglab.data.deduplication.tokenizers import tokenize_text_job
from buglab.utils.msgpackutils import load_msgpack_l_gz, save_msgpack_l_gz

LOGGER = logging.getLogger("buglab.data.deduplication")
MAX_WORKERS = 16
MAX_NUM_PERM = 256  # hip_ops.DEDUP_MAX_PERM (not imported here: tokenizer workers and the parser stay free of torch)


def document_key(datapoint) -> str:
    graph = datapoint["graph"]
    start = graph["code_range"][0]
    return f"{datapoint['package_name']}::{graph['path']}::{int(start[0])}:{int(start[1])}"


def load_datapoints(path: str) -> Iterator[dict]:
    """Every datapoint of the directory's shards in sorted file order, as plain dicts (they are written back as they were read)."""
    for shard in sorted(Path(path).glob("*.msgpack.l.gz")):
        for datapoint in load_msgpack_l_gz(str(shard), native=False):
            if datapoint is not None:
                yield datapoint


def read_documents(path: str) -> Dict[str, str]:
    """key -> text of the key's first datapoint, in order of first appearance."""
    documents: Dict[str, str] = {}
    for datapoint in load_datapoints(path):
        documents.setdefault(document_key(datapoint), datapoint["graph"]["text"])
    return documents


def default_workers() -> int:
    return max(1, min(MAX_WORKERS, len(os.sched_getaffinity(0))))  # the CPUs this process may use, never the machine's count


def tokenize_documents(texts: Sequence[str], all_tokens: bool, workers: int) -> List[List[str]]:
    jobs = [(t, all_tokens) for t in texts]
    if workers <= 1 or len(jobs) < 64:
        return [tokenize_text_job(j) for j in jobs]
    # fresh interpreters (spawn), which import the tokenizer alone: never a fork of a process that may hold the GPU open
    with multiprocessing.get_context("spawn").Pool(workers) as pool:
        return pool.map(tokenize_text_job, jobs, chunksize=max(1, min(256, len(jobs) // (4 * workers))))


def _batches(n: int, size: int) -> Iterator[Tuple[int, int]]:
    for lo in range(0, n, size):
        yield lo, min(n, lo + size)


def _resharded(datapoints, per_shard: int, out_dir: Path) -> int:
    shard, written, num_shards = [], 0, 0
    for datapoint in datapoints:
        shard.append(datapoint)
        if len(shard) == per_shard:
            save_msgpack_l_gz(shard, out_dir / f"deduplicated-{num_shards:05d}.msgpack.l.gz")
            written, num_shards, shard = written + len(shard), num_shards + 1, []
    if shard:
        save_msgpack_l_gz(shard, out_dir / f"deduplicated-{num_shards:05d}.msgpack.l.gz")
        written += len(shard)
    return written


def deduplicate(data_path: str, out_dir: str, *, against: Sequence[str] = (), make_index: Callable[[], object], all_tokens: bool = False,
                batch_size: int = 4096, workers: Optional[int] = None, datapoints_per_shard: int = 5000) -> dict:
    """-> the report.  `make_index()`: an empty index with `check_batch`, `collisions` and `min_num_tokens`."""
    workers = default_workers() if workers is None else workers
    t0 = time.perf_counter()
    against_docs = [read_documents(p) for p in against]
    documents = read_documents(data_path)
    t1 = time.perf_counter()
    texts = [t for docs in against_docs for t in docs.values()] + list(documents.values())
    tokens = tokenize_documents(texts, all_tokens, workers)
    t2 = time.perf_counter()

    index = make_index()
    seen: set = set()
    position = 0
    for docs in against_docs:  # keys of one `--against` path repeat in another: indexed once
        keys, sets = [], []
        for k in docs:
            if k not in seen:
                seen.add(k)
                keys.append(k)
                sets.append(tokens[position])
            position += 1
        for lo, hi in _batches(len(keys), batch_size):
            index.check_batch(keys[lo:hi], sets[lo:hi])
    keys = list(documents)
    sets = tokens[position:]
    flags = []
    for lo, hi in _batches(len(keys), batch_size):
        flags.extend(bool(f) for f in index.check_batch(keys[lo:hi], sets[lo:hi]))
    t3 = time.perf_counter()

    too_short = [k for k, s in zip(keys, sets) if len(s) < index.min_num_tokens]
    duplicate_keys = [k for k, f in zip(keys, flags) if f and k in seen]  # the very function is in the `--against` data
    dropped = [k for k, f in zip(keys, flags) if f]
    collided = index.collisions([k for k in dropped if k not in seen])
    drop = set(dropped)
    out = Path(out_dir)
    out.mkdir(parents=True, exist_ok=True)
    read, kept = [0], [0]

    def kept_datapoints():
        for datapoint in load_datapoints(data_path):
            read[0] += 1
            if document_key(datapoint) not in drop:
                kept[0] += 1
                yield datapoint

    _resharded(kept_datapoints(), datapoints_per_shard, out)
    t4 = time.perf_counter()
    return {
        "documents": len(keys),
        "against_documents": len(seen),
        "too_short": len(too_short),
        "duplicate_keys": len(duplicate_keys),
        "dropped": len(dropped),
        "kept": len(keys) - len(dropped),
        "datapoints_read": read[0],
        "datapoints_kept": kept[0],
        "dropped_documents": [{"key": k, "collided_with": collided.get(k, [k] if k in seen else [])} for k in dropped],
        "seconds": {"read": t1 - t0, "tokenize": t2 - t1, "index": t3 - t2, "write": t4 - t3},
        "workers": workers,
    }


def build_parser() -> argparse.ArgumentParser:
    p = argparse.ArgumentParser(prog="python -m buglab.data.deduplication", description=__doc__.split("\n\n")[0])
    p.add_argument("data_path", metavar="DATA_PATH", help="directory of *.msgpack.l.gz shards to filter")
    p.add_argument("out_dir", metavar="OUT_DIR", help="where the kept datapoints are written, re-sharded")
    p.add_argument("--against", action="append", default=[], metavar="PATH", help="data indexed first and never written (repeatable)")
    p.add_argument("--threshold", type=float, default=0.85, help="Jaccard threshold the bands are chosen for")
    p.add_argument("--num-perm", type=int, default=256)
    p.add_argument("--min-num-tokens", type=int, default=10, help="documents with fewer distinct tokens are kept and not indexed")
    p.add_argument("--all-tokens", action="store_true", help="tokens of every kind, not NAME and STRING alone")
    p.add_argument("--report-json", metavar="FILE")
    p.add_argument("--batch-size", type=int, default=4096, help="documents per device call")
    p.add_argument("--workers", type=int, default=None, help=f"tokenizer processes (default: the CPUs of this process, at most {MAX_WORKERS})")
    return p


def parse_args(argv=None) -> argparse.Namespace:
    p = build_parser()
    args = p.parse_args(argv)
    if not 0.0 <= args.threshold <= 1.0:
        p.error(f"--threshold must be in [0, 1] (got {args.threshold})")
    if args.batch_size < 1:
        p.error(f"--batch-size must be at least 1 (got {args.batch_size})")
    if not 2 <= args.num_perm <= MAX_NUM_PERM:
        p.error(f"--num-perm must be in 2 .. {MAX_NUM_PERM}, what the MinHash kernel covers (got {args.num_perm})")
    if args.min_num_tokens < 0:
        p.error(f"--min-num-tokens must not be negative (got {args.min_num_tokens})")
    if args.workers is not None and not 1 <= args.workers <= MAX_WORKERS:
        p.error(f"--workers must be in 1 .. {MAX_WORKERS} (got {args.workers})")
    for path in [args.data_path] + args.against:
        if not os.path.isdir(path):
            p.error(f"{path}: not a directory")
    if os.path.realpath(args.out_dir) in {os.path.realpath(q) for q in [args.data_path] + args.against}:
        p.error("OUT_DIR must differ from DATA_PATH and from every --against path")
    return args


def main(argv=None, make_index: Optional[Callable[[argparse.Namespace], object]] = None) -> dict:
    args = parse_args(argv)

    def device_index():
        from buglab.data.deduplication.index import DuplicationIndex

        return DuplicationIndex(None, duplication_jaccard_threshold=args.threshold, num_perm=args.num_perm,
                                min_num_tokens=args.min_num_tokens)

    if make_index is None:  # fail before the shards are read and tokenized, not after
        import torch

        from buglab.models import hip_ops

        assert hip_ops.DEDUP_MAX_PERM == MAX_NUM_PERM
        hip_ops.load_library()
        if not torch.cuda.is_available():
            raise SystemExit("python -m buglab.data.deduplication: the index runs on a ROCm GPU and none is available (no CPU fallback)")
    report = deduplicate(args.data_path, args.out_dir, against=args.against,
                         make_index=(lambda: make_index(args)) if make_index is not None else device_index,
                         all_tokens=args.all_tokens, batch_size=args.batch_size, workers=args.workers)
    if args.report_json:
        with open(args.report_json, "w") as f:
            json.dump(report, f, indent=1)
    summary = {k: v for k, v in report.items() if k != "dropped_documents"}
    print(json.dumps(summary))
    return report


if __name__ == "__main__":
    logging.basicConfig(level=logging.WARNING)
    main(sys.argv[1:])

#!/usr/bin/env python
"""
Usage:
    python -m buglab.controllers.bugselector MODEL_FILENAME DATA_PATH OUT_FILENAME [options]

Bug selection with a trained selector ("generator") model -- the compute of reference
buglab/controllers/bugselectorserver.py without its ZeroMQ server: for every datapoint of DATA_PATH (`*.msgpack.l.gz`), the
rewrites the selector wants generated, written to OUT_FILENAME as one `{"selected_rewrites": {"NO_BUG" | str(idx): logprob}}`
per datapoint, in input order; the selection statistics go to stdout.

The reference answers one request at a time: `model.predict` on one datapoint, every prediction value copied to the host,
the distribution and `np.random.choice` in NumPy (:120-150).  Here datapoints go through the minibatches of the model's own
`predict`; after the forward one kernel (hip_ops.selector_sample, csrc/bl_selfsup.hip) computes, in fp64, each rewrite's
log-probability `rewrite_logprob + location_logprobs[reference node]` (NO_BUG: `location_logprobs[-1]`), the temperature /
epsilon distribution of `calculate_selection_distribution`, its entropy, and draws `num_rewrites_per_sample` rewrites without
replacement; the selection, the selected log-probabilities and the entropy are copied back, not the model's output.

Where this differs from the reference ("Self-supervision services"):
  * the draw is Gumbel top-k on uniforms from a seeded `torch.Generator` -- the distribution of
    `np.random.choice(..., replace=False, p=p)` (successive sampling proportional to p), not NumPy's random stream;
  * a sample with fewer entries of non-zero probability than requested gets those there are (the reference raises), and the
    random fallback for a datapoint the model's `tensorize` rejects picks min(num, n) rewrites (the reference raises below 4).
"""
from __future__ import annotations

import argparse
import logging
import random
import sys
from collections import Counter, defaultdict
from pathlib import Path
from typing import Any, Dict, Iterable, Iterator, List, Optional, Tuple

import numpy as np

if __package__ in (None, ""):
    sys.path.insert(0, str(Path(__file__).resolve().parents[2]))

LOGGER = logging.getLogger(__name__)


def calculate_selection_distribution(logprobs: List[float], temperature: float = 1, epsilon: float = 0) -> np.ndarray:
    """reference bugselectorserver.py:22-28: with probability epsilon the uniform distribution, else exp(l / T) / sum_j
    exp(l_j / T) -- no max subtraction, as there.  Draws the epsilon decision from NumPy's global stream, as there."""
    if np.random.rand() < epsilon:
        return np.ones(len(logprobs)) * (1 / len(logprobs))
    # element by element and summed left to right, as there: a vectorised exp or a pairwise sum may round differently
    unnormalised = [np.exp(logprob / temperature) for logprob in logprobs]
    return unnormalised / sum(unnormalised)


class BugSelectionStats:
    """reference bugselectorserver.py:31-75: entropy of the selection distribution against the uniform baseline, and how often
    each rewrite type is selected against how often it is available."""

    def __init__(self):
        self.reset()

    def reset(self) -> None:
        self.available_rewrite_frequency: Dict[str, float] = defaultdict(float)
        self.selected_rewrite_frequency: Dict[str, float] = defaultdict(float)
        self.entropy_sum = 0.0
        self.uniform_baseline_entropy_sum = 0.0
        self.total_samples = 0

    def add(self, sample, distribution, selected, entropy: Optional[float] = None) -> None:
        """`entropy`: the distribution's entropy when it has been computed already (the kernel's); `distribution` may then be
        None -- its length is the number of candidate rewrites + 1."""
        self.total_samples += 1
        if entropy is None:
            distribution = np.asarray(distribution, dtype=np.float64)
            entropy = -np.sum(distribution * np.log(distribution))
        num_entries = len(sample["candidate_rewrite_metadata"]) + 1 if distribution is None else len(distribution)
        self.entropy_sum += float(entropy)
        self.uniform_baseline_entropy_sum += float(np.log(num_entries))  # == -log(1/N)

        rewrites = Counter(rewrite_type for rewrite_type, _ in sample["candidate_rewrite_metadata"])
        rewrites["NO_REWRITE"] = 1
        num_rewrites = sum(rewrites.values())
        for rewrite_type, rewrite_count in rewrites.items():
            self.available_rewrite_frequency[rewrite_type] += rewrite_count / num_rewrites
        for rewrite_idx in selected.keys():
            rewrite_type = "NO_REWRITE" if rewrite_idx == "NO_BUG" else sample["candidate_rewrite_metadata"][int(rewrite_idx)][0]
            self.selected_rewrite_frequency[rewrite_type] += 1.0 / len(selected)

    def report(self) -> Dict[str, float]:
        entropy = self.entropy_sum / self.total_samples
        uniform_baseline_entropy = self.uniform_baseline_entropy_sum / self.total_samples
        print(f"Avg Entropy: {entropy:.3f}")
        print(f"Avg Uniform Entropy (Baseline): {uniform_baseline_entropy:.3f}")
        for rewrite_type in sorted(self.available_rewrite_frequency):
            print(f"{rewrite_type} {self.selected_rewrite_frequency[rewrite_type] / self.total_samples :.2%} "
                  f"(in-data {self.available_rewrite_frequency[rewrite_type] / self.total_samples :.2%})")
        self.reset()
        return {"entropy": entropy, "uniform_baseline_entropy": uniform_baseline_entropy}


def select_random_rewrites(all_candidate_rewrites, num_rewrites: int = 4, rng: Optional[random.Random] = None) -> Dict[str, float]:
    """reference helper/randombugselectorserver.py:41-46: NO_BUG and `num_rewrites` rewrites uniformly at random, each with the
    value 1 / (n + 1).  With fewer than `num_rewrites` candidates all of them are taken (the reference raises)."""
    n = len(all_candidate_rewrites)
    random_prob = 1 / (n + 1)
    selected = {"NO_BUG": random_prob}
    for idx in (rng or random).sample(range(n), k=min(num_rewrites, n)):
        selected[str(idx)] = random_prob
    return selected


class _Slot:
    __slots__ = ("datapoint", "selected", "done")

    def __init__(self, datapoint):
        self.datapoint, self.selected, self.done = datapoint, None, False


def select_rewrites(model, nn, datapoints: Iterable[Any], device, *, num_rewrites_per_sample: int = 4, temperature: float = 1.0,
                    epsilon: float = 0.02, seed: Optional[int] = None, parallelize: bool = False,
                    stats: Optional[BugSelectionStats] = None) -> Iterator[Tuple[Any, Dict[str, float]]]:
    """-> (datapoint, {"NO_BUG" | str(rewrite idx): log-probability}) per datapoint, in input order: the reference server's
    reply.  `seed` fixes the uniforms (device generator) and the random fallback; the same seed, data and model give the same
    selection, with or without `parallelize`."""
    import torch

    from buglab.controllers import _batching as Bt
    from buglab.models import hip_ops

    Bt.require_single_model(model, "select_rewrites")
    K = int(num_rewrites_per_sample)
    if not 1 <= K <= hip_ops.SELECTOR_MAX_K:
        raise ValueError(f"num_rewrites_per_sample must be in 1..{hip_ops.SELECTOR_MAX_K} (got {num_rewrites_per_sample})")
    if not temperature > 0:
        raise ValueError(f"temperature must be positive (got {temperature})")
    device = torch.device(device)
    gen = torch.Generator(device=device)
    if seed is None:
        gen.seed()
    else:
        gen.manual_seed(int(seed))
    fallback_rng = random.Random(seed)
    order = Bt.InOrder()

    def tagged():
        for point in datapoints:
            slot = _Slot(point)
            order.open(slot)
            yield point, slot

    def rejected(slot):  # the reference's `except StopIteration` branch (:152-153)
        slot.selected = select_random_rewrites(slot.datapoint["candidate_rewrites"], K, fallback_rng)
        slot.done = True

    def extend(layout, points, dev):
        ix = Bt.selfsup_indices(layout, points)
        entry_off = layout.rw_off.astype(np.int64) + np.arange(layout.num_samples + 1)  # sample b's n_b + 1 entries start here
        names = ("rw_idx", "rw_loc_idx", "rw_off", "nobug_idx", "entry_off")
        return dict(zip(names, Bt.to_device_i32([layout.rw_idx, ix.rw_loc_idx, layout.rw_off, ix.nobug_idx, entry_off], dev)))

    def emit():
        for slot in order.drain():
            yield slot.datapoint, slot.selected

    nn.eval()
    with torch.no_grad(), model._tensorize_all_location_rewrites():
        for mb, slots in Bt.prediction_minibatches(model, tagged(), device, parallelize, extend, rejected):
            ss = mb["selfsup"]
            B, total = len(slots), int(ss["rw_idx"].shape[0]) + len(slots)
            flat = Bt.flat_prediction_output(nn, mb)
            # torch.rand is [0, 1): the clamp keeps the Gumbel keys finite (2^-53 is below every value rand can give but 0)
            u = torch.rand(B + total, dtype=torch.float64, device=device, generator=gen).clamp_(min=2.0 ** -53)
            logprob, _, entropy, selected = hip_ops.selector_sample(
                flat, ss["rw_idx"], ss["rw_loc_idx"], ss["rw_off"], ss["nobug_idx"], u[:B], u[B:], temperature=temperature,
                epsilon=epsilon, k=K)
            start, end = ss["entry_off"][:-1].long(), ss["entry_off"][1:].long()
            picked = logprob[(start[:, None] + selected.clamp(min=0).long()).reshape(-1)]
            # the one device->host copy of the minibatch: [selection | its log-probabilities | NO_BUG's | entropy]
            back = torch.cat([selected.reshape(-1).double(), picked, logprob[end - 1], entropy]).cpu().numpy()
            sel = back[:B * K].astype(np.int64).reshape(B, K)
            sel_lp, nobug_lp, ent = back[B * K:2 * B * K].reshape(B, K), back[2 * B * K:2 * B * K + B], back[2 * B * K + B:]
            for b, slot in enumerate(slots):
                n = len(slot.datapoint["candidate_rewrites"])
                reply = {("NO_BUG" if i == n else str(i)): float(lp) for i, lp in zip(sel[b].tolist(), sel_lp[b].tolist()) if i >= 0}
                reply.setdefault("NO_BUG", float(nobug_lp[b]))  # no computational cost: always included (:146-148)
                if stats is not None:
                    stats.add(slot.datapoint, None, reply, entropy=float(ent[b]))
                slot.selected, slot.done = reply, True
            yield from emit()
    yield from emit()
    assert len(order) == 0


def parse_args(argv=None) -> argparse.Namespace:
    p = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    p.add_argument("MODEL_FILENAME", help="A trained selector checkpoint (`*.pkl.gz`).")
    p.add_argument("DATA_PATH", help="A `*.msgpack.l.gz` file, or a folder of them.")
    p.add_argument("OUT_FILENAME", help="The `*.msgpack.l.gz` file to write the selections to.")
    p.add_argument("--num-rewrites-per-sample", type=int, default=4, help="The number of rewrites to sample for each data sample.")
    p.add_argument("--temperature-scaling", type=float, default=1.0,
                   help="The temperature used to scale the bug selection distribution. Higher gives closer to uniform. [Default = 1.0]")
    p.add_argument("--epsilon", type=float, default=0.02, help="The epsilon-greedy used to use a fully random selection. [Default = 0.02]")
    p.add_argument("--seed", type=int, default=None, help="Seed of the selection; the same seed gives the same file.")
    p.add_argument("--sequential", action="store_true", help="Tensorise and collate in the calling thread.")
    return p.parse_args(argv)


def load_datapoints(path) -> Iterator[Any]:
    from buglab.utils.msgpackutils import load_all_msgpack_l_gz, load_msgpack_l_gz

    path = Path(path)
    return load_all_msgpack_l_gz(path) if path.is_dir() else load_msgpack_l_gz(path)


def run(args: argparse.Namespace) -> Dict[str, float]:
    from buglab.controllers._batching import save_msgpack_l_gz_reproducibly
    from buglab.models._cli import open_model, require_gpu

    require_gpu(None, "bugselector")
    model, nn, device, _ = open_model(args.MODEL_FILENAME)
    stats = BugSelectionStats()
    replies = select_rewrites(model, nn, load_datapoints(args.DATA_PATH), device, num_rewrites_per_sample=args.num_rewrites_per_sample,
                              temperature=args.temperature_scaling, epsilon=args.epsilon, seed=args.seed,
                              parallelize=not args.sequential, stats=stats)
    save_msgpack_l_gz_reproducibly(({"selected_rewrites": selected} for _, selected in replies), args.OUT_FILENAME)
    if stats.total_samples == 0:
        print("No datapoint reached the model.")
        return {}
    return stats.report()


if __name__ == "__main__":
    logging.basicConfig(level=logging.INFO)
    run(parse_args())

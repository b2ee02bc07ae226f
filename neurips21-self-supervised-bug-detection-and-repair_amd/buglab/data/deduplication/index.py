"""`DuplicationIndex` (reference buglab/data/deduplication/index.py:15-70) over the kernels of csrc/bl_dedup.hip.

Signatures and the band index live on the device; filenames on the host.  The arithmetic is the specification of DESIGN.md
"Near-duplicate detection" (the reference delegates it to `datasketch`): SHA-1 token hashes, 2^61 - 1 permutations from
`numpy.random.RandomState(1)`, bands chosen by the equal-weight false-positive / false-negative search.  `check_batch` answers
exactly what `check_if_duplicate_and_add` answers one document at a time in list order, for every batch split."""
import functools
import logging
from pathlib import Path
from typing import Dict, Iterable, List, Sequence, Tuple, Union

import numpy as np

LOGGER = logging.getLogger(__name__)

_MERSENNE = (1 << 61) - 1
_MIN_SLOTS = 1024  # per band; the table is rebuilt at a larger power of two whenever documents > slots / 2


def _area(f, lo: float, hi: float) -> float:
    step, area, x = 0.001, 0.0, lo
    while x < hi:  # midpoint rule; x accumulates in floating point, which fixes the number of steps
        area += f(x + 0.5 * step) * step
        x += step
    return area


@functools.lru_cache(maxsize=None)
def optimal_bands(threshold: float, num_perm: int) -> Tuple[int, int]:
    """(bands, rows) minimising 0.5 * false-positive area + 0.5 * false-negative area of the S-curve 1 - (1 - s^r)^b over
    b in 1 .. num_perm, r in 1 .. num_perm // b; the first minimum wins.  (0.85, 256) -> (13, 19)."""
    best, opt = float("inf"), (0, 0)
    for b in range(1, num_perm + 1):
        for r in range(1, num_perm // b + 1):
            fp = _area(lambda s: 1 - (1 - s ** float(r)) ** float(b), 0.0, threshold)
            fn = _area(lambda s: 1 - (1 - (1 - s ** float(r)) ** float(b)), threshold, 1.0)
            error = 0.5 * fp + 0.5 * fn
            if error < best:
                best, opt = error, (b, r)
    return opt


def permutations(num_perm: int) -> Tuple[np.ndarray, np.ndarray]:
    gen = np.random.RandomState(1)
    ab = [(gen.randint(1, _MERSENNE, dtype=np.uint64), gen.randint(0, _MERSENNE, dtype=np.uint64)) for _ in range(num_perm)]
    return np.array([a for a, _ in ab], dtype=np.uint64), np.array([b for _, b in ab], dtype=np.uint64)


def pack_tokens(token_sets: Sequence[Iterable[str]]) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
    """-> (UTF-8 bytes of all tokens back to back uint8, token offsets int64 [ntokens + 1], document offsets into the tokens
    int64 [ndocs + 1])."""
    encoded = [t.encode("utf-8") for tokens in token_sets for t in tokens]
    tok_off = np.zeros(len(encoded) + 1, dtype=np.int64)
    np.cumsum(np.fromiter(map(len, encoded), dtype=np.int64, count=len(encoded)), out=tok_off[1:])
    doc_off = np.zeros(len(token_sets) + 1, dtype=np.int64)
    np.cumsum(np.fromiter(map(len, token_sets), dtype=np.int64, count=len(token_sets)), out=doc_off[1:])
    return np.frombuffer(b"".join(encoded), dtype=np.uint8), tok_off, doc_off


class DuplicationIndex:
    """A duplication index that checks for an overlap on the tokens of indexed sets."""

    def __init__(self, checkpoint_path: Union[str, Path, None], *, duplication_jaccard_threshold: float = 0.85, num_perm: int = 256,
                 min_num_tokens: int = 10, device="cuda:0"):
        from buglab.models import hip_ops

        if not 0.0 <= duplication_jaccard_threshold <= 1.0:
            raise ValueError(f"duplication_jaccard_threshold must be in [0, 1] (got {duplication_jaccard_threshold})")
        if not 2 <= num_perm <= hip_ops.DEDUP_MAX_PERM:
            raise ValueError(f"num_perm must be in 2 .. {hip_ops.DEDUP_MAX_PERM}, what the MinHash kernel covers (got {num_perm})")
        self.threshold = float(duplication_jaccard_threshold)
        self.num_perm = int(num_perm)
        self.min_num_tokens = int(min_num_tokens)
        self.checkpoint_path = checkpoint_path
        self.bands, self.rows = optimal_bands(self.threshold, self.num_perm)
        self._device = device
        self._ops = hip_ops
        self.rebuilds = 0  # how often the band index was re-built at a larger capacity
        self.clear()

    # ---- device state --------------------------------------------------------------------------------------------------------
    def clear(self) -> None:
        """Clear the index."""
        import torch

        self._ops.load_library()
        if not torch.cuda.is_available():
            raise self._ops.HipOpsUnavailable("DuplicationIndex keeps its signatures and band index on a ROCm GPU; none is available "
                                              "(there is no CPU fallback)")
        a, b = permutations(self.num_perm)
        self._perm_a = torch.from_numpy(a.view(np.int64)).to(self._device)
        self._perm_b = torch.from_numpy(b.view(np.int64)).to(self._device)
        self._sigs = torch.empty((_MIN_SLOTS // 2, self.num_perm), dtype=torch.int32, device=self._device)
        self._status = torch.zeros(1, dtype=torch.int32, device=self._device)
        self._table = self._new_table(_MIN_SLOTS)
        self._filenames: List[str] = []
        self._known = set()

    def _new_table(self, slots: int):
        import torch

        return torch.full((self.bands, slots), self._ops.DEDUP_EMPTY_SLOT, dtype=torch.int32, device=self._device)

    def _reserve(self, total: int) -> int:
        """Room for `total` documents; -> the first document the next insert call has to file (0 after a re-build)."""
        import torch

        if total > self._sigs.shape[0]:
            grown = torch.empty((max(total, 2 * self._sigs.shape[0]), self.num_perm), dtype=torch.int32, device=self._device)
            grown[:len(self)] = self._sigs[:len(self)]
            self._sigs = grown
        if 2 * total <= self._table.shape[1]:
            return len(self)
        slots = self._table.shape[1]
        while slots < 4 * total:  # a re-build leaves the load at 1/4 or less
            slots *= 2
        self._table = self._new_table(slots)
        self.rebuilds += 1
        return 0

    def __len__(self) -> int:
        return len(self._filenames)

    # ---- the reference's interface ---------------------------------------------------------------------------------------------
    def check_if_duplicate_and_add(self, filename: str, tokens: Iterable[str]) -> bool:
        return bool(self.check_batch([filename], [tokens])[0])

    def check_batch(self, filenames: Sequence[str], token_sets: Sequence[Iterable[str]]) -> np.ndarray:
        """One answer per document, those of `check_if_duplicate_and_add` called on them in list order."""
        import torch

        if len(filenames) != len(token_sets):
            raise ValueError(f"check_batch: {len(filenames)} filenames for {len(token_sets)} token sets")
        flags = np.zeros(len(filenames), dtype=bool)
        positions, new_names, new_sets, in_batch = [], [], [], set()
        for i, (name, tokens) in enumerate(zip(filenames, token_sets)):
            tokens = tokens if isinstance(tokens, (set, frozenset)) else set(tokens)
            if len(tokens) < self.min_num_tokens:
                continue
            if name in self._known or name in in_batch:
                LOGGER.info("Duplicate key %s", name)  # (a warning in the reference: one line per document is too loud for batches)
                flags[i] = True
                continue
            in_batch.add(name)
            positions.append(i)
            new_names.append(name)
            new_sets.append(tokens)
        if not positions:
            return flags
        base, total = len(self), len(self) + len(positions)
        token_bytes, tok_off, doc_off = pack_tokens(new_sets)
        dev = self._device
        hashes = self._ops.dedup_sha1_u32(torch.from_numpy(token_bytes.copy()).to(dev), torch.from_numpy(tok_off).to(dev))
        insert_from = self._reserve(total)
        self._ops.dedup_minhash(hashes, torch.from_numpy(doc_off).to(dev), self._perm_a, self._perm_b, out=self._sigs[base:total])
        try:
            answers = self._ops.dedup_lsh_insert_query(self._sigs, self.bands, self.rows, self._table, self._status,
                                                       insert_from=insert_from, query_from=base, total=total)
            host = torch.cat([answers, self._status]).cpu().numpy()  # one copy back
            if host[-1] != 0:
                raise RuntimeError(f"DuplicationIndex: the band index reported status {int(host[-1])} (load bound broken)")
        except Exception:
            # the table may hold numbers of documents that were never recorded: re-file the recorded ones into a clean one
            self._status.zero_()
            self._table = self._new_table(self._table.shape[1])
            if base:
                self._ops.dedup_lsh_insert_query(self._sigs, self.bands, self.rows, self._table, self._status, insert_from=0,
                                                 query_from=base, total=base)
            raise
        # recorded only now that every device call went through: a failed batch leaves the index as it was
        self._filenames.extend(new_names)
        self._known.update(new_names)
        flags[positions] = host[:-1] != 0
        return flags

    # ---- state on the host -----------------------------------------------------------------------------------------------------
    def signatures(self) -> np.ndarray:
        """uint32 [len(self), num_perm], in insertion order."""
        return self._sigs[:len(self)].cpu().numpy().view(np.uint32)

    def filenames(self) -> List[str]:
        return list(self._filenames)

    def collisions(self, filenames: Sequence[str]) -> Dict[str, List[str]]:
        """For inserted documents: the documents inserted before them that share a whole band, in insertion order.  A host-side
        look-up over a copy of the signatures, meant for the few documents a report names."""
        number = {f: i for i, f in enumerate(self._filenames)}
        wanted = [f for f in filenames if f in number]
        if not wanted:
            return {}
        sigs = self.signatures()
        out = {}
        for f in wanted:
            i = number[f]
            hit = np.zeros(i, dtype=bool)
            for j in range(self.bands):
                cols = slice(j * self.rows, (j + 1) * self.rows)
                hit |= (sigs[:i, cols] == sigs[i, cols]).all(axis=1)
            out[f] = [self._filenames[k] for k in np.flatnonzero(hit)]
        return out

    def save(self) -> None:
        """Signatures and filenames as one .npz at `checkpoint_path`; the band index is re-built on load."""
        if self.checkpoint_path is None:
            raise ValueError("DuplicationIndex.save: no checkpoint_path was given")
        name_bytes, name_off, _ = pack_tokens([self._filenames])  # a blob with offsets: any string survives, trailing NULs included
        with open(self.checkpoint_path, "wb") as f:
            np.savez(f, signatures=self.signatures(), filename_bytes=name_bytes, filename_offsets=name_off,
                     duplication_jaccard_threshold=np.float64(self.threshold), num_perm=np.int64(self.num_perm),
                     min_num_tokens=np.int64(self.min_num_tokens))

    @classmethod
    def load(cls, path: Union[str, Path], device="cuda:0") -> "DuplicationIndex":
        import torch

        with np.load(path, allow_pickle=False) as z:
            blob, off = z["filename_bytes"].tobytes(), z["filename_offsets"]
            sigs, names = z["signatures"], [blob[off[i]:off[i + 1]].decode("utf-8") for i in range(len(off) - 1)]
            index = cls(path, duplication_jaccard_threshold=float(z["duplication_jaccard_threshold"]), num_perm=int(z["num_perm"]),
                        min_num_tokens=int(z["min_num_tokens"]), device=device)
        if sigs.dtype != np.uint32 or sigs.shape != (len(names), index.num_perm) or len(set(names)) != len(names):
            raise ValueError(f"{path}: not a DuplicationIndex checkpoint (signatures {sigs.dtype} {sigs.shape}, {len(names)} filenames)")
        if names:
            total = len(names)
            index._reserve(total)
            index._sigs[:total] = torch.from_numpy(sigs.view(np.int32)).to(device)
            index._filenames, index._known = names, set(names)
            index._ops.dedup_lsh_insert_query(index._sigs, index.bands, index.rows, index._table, index._status, insert_from=0,
                                              query_from=total, total=total)
        return index

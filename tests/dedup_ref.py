"""The sequential restatement of near-duplicate detection: the yardstick of tests/test_dedup_host.py and
tests/test_dedup_gpu.py.  Written from the specification in DESIGN.md ("Near-duplicate detection"), not from the device code:
`hashlib` for SHA-1, NumPy `uint64` for the permutations, one dict per band, one document at a time -- the shape of reference
buglab/data/deduplication/index.py:32-46.

The reference delegates this arithmetic to the `datasketch` package, which is not a dependency of this project and could not be run against it, so
the signatures are UNPINNED against datasketch itself: they follow its published definition as restated in DESIGN.md."""
import hashlib
import struct
from typing import Dict, Iterable, List, Sequence, Tuple

import numpy as np

MERSENNE = np.uint64((1 << 61) - 1)
MAX_HASH = np.uint64((1 << 32) - 1)


def token_hash(token: str) -> int:
    return struct.unpack("<I", hashlib.sha1(token.encode("utf-8")).digest()[:4])[0]


def permutations(num_perm: int) -> Tuple[np.ndarray, np.ndarray]:
    gen = np.random.RandomState(1)
    a, b = [], []
    for _ in range(num_perm):
        a.append(gen.randint(1, (1 << 61) - 1, dtype=np.uint64))
        b.append(gen.randint(0, (1 << 61) - 1, dtype=np.uint64))
    return np.array(a, dtype=np.uint64), np.array(b, dtype=np.uint64)


def signature(tokens: Iterable[str], perm: Tuple[np.ndarray, np.ndarray]) -> np.ndarray:
    a, b = perm
    sig = np.full(a.shape[0], MAX_HASH, dtype=np.uint64)
    with np.errstate(over="ignore"):
        for token in tokens:
            hv = np.uint64(token_hash(token))
            sig = np.minimum(sig, np.bitwise_and((a * hv + b) % MERSENNE, MAX_HASH))  # a * hv + b wraps at 64 bits
    return sig.astype(np.uint32)


def _area(f, lo: float, hi: float) -> float:
    p, area, x = 0.001, 0.0, lo
    while x < hi:
        area += f(x + 0.5 * p) * p
        x += p
    return area


def optimal_bands(threshold: float, num_perm: int) -> Tuple[int, int]:
    best, opt = float("inf"), (0, 0)
    for b in range(1, num_perm + 1):
        for r in range(1, num_perm // b + 1):
            fp = _area(lambda s: 1 - (1 - s ** float(r)) ** float(b), 0.0, threshold)
            fn = _area(lambda s: 1 - (1 - (1 - s ** float(r)) ** float(b)), threshold, 1.0)
            err = 0.5 * fp + 0.5 * fn
            if err < best:
                best, opt = err, (b, r)
    return opt


_BANDS_CACHE: Dict[Tuple[float, int], Tuple[int, int]] = {}


class RefDuplicationIndex:
    def __init__(self, *, duplication_jaccard_threshold: float = 0.85, num_perm: int = 256, min_num_tokens: int = 10):
        key = (duplication_jaccard_threshold, num_perm)
        if key not in _BANDS_CACHE:
            _BANDS_CACHE[key] = optimal_bands(*key)
        self.bands, self.rows = _BANDS_CACHE[key]
        self.perm = permutations(num_perm)
        self.min_num_tokens = min_num_tokens
        self.clear()

    def clear(self) -> None:
        self.tables: List[Dict[bytes, List[str]]] = [dict() for _ in range(self.bands)]
        self.keys: Dict[str, np.ndarray] = {}

    def __len__(self) -> int:
        return len(self.keys)

    def _band_keys(self, sig: np.ndarray) -> List[bytes]:
        return [sig[j * self.rows:(j + 1) * self.rows].tobytes() for j in range(self.bands)]

    def check_if_duplicate_and_add(self, filename: str, tokens) -> bool:
        tokens = set(tokens)
        if len(tokens) < self.min_num_tokens:
            return False
        sig = signature(tokens, self.perm)
        band_keys = self._band_keys(sig)
        close = any(k in t for k, t in zip(band_keys, self.tables))
        if filename in self.keys:
            return True
        self.keys[filename] = sig
        for k, t in zip(band_keys, self.tables):
            t.setdefault(k, []).append(filename)
        return close

    def check_batch(self, filenames: Sequence[str], token_sets: Sequence) -> np.ndarray:
        return np.array([self.check_if_duplicate_and_add(f, t) for f, t in zip(filenames, token_sets)], dtype=bool)

    def signatures(self) -> np.ndarray:
        return np.stack(list(self.keys.values())) if self.keys else np.zeros((0, self.perm[0].shape[0]), np.uint32)

    def filenames(self) -> List[str]:
        return list(self.keys)

    def collisions(self, filenames: Sequence[str]) -> Dict[str, List[str]]:
        """For inserted documents: the documents inserted before them that share a band, in insertion order."""
        order = {f: i for i, f in enumerate(self.keys)}
        out = {}
        for f in filenames:
            if f not in self.keys:
                continue
            hit = set()
            for k, t in zip(self._band_keys(self.keys[f]), self.tables):
                hit.update(g for g in t.get(k, ()) if order[g] < order[f])
            out[f] = sorted(hit, key=order.get)
        return out

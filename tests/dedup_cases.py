"""Token-set corpora for the near-duplicate tests (tests/test_dedup_host.py, tests/test_dedup_gpu.py): documents given directly
as (filename, set of tokens), in families whose answer the restatement (tests/dedup_ref.py) gives the same way for every member."""
from typing import List, Set, Tuple

import numpy as np

FAMILIES = ("base", "base", "copy", "near", "far", "short", "repeat", "base")
NEAR_REPLACED, FAR_REPLACED = 5, 40  # of 200 tokens: Jaccard 195 / 205 = 0.95 and 160 / 240 = 0.67


def _token(rng) -> str:
    word = f"tok{int(rng.integers(0, 1 << 40)):x}"
    kind = int(rng.integers(0, 12))
    if kind == 0:
        return word + "_é中\U0001f600"  # 2-, 3- and 4-byte UTF-8
    if kind == 1:
        return repr(word * int(rng.integers(2, 9)))  # a string literal, up to two SHA-1 blocks and more
    return word


def replaced(rng, tokens: Set[str], k: int) -> Set[str]:
    ordered = sorted(tokens)
    drop = set(int(i) for i in rng.choice(len(ordered), size=k, replace=False))
    kept = {t for i, t in enumerate(ordered) if i not in drop}
    while len(kept) < len(ordered):
        kept.add(_token(rng))
    return kept


def token_set_corpus(n: int, seed: int = 0, tokens_per_doc: int = 200) -> Tuple[List[str], List[Set[str]], List[str]]:
    """-> (filenames, token sets, family of each document).  "copy" / "near" / "far" derive from an earlier "base" document (the
    same tokens / NEAR_REPLACED / FAR_REPLACED of them replaced); "short" has fewer than 10 tokens; "repeat" re-uses the filename
    of an earlier document with tokens of its own."""
    rng = np.random.default_rng(seed)
    names, sets, families, bases = [], [], [], []
    for i in range(n):
        family = FAMILIES[i % len(FAMILIES)]
        name = f"pkg{i % 11}/module_{i}.py::{i}"
        if family == "base" or not bases:
            family = "base"
            tokens = set()
            while len(tokens) < tokens_per_doc:
                tokens.add(_token(rng))
            bases.append(i)
        elif family == "short":
            tokens = {_token(rng) for _ in range(int(rng.integers(0, 9)))}
        elif family == "repeat":
            name = names[int(rng.integers(0, len(names)))]
            tokens = set()
            while len(tokens) < tokens_per_doc:
                tokens.add(_token(rng))
        else:
            source = sets[bases[int(rng.integers(0, len(bases)))]]
            tokens = set(source) if family == "copy" else replaced(rng, source, NEAR_REPLACED if family == "near" else FAR_REPLACED)
        names.append(name)
        sets.append(tokens)
        families.append(family)
    return names, sets, families

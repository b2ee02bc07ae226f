"""Seeded synthetic records in the GREAT var-misuse JSON-lines format (the input of buglab/models/traingreat.py): there is no
network for the original GREAT data, so tests and tools/great_bench.py use records of the same shape.

A record: `source_tokens` (identifiers, keywords, punctuation), `edges` [[src, tgt, edge_id, edge_name], ...] over token
positions, `error_location` (0 = no bug), `repair_candidates` (positions of variable tokens), `repair_targets` (positions that
hold the variable the misused one should have been), `has_bug`, `bug_kind`, `bug_kind_name`, `provenances`.  In a buggy record
the token at `error_location` names a different candidate variable than the targets hold."""
from __future__ import annotations

import gzip
import json
import os
from typing import Dict, List

import numpy as np

EDGE_KINDS = ("enum_CFG_NEXT", "enum_LAST_READ", "enum_LAST_WRITE", "enum_COMPUTED_FROM", "enum_RETURNS_TO", "enum_FORMAL_ARG_NAME",
              "enum_FIELD", "enum_SYNTAX", "enum_NEXT_SYNTAX", "enum_LAST_LEXICAL_USE", "enum_CALLS")
_WORDS = ("value", "count", "item", "result", "index", "node", "name", "data", "total", "buffer", "path", "key", "size", "parent")
_FILLER = ("(", ")", ":", "=", "+", ".", ",", "return", "if", "for", "in", "def", "self", "None", "#NEWLINE#", "#INDENT#")


def make_great_records(num: int, seed: int = 0, min_len: int = 24, max_len: int = 120, num_edge_ids: int = 6,
                       edges_per_token: float = 1.5, buggy_fraction: float = 0.5) -> List[Dict]:
    rng = np.random.default_rng(seed)
    kinds = EDGE_KINDS[:num_edge_ids]
    out = []
    for _ in range(num):
        n = int(rng.integers(min_len, max_len + 1))
        variables = [f"{rng.choice(_WORDS)}_{int(rng.integers(0, 4))}" for _ in range(int(rng.integers(2, 6)))]
        is_var = rng.random(n) < 0.35
        is_var[1] = is_var[2] = True  # at least two variable positions after position 0
        tokens = [str(rng.choice(variables)) if v else str(rng.choice(_FILLER)) for v in is_var]
        var_pos = np.flatnonzero(is_var)
        var_pos = var_pos[var_pos > 0]
        E = int(edges_per_token * n)
        src, tgt = rng.integers(0, n, E), rng.integers(0, n, E)
        ids = rng.integers(0, len(kinds), E)
        edges = [[int(a), int(b), int(e) + 1, kinds[int(e)]] for a, b, e in zip(src, tgt, ids)]  # GREAT edge ids start at 1
        rec = {"source_tokens": tokens, "edges": edges, "bug_kind": 1, "bug_kind_name": "VARIABLE_MISUSE", "provenances": []}
        candidates = sorted({int(p) for p in var_pos})
        if rng.random() < buggy_fraction and len(set(tokens[p] for p in candidates)) >= 2:
            loc = int(rng.choice(var_pos))
            right = tokens[loc]
            wrong = str(rng.choice([v for v in {tokens[p] for p in candidates} if v != right]))
            tokens[loc] = wrong
            targets = [p for p in candidates if tokens[p] == right and p != loc]
            if not targets:  # the correct variable has no other occurrence: let it appear once more
                p = int(rng.choice([c for c in candidates if c != loc]))
                tokens[p] = right
                targets = [p]
            rec.update(has_bug=True, error_location=loc, repair_candidates=candidates, repair_targets=targets)
        else:
            rec.update(has_bug=False, error_location=0, repair_candidates=candidates, repair_targets=[])
        out.append(rec)
    return out


def write_great_dir(path: str, records: List[Dict], per_file: int = 64, prefix: str = "part") -> List[str]:
    """`records` -> `path/<prefix>-00000.jsonl.gz`, ... (`per_file` records each)."""
    os.makedirs(path, exist_ok=True)
    names = []
    for k in range(0, max(len(records), 1), per_file):
        name = os.path.join(path, f"{prefix}-{k // per_file:05d}.jsonl.gz")
        with gzip.open(name, "wt", encoding="utf-8") as f:
            for r in records[k : k + per_file]:
                f.write(json.dumps(r) + "\n")
        names.append(name)
    return names

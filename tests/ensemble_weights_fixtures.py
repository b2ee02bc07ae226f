"""Synthetic pools for the fitted-ensemble tests (tests only): the members' fp32 log-probabilities in the canonical layout, as
buglab/models/ensemble/_weights.py::LocPool / RwPool hold them."""
import numpy as np


def _log_softmax32(x):
    x = x.astype(np.float64)
    x = x - x.max()
    return (x - np.log(np.exp(x).sum())).astype(np.float32)


def edge_pools(extra_lengths=(), seed=7):
    """M = 3.  Segments of 1 (NO_BUG alone), 65, 5, 9, 2 and 33 entries (and `extra_lengths`); member 1 is absent from samples 2
    and 4; member 2 has a -inf entry in the 65-entry segment (neither the target nor NO_BUG); member 0's entry at the target of
    the 9-entry segment is -inf; targets alternate between NO_BUG and an inner entry.  The buggy samples' truth entries: one of member 0's is -inf."""
    from buglab.models.ensemble._weights import LocPool, RwPool

    rng = np.random.default_rng(seed)
    M, lengths = 3, (1, 65, 5, 9, 2, 33) + tuple(extra_lengths)
    S = len(lengths)
    off = np.zeros(S + 1, np.int64)
    np.cumsum(lengths, out=off[1:])
    vals = np.zeros((M, int(off[-1])), np.float32)
    present = np.ones((M, S), np.int32)
    present[1, [2, 4]] = 0
    tgt = np.array([n - 1 if s % 2 == 0 else (n * 2) // 3 for s, n in enumerate(lengths)], np.int32)
    for s, n in enumerate(lengths):
        for m in range(M):
            draw = rng.normal(0.0, 2.0, n)
            if m == 2 and n == 65:
                draw[11] = -np.inf
            if m == 0 and n == 9:
                draw[tgt[s]] = -np.inf  # member 0 gives this sample's target no probability: responsibility 0
            vals[m, off[s]:off[s + 1]] = _log_softmax32(draw) if present[m, s] else np.float32(np.nan)  # absent: never read
    buggy = np.flatnonzero(tgt != np.array(lengths) - 1)
    rw_vals = -np.abs(rng.normal(1.0, 1.0, (M, buggy.shape[0]))).astype(np.float32)
    rw_vals[0, 1] = -np.inf
    rw_present = present[:, buggy].copy()
    rw_vals[rw_present == 0] = np.nan
    return LocPool(vals, present, off.astype(np.int32), tgt), RwPool(rw_vals, rw_present)


def fit_pools(S=48, seed=11, absent_member=None, buggy=True):
    """M = 3 members of different quality on S samples: member 0 sees the signal sharply and is over-confident, member 1 sees it
    through noise, member 2 sees noise alone.  Member 1 drops out of every fifth sample.  `absent_member`: present nowhere."""
    from buglab.models.ensemble._weights import LocPool, RwPool

    rng = np.random.default_rng(seed)
    M = 3
    lengths = rng.integers(2, 12, S)
    off = np.zeros(S + 1, np.int64)
    np.cumsum(lengths, out=off[1:])
    vals = np.zeros((M, int(off[-1])), np.float32)
    present = np.ones((M, S), np.int32)
    present[1, ::5] = 0
    if absent_member is not None:
        present[absent_member] = 0
    tgt = np.zeros(S, np.int32)
    for s, n in enumerate(lengths):
        signal = rng.normal(0.0, 1.0, n)
        p = np.exp(1.5 * signal)
        tgt[s] = n - 1 if not buggy else rng.choice(n, p=p / p.sum())
        for m, (gain, noise) in enumerate(((4.0, 1.0), (1.0, 1.5), (0.0, 1.0))):
            vals[m, off[s]:off[s + 1]] = _log_softmax32(gain * signal + noise * rng.normal(0.0, 1.0, n))
    is_buggy = np.flatnonzero(tgt != lengths - 1)
    truth = rng.normal(0.0, 1.0, is_buggy.shape[0])
    rw_vals = np.stack([-np.abs(g * truth + rng.normal(0.0, 1.0, truth.shape[0])) for g in (0.2, 1.0, 2.0)]).astype(np.float32)
    return LocPool(vals, present, off.astype(np.int32), tgt), RwPool(rw_vals, present[:, is_buggy].copy())


def wide_samples(with_unpredicted=False):
    """Three samples of 65 location entries (64 nodes and NO_BUG: one more than a wave) and 70 rewrites for M = 3 members -- the
    `m3_65_entries` shape of tests/test_ensemble_gpu.py.  Sample 2: member 0 is absent, member 1 has a NaN and a -inf among its
    entries.  `with_unpredicted`: a fourth sample that no member predicts.  -> per sample {"nodes", "n_rw", "members": per member
    None or (location values, rewrite values) in fp32}."""
    rng = np.random.default_rng(65)
    M, n_nodes, n_rw = 3, 64, 70
    nodes = sorted(rng.choice(500, n_nodes, replace=False).tolist())
    samples = []
    for s in range(3):
        members = []
        for m in range(M):
            loc = rng.normal(-3.0, 1.0, n_nodes + 1).astype(np.float32)
            rw = rng.normal(-2.0, 1.0, n_rw).astype(np.float32)
            loc[64] = 2.0 + m
            if s == 2 and m == 1:
                loc[5], loc[9], rw[3] = np.nan, -np.inf, -np.inf
            members.append(None if (s == 2 and m == 0) else (loc, rw))
        samples.append({"nodes": nodes, "n_rw": n_rw, "members": members})
    if with_unpredicted:
        samples.append({"nodes": nodes[:6], "n_rw": 4, "members": [None] * M})
    return samples


def gather_arrays(samples):
    """The arguments of hip_ops.ensemble_combine for `samples`: src float32, loc_idx / rw_idx int32 [M, total] (-1: absent),
    loc_off / rw_off int32 [B + 1]."""
    M = len(samples[0]["members"])
    src, loc_idx, rw_idx = [np.zeros(3, np.float32)], [[] for _ in range(M)], [[] for _ in range(M)]  # three values nobody reads
    loc_off, rw_off = [0], [0]
    for s in samples:
        n_loc = len(s["nodes"]) + 1
        for m, mem in enumerate(s["members"]):
            if mem is None:
                loc_idx[m] += [-1] * n_loc
                rw_idx[m] += [-1] * s["n_rw"]
                continue
            n = sum(len(x) for x in src)
            loc_idx[m] += list(range(n, n + n_loc))
            rw_idx[m] += list(range(n + n_loc, n + n_loc + s["n_rw"]))
            src += [np.asarray(mem[0], np.float32), np.asarray(mem[1], np.float32)]
        loc_off.append(loc_off[-1] + n_loc)
        rw_off.append(rw_off[-1] + s["n_rw"])
    i32 = lambda a: np.asarray(a, np.int32).reshape(M, -1) if isinstance(a[0], list) else np.asarray(a, np.int32)
    return np.concatenate(src), i32(loc_idx), i32(loc_off), i32(rw_idx), i32(rw_off)

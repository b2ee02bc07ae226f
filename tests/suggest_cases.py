"""Shared by tests/test_suggest_host.py and tests/test_suggest_gpu.py: handmade minibatches for bl_rank_suggestions and a
literal Python restatement of its contract (include/buglab_hip.h), written without NumPy so that it shares nothing with the
twin (buglab/models/_suggest.py::rank_host) but the contract."""
import numpy as np

NAN, INF = float("nan"), float("inf")
STAGE = 4096  # SG_STAGE of csrc/bl_suggest.hip: segments of at most this many entries are staged in LDS


def minibatch(samples):
    """samples: (location values, key nodes (NO_BUG's -1 last), rewrite values, rewrite nodes, target) -> (src fp32,
    SuggestIndices); every value gets its own place in src; a rewrite whose node has no key gets rw_loc_idx -1"""
    from buglab.models._suggest import SuggestIndices

    src, loc_idx, key_node, rw_idx, rw_node, rw_loc, loc_off, rw_off, nobug, tgt = [], [], [], [], [], [], [0], [0], [], []
    for loc, keys, rw, nodes, target in samples:
        assert len(loc) == len(keys) and len(rw) == len(nodes) and keys[-1] == -1
        first = len(src)
        loc_idx += range(first, first + len(loc))
        src += list(loc)
        entry_of = {}
        for j, key in enumerate(keys[:-1]):
            entry_of.setdefault(key, first + j)
        rw_idx += range(len(src), len(src) + len(rw))
        src += list(rw)
        key_node += list(keys)
        rw_node += list(nodes)
        rw_loc += [entry_of.get(n, -1) for n in nodes]
        nobug.append(first + len(loc) - 1)
        loc_off.append(len(loc_idx))
        rw_off.append(len(rw_idx))
        tgt.append(target)
    i32 = lambda a: np.asarray(a, dtype=np.int32)
    return np.asarray(src, dtype=np.float32), SuggestIndices(i32(rw_idx), i32(rw_loc), i32(rw_off), i32(nobug), i32(tgt), i32(loc_idx),
                                                             i32(loc_off), i32(key_node), i32(rw_node))


def restate(src, ix, k, skip_nobug=False):
    """The contract, literally: sorted() with key (-value, index) over the rankable entries -> (rank [2][B], entry [B][k],
    logprob [B][k]) as Python lists"""
    read = lambda j: float(src[j]) if 0 <= j < len(src) else NAN
    rankable = lambda v: v > -INF  # False for NaN
    order_of = lambda values: sorted((i for i, v in enumerate(values) if rankable(v)), key=lambda i: (-values[i], i))
    rank, entry, logprob = [[], []], [], []
    for b in range(len(ix.tgt_rw)):
        lo, hi, r0, r1 = int(ix.loc_off[b]), int(ix.loc_off[b + 1]), int(ix.rw_off[b]), int(ix.rw_off[b + 1])
        n, target = r1 - r0, int(ix.tgt_rw[b])
        values = [read(int(ix.rw_idx[i])) + read(int(ix.rw_loc_idx[i])) for i in range(r0, r1)]
        if not skip_nobug:
            values.append(read(int(ix.nobug_idx[b])))
        order = order_of(values)
        entry.append((order + [-1] * k)[:k])
        logprob.append(([values[i] for i in order] + [-INF] * k)[:k])
        truth = (target if target < n else None) if target >= 0 else (None if skip_nobug else n)
        rank[0].append(order.index(truth) if truth in order else -1)
        loc = [read(int(j)) for j in ix.loc_idx[lo:hi]]
        nodes = [int(x) for x in ix.key_node[lo:hi]]
        if skip_nobug:
            loc, nodes = loc[:-1], nodes[:-1]
        if target < 0:
            truth = None if skip_nobug or not loc else len(loc) - 1
        elif target < n and int(ix.rw_node[r0 + target]) >= 0 and int(ix.rw_node[r0 + target]) in nodes:
            truth = nodes.index(int(ix.rw_node[r0 + target]))
        else:
            truth = None
        order = order_of(loc)
        rank[1].append(order.index(truth) if truth in order else -1)
    return rank, entry, logprob


def assert_equal_bits(got, want, where=""):
    """(rank, entry, logprob) arrays against arrays or the restatement's lists: integers equal, doubles bit for bit"""
    for name, g, w, dtype in zip(("rank", "entry", "logprob"), got, want, (np.int32, np.int32, np.float64)):
        g, w = np.asarray(g), np.asarray(w, dtype=dtype)
        assert g.dtype == dtype and g.shape == w.shape, (where, name, g.dtype, g.shape, w.shape)
        assert g.tobytes() == w.tobytes(), (where, name, np.argwhere(g != w)[:5].tolist())


def _grid(rng, n):
    """fp32 log-probabilities on a grid of a few levels: exact ties are common"""
    return (np.round(np.log(rng.uniform(0.02, 1.0, size=n)) * 2) / 2).tolist()


def _long(rng, n_rw, n_nodes=7, target=None):
    loc, rw = _grid(rng, n_nodes + 1), _grid(rng, n_rw)
    nodes = rng.integers(0, n_nodes, size=n_rw).tolist()
    return (loc, list(range(n_nodes)) + [-1], rw, nodes, int(rng.integers(0, n_rw)) if target is None else target)


def handcrafted(seed=0):
    """The smallest shapes that can break the kernel, in one minibatch -> (src, ix, {name: sample index}).  Lengths count the
    rewrites; NO_BUG adds one entry unless it is skipped."""
    rng = np.random.default_rng(seed)
    samples, at = [], {}

    def add(name, sample):
        at[name] = len(samples)
        samples.append(sample)

    add("nobug_only", ([-0.5], [-1], [], [], -1))
    # three rewrites, two of them -inf: two rankable entries with NO_BUG, one without
    add("few_rankable", ([-1.0, -2.0, -0.25], [0, 1, -1], [-INF, -0.5, -INF], [0, 1, 1], 1))
    for n in (63, 64, 65, 257):
        add(f"len{n}", _long(rng, n))
    add("stage_minus", _long(rng, STAGE - 1))  # STAGE entries with NO_BUG: the last staged length
    add("stage", _long(rng, STAGE))            # STAGE + 1 entries with NO_BUG; STAGE (staged) without
    add("stage_plus", _long(rng, STAGE + 1))   # recomputed with and without
    # the maximum at rewrites 63 and 64 (two waves of the first stride) and again at 256 (the second stride); the target is the
    # second of the three: rank 1
    rw = [-3.0] * 300
    rw[63] = rw[64] = rw[256] = -0.5
    add("tie_waves", ([-0.25, -9.0], [0, -1], rw, [0] * 300, 64))
    # all entries equal, NO_BUG included (-1.0 = -0.5 + -0.5): index order; the truth is tied with everything
    add("tie_all", ([-0.5, -0.5, -1.0], [0, 1, -1], [-0.5] * 6, [0, 1, 0, 1, 0, 1], 4))
    add("tie_nobug_truth", ([-0.5, -0.5, -1.0], [0, 1, -1], [-0.5] * 6, [0, 1, 0, 1, 0, 1], -1))
    # -inf and NaN among the rewrites and among the locations; the truth's location is NaN
    add("nan_inf", ([NAN, -0.5, -INF, -1.5], [0, 1, 2, -1], [-0.5, NAN, -0.25, -INF, -0.75, -1.0], [0, 1, 1, 1, 2, 0], 5))
    add("truth_not_rankable", ([-0.5, -1.0], [0, -1], [-INF, -0.5], [0, 0], 0))
    add("truth_nobug_not_rankable", ([-0.5, NAN], [0, -1], [-1.0], [0], -1))
    add("no_bug", ([-2.0, -1.0, -0.1], [0, 1, -1], [-0.5, -0.25], [0, 1], -1))
    # node 2 (the target's) and node 3 have no key: their rewrites are NaN, the location rank is -1
    add("target_without_key", ([-0.5, -1.0, -2.0], [0, 1, -1], [-0.5, -0.1, -0.2, -0.3], [0, 2, 1, 3], 1))
    add("target_out_of_range", ([-0.5, -1.0], [0, -1], [-0.5, -0.25], [0, 0], 2))
    add("out_of_range_indices", ([-0.5, -1.0, -1.5], [0, 1, -1], [-0.5, -0.25, -0.75, -1.0], [0, 1, 0, 1], 0))
    src, ix = minibatch(samples)
    b = at["out_of_range_indices"]
    r0, l0 = int(ix.rw_off[b]), int(ix.loc_off[b])
    ix.rw_idx[r0 + 1] = src.shape[0]        # one past the end
    ix.rw_loc_idx[r0 + 2] = -7              # negative, and not the -1 of "no key"
    ix.rw_idx[r0 + 3] = np.iinfo(np.int32).max
    ix.loc_idx[l0 + 1] = src.shape[0] + 5
    return src, ix, at


def drawn(seed, B=40):
    """B samples on a coarse grid (ties everywhere) with -inf, NaN and keyless nodes sprinkled in; NaN-free when seed < 0"""
    rng = np.random.default_rng(abs(seed))
    clean = seed < 0
    samples = []
    for b in range(B):
        n_nodes = int(rng.integers(1, 12))
        keys = rng.permutation(n_nodes)[:n_nodes if clean else int(rng.integers(1, n_nodes + 1))].tolist()
        n_rw = int(rng.integers(0, 600 if b % 10 == 5 else 40))

        def draw(n):
            v = np.asarray(_grid(rng, n), dtype=np.float64)
            if not clean:
                v = np.where(rng.uniform(size=n) < 0.15, -INF, np.where(rng.uniform(size=n) < 0.03, NAN, v))
            return v.tolist()

        nodes = (rng.choice(keys, size=n_rw) if clean else rng.integers(0, n_nodes, size=n_rw)).tolist()
        target = int(rng.integers(0, n_rw)) if n_rw and rng.uniform() < 0.6 else -1
        samples.append((draw(len(keys) + 1), keys + [-1], draw(n_rw), nodes, target))
    return minibatch(samples)

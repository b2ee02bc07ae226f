"""The cases of tests/test_explain_host.py and tests/test_explain_gpu.py (not a test itself): node scores and graph layouts for
bl_attr_topk, operand pairs for bl_attr_node_scores, and the contract restated in plain Python loops."""
import math

import numpy as np

SIZES = (0, 1, 63, 64, 65, 255, 256, 257, 1000)  # nodes per graph: around the wave (64) and the workgroup (256)
WIDTHS = (1, 3, 32, 64, 65, 128, 257)            # D: below a quad, a partial quad, one pass of 64 quads = 256 columns and beyond
TIE = 9.5


def _grid(rng, n):
    """multiples of 1/2 in [-4, 4]: every sum of a few thousand of them is exact in fp64, whatever the order"""
    return rng.integers(-8, 9, size=n).astype(np.float64) / 2


def handmade(seed=0):
    """-> (score float64 [N], node_off int32 [B + 1], at: name -> graph).  Graphs of SIZES nodes, alternately on the grid of
    halves (sums exact) and drawn (sums not exact), then the special ones."""
    rng = np.random.default_rng(seed)
    graphs, at = [], {}
    for i, n in enumerate(SIZES):
        at[f"n{n}"] = len(graphs)
        graphs.append(_grid(rng, n) if i % 2 == 0 else rng.standard_normal(n))
    tie = _grid(rng, 300)  # |a| equal at local nodes 63, 64 and 256: a tie across lanes, waves and the workgroup's stride
    tie[63], tie[64], tie[256] = -TIE, TIE, TIE
    at["tie_waves"] = len(graphs)
    graphs.append(tie)
    pm = _grid(rng, 10)  # +v and -v of the same magnitude, the negative one first
    pm[2], pm[5] = -7.0, 7.0
    at["plus_minus"] = len(graphs)
    graphs.append(pm)
    one = rng.standard_normal(70)
    one[10] = np.nan
    at["one_nan"] = len(graphs)
    graphs.append(one)
    at["all_nan"] = len(graphs)
    graphs.append(np.full(5, np.nan))
    at["few"] = at["n1"]  # fewer nodes than any k > 1
    off = np.concatenate([[0], np.cumsum([g.shape[0] for g in graphs])]).astype(np.int32)
    return np.concatenate(graphs), off, at


def drawn(seed, B=40):
    """-> (score, node_off): B graphs of 0 .. 600 nodes, scores rounded to one decimal (many ties)"""
    rng = np.random.default_rng(1000 + seed)
    sizes = rng.integers(0, 601, size=B)
    off = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int32)
    return np.round(rng.standard_normal(int(off[-1])) * 3, 1), off


def operands(D, seed=0, N=11):
    """-> (x, g) float32 [N, D]: the first rows on the grid of halves (every product and sum exact), the others drawn.  N = 11: three
    workgroups of four waves, the last one not full."""
    rng = np.random.default_rng(100 * D + seed)
    x, g = rng.standard_normal((N, D)), rng.standard_normal((N, D))
    x[:N // 2], g[:N // 2] = _grid(rng, (N // 2, D)), _grid(rng, (N // 2, D))
    return x.astype(np.float32), g.astype(np.float32)


# ------------------------------------------------------------------------------------------------
# the contract, literally
def butterfly(lanes):
    """64 values -> lane 0's value after the xor butterfly, strides 32 .. 1"""
    v = list(lanes)
    assert len(v) == 64
    for o in (32, 16, 8, 4, 2, 1):
        v = [v[l] + v[l ^ o] for l in range(64)]
    return v[0]


def restate_node_scores(x, g, score=None, weight=1.0):
    N, D = x.shape
    out = []
    for n in range(N):
        lanes = [0.0] * 64
        for c in range(D):  # ascending columns; column c belongs to lane (c // 4) % 64
            lanes[(c // 4) % 64] = lanes[(c // 4) % 64] + float(x[n, c]) * float(g[n, c])
        t = float(weight) * butterfly(lanes)
        out.append(t if score is None else float(score[n]) + t)
    return np.asarray(out, dtype=np.float64)


def restate_block_sum(values):
    threads = [0.0] * 256
    for i, v in enumerate(values):  # thread t adds nodes t, t + 256, .. in that order
        threads[i % 256] = threads[i % 256] + float(v)
    waves = [butterfly(threads[64 * w:64 * w + 64]) for w in range(4)]
    return ((waves[0] + waves[1]) + waves[2]) + waves[3]


def restate_topk(score, node_off, k, by_abs=True):
    B = len(node_off) - 1
    node, picked, sums = np.full((B, k), -1, np.int32), np.zeros((B, k), np.float64), np.zeros((2, B), np.float64)
    for b in range(B):
        a = [float(v) for v in score[node_off[b]:node_off[b + 1]]]
        sums[0, b], sums[1, b] = restate_block_sum(a), restate_block_sum([abs(v) for v in a])
        key = [abs(v) for v in a] if by_abs else a
        prev = None
        for r in range(k):  # k rounds: the first maximum among the nodes strictly after the previous pick
            best = None
            for i, v in enumerate(key):
                if math.isnan(v):
                    continue
                if prev is not None and not (key[prev] > v or (key[prev] == v and prev < i)):
                    continue
                if best is None or v > key[best]:  # ascending i: an equal key later never replaces
                    best = i
            if best is None:
                break
            node[b, r], picked[b, r] = best, a[best]
            prev = best
    return node, picked, sums


def assert_equal_bits(got, want, where=""):
    assert len(got) == len(want)
    for name, a, b in zip(("node / scores", "score", "sums"), got, want):
        a, b = np.asarray(a), np.asarray(b)
        assert a.dtype == b.dtype and a.shape == b.shape, (where, name, a.dtype, b.dtype, a.shape, b.shape)
        assert a.tobytes() == b.tobytes(), (where, name, np.argwhere(~((a == b) | ((a != a) & (b != b))))[:5])

"""What the FDR tests share (tests/test_fdr_host.py, tests/test_fdr_gpu.py): the contract of include/buglab_hip.h::bl_fdr_counts /
bl_fdr_bh restated in plain Python loops -- Python ints and floats, no NumPy arithmetic, so the twin and the restatement cannot
share a vectorisation mistake -- a sort-based textbook Benjamini-Hochberg, the case builders, and bit-exact comparison."""
import math

import numpy as np

NAN = float("nan")


# ---- the contract, in loops --------------------------------------------------------------------------------------------------
def restate_counts(src, nobug_idx, ref):
    """(score float32 [B], count int32 [B]): s = src[idx] (NaN outside src), c = #{j : ref[j] <= s}, n for a NaN s"""
    n = len(ref)
    score = np.empty(len(nobug_idx), np.float32)
    count = np.empty(len(nobug_idx), np.int32)
    for b, j in enumerate(nobug_idx):
        j = int(j)
        s = src[j] if 0 <= j < len(src) else np.float32(NAN)
        score[b] = s  # (a float32 assignment keeps a NaN's bits)
        if s != s:
            count[b] = n
            continue
        c = 0
        for r in ref:
            if r <= s:  # fp32 compares as IEEE makes them: -0.0 == 0.0
                c += 1
        count[b] = c
    return score, count


def restate_bh(count, n_ref, q):
    """(cutoff [2], flag [N], q_value [N], R [n_ref + 1]) by the definitions, one bin at a time"""
    N, n = len(count), int(n_ref)
    clamped = [min(max(int(c), 0), n) for c in count]
    hist = [0] * (n + 1)
    for c in clamped:
        hist[c] += 1
    R, run = [], 0
    for c in range(n + 1):
        run += hist[c]
        R.append(run)
    cut = -1
    for c in range(n + 1):
        if R[c] > 0 and float((c + 1) * N) <= q * float((n + 1) * R[c]):  # an exact integer against ONE rounded product
            cut = c
    table, least = [math.inf] * (n + 1), math.inf
    for c in range(n, -1, -1):
        if R[c] > 0:
            least = min(least, min(1.0, float((c + 1) * N) / float((n + 1) * R[c])))  # one correctly rounded quotient
        table[c] = least
    return (np.array([cut, R[cut] if cut >= 0 else 0], np.int32), np.array([1 if c <= cut else 0 for c in clamped], np.int32),
            np.array([table[c] for c in clamped], np.float64), np.array(R, np.int32))


def textbook_bh(count, n_ref, q):
    """The step-up as the textbooks state it: sort the p-values, take the largest k with p_(k) <= q k / N, reject the k
    smallest.  p_(k) = (c_(k) + 1) / (n + 1), and the comparison is made in the contract's form, (c_(k) + 1) N <= q (n + 1) k.
    Within a group of equal p-values the largest k decides, so the rejected set is `p <= p_(k*)`.  bool [N]."""
    N, n = len(count), int(n_ref)
    order = sorted(range(N), key=lambda i: int(count[i]))
    k_star = 0
    for k in range(1, N + 1):
        c = min(max(int(count[order[k - 1]]), 0), n)
        if float((c + 1) * N) <= q * float((n + 1) * k):
            k_star = k
    flagged = np.zeros(N, bool)
    if k_star:
        bar = min(max(int(count[order[k_star - 1]]), 0), n)
        for i in range(N):
            flagged[i] = min(max(int(count[i]), 0), n) <= bar
    return flagged


# ---- comparison --------------------------------------------------------------------------------------------------------------
def assert_equal_bits(got, want, where=""):
    assert len(got) == len(want), where
    for k, (a, b) in enumerate(zip(got, want)):
        a, b = np.asarray(a), np.asarray(b)
        assert a.dtype == b.dtype and a.shape == b.shape, (where, k, a.dtype, b.dtype, a.shape, b.shape)
        if a.tobytes() != b.tobytes():
            bad = np.flatnonzero(a.reshape(-1).view(np.uint8 if a.itemsize == 1 else f"u{a.itemsize}")
                                 != b.reshape(-1).view(np.uint8 if b.itemsize == 1 else f"u{b.itemsize}"))
            raise AssertionError(f"{where}: output {k} differs at {bad[:8].tolist()} ({bad.shape[0]} places): "
                                 f"{a.reshape(-1)[bad[:8]].tolist()} != {b.reshape(-1)[bad[:8]].tolist()}")


# ---- case builders -----------------------------------------------------------------------------------------------------------
SPECIALS = np.array([-np.inf, np.inf, -0.0, 0.0, NAN, -1.5, 2.5], np.float32)


def reference(n_ref, seed):
    """n_ref sorted fp32 scores on a grid of halves (many ties), with -0.0, 0.0 and both infinities among them from 8 entries
    on; no NaN"""
    rng = np.random.default_rng([seed, n_ref])
    ref = (np.round(rng.normal(-2.0, 2.0, size=n_ref) * 2) / 2).astype(np.float32)
    if n_ref >= 8:
        ref[:4] = [-np.inf, np.inf, -0.0, 0.0]
    ref = np.sort(ref)
    assert ref.shape[0] == n_ref and not np.isnan(ref).any()
    return ref


def counts_case(B, n_ref, seed):
    """(src, nobug_idx, ref): scores on the reference's grid (ties with its entries, the `<=` boundary), between its entries,
    NaN, +-inf and both zeros; indices that reach every special value, -1 and n_src"""
    rng = np.random.default_rng([seed, B, n_ref, 1])
    ref = reference(n_ref, seed)
    n_src = 3 * B + SPECIALS.shape[0] + 5
    src = (np.round(rng.normal(-2.0, 2.5, size=n_src) * 4) / 4).astype(np.float32)  # quarters: on and between the halves
    src[:SPECIALS.shape[0]] = SPECIALS
    src[SPECIALS.shape[0]:SPECIALS.shape[0] + 3] = ref[[0, n_ref // 2, n_ref - 1]]  # exactly a reference entry
    idx = rng.integers(0, n_src, size=B).astype(np.int32)
    take = min(B, SPECIALS.shape[0] + 3)
    idx[:take] = np.arange(take)
    if B >= 16:
        idx[-1], idx[-2], idx[-3] = -1, n_src, n_src + 7
    return src, idx, ref


def bh_counts(N, n_ref, kind, seed=0):
    """int32 [N] counts against a reference of n_ref scores.  mixed: a fifth of the samples low (the discoveries), the rest
    uniform over [0, n_ref], a few out of range (clamped); equal: one value in the middle; top: all n_ref; bottom: all 0"""
    rng = np.random.default_rng([seed, N, n_ref, 2])
    if kind == "equal":
        return np.full(N, n_ref // 2, np.int32)
    if kind == "top":
        return np.full(N, n_ref, np.int32)
    if kind == "bottom":
        return np.zeros(N, np.int32)
    assert kind == "mixed"
    count = rng.integers(0, n_ref + 1, size=N).astype(np.int32)
    low = rng.random(N) < 0.2
    count[low] = rng.integers(0, max(1, n_ref // 50) + 1, size=int(low.sum()))
    if N >= 64:
        count[5], count[6] = -3, n_ref + 9
    return count


def simulate_fdp(rng, n_ref, N, share_buggy, shift, q, scans):
    """`scans` simulated scans: clean scores standard normal as fp32, buggy ones the same shifted down by `shift`, a fresh
    reference of n_ref clean scores per scan; round(share_buggy N) samples are buggy.  The false discovery proportion (false
    alarms / max(flagged, 1)) and the share of buggy samples flagged of every scan."""
    from buglab.models._fdr import bh_host, counts_host

    num_buggy = int(round(share_buggy * N))
    fdp, power = np.empty(scans), np.empty(scans)
    identity = np.arange(N)
    for t in range(scans):
        ref = np.sort(rng.standard_normal(n_ref).astype(np.float32))
        scores = rng.standard_normal(N).astype(np.float32)
        scores[:num_buggy] -= np.float32(shift)
        _, count = counts_host(scores, identity, ref)
        flag = bh_host(count, n_ref, q)[1] != 0
        fdp[t] = flag[num_buggy:].sum() / max(int(flag.sum()), 1)
        power[t] = flag[:num_buggy].mean() if num_buggy else 0.0
    return fdp, power

"""Small hand-built graphs for svt_kernel (csrc/mvmc_svt.hip), deterministic from fixed seeds, and the rule that admits a graph to
the device gates (tests/test_gpu_svt_small.py).  tests/test_svt_cases_cpu.py checks the set on the CPU.

Affinities come from planted identities: the same person seen in two groups gets uniform [0.7, 1.0], everything else uniform
[0, 0.3], symmetrised; about 15 % of the nodes are junk (nobody).  Three graphs per shape, the third quantised to multiples of 1/64
so that equal entries occur.  The shapes are the smallest at which each path of the kernel can go wrong."""
import functools

import numpy as np

import oracle_np as o
import svt_np

MARGIN = 1e-6      # every decision of an admitted graph is at least this far (relative) from its threshold, |X - 0.5| absolute
X_TOL = 1e-9       # the bar on X, device against restatement and restatement against oracle: a factor 1000 inside MARGIN
N_MAX, G_MAX, GROUPS = 64, 16, 16

SHAPES = {
    "n1": [1], "n2": [1, 1],                      # ([1, 1] is also the two-singleton-groups shape)
    "n3": [2, 1], "n4": [2, 2], "n5": [2, 3], "n6": [3, 2, 1], "n7": [3, 4], "n8": [3, 3, 2], "n9": [4, 3, 2],
    "singletons16": [1] * 16,
    "gaps": [3, 0, 2, 0, 4, 0, 0, 1],             # empty groups between non-empty ones
    "four8": [8] * 4, "four9": [9] * 4,           # either side of the svt_kernel<TS, 8> / <TS, 16> boundary
    "four16": [16] * 4,                           # n = 64 at g_max = 16
    "ragged16": [16, 1, 0, 9, 2],
    "sixteen4": [4] * 16,                         # G = 16, n = 64
    "n63_w8": [8] * 7 + [7], "n63_w9": [9] * 7,   # n = 63: the Jacobi pairing needs the pad row
    "mixed": [12, 11, 10, 12, 12],
    "single5": [5],                               # one group: nothing can pair
}
# a shape whose graph came out within MARGIN of a decision gets another seed here, not another margin
RESEED = {}
DEGENERATE = ("zero", "constant", "twins", "fast", "round10")
ROUND10 = [[2, 950, 30, 365, 510, 471, 53, 772, 864], [950, 847, 113, 239, 236, 174, 39, 678, 672],
           [30, 113, 593, 851, 189, 834, 291, 734, 741], [365, 239, 851, 1005, 756, 814, 673, 842, 744],
           [510, 236, 189, 756, 181, 854, 435, 541, 480], [471, 174, 834, 814, 854, 809, 403, 719, 312],
           [53, 39, 291, 673, 435, 403, 523, 1024, 391], [772, 678, 734, 842, 541, 719, 1024, 643, 722],
           [864, 672, 741, 744, 480, 312, 391, 722, 574]]


def planted(counts, seed, quantise=False):
    rng = np.random.RandomState(seed)
    n = int(np.sum(counts))
    pool = max(2, int(np.max(counts)))
    who = np.full(n, -1)
    at = 0
    for c in counts:
        ids = rng.permutation(pool)[:c]
        ids[rng.rand(c) < 0.15] = -1
        who[at:at + c] = ids
        at += c
    grp = np.repeat(np.arange(len(counts)), counts)
    same = (who[:, None] == who[None, :]) & (who[:, None] >= 0) & (grp[:, None] != grp[None, :])
    A = np.where(same, rng.uniform(0.7, 1.0, (n, n)), rng.uniform(0.0, 0.3, (n, n)))
    S = 0.5 * (A + A.T)
    if quantise:
        S = np.round(S * 64) / 64
    return S


def _degenerate(name):
    if name == "zero":
        counts = [3, 3, 2]
        return np.zeros((8, 8)), counts
    if name == "constant":     # one value across groups: M has repeated eigenvalues
        counts = [3, 3, 3]
        grp = np.repeat(np.arange(3), counts)
        return np.where(grp[:, None] != grp[None, :], 0.8, 0.0), counts
    if name == "twins":
        # two people seen identically in every view: duplicate rows, a rank-2 S and a rank-deficient M.  The affinity is weak on
        # purpose: from 0.12 up the block projection splits each twin row into (0.5, 0.5) to within rounding, where X > 0.5 has no
        # answer to gate (the restatement and the oracle themselves disagree on x_bin there)
        counts = [3, 3, 3, 3]
        who = np.tile([0, 0, 2], 4)
        return np.where(who[:, None] == who[None, :], 0.1, 0.05), counts
    if name == "round10":
        # found by a random search over symmetric 9 x 9 matrices in multiples of 1/1024, for a block whose alternating projection
        # still moves by more than 1e-2 per entry after nine rounds (none of the planted graphs has one)
        counts = [3, 3, 3]
        return np.array(ROUND10, dtype=np.float64) / 1024, counts
    if name == "fast":         # three isolated nodes: converges within three calls at the default tol
        counts = [1, 1, 1]
        return np.full((3, 3), 1.0 / 64), counts
    raise KeyError(name)


@functools.lru_cache(maxsize=None)
def names():
    return tuple(f"{s}/{k}" for s in SHAPES for k in range(3)) + tuple(f"degenerate/{d}" for d in DEGENERATE)


def shape_of(name):
    return name.split("/")[0]


@functools.lru_cache(maxsize=None)
def case(name):
    """-> (S float64 (n,n), counts list)"""
    s, k = name.split("/")
    if s == "degenerate":
        S, counts = _degenerate(k)
        return np.ascontiguousarray(S, dtype=np.float64), list(counts)
    counts = SHAPES[s]
    seed = RESEED.get(name, 7000 + 10 * list(SHAPES).index(s) + int(k))
    return planted(counts, seed, quantise=(k == "2")), list(counts)


def case_input(name, dtype):
    S, counts = case(name)
    return S.astype(dtype), counts


def restated(name, dtype=np.float64):
    """The restatement's run of the case at the default options: (X, x_bin, calls, rec).  Computed once, never modified."""
    return _restated(name, np.dtype(dtype))


@functools.lru_cache(maxsize=None)
def _restated(name, dtype):
    S, counts = case_input(name, dtype)
    if dtype == np.float32 and np.array_equal(S.astype(np.float64), case(name)[0]):
        return restated(name)      # (the quantised graphs are exact in float32)
    out = svt_np.match_svt(S, counts)
    for a in out[:2]:
        a.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def oracle(name):
    """oracle_np.match_svt (SVD form) on the float64 case: (X, x_bin, calls in the device's convention)."""
    S, counts = case(name)
    dim = np.concatenate([[0], np.cumsum(counts)])
    _, xb, info = o.match_svt(S, dim, return_info=True)
    calls = info["iter"] + 1 if info["iter"] < 20 else 20
    return info["X"], xb, calls


def clear(rec):
    return rec["margin_half"] >= MARGIN and rec["margin"] >= MARGIN


@functools.lru_cache(maxsize=None)
def agrees(name):
    X, xb, calls, _ = restated(name)
    Xo, xbo, co = oracle(name)
    return bool(calls == co and np.array_equal(xb, xbo) and (X.size == 0 or np.abs(X - Xo).max() <= X_TOL))


def admitted(dtype=np.float64):
    return _admitted(np.dtype(dtype))


@functools.lru_cache(maxsize=None)
def _admitted(dtype):
    """The cases the device gates run for this input type: the restatement agrees with the oracle on the float64 case, and every
    decision of the restatement's run ON THIS INPUT is clear of its threshold."""
    return tuple(nm for nm in names() if agrees(nm) and clear(restated(nm)[3]) and clear(restated(nm, dtype)[3]))


def labels(x_bin):
    n = x_bin.shape[0]
    return o.cluster_labels(o.transform_closure(x_bin), n)


def n_clusters(x_bin):
    """The columns parse_match_result keeps (oracle_np.cluster_labels' rule): on an x_bin that is no matching, some stay empty."""
    return int((o.transform_closure(x_bin).astype(np.float64).sum(axis=0) > 1.9).sum())


def batch(cases, dtype, n_max=N_MAX, groups=GROUPS):
    """[(S, counts)] -> S (B, n_max, n_max) dtype (zero padded), counts (B, groups) int32"""
    S = np.zeros((len(cases), n_max, n_max), dtype=dtype)
    cnt = np.zeros((len(cases), groups), dtype=np.int32)
    for k, (s, c) in enumerate(cases):
        n = s.shape[0]
        S[k, :n, :n] = s
        cnt[k, :len(c)] = c
    return S, cnt

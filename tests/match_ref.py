"""The yardstick of the matching tests: the "Matching" section of include/geglove.h in numpy, operation for operation.  Never
the library itself.

Prepared rows come from kmeans_ref.prepare, scores from chain_ref.chain (the fp32 fmaf chain from +0 over ascending d), the pair
list is the header's rule (a < b, s >= T as fp32 compares, a NaN counting as -inf, ascending (a, b)), and the components come
from a plain sequential union-find labelled by the smallest id.  The model inherits chain's conditions: no nonzero product below
2^-100, finite partial sums (asserted where the tables are built).

The designed families the tests share are built here too, each with the structure it is named for; test_match_ref.py checks
that structure without a device."""
import functools

import numpy as np

import chain_ref as CH
import kmeans_ref as KR
import nn_ref as NR

F32 = np.float32
MODEL_METRIC = {"cosine": KR.COSINE, "dot": KR.EUCLID}      # kmeans_ref.prepare: EUCLID leaves the rows as they are, as DOT does


def scores(X, metric):
    """(prepared rows, fp32 [n][n] chain scores of every row against every row)."""
    XH = KR.prepare(X, MODEL_METRIC[metric])
    return XH, CH.chain(XH, XH)


def pair_list(S, ids, T):
    """All pairs of positions p < q with S[p, q] >= T under fp32 compare (NaN as -inf), as (a, b, score) with a = ids[p],
    b = ids[q], in ascending (a, b): ids ascend with the position, so that is the row-major order of the upper triangle."""
    S = CH.ranked(S)
    n = S.shape[0]
    ids = np.asarray(ids, np.int64)
    assert np.all(np.diff(ids) > 0)
    p, q = np.triu_indices(n, 1)                                  # row-major: ascending (p, q)
    keep = S[p, q] >= F32(T)
    return ids[p[keep]].astype(np.int32), ids[q[keep]].astype(np.int32), S[p[keep], q[keep]].astype(F32), p[keep], q[keep]


def components(n, p, q, ids):
    """label[position] = the smallest id of its component, by a sequential union-find over the pairs of positions."""
    parent = list(range(n))

    def find(x):
        while parent[x] != x:
            parent[x] = parent[parent[x]]
            x = parent[x]
        return x

    for u, v in zip(p.tolist(), q.tolist()):
        ru, rv = find(u), find(v)
        if ru != rv:
            parent[max(ru, rv)] = min(ru, rv)
    root = np.array([find(x) for x in range(n)], np.int64)
    assert all(root[x] <= x for x in range(n))                     # the root is the smallest position, hence the smallest id
    return np.asarray(ids, np.int64)[root].astype(np.int32)


def summary(label, pairs):
    _, counts = np.unique(label, return_counts=True)
    big = counts[counts >= 2]
    return {"pairs": int(pairs), "components": int(counts.size), "groups": int(big.size), "grouped_rows": int(big.sum()),
            "largest": int(counts.max())}


def match_scores(S, ids, T):
    """(a, b, score, label, summary) from a score matrix over the indexed rows."""
    a, b, s, p, q = pair_list(S, ids, T)
    label = components(S.shape[0], p, q, ids)
    return a, b, s, label, summary(label, a.size)


def match(X, metric, T, subset=None):
    X = np.ascontiguousarray(X, F32)
    ids = np.arange(X.shape[0]) if subset is None else np.asarray(subset, np.int64)
    _, S = scores(X[ids], metric)
    return match_scores(S, ids, T)


def below(x):
    """The fp32 value one ulp below x."""
    return np.nextafter(F32(x), F32(-np.inf))


# ----------------------------------------------------------------------------------------------------------------------
# Tile edges: general floats, the second half of every table a copy of the first (duplicates and exact ties).  Under cosine a
# table of dim 1 has scores in {-1, 0, +1} only, so between 1 % and 20 % of its pairs can qualify only if many rows are zero
# rows: at dim 1 five in eight of the rows of the first half are zero rows, at every other dim one in eight (a zero row is an edge of its
# own: it stays zero under cosine and scores 0 against everything).
# ----------------------------------------------------------------------------------------------------------------------
TILE_SIZES = (63, 64, 65, 127, 128, 129, 193, 300)          # the query tile holds 64 rows, the candidate tile 128
TILE_DIMS = (1, 3, 4, 31, 32, 33, 200)                      # below / at / above the panel of 32 columns, no multiple of 4
METRICS = ("cosine", "dot")
SHARE = (0.01, 0.20)


def tile_rows(dim, n):
    seed = 9000 + 7 * dim + n
    X = NR.random_rows(seed, n, dim)
    zero = NR.integers(seed ^ 0x5A5A, (n,), 0, 7) < (5 if dim == 1 else 1)
    X[zero] = 0
    h = n // 2
    X[h:2 * h] = X[:h]
    return X


@functools.lru_cache(maxsize=None)
def tile_case(dim, n, metric):
    """(rows, scores, T, share): T is an attained score, the smallest one that at most 15 % of the upper triangle's scores
    reach (the largest score where even that one is reached by more); `share` is the fraction of pairs at or above it."""
    X = tile_rows(dim, n)
    _, S = scores(X, metric)
    assert np.all(np.isfinite(S))
    p, q = np.triu_indices(n, 1)
    upper = np.sort(S[p, q])[::-1]
    T = F32(upper[int(0.15 * upper.size)])
    if (upper >= T).sum() > 0.15 * upper.size:                    # ties carry it past 15 %: the next attained score above, if any
        above = upper[upper > T]
        T = F32(above[-1] if above.size else upper[0])
    share = float((upper >= T).sum()) / upper.size
    for arr in (X, S):
        arr.setflags(write=False)
    return X, S, T, share


# ----------------------------------------------------------------------------------------------------------------------
# Exactly at the threshold: integer-valued rows under dot whose scores are exact integers in [2^23, 2^24), where one ulp is 1:
# row r = (2900, u_r, v_r, 1) with u, v in [-8, 8], so s(a, b) = 8 410 001 + u_a u_b + v_a v_b, every product and partial sum
# exact.  T is an attained score; the scores T - 1 -- one ulp below -- are attained too.
# ----------------------------------------------------------------------------------------------------------------------
AT_BASE = 2900 * 2900 + 1


@functools.lru_cache(maxsize=None)
def threshold_case(n=200):
    X = np.empty((n, 4), F32)
    X[:, 0], X[:, 3] = 2900, 1
    X[:, 1] = NR.integers(31, (n,), -8, 8)
    X[:, 2] = NR.integers(32, (n,), -8, 8)
    _, S = scores(X, "dot")
    exact = X.astype(np.float64) @ X.astype(np.float64).T
    assert np.array_equal(S.astype(np.float64), exact) and exact.min() >= 2 ** 23 and exact.max() < 2 ** 24
    T = F32(AT_BASE + 40)
    for arr in (X, S):
        arr.setflags(write=False)
    return X, S, T


# ----------------------------------------------------------------------------------------------------------------------
# Components: rows of zeros and ones under dot, T = 1.  A graph's vertex holds a one in the column of every edge it touches, so
# two vertices score the number of edges they share: 1 when adjacent, 0 otherwise.  Ids are shuffled by a fixed permutation, so
# labels cannot settle in id order.
# ----------------------------------------------------------------------------------------------------------------------
def permutation(n, seed):
    return np.argsort(NR.integers(seed, (n,), 0, 2 ** 30), kind="stable")


@functools.lru_cache(maxsize=None)
def path_case():
    """A path of 511 rows at dim 512: path vertex r holds ones at columns r and r + 1 and lives at row perm[r].
    Returns (rows, scores, perm)."""
    n = 511
    perm = permutation(n, 77)
    X = np.zeros((n, 512), F32)
    X[perm, np.arange(n)] = 1
    X[perm, np.arange(n) + 1] = 1
    _, S = scores(X, "dot")
    for arr in (X, S, perm):
        arr.setflags(write=False)
    return X, S, perm


def graph_rows(n, edges, perm):
    X = np.zeros((n, len(edges)), F32)
    for e, (u, v) in enumerate(edges):
        X[perm[u], e] = 1
        X[perm[v], e] = 1
    return X


@functools.lru_cache(maxsize=None)
def forest_case():
    """Two paths of 150 vertices joined by one pair, a star of 100 leaves, and 30 isolated vertices, interleaved by the
    permutation.  Returns (rows, scores, perm, edges, vertex ranges)."""
    A, B, star, iso = range(0, 150), range(150, 300), range(300, 401), range(401, 431)
    edges = [(r, r + 1) for r in range(0, 149)] + [(r, r + 1) for r in range(150, 299)] + [(74, 225)]
    edges += [(300, leaf) for leaf in range(301, 401)]
    n = 431
    perm = permutation(n, 78)
    X = graph_rows(n, edges, perm)
    _, S = scores(X, "dot")
    for arr in (X, S, perm):
        arr.setflags(write=False)
    return X, S, perm, tuple(edges), (A, B, star, iso)

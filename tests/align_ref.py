"""The yardstick of the alignment tests: the "Alignment" section of include/geglove.h in numpy and plain Python, operation for
operation.  Never the library itself.

Prepared rows come from kmeans_ref.prepare (through match_ref), scores from chain_ref.chain over X[source] x X[target] (the fp32
fmaf chain from +0 over ascending d, a NaN counting as -inf), the candidate list is the header's rule, and the assignment is
written twice, independently: `greedy` sorts the candidates by the header's order and walks them; `rounds` runs the synchronous
rounds of the locally-dominant rule on per-vertex lists and also returns the number of assigning rounds and the pairs of round
1.  `blocking_pairs` lists the candidates that are ahead of both their ends' assigned pairs: the greedy set has none.

The designed families the tests share are built here too, each with the structure it is named for; test_align_ref.py checks
that structure, and that the two assignments agree, without a device."""
import functools

import numpy as np

import chain_ref as CH
import match_ref as M

F32 = np.float32
METRICS = M.METRICS
SHARE = (0.01, 0.20)


def scores(X, source, target, metric):
    """fp32 [nA][nB]: the chain scores of every source row against every target row."""
    XH = M.KR.prepare(np.ascontiguousarray(X, F32), M.MODEL_METRIC[metric])
    return CH.chain(XH[np.asarray(source)], XH[np.asarray(target)])


def candidates(S, T):
    """The positions (p, q) with S[p, q] >= T under fp32 compare (NaN as -inf), in ascending (p, q), and their scores."""
    S = CH.ranked(S)
    p, q = np.nonzero(S >= F32(T))                                # row-major: ascending (p, q)
    return p, q, S[p, q].astype(F32)


def order(p, q, s):
    """The candidates' indices in the header's order: score descending as fp32 compares (-0 equals +0), then a, then b.
    Positions ascend with the ids, so (p, q) stands for (a, b)."""
    return np.lexsort((q, p, -(s.astype(np.float64) + 0.0)))


def greedy(nA, nB, p, q, s):
    """(i) Sort by the order and walk.  Returns (mate of every source position or -1, mate of every target position or -1,
    candidate index of every source's pair or -1)."""
    mate_a, mate_b, pair = [-1] * nA, [-1] * nB, [-1] * nA
    for i in order(p, q, s).tolist():
        x, y = int(p[i]), int(q[i])
        if mate_a[x] < 0 and mate_b[y] < 0:
            mate_a[x], mate_b[y], pair[x] = y, x, i
    return np.array(mate_a, np.int64), np.array(mate_b, np.int64), np.array(pair, np.int64)


def rounds(nA, nB, p, q, s):
    """(ii) Synchronous rounds.  Every vertex keeps its own list, best first (a source's ties by ascending target, a target's by
    ascending source); in a round every free vertex moves a cursor past assigned partners and points at the first free one, then
    every source and target that point at each other are assigned.  Returns (mate_a, mate_b, assigning rounds, round-1 pairs)."""
    key = -(s.astype(np.float64) + 0.0)
    list_a = [[] for _ in range(nA)]
    list_b = [[] for _ in range(nB)]
    for x, y, k in sorted(zip(p.tolist(), q.tolist(), key.tolist()), key=lambda c: (c[0], c[2], c[1])):
        list_a[x].append(y)
    for x, y, k in sorted(zip(p.tolist(), q.tolist(), key.tolist()), key=lambda c: (c[1], c[2], c[0])):
        list_b[y].append(x)
    mate_a, mate_b, cur_a, cur_b = [-1] * nA, [-1] * nB, [0] * nA, [0] * nB
    count, first = 0, None
    while True:
        point_a, point_b = [-1] * nA, [-1] * nB
        for x in range(nA):
            if mate_a[x] < 0:
                while cur_a[x] < len(list_a[x]) and mate_b[list_a[x][cur_a[x]]] >= 0:
                    cur_a[x] += 1
                if cur_a[x] < len(list_a[x]):
                    point_a[x] = list_a[x][cur_a[x]]
        for y in range(nB):
            if mate_b[y] < 0:
                while cur_b[y] < len(list_b[y]) and mate_a[list_b[y][cur_b[y]]] >= 0:
                    cur_b[y] += 1
                if cur_b[y] < len(list_b[y]):
                    point_b[y] = list_b[y][cur_b[y]]
        made = [(x, point_a[x]) for x in range(nA) if point_a[x] >= 0 and point_b[point_a[x]] == x]
        if first is None:
            first = made
        if not made:
            break
        count += 1
        assert count <= min(nA, nB)
        for x, y in made:
            mate_a[x], mate_b[y] = y, x
    return np.array(mate_a, np.int64), np.array(mate_b, np.int64), count, first


def mutual_pairs(nA, nB, p, q, s):
    """The (p, q) where q is p's first candidate in the order and p is q's: read off the sorted list, no rounds involved."""
    best_a, best_b = {}, {}
    for i in order(p, q, s).tolist():
        best_a.setdefault(int(p[i]), int(q[i]))
        best_b.setdefault(int(q[i]), int(p[i]))
    return sorted((x, y) for x, y in best_a.items() if best_b[y] == x)


def blocking_pairs(p, q, s, mate_a, mate_b):
    """The candidates (x, y) ahead, in the order, of both x's and y's assigned pair; an unassigned end is worse than anything."""
    rank = np.empty(p.size, np.int64)
    rank[order(p, q, s)] = np.arange(p.size)
    worst = p.size
    at = {(int(x), int(y)): int(r) for x, y, r in zip(p, q, rank)}
    rank_a = [at[(x, int(y))] if y >= 0 else worst for x, y in enumerate(mate_a)]
    rank_b = [at[(int(x), y)] if x >= 0 else worst for y, x in enumerate(mate_b)]
    return [(int(x), int(y)) for x, y, r in zip(p, q, rank) if r < rank_a[x] and r < rank_b[y]]


def align_scores(S, source, target, T):
    """(a, b, score, target_of, target_score, flags, source_of, summary) from the score matrix source x target: what
    capi.Alignment.run returns."""
    source, target = np.asarray(source, np.int64), np.asarray(target, np.int64)
    assert np.all(np.diff(source) > 0) and np.all(np.diff(target) > 0) and not np.intersect1d(source, target).size
    nA, nB = source.size, target.size
    p, q, s = candidates(S, T)
    mate_a, mate_b, pair = greedy(nA, nB, p, q, s)
    have = mate_a >= 0
    target_of = np.where(have, target[np.maximum(mate_a, 0)], -1).astype(np.int32)
    target_score = np.zeros(nA, F32)
    target_score[have] = s[pair[have]]
    flags = have.astype(np.uint8)
    for x, y in mutual_pairs(nA, nB, p, q, s):
        assert mate_a[x] == y                                     # every mutual pair is accepted
        flags[x] |= 2
    source_of = np.where(mate_b >= 0, source[np.maximum(mate_b, 0)], -1).astype(np.int32)
    per_a, per_b = np.bincount(p, minlength=nA), np.bincount(q, minlength=nB)
    summary = {"candidates": int(p.size), "assigned": int(have.sum()), "mutual": int((flags & 2 != 0).sum()),
               "sources_with_candidates": int((per_a >= 1).sum()), "targets_with_candidates": int((per_b >= 1).sum()),
               "ambiguous_sources": int((per_a >= 2).sum())}
    return source[p].astype(np.int32), target[q].astype(np.int32), s, target_of, target_score, flags, source_of, summary


def _frozen(*arrays):
    for arr in arrays:
        arr.setflags(write=False)
    return arrays


# ----------------------------------------------------------------------------------------------------------------------
# Tile edges: match_ref's general-float rows (the second half copies the first, so duplicates and exact ties fall across the
# two sets; zero rows included), split into the two sets by a fixed permutation.  T is an attained score chosen as
# match_ref.tile_case chooses it: the smallest one that at most 15 % of the rectangle's scores reach.
# ----------------------------------------------------------------------------------------------------------------------
TILE_SHAPES = ((63, 127, 1), (64, 128, 4), (65, 129, 3), (64, 128, 32), (129, 65, 31), (65, 129, 33), (193, 300, 200), (1, 300, 200),
               (300, 1, 200))                                     # (nA, nB, dim): the query tile holds 64 rows, the candidate tile 128


def split(n, nA, seed=93):
    """The sorted first nA entries of a fixed permutation and the sorted rest.  (Seed 90 makes the single target of shape
    (300, 1, 200) a zero row: every pair scores 0 there and no threshold keeps between 1 % and 20 % of them.)"""
    perm = M.permutation(n, seed)
    return np.sort(perm[:nA]).astype(np.int32), np.sort(perm[nA:]).astype(np.int32)


@functools.lru_cache(maxsize=None)
def tile_case(nA, nB, dim, metric):
    """(rows, source, target, scores, T, share)."""
    X = M.tile_rows(dim, nA + nB)
    source, target = split(nA + nB, nA)
    S = scores(X, source, target, metric)
    assert np.all(np.isfinite(S))
    flat = np.sort(S.ravel())[::-1]
    T = F32(flat[int(0.15 * flat.size)])
    if (flat >= T).sum() > 0.15 * flat.size:                      # ties carry it past 15 %: the next attained score above, if any
        above = flat[flat > T]
        T = F32(above[-1] if above.size else flat[0])
    share = float((flat >= T).sum()) / flat.size
    return _frozen(X, source, target, S) + (T, share)


# ----------------------------------------------------------------------------------------------------------------------
# Exactly at the threshold: match_ref.threshold_case's rows (integer scores under dot, one ulp = 1); even ids are sources, odd
# ids are targets.
# ----------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def threshold_case():
    """(rows, source, target, scores, T): T and T - 1 are both attained in the rectangle."""
    X, S, T = M.threshold_case()
    source, target = np.arange(0, X.shape[0], 2, dtype=np.int32), np.arange(1, X.shape[0], 2, dtype=np.int32)
    R = np.ascontiguousarray(S[np.ix_(source, target)])
    return _frozen(X, source, target, R) + (T,)


# ----------------------------------------------------------------------------------------------------------------------
# All ties: 64 + 80 identical rows under dot.  Every candidate has the same score, so the order is (a, b) alone: source i takes
# target i, and each round assigns exactly one pair -- the round bound's worst case.
# ----------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def ties_case():
    """(rows, source, target, scores, T)."""
    X = np.tile(np.array([[1.5, -2.0, 0.25, 3.0, 1.0]], F32), (144, 1))
    source, target = np.arange(64, dtype=np.int32), np.arange(64, 144, dtype=np.int32)
    S = scores(X, source, target, "dot")
    return _frozen(X, source, target, S) + (F32(S[0, 0]),)


# ----------------------------------------------------------------------------------------------------------------------
# Weighted chain: a path s0 - t0 - s1 - t1 - ... - s299 - t299 whose 599 edges have strictly decreasing integer weights.  Edge e
# joins path vertices e and e + 1 and owns column e: vertex e holds the weight there, vertex e + 1 holds 1.  Under dot an edge
# scores its weight exactly and a non-edge 0.  Path vertex k lives at row perm[k].  s_i prefers t_(i-1), which prefers s_(i-1):
# every source but the first ends with its second choice, one pair per round.
# ----------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def chain_case(pairs=300):
    """(rows, source, target, scores, T, perm)."""
    n = 2 * pairs
    perm = M.permutation(n, 91)
    X = np.zeros((n, n - 1), F32)
    for e in range(n - 1):
        X[perm[e], e] = n - e                                     # weights n .. 2
        X[perm[e + 1], e] = 1
    source, target = np.sort(perm[0::2]).astype(np.int32), np.sort(perm[1::2]).astype(np.int32)
    S = scores(X, source, target, "dot")
    _frozen(X, source, target, S, perm)
    return X, source, target, S, F32(1), perm


# ----------------------------------------------------------------------------------------------------------------------
# Star: one hub target is the first choice of all 300 sources (source i scores 100 + i with it); source i's second choice is
# target 1 + i % 40, with the score 1 + i // 40.  Exactly one source gets the hub, and the others compete for the 40 targets.
# ----------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def star_case(n_sources=300, spread=40):
    """(rows, source, target, scores, T, perm): vertex k < n_sources is source k, vertex n_sources the hub, the rest the further
    targets; vertex k lives at row perm[k]."""
    n = n_sources + 1 + spread
    perm = M.permutation(n, 92)
    X = np.zeros((n, 1 + spread), F32)
    for i in range(n_sources):
        X[perm[i], 0] = 100 + i
        X[perm[i], 1 + i % spread] = 1 + i // spread
    X[perm[n_sources], 0] = 1
    for j in range(spread):
        X[perm[n_sources + 1 + j], 1 + j] = 1
    source, target = np.sort(perm[:n_sources]).astype(np.int32), np.sort(perm[n_sources:]).astype(np.int32)
    S = scores(X, source, target, "dot")
    _frozen(X, source, target, S, perm)
    return X, source, target, S, F32(1), perm

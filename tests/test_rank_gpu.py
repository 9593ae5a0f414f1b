"""Ranking on the device (ge_glove_rank_*, csrc/rank.hip) against numpy (tests/rank_ref.py).  Designed tables go into handles
with ge_glove_set_state:
  A  integer-valued tables: fp32 arithmetic is exact, ranks and scores equal the yardstick with no tolerance, ties included, at
     every edge of the 64-query / 128-candidate / 32-column tile, with and without filter lists;
  B  the same case on every kind of handle (records, separate tables, packed records, bf16 rows with fp32 hub masters,
     deterministic, stratified, a shard): identical ranks and scores;
  C  generic floats inside the bracket lo <= rank <= hi derived in rank_ref.py, which is shown not to be vacuous first;
  D  twin columns: the gather kernel and the matrix-core kernel give the same bits for the same (query, column);
  E  a function of the input alone, and a pure read;
  F  planted clusters."""
import functools

import numpy as np
import pytest

import geglove
from geglove import capi, synth
from helpers import make_config
import nn_ref as N
import rank_ref as R
from test_nn_gpu import _value_range

pytestmark = pytest.mark.gpu

KINDS = {
    "hogwild": dict(mode="hogwild", shuffle="device", seed=42),
    "separate": dict(mode="hogwild", shuffle="device", seed=42, layout=["separate_tables"]),
    "packed": dict(mode="hogwild", shuffle="device", seed=42, layout=["packed_records"]),
    "bf16": dict(mode="hogwild", shuffle="device", seed=42, dtype="bf16", hot="all"),
    "deterministic": dict(mode="deterministic", shuffle="java", seed=42),
    "stratified": dict(mode="stratified", shuffle="device", seed=42),
    "sharded": dict(mode="hogwild", shuffle="device", seed=42, row_range=(100, 230)),
}


def _handle(V, D, kind="hogwild"):
    """A handle of that kind over a matrix with a few nonzeros in every owned row (the tables are set by the test)."""
    device = KINDS[kind]
    lo, hi = device.get("row_range", (0, V))
    I = np.repeat(np.arange(lo, hi, dtype=np.int64), 3)
    J = (I * 7 + np.tile(np.arange(3), hi - lo) * 11 + 1) % V
    X = np.full(len(I), 0.05, np.float32)
    order = np.lexsort((J, I))
    keep = np.ones(len(I), bool)
    keep[1:] = (np.diff(I[order]) != 0) | (np.diff(J[order]) != 0)            # V < 3: the three columns of a row coincide
    I, J, X = I[order][keep].astype(np.int32), J[order][keep].astype(np.int32), X[order][keep]
    return geglove.createOptimizer(make_config(D, "glove", **device), geglove.CooMatrix(V, I, J, X, 0.2))


def _set(h, F, C, fb, cb, rows=None):
    lo, hi = rows or (0, F.shape[0])
    h.set_state("focus", F[lo:hi]); h.set_state("context", C)
    h.set_state("fbias", fb[lo:hi]); h.set_state("cbias", cb)


def _pairs(seed, n, V, rows=None):
    lo, hi = rows or (0, V)
    u = synth.splitmix64(seed, 2 * n) >> np.uint64(33)
    return (lo + u[:n] % np.uint64(hi - lo)).astype(np.int32), (u[n:] % np.uint64(V)).astype(np.int32)


def _filters(seed, J, V):
    """Per pair, in turn: an empty list, a list that holds the target, every column, a list that ends at V - 1, any list."""
    lists = []
    for k, j in enumerate(J):
        pick = synth.splitmix64(seed + k, V) % np.uint64(4) == 0
        kind = k % 5
        if kind == 0:
            pick[:] = False
        elif kind == 1:
            pick[j] = True
        elif kind == 2:
            pick[:] = True
        elif kind == 3:
            pick[V - 1] = True
        lists.append(np.flatnonzero(pick))
    return R.csr(lists)


def _integer_tables(seed, V, D):
    v = _value_range(D)
    assert v * v * D + v < 2 ** 24
    return (N.integers(seed, (V, D), -v, v), N.integers(seed + 1, (V, D), -v, v), N.integers(seed + 2, (V,), -9, 9),
            N.integers(seed + 3, (V,), -v, v))


def _rank(h, I, J, filters=None):
    rk = capi.Ranking(h._h, I, J, *(filters or (None, None)))
    try:
        out = rk.run()
        assert rk.kernel_ms() > 0 and abs(sum(rk.phase_ms()) - rk.kernel_ms()) <= 1e-3 * rk.kernel_ms()
        return out
    finally:
        rk.close()


def _check_exact(h, F, C, cb, I, J, filters, what):
    Z = R.scores(F, C, cb, I)
    want = R.ranks(Z, J, filters)
    rank, score, s = _rank(h, I, J, filters)
    assert rank.dtype == np.int32 and score.dtype == np.float32
    bad = np.flatnonzero(rank != want)
    assert bad.size == 0, (what, "pair %d: rank %d, want %d" % (bad[0], rank[bad[0]], want[bad[0]]))
    assert np.array_equal(score, Z[np.arange(len(J)), J].astype(np.float32)), what
    assert s == R.summary(rank), (what, s)


# ------------------------------------------------------------------ A
@pytest.mark.parametrize("V,D,n", [(1, 1, 1), (2, 3, 63), (127, 32, 64), (128, 33, 65), (129, 50, 200), (300, 200, 64), (1000, 1024, 65),
                                   (1000, 50, 200), (300, 1, 200)])
def test_exact_on_integer_tables(gpu, V, D, n):
    F, C, fb, cb = _integer_tables(1000 * V + D, V, D)
    I, J = _pairs(V + D + n, n, V)
    h = _handle(V, D)
    try:
        _set(h, F, C, fb, cb)
        Z = R.scores(F, C, cb, I)
        tied = np.mean(((Z == Z[np.arange(n), J][:, None]).sum(axis=1) > 1))
        print("V %d dim %d n %d: the target's score is shared with another column in %.0f %% of the pairs" % (V, D, n, 100 * tied))
        _check_exact(h, F, C, cb, I, J, None, (V, D, n, "plain"))
        _check_exact(h, F, C, cb, I, J, _filters(7 * V + D, J, V), (V, D, n, "filtered"))
    finally:
        h.close()


def test_upper_limits_are_checked_on_the_host(gpu):
    for kind, (lo, hi) in (("hogwild", (0, 300)), ("sharded", (100, 230))):
        h = _handle(300, 8, kind)
        try:
            ok_ptr, ok_idx = np.array([0, 1, 2], np.int64), np.array([0, 299], np.int32)
            capi.Ranking(h._h, [lo, hi - 1], [0, 299], ok_ptr, ok_idx).close()
            for I, J, idx in (([lo, hi], [0, 1], ok_idx), ([lo - 1 if lo else 300, lo], [0, 1], ok_idx), ([lo, lo], [0, 300], ok_idx),
                              ([lo, lo], [0, 1], np.array([0, 300], np.int32))):
                with pytest.raises(capi.GeError) as e:
                    capi.Ranking(h._h, I, J, ok_ptr, idx)
                assert e.value.status == capi.GE_ERR_ARG, (I, J, idx)
        finally:
            h.close()


# ------------------------------------------------------------------ B
@functools.lru_cache(maxsize=None)
def _layout_case():
    V, D, n = 300, 40, 200
    F, C, fb, cb = _integer_tables(4242, V, D)
    I, J = _pairs(99, n, V, rows=(100, 230))                     # rows every kind of handle owns
    filters = _filters(5, J, V)
    Z = R.scores(F, C, cb, I)
    return V, D, F, C, fb, cb, I, J, filters, R.ranks(Z, J), R.ranks(Z, J, filters), Z[np.arange(n), J].astype(np.float32)


@pytest.mark.parametrize("kind", list(KINDS))
def test_every_layout_gives_the_same_ranks(gpu, kind):
    V, D, F, C, fb, cb, I, J, filters, want_plain, want_filtered, want_score = _layout_case()
    h = _handle(V, D, kind)
    try:
        _set(h, F, C, fb, cb, rows=KINDS[kind].get("row_range"))
        if kind == "bf16":
            assert h.info()["hot_columns"] > 0, "no column has an fp32 master row"
        for filt, want in ((None, want_plain), (filters, want_filtered)):
            rank, score, s = _rank(h, I, J, filt)
            assert np.array_equal(rank, want) and score.tobytes() == want_score.tobytes(), kind
            assert s == R.summary(want)
    finally:
        h.close()


# ------------------------------------------------------------------ C
def _float_tables(seed, V, D):
    return (N.random_rows(seed, V, D), N.random_rows(seed + 1, V, D), N.uniform(seed + 2, (V,)).astype(np.float32),
            N.uniform(seed + 3, (V,)).astype(np.float32))


@pytest.mark.parametrize("D", [50, 200])
def test_generic_floats_inside_the_bracket(gpu, D):
    V, n = 1000, 200
    F, C, fb, cb = _float_tables(300 + D, V, D)
    I, J = _pairs(D, n, V)
    h = _handle(V, D)
    try:
        _set(h, F, C, fb, cb)
        for filters in (None, _filters(11 * D, J, V)):
            lo, hi, tj, Ej = R.bracket(F, C, cb, I, J, filters)
            sharp = np.mean(lo == hi)
            print("V %d dim %d %s: lo == hi for %.1f %% of the pairs, widest bracket %d" % (V, D, "filtered" if filters else "plain", 100 * sharp, (hi - lo).max() + 1))
            assert sharp >= 0.8, "the bracket decides too few ranks to test anything"
            rank, score, _ = _rank(h, I, J, filters)
            bad = np.flatnonzero((rank < lo) | (rank > hi))
            assert bad.size == 0, "pair %d: rank %d outside [%d, %d]" % (bad[0], rank[bad[0]], lo[bad[0]], hi[bad[0]])
            err = np.abs(score.astype(np.float64) - tj)
            print("    scores within %.3g of their bound" % (err / Ej).max())
            assert np.all(err <= Ej)
    finally:
        h.close()


# ------------------------------------------------------------------ D
@pytest.mark.parametrize("D", [33, 200])
def test_the_two_kernels_agree_bit_for_bit(gpu, D):
    """Column t + m is a copy of column t, so z(i, t) == z(i, t + m) whatever the rounding -- if, and only if, the gather chain
    (which scores the target) and the matrix-core chain (which scores the twin as a candidate) round alike."""
    m, q = 150, 100
    V = 2 * m
    F, C, fb, cb = _float_tables(700 + D, V, D)
    C[m:] = C[:m]; cb[m:] = cb[:m]
    i, t = _pairs(3 * D, q, m)
    I = np.repeat(i, 2).astype(np.int32)
    J = np.stack([t, t + m], axis=1).reshape(-1).astype(np.int32)
    twin = np.stack([t + m, t], axis=1).reshape(-1)
    h = _handle(V, D)
    try:
        _set(h, F, C, fb, cb)
        rank, score, _ = _rank(h, I, J)
        assert np.array_equal(score[0::2].view(np.uint32), score[1::2].view(np.uint32))
        assert np.array_equal(rank[1::2], rank[0::2] + 1), np.flatnonzero(rank[1::2] != rank[0::2] + 1)[:5]
        lo, hi, _, _ = R.bracket(F, C, cb, I, J)
        assert np.all((lo <= rank) & (rank <= hi)) and len(set(rank.tolist())) > 20           # not all alike: real ranks
        only_twin = _rank(h, I, J, R.csr([[c] for c in twin]))[0]
        assert np.array_equal(only_twin[0::2], only_twin[1::2]) and np.array_equal(only_twin[0::2], rank[0::2])
        everything = _rank(h, I, J, R.csr([np.arange(V)] * (2 * q)))[0]
        assert np.all(everything == 1)
    finally:
        h.close()


# ------------------------------------------------------------------ E
def _snapshot(h):
    snap = {name: h.get_state(name).tobytes() for name in capi.STATE_NAMES}
    snap["rng_state"] = h.rng_state()
    snap["perm"] = h.perm().tobytes()
    return snap


def test_a_function_of_the_input_alone_and_a_pure_read(gpu):
    V, D, n = 300, 33, 130
    F, C, fb, cb = _float_tables(55, V, D)
    F, C, fb, cb = F * np.float32(0.125), C * np.float32(0.125), fb * np.float32(0.125), cb * np.float32(0.125)       # trainable magnitudes
    I, J = _pairs(8, n, V)
    ptr, idx = _filters(21, J, V)
    lists = [idx[ptr[k]:ptr[k + 1]] for k in range(n)]
    h, twin = _handle(V, D, "deterministic"), _handle(V, D, "deterministic")
    try:
        _set(h, F, C, fb, cb); _set(twin, F, C, fb, cb)
        before = _snapshot(h)
        assert len(before) == 10 and before == _snapshot(twin)
        rk = capi.Ranking(h._h, I, J, ptr, idx)
        try:
            rank, score, s = rk.run()
            again = rk.run()
            assert rank.tobytes() == again[0].tobytes() and score.tobytes() == again[1].tobytes() and s == again[2]
            only = rk.run(rank=False, score=False)
            assert only[0] is None and only[1] is None and only[2] == s
        finally:
            rk.close()
        back = _rank(h, I[::-1], J[::-1], R.csr(lists[::-1]))
        assert back[0][::-1].tobytes() == rank.tobytes() and back[1][::-1].tobytes() == score.tobytes()
        for k in range(n):
            one = _rank(h, I[k:k + 1], J[k:k + 1], R.csr(lists[k:k + 1]))
            assert one[0][0] == rank[k] and one[1].tobytes() == score[k:k + 1].tobytes(), k
            assert one[2] == R.summary(rank[k:k + 1])
        want = R.summary(rank)
        assert s == want and np.float64(s["mrr"]).tobytes() == np.float64(want["mrr"]).tobytes()
        lo, hi, _, _ = R.bracket(F, C, cb, I, J, (ptr, idx))
        assert np.all((lo <= rank) & (rank <= hi))
        assert _snapshot(h) == before, "a ranking wrote to the trainer"
        assert h.epoch(0) == twin.epoch(0) and _snapshot(h) == _snapshot(twin), "an epoch after a ranking differs from one without"
    finally:
        h.close(); twin.close()


# ------------------------------------------------------------------ F
def test_a_planted_answer(gpu):
    clusters, size, D = 20, 15, 50
    V = clusters * size
    C, label = N.planted(77, clusters, size, D, 0.1)
    centre = N.uniform(77, (clusters, D))
    centre /= np.linalg.norm(centre, axis=1, keepdims=True)
    F = centre[label].astype(np.float32)
    zero = np.zeros(V, np.float32)
    I = np.arange(V, dtype=np.int32)
    member = [np.flatnonzero(label == c) for c in range(clusters)]
    J = np.array([member[label[i]][(i * 7) % size] for i in range(V)], np.int32)
    h = _handle(V, D)
    try:
        _set(h, F, C, zero, zero)
        rank, _, s = _rank(h, I, J)
        assert rank.max() <= size and rank.min() == 1 and s["hits100"] == V == s["n"]
        assert s["mean_rank"] <= size and s["mrr"] > 1.0 / size
    finally:
        h.close()

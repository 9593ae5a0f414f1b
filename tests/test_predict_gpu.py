"""Link prediction on the device (ge_glove_predict_*, csrc/predict.hip) against numpy (tests/predict_ref.py).  Designed tables go
into handles with ge_glove_set_state:
  A  integer-valued tables: fp32 arithmetic is exact, so index, score bits and count equal the yardstick with no tolerance, ties
     included, at every edge of the 64-query / 128-candidate / 32-column tile and of every list capacity, with filter lists of
     every designed kind, subsets and the query's own column; and a table long enough for candidate ranges of several tiles,
     whose best columns are filtered and met after the thresholds are set;
  B  the same case on every kind of handle: identical bytes;
  C  every prediction handed to ge_glove_rank_run with the same filter comes back with rank t + 1 and the same score bits; and on
     generic floats index, score bits and count are those of the header's fmaf chain in numpy (tests/chain_ref.py), no bound;
  D  generic floats inside the bound derived in predict_ref.py, whose undecided share is capped before the device is asked;
  E  a function of the input alone, and a pure read;
  F  a planted answer."""
import functools

import numpy as np
import pytest

import geglove
from geglove import capi, synth
from helpers import make_config
import chain_ref as CH
import nn_ref as N
import predict_ref as P
import rank_ref as R
from test_rank_gpu import KINDS, _handle, _set, _pairs

pytestmark = pytest.mark.gpu

ALL_K = (1, 10, 32, 33, 64, 65, 128)            # both sides of every list capacity (k <= 16, 32, 64, 128)


def _predict(h, I, Ks, filters=None, subset=None, exclude_self=False):
    """{K: (index, score, count)} of one set, and the set's info after the last run."""
    pr = capi.Prediction(h._h, I, filters, subset, exclude_self)
    try:
        out = {}
        for K in Ks:
            out[K] = pr.run(K)
            ms = pr.kernel_ms()
            assert len(ms) == 3 and all(m > 0 for m in ms), ms
        info = pr.info()
        assert info["n"] == len(I) and (subset is None or info["candidates"] == len(subset))
        return out, info
    finally:
        pr.close()


def _same(got, want, what):
    (gi, gs, gc), (wi, ws, wc) = got, want
    assert gi.dtype == np.int32 and gs.dtype == np.float32 and gc.dtype == np.int32
    assert np.array_equal(gc, wc), (what, "count", np.flatnonzero(gc != wc)[:5], gc[gc != wc][:5], wc[gc != wc][:5])
    bad = np.argwhere(gi != wi)
    assert bad.size == 0, (what, "query %d slot %d: column %d, want %d" % (bad[0][0], bad[0][1], gi[tuple(bad[0])], wi[tuple(bad[0])]))
    assert gs.tobytes() == ws.tobytes(), (what, "score bits", np.argwhere(gs.view(np.uint32) != ws.view(np.uint32))[:5])


def _designed_filters(seed, Z, K, subset, self_col):
    """Per query, in turn: an empty list; the whole row but one column; the whole row; entries on tile edges (127, 128, V - 1); exactly
    the unfiltered top K (a missing filter test changes every slot); any quarter of the columns."""
    n, V = Z.shape
    top = P.topk(Z, K, None, subset, self_col)[0]
    lists = []
    for k in range(n):
        kind = k % 6
        if kind == 0:
            pick = np.zeros(V, bool)
        elif kind == 1:
            pick = np.ones(V, bool); pick[(7 * k) % V] = False
        elif kind == 2:
            pick = np.ones(V, bool)
        elif kind == 3:
            pick = np.zeros(V, bool); pick[[c for c in (127, 128, V - 1) if c < V]] = True
        elif kind == 4:
            pick = np.zeros(V, bool); pick[top[k][top[k] >= 0]] = True
        else:
            pick = synth.splitmix64(seed + k, V) % np.uint64(4) == 0
        lists.append(np.flatnonzero(pick))
    return P.csr(lists)


# ------------------------------------------------------------------ A
@pytest.mark.parametrize("V,D,n", [(1, 1, 1), (2, 3, 63), (127, 32, 64), (128, 33, 65), (129, 50, 200), (300, 200, 64), (1000, 1024, 65)])
def test_exact_on_integer_tables(gpu, V, D, n):
    F, C, fb, cb = P.integer_tables(1000 * V + D, V, D)
    I, _ = _pairs(V + D + n, n, V)
    Z = R.scores(F, C, cb, I)
    subsets = {"all": None, "every other": np.arange(0, V, 2, dtype=np.int32), "one": np.array([I[0]], np.int32)}
    h = _handle(V, D)
    try:
        _set(h, F, C, fb, cb)
        top = -np.sort(-Z, axis=1)[:, :11]
        tied = np.mean((top[:, 1:] == top[:, :-1]).any(axis=1))
        print("V %d dim %d n %d: two of the ten best scores are equal in %.0f %% of the queries" % (V, D, n, 100 * tied))
        for sname, subset in subsets.items():
            inside = np.isin(I, subset) if subset is not None else np.ones(n, bool)
            if sname == "every other" and V > 2:
                assert inside.any() and not inside.all()                     # queries inside and outside the subset
            for own in (False, True):
                self_col = I if own else None
                got, info = _predict(h, I, ALL_K, None, subset, own)
                if V == 1000 and subset is None:
                    assert info["ranges"] > 1, info                          # the merge has something to merge
                for K in ALL_K:
                    _same(got[K], P.topk(Z, K, None, subset, self_col), (V, D, n, sname, own, K, "no filter"))
                # the designed lists depend on K (kind 4), so they are a set of their own per K: every capacity and its edges again
                for K in ALL_K:
                    filters = _designed_filters(7 * V + D, Z, K, subset, self_col)
                    got, _ = _predict(h, I, (K,), filters, subset, own)
                    want = P.topk(Z, K, filters, subset, self_col)
                    if subset is None and V - 1 >= 2 * K:                      # kind 4: the next K candidates move up, every slot changes
                        plain = P.topk(Z, K, None, subset, self_col)[0]
                        assert np.all(want[0][4::6] != plain[4::6])
                    _same(got[K], want, (V, D, n, sname, own, K, "designed filters"))
    finally:
        h.close()


def test_filtered_best_columns_met_after_the_thresholds(gpu):
    """A table long enough that a candidate range is several tiles: the best scores of every row sit in the last tile of the last
    range and all of them are filtered -- they beat every threshold set before them and only the filter test keeps them out.  More
    than was asked for (the best filtered columns only in the last range): the last tile of every fourth range, range 0 included,
    is planted and filtered too, so that the same happens in workgroups whose range is not the table's end."""
    V, D, n = 128 * 3 * 782 - 50, 4, 8
    F, C, fb, cb = P.integer_tables(31, V, D)
    cb = cb.copy()
    I = np.arange(n, dtype=np.int32) * 1000
    h = _handle(V, D)
    try:
        _set(h, F, C, fb, cb)
        _, info = _predict(h, I, (10,))
        ranges = info["ranges"]
        tiles = (V + 127) // 128
        per = (tiles + ranges - 1) // ranges
        assert ranges > 1 and per >= 2 and (tiles - 1) % per == per - 1, info    # several ranges of several tiles, the last one whole
        best = [np.arange((tiles - 1) * 128, V)]
        best += [np.arange(((r + 1) * per - 1) * 128, ((r + 1) * per - 1) * 128 + 128) for r in range(0, ranges - 1, 4)]
        best = np.unique(np.concatenate(best))
        cb[best] += 1000.0                                                   # far above every other z, still exact
        h.set_state("cbias", cb)
        Z = R.scores(F, C, cb, I)
        filters = P.csr([best] * n)
        for K in (10, 100):
            plain = P.topk(Z, K)[0]
            assert np.all(np.isin(plain, best))                              # unfiltered, the planted columns fill every list
            got, _ = _predict(h, I, (K,), filters)
            want = P.topk(Z, K, filters)
            assert not np.any(np.isin(want[0], best))
            _same(got[K], want, ("after the thresholds", K))
            got, _ = _predict(h, I, (K,))
            _same(got[K], P.topk(Z, K), ("after the thresholds, unfiltered", K))
    finally:
        h.close()


def test_more_queries_than_one_launch_holds(gpu):
    """20 000 queries at K = 128 over 64 candidate tiles are more (query, range, slot) entries than one launch keeps: the queries go
    in two batches, and the second one reads its rows, its own columns and its filter lists at the right offsets.  The queries are
    200 rows, each a hundred times, so the yardstick is computed for 200."""
    V, D, distinct, times, K = 128 * 64, 4, 200, 100, 128
    F, C, fb, cb = P.integer_tables(77, V, D)
    rows, _ = _pairs(5, distinct, V)
    lists = [np.flatnonzero(synth.splitmix64(300 + k, V) % np.uint64(400) == 0) for k in range(distinct)]
    Z = R.scores(F, C, cb, rows)
    want = P.topk(Z, K, P.csr(lists), None, rows)
    top = P.topk(Z, K, None, None, rows)[0]
    assert np.mean([np.isin(top[k], lists[k]).any() for k in range(distinct)]) > 0.2          # the filters matter
    order = np.argsort(synth.splitmix64(9, distinct * times), kind="stable") % distinct      # every row all over both batches
    h = _handle(V, D)
    try:
        _set(h, F, C, fb, cb)
        got, info = _predict(h, rows[order], (K,), P.csr([lists[k] for k in order]), None, True)
        assert info["ranges"] * len(order) * K > 2 ** 24, info                                # one launch would not have held them
        _same(got[K], tuple(w[order] for w in want), "two batches")
    finally:
        h.close()


def test_upper_limits_are_checked_on_the_host(gpu):
    for kind, (lo, hi) in (("hogwild", (0, 300)), ("sharded", (100, 230))):
        h = _handle(300, 8, kind)
        try:
            ok = (np.array([0, 1, 2], np.int64), np.array([0, 299], np.int32))
            capi.Prediction(h._h, [lo, hi - 1], ok, [0, 299], True).close()
            for I, filters, subset in (([lo, hi], ok, None), ([lo - 1 if lo else 300, lo], ok, None),
                                       ([lo, lo], (ok[0], np.array([0, 300], np.int32)), None), ([lo, lo], ok, [0, 300])):
                with pytest.raises(capi.GeError) as e:
                    capi.Prediction(h._h, I, filters, subset)
                assert e.value.status == capi.GE_ERR_ARG, (I, filters, subset)
            pr = capi.Prediction(h._h, [lo])
            try:
                for K in (0, 129):
                    with pytest.raises(capi.GeError) as e:
                        pr.run(K)
                    assert e.value.status == capi.GE_ERR_ARG
            finally:
                pr.close()
        finally:
            h.close()


# ------------------------------------------------------------------ B
@functools.lru_cache(maxsize=None)
def _layout_case():
    V, D, n = 300, 40, 200
    F, C, fb, cb = P.integer_tables(4242, V, D)                  # |values| <= 2: exact in bf16
    I, _ = _pairs(99, n, V, rows=(100, 230))                     # rows every kind of handle owns
    Z = R.scores(F, C, cb, I)
    subset = np.arange(1, V, 2, dtype=np.int32)
    filters = _designed_filters(5, Z, 10, subset, I)
    want = {K: P.topk(Z, K, filters, subset, I) for K in (10, 64)}
    plain = {K: P.topk(Z, K) for K in (10, 64)}
    return V, D, F, C, fb, cb, I, filters, subset, want, plain


@pytest.mark.parametrize("kind", list(KINDS))
def test_every_layout_gives_the_same_bytes(gpu, kind):
    V, D, F, C, fb, cb, I, filters, subset, want, plain = _layout_case()
    h = _handle(V, D, kind)
    try:
        _set(h, F, C, fb, cb, rows=KINDS[kind].get("row_range"))
        if kind == "bf16":
            assert h.info()["hot_columns"] > 0, "no column has an fp32 master row"
        got, _ = _predict(h, I, (10, 64), filters, subset, True)
        for K in (10, 64):
            _same(got[K], want[K], (kind, K, "filtered"))
        got, _ = _predict(h, I, (10, 64))
        for K in (10, 64):
            _same(got[K], plain[K], (kind, K, "plain"))
    finally:
        h.close()


# ------------------------------------------------------------------ C
@pytest.mark.parametrize("D", [33, 200])
def test_every_prediction_has_its_rank_bit_for_bit(gpu, D):
    """The t-th prediction of a row, handed to ge_glove_rank_run with the same filter (plus the row itself under exclude_self), comes
    back with rank t + 1 and the same score bits -- which a single differing bit between the two score tiles, or between them and
    the gather chain that scores the rank's target, would break.  Twin columns (t + m a copy of t) put exact ties in every list."""
    m, n = 150, 100
    V = 2 * m
    F, C, fb, cb = P.float_tables(700 + D, V, D)
    C[m:] = C[:m]; cb[m:] = cb[:m]
    I, _ = _pairs(3 * D, n, V)
    lists = [np.flatnonzero(synth.splitmix64(900 + k, V) % np.uint64(4) == 0) for k in range(n)]
    h = _handle(V, D)
    try:
        _set(h, F, C, fb, cb)
        for filters, own, K in ((None, False, 128), (lists, True, 33), (lists, False, 10)):
            got, _ = _predict(h, I, (K,), None if filters is None else P.csr(filters), None, own)
            index, score, count = got[K]
            assert np.all(count == K)
            ties = np.mean((score[:, 1:] == score[:, :-1]).any(axis=1))
            print("dim %d K %d: %.0f %% of the lists hold two equal scores" % (D, K, 100 * ties))
            assert ties > 0.5
            rI = np.repeat(I, K).astype(np.int32)
            rJ = index.reshape(-1)
            per_query = [np.union1d(filters[k] if filters is not None else [], [I[k]] if own else []).astype(np.int32) for k in range(n)]
            ptr, idx = P.csr([per_query[k] for k in range(n) for _ in range(K)])
            rk = capi.Ranking(h._h, rI, rJ, ptr, idx)
            try:
                rank, zt, _ = rk.run()
            finally:
                rk.close()
            bad = np.flatnonzero(rank.reshape(n, K) != np.arange(1, K + 1)[None, :])
            assert bad.size == 0, "query %d slot %d has rank %d" % (bad[0] // K, bad[0] % K, rank[bad[0]])
            assert zt.tobytes() == score.tobytes()
    finally:
        h.close()


@pytest.mark.parametrize("D", [33, 200])
def test_generic_floats_are_the_chain_bit_for_bit(gpu, D):
    """C holds the two score tiles and the gather chain to one another, device against device; this holds all three to the header:
    z = chain(F[I], C) + cBias with one fp32 add, the chain "the fp32 fmaf chain from 0.0f over ascending d" in numpy
    (tests/chain_ref.py; test_chain_ref.py shows it differs from any other order of summation in most scores at these dims).
    Index, score bits and count equal the model under the total order, K = 33 and 128, twin columns for exact ties; and every
    prediction handed to ge_glove_rank_run comes back with rank t + 1 and the MODEL's score bits."""
    m, n = 150, 100
    V = 2 * m
    F, C, fb, cb = P.float_tables(1700 + D, V, D)
    C[m:] = C[:m]; cb[m:] = cb[:m]
    I, _ = _pairs(5 * D, n, V)
    Z = CH.chain(F[I], C) + cb[None, :]
    assert Z.dtype == np.float32 and np.all(np.isfinite(Z))
    lists = [np.flatnonzero(synth.splitmix64(1900 + k, V) % np.uint64(4) == 0) for k in range(n)]
    h = _handle(V, D)
    try:
        _set(h, F, C, fb, cb)
        for filters, own, K in ((None, False, 128), (lists, True, 33), (None, True, 33), (lists, False, 128)):
            csr = None if filters is None else P.csr(filters)
            want = P.topk(Z, K, csr, None, I if own else None)
            assert np.all(want[2] == K) and np.mean((want[1][:, 1:] == want[1][:, :-1]).any(axis=1)) > 0.5
            got, _ = _predict(h, I, (K,), csr, None, own)
            _same(got[K], want, (D, K, own, "filtered" if filters else "plain", "chain model"))
            per_query = [np.union1d(filters[k] if filters is not None else [], [I[k]] if own else []).astype(np.int32) for k in range(n)]
            ptr, idx = P.csr([per_query[k] for k in range(n) for _ in range(K)])
            rk = capi.Ranking(h._h, np.repeat(I, K).astype(np.int32), want[0].reshape(-1), ptr, idx)
            try:
                rank, zt, _ = rk.run()
            finally:
                rk.close()
            bad = np.flatnonzero(rank.reshape(n, K) != np.arange(1, K + 1)[None, :])
            assert bad.size == 0, "query %d slot %d has rank %d" % (bad[0] // K, bad[0] % K, rank[bad[0]])
            assert zt.tobytes() == want[1].tobytes()
    finally:
        h.close()


# ------------------------------------------------------------------ D
@pytest.mark.parametrize("D", [50, 200])
def test_generic_floats_inside_the_bound(gpu, D):
    V, n = 1000, 200
    F, C, fb, cb = P.float_tables(300 + D, V, D)
    I, _ = _pairs(D, n, V)
    t, E = P.bound(F, C, cb, I)
    lists = [np.flatnonzero(synth.splitmix64(11 * D + k, V) % np.uint64(4) == 0) for k in range(n)]
    every_other = np.arange(0, V, 2, dtype=np.int32)
    h = _handle(V, D)
    try:
        _set(h, F, C, fb, cb)
        for filters, subset, own in ((None, None, False), (P.csr(lists), every_other, True)):
            keep = P.candidates(n, V, filters, subset, I if own else None)
            # K = 10 and 40 (list capacities 32 and 128): deeper in a list of 1000 candidates the scores crowd, and at K = 100 and
            # dim 200 the numpy model alone leaves 3.6 % of the slots undecided, past the cap
            for K in (10, 40):
                model, ok = P.decided(t, E, keep, K)
                left_out = 1.0 - ok.mean()
                print("V %d dim %d K %d %s: %.2f %% of the slots are undecided" % (V, D, K, "filtered" if filters else "plain", 100 * left_out))
                assert left_out <= 0.02, "the bound decides too few slots to test the order"        # before any device output
                got, _ = _predict(h, I, (K,), filters, subset, own)
                worst = P.check_within_bound(*got[K], t, E, keep, model, ok)
                print("    scores within %.3g of their bound" % worst)
    finally:
        h.close()


# ------------------------------------------------------------------ E
def _snapshot(h):
    snap = {name: h.get_state(name).tobytes() for name in capi.ALL_STATE_NAMES if h._count(capi.ALL_STATE_NAMES.index(name)) > 0 and
            (h.OPT != capi.GE_OPT_ADAGRAD or not name.startswith("m2_"))}
    snap["rng_state"] = h.rng_state()
    if h._cfg.shuffle == capi.GE_SHUFFLE_JAVA:
        snap["perm"] = h.perm().tobytes()
    return snap


@pytest.mark.parametrize("opt,device,tables", [("adam", dict(mode="hogwild", shuffle="device", seed=42), 12),
                                               ("adagrad", dict(mode="deterministic", shuffle="java", seed=42), 8)])
def test_a_function_of_the_input_alone_and_a_pure_read(gpu, opt, device, tables):
    V, D, n, K = 300, 33, 130, 33
    F, C, fb, cb = P.float_tables(55, V, D)
    F, C, fb, cb = F * np.float32(0.125), C * np.float32(0.125), fb * np.float32(0.125), cb * np.float32(0.125)       # trainable magnitudes
    I, _ = _pairs(8, n, V)
    filters = P.csr([np.flatnonzero(synth.splitmix64(21 + k, V) % np.uint64(4) == 0) for k in range(n)])
    subset = np.arange(0, V, 3, dtype=np.int32)
    rows = np.repeat(np.arange(V, dtype=np.int64), 3)
    cols = (rows * 7 + np.tile(np.arange(3), V) * 11 + 1) % V
    order = np.lexsort((cols, rows))
    m = geglove.CooMatrix(V, rows[order].astype(np.int32), cols[order].astype(np.int32), np.full(len(rows), 0.05, np.float32), 0.2)
    h = geglove.createOptimizer(make_config(D, "glove", opt=opt, **device), m)
    try:
        _set(h, F, C, fb, cb)
        before = _snapshot(h)
        assert len([k for k in before if k in capi.ALL_STATE_NAMES]) == tables, sorted(before)
        assert "rng_state" in before and ("perm" in before) == (device["shuffle"] == "java")
        pr = capi.Prediction(h._h, I, filters, subset, True)
        try:
            first = pr.run(K)
            again = pr.run(K)
            other = capi.Prediction(h._h, I, filters, subset, True)
            try:
                second_set = other.run(K)
            finally:
                other.close()
            for a, b, c in zip(first, again, second_set):
                assert a.tobytes() == b.tobytes() == c.tobytes()
            t, E = P.bound(F, C, cb, I)
            keep = P.candidates(n, V, filters, subset, I)
            model, ok = P.decided(t, E, keep, K)
            P.check_within_bound(*first, t, E, keep, model, ok)
            assert _snapshot(h) == before, "a prediction wrote to the trainer"
            h.epoch(0)
            assert _snapshot(h) != before
            moved = pr.run(K)
            assert moved[1].tobytes() != first[1].tobytes(), "a run after an epoch did not stage the tables again"
        finally:
            pr.close()
    finally:
        h.close()


# ------------------------------------------------------------------ F
def test_a_planted_answer(gpu):
    """Query i is row i of a 64 x 64 Hadamard matrix; column 64 + i is twice that row (z = 128), column 128 + i three times it
    (z = 192), every other special column is orthogonal to it (z = 0) and the rest hold -1, 0, 1 (|z| <= 64).  With column 128 + i
    in the filter of query i the answer is 64 + i; without it, 128 + i and then 64 + i."""
    D, n, V = 64, 64, 256
    H = np.array([[1.0]])
    while H.shape[0] < D:
        H = np.block([[H, H], [H, -H]])
    F = N.integers(3, (V, D), -1, 1); F[:n] = H
    C = N.integers(4, (V, D), -1, 1); C[64:128] = 2 * H; C[128:192] = 3 * H
    zero = np.zeros(V, np.float32)
    I = np.arange(n, dtype=np.int32)
    h = _handle(V, D)
    try:
        _set(h, F.astype(np.float32), C.astype(np.float32), zero, zero)
        got, _ = _predict(h, I, (2,), P.csr([[128 + i] for i in range(n)]))
        index, score, count = got[2]
        assert np.array_equal(index[:, 0], 64 + I) and np.all(score[:, 0] == 128) and np.all(score[:, 1] <= 64) and np.all(count == 2)
        got, _ = _predict(h, I, (2,))
        index, score, count = got[2]
        assert np.array_equal(index, np.stack([128 + I, 64 + I], axis=1)) and np.array_equal(score, np.tile(np.float32([192, 128]), (n, 1)))
    finally:
        h.close()

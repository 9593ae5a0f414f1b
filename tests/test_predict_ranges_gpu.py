"""Link prediction on candidate ranges of several tiles, at real row widths (ge_glove_predict_*, csrc/predict.hip k_predict_select
and k_predict_merge) against numpy.  test_predict_gpu.py has ranges of several tiles only at dim 4, where a row is one partial
panel and the column loop of a tile runs once; a real table has dim 200 (six whole 32-column panels and one of 8) or an odd dim
such as 33 (D4 = 36).  There the first panel of the next tile is requested from inside the last panel of the current one while
the thresholds, the filter cursors and the compacted lists are carried from tile to tile.

19 200 queries -- 150 distinct (row, filter list) pairs, each 128 times, in a scattered order -- against V = 1100 columns are 300
query tiles and 9 candidate tiles: five ranges of two tiles by the rule of predict_run_impl, which every run asserts from
ge_predict_get.  At K = 128 that is 19 200 x 5 x 128 (query, range, slot) entries, fewer than one launch keeps: one batch.
  integer   small integers, exact in fp32 (predict_ref.integer_tables, rank_ref.scores), ties plentiful;
  floats    z = chain(focus[i], context) + cBias, the header's fmaf chain in numpy (tests/chain_ref.py with its condition, no nonzero
            product below 2^-100), columns c + 550 copies of columns c.
Index, score bits and count equal the yardstick in every slot of every query.  Then every K = 10 prediction goes to
ge_glove_rank_run (192 000 pairs: 3000 query tiles, one range of all nine tiles there) and comes back with rank t + 1 and the
model's score bits.  And the planted case of test_predict_gpu.py, the best columns in the last tile of every fourth range and all
of them filtered, is repeated at dim 200."""
import numpy as np
import pytest

from geglove import capi, synth
import chain_ref as CH
import predict_ref as P
import rank_ref as R
from test_rank_gpu import _handle, _set, _pairs
from test_predict_gpu import _same, _designed_filters

pytestmark = pytest.mark.gpu

V, DISTINCT, TIMES = 1100, 150, 128
N = DISTINCT * TIMES
TILES = (V + 127) // 128


def _predict(h, I, K, filters, own, tiles=TILES):
    """One run; asserts several ranges of several tiles, and that the queries went in one batch."""
    pr = capi.Prediction(h._h, I, filters, None, own)
    try:
        out = pr.run(K)
        info = pr.info()
        ranges = info["ranges"]
        per = (tiles + ranges - 1) // ranges
        assert info["n"] == len(I) and ranges > 1 and per >= 2, ("no several ranges of several tiles: this test no longer tests what it is for", info)
        # 2^24 is PD_BATCH_ENTRIES of csrc/predict.hip (ge_predict_get reports no batch count): keep the two in step
        assert len(I) * ranges * K <= 2 ** 24, ("more (query, range, slot) entries than one launch keeps: adapt n", info)
        return out, info
    finally:
        pr.close()


def _expand(lists, order):
    length = np.array([len(l) for l in lists], np.int64)
    ptr = np.zeros(len(order) + 1, np.int64)
    ptr[1:] = np.cumsum(length[order])
    return ptr, np.concatenate([np.asarray(lists[k], np.int32) for k in order]).astype(np.int32)


def _lists_of(csr):
    ptr, idx = csr
    return [idx[ptr[k]:ptr[k + 1]] for k in range(len(ptr) - 1)]


def _order(seed, n, distinct):
    return (np.argsort(synth.splitmix64(seed, n), kind="stable") % distinct).astype(np.int64)


def _tables(kind, D):
    if kind == "integer":
        return P.integer_tables(1000 * V + D, V, D)
    F, C, fb, cb = P.float_tables(1000 * V + D + 1, V, D)
    m = V // 2
    C[m:] = C[:m]; cb[m:] = cb[:m]
    return F, C, fb, cb


def _scores(kind, F, C, cb, rows):
    if kind == "integer":
        return R.scores(F, C, cb, rows)
    Z = CH.chain(F[rows], C) + cb[None, :]
    assert Z.dtype == np.float32 and np.all(np.isfinite(Z))
    return Z


@pytest.mark.parametrize("kind", ["integer", "floats"])
@pytest.mark.parametrize("D", [200, 33])
def test_ranges_of_several_tiles(gpu, D, kind):
    F, C, fb, cb = _tables(kind, D)
    rows, _ = _pairs(D + 5, DISTINCT, V)
    Z = _scores(kind, F, C, cb, rows)
    order = _order(9 + D, N, DISTINCT)
    I = rows[order]
    h = _handle(V, D)
    try:
        _set(h, F, C, fb, cb)
        for K in (10, 128):
            for own in (False, True):
                self_col = rows if own else None
                plain = P.topk(Z, K, None, None, self_col)
                assert np.all(plain[2] == K)
                if kind == "floats":
                    assert np.mean((plain[1][:, 1:] == plain[1][:, :-1]).any(axis=1)) > 0.5              # twins in the lists
                (got, info) = _predict(h, I, K, None, own)
                _same(got, tuple(w[order] for w in plain), (D, kind, K, own, "plain", info))
                designed = _designed_filters(7 * V + D + K, Z, K, None, self_col)
                want = P.topk(Z, K, designed, None, self_col)
                assert np.all(want[0][4::6] != plain[0][4::6])                                          # kind 4: every slot changes
                (got, info) = _predict(h, I, K, _expand(_lists_of(designed), order), own)
                _same(got, tuple(w[order] for w in want), (D, kind, K, own, "designed filters", info))
    finally:
        h.close()


@pytest.mark.parametrize("D", [200, 33])
def test_every_prediction_of_a_large_set_has_its_rank(gpu, D):
    """Every K = 10 prediction of the 19 200 queries, handed to ge_glove_rank_run with the query's list (plus the row itself under
    exclude_self), has rank t + 1 and the score bits of the chain model.  192 000 pairs are 3000 query tiles: the rank grid is one
    range of all nine candidate tiles, asserted from ge_rank_get."""
    K = 10
    F, C, fb, cb = _tables("floats", D)
    rows, _ = _pairs(D + 5, DISTINCT, V)
    Z = _scores("floats", F, C, cb, rows)
    order = _order(9 + D, N, DISTINCT)
    I = rows[order]
    lists = [np.flatnonzero(synth.splitmix64(1900 + D + k, V) % np.uint64(16) == 0) for k in range(DISTINCT)]
    h = _handle(V, D)
    try:
        _set(h, F, C, fb, cb)
        for filters, own in ((None, False), (lists, True)):
            want = P.topk(Z, K, None if filters is None else P.csr(filters), None, rows if own else None)
            assert np.all(want[2] == K)
            got, _ = _predict(h, I, K, None if filters is None else _expand(filters, order), own)
            _same(got, tuple(w[order] for w in want), (D, own, "chain model"))
            per_row = [np.union1d(filters[k] if filters is not None else [], [rows[k]] if own else []).astype(np.int32) for k in range(DISTINCT)]
            rk = capi.Ranking(h._h, np.repeat(I, K).astype(np.int32), got[0].reshape(-1), *_expand(per_row, np.repeat(order, K)))
            try:
                rank, zt, s = rk.run()
                info = rk.get()
            finally:
                rk.close()
            assert info["n"] == N * K and (TILES + info["ranges"] - 1) // info["ranges"] >= 2, ("the rank grid has no range of two tiles", info)
            bad = np.flatnonzero(rank.reshape(N, K) != np.arange(1, K + 1)[None, :])
            assert bad.size == 0, "query %d slot %d has rank %d" % (bad[0] // K, bad[0] % K, rank[bad[0]])
            assert zt.tobytes() == want[1][order].tobytes()
            assert s == R.summary(np.tile(np.arange(1, K + 1), N))
    finally:
        h.close()


def test_filtered_best_columns_met_after_the_thresholds_at_dim_200(gpu):
    """test_predict_gpu.test_filtered_best_columns_met_after_the_thresholds at dim 200: the best scores of every row sit in the last
    tile of the last range and in the last tile of every fourth range before it, range 0 included, and all of them are filtered --
    they beat every threshold set before them and only the filter test keeps them out.  The table is 28 tiles under 300 query tiles:
    seven ranges of four tiles, so the planted tiles close ranges 0, 4 and 6."""
    Vp, D = 128 * 28 - 50, 200
    tiles = (Vp + 127) // 128
    F, C, fb, cb = P.integer_tables(31, Vp, D)
    cb = cb.copy()
    rows, _ = _pairs(3, DISTINCT, Vp)
    order = _order(4, N, DISTINCT)
    I = rows[order]
    h = _handle(Vp, D)
    try:
        _set(h, F, C, fb, cb)
        _, info = _predict(h, I, 10, None, False, tiles)
        ranges = info["ranges"]
        per = (tiles + ranges - 1) // ranges
        assert ranges > 4 and (tiles - 1) % per == per - 1, info                  # the last range is whole, and a fourth range exists
        best = [np.arange((tiles - 1) * 128, Vp)]
        best += [np.arange(((r + 1) * per - 1) * 128, ((r + 1) * per - 1) * 128 + 128) for r in range(0, ranges - 1, 4)]
        best = np.unique(np.concatenate(best))
        cb[best] += 1000.0                                                   # far above every other z, still exact
        h.set_state("cbias", cb)
        Z = R.scores(F, C, cb, rows)
        filters = P.csr([best] * DISTINCT)
        for K in (10, 100):
            plain = P.topk(Z, K)
            assert np.all(np.isin(plain[0], best))                           # unfiltered, the planted columns fill every list
            want = P.topk(Z, K, filters)
            assert not np.any(np.isin(want[0], best))
            got, _ = _predict(h, I, K, _expand([best] * DISTINCT, order), False, tiles)
            _same(got, tuple(w[order] for w in want), ("after the thresholds", K))
            got, _ = _predict(h, I, K, None, False, tiles)
            _same(got, tuple(w[order] for w in plain), ("after the thresholds, unfiltered", K))
    finally:
        h.close()

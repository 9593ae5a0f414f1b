"""Ranking on candidate ranges of several tiles, at real row widths (ge_glove_rank_*, csrc/rank.hip k_rank_count) against numpy.
A held-out evaluation is tens of thousands of pairs against hundreds of candidate tiles: every workgroup then walks a range of
several 128-candidate tiles, which is where the next tile's first panel is requested from inside the last panel of the current one,
the accumulators are cleared between tiles and the counts are carried over them.  No other ranking test reaches that shape (their
grids give one tile per range), so each run here first asserts, from ge_rank_get, that its grid had ranges of at least two tiles.

The n pairs are 256 distinct (row, column, filter list) triples, each many times and in a scattered order, so the yardstick is
computed for 256 rows and indexed.  Two kinds of tables:
  integer   small integers, exact in fp32: the fp64 scores of rank_ref.scores ARE the library's, ties are frequent;
  floats    z = chain(focus[i], context) + cBias in one fp32 add, the chain the header's fmaf chain in numpy (tests/chain_ref.py, which
            asserts its condition: no nonzero product below 2^-100); columns c + 550 are copies of columns c, so exact ties
            cross a range boundary.
Ranks, the bits of the reported scores and the summary equal the yardstick for every pair, plain and with filter lists: the five
kinds of test_rank_gpu._filters and a sixth, every column of the last tile of a range that is not the table's last."""
import numpy as np
import pytest

from geglove import capi, synth
import chain_ref as CH
import predict_ref as P
import rank_ref as R
from test_rank_gpu import _handle, _set, _pairs, _integer_tables

pytestmark = pytest.mark.gpu

DISTINCT = 256
TQ, TC = 64, 128                                  # the query and candidate tile of k_rank_count

# (V, D, n): 9 candidate tiles each.  By the rule of rank_run_impl (want = max(1, min(ctiles, 1024, ceil(2048 / qtiles))),
# range_tiles = ceil(ctiles / want)): 300 query tiles give want 7, five ranges of two tiles, the last one a single tile of 76
# candidates; 2048 query tiles give want 1, one range of all nine tiles.  dim 200 is six whole 32-column panels and one of 8,
# dim 33 one panel and a partial one of 4 (D4 = 36), dim 64 two whole panels and no partial one.
SHAPES = [(1100, 200, 19200), (1100, 33, 131072), (1100, 64, 19200)]


def _tile_filters(seed, J, V, range_tiles):
    """test_rank_gpu._filters with a sixth kind: per pair, in turn, an empty list, a list that holds the target, every column, a
    list that ends at V - 1, any list, and every column of one whole tile -- the last tile of a range that is not the last one
    (with a single range: any tile but the table's last)."""
    tiles = (V + TC - 1) // TC
    ranges = (tiles + range_tiles - 1) // range_tiles
    lists = []
    for k, j in enumerate(J):
        pick = synth.splitmix64(seed + k, V) % np.uint64(4) == 0
        kind = k % 6
        if kind == 0:
            pick[:] = False
        elif kind == 1:
            pick[j] = True
        elif kind == 2:
            pick[:] = True
        elif kind == 3:
            pick[V - 1] = True
        elif kind == 5:
            tile = ((k // 6) % (ranges - 1) + 1) * range_tiles - 1 if ranges > 1 else (k // 6) % (tiles - 1)
            assert tile < tiles - 1
            pick[:] = False
            pick[tile * TC:(tile + 1) * TC] = True
        lists.append(np.flatnonzero(pick))
    return lists


def _expand(lists, order):
    """The CSR arrays of lists[order[0]], lists[order[1]], ..."""
    length = np.array([len(l) for l in lists], np.int64)
    ptr = np.zeros(len(order) + 1, np.int64)
    ptr[1:] = np.cumsum(length[order])
    return ptr, np.concatenate([lists[k] for k in order]).astype(np.int32)


def _run(h, I, J, filters, V, D):
    tiles = (V + TC - 1) // TC
    rk = capi.Ranking(h._h, I, J, *(filters or (None, None)))
    try:
        assert rk.get() == {"n": len(I), "candidates": V, "dim": D, "ranges": 0}                  # no run yet
        out = rk.run()
        info = rk.get()
        assert info["ranges"] >= 1 and dict(info, ranges=0) == {"n": len(I), "candidates": V, "dim": D, "ranges": 0}, info
        per = (tiles + info["ranges"] - 1) // info["ranges"]
        assert per >= 2, ("the grid has no range of two tiles: this test no longer tests what it is for", info)
        return out, info
    finally:
        rk.close()


def _case(V, D, n, tables):
    """What needs no device and no grid: the tables, the 256 distinct pairs, their scores and their order among the n pairs."""
    m = V // 2
    if tables == "integer":
        F, C, fb, cb = _integer_tables(1000 * V + D, V, D)
    else:
        F, C, fb, cb = P.float_tables(1000 * V + D + 1, V, D)
        C[m:] = C[:m]; cb[m:] = cb[:m]                               # column c + 550 is column c: exact ties across a range boundary
    i, j = _pairs(V + D, DISTINCT, V)
    if tables == "floats":
        j[::2] = j[::2] % m + m                                      # the later twin as a target: its copy in another range ties and precedes
        Z = CH.chain(F[i], C) + cb[None, :]
        assert Z.dtype == np.float32 and np.all(np.isfinite(Z))
    else:
        Z = R.scores(F, C, cb, i)
    rows = np.arange(DISTINCT)
    zt = Z[rows, j].astype(np.float32)
    tied = np.mean((Z == Z[rows, j][:, None]).sum(axis=1) > 1)
    print("V %d dim %d n %d %s: the target's score is shared with another column in %.0f %% of the distinct pairs" % (V, D, n, tables, 100 * tied))
    assert tied > 0.5
    assert n % DISTINCT == 0
    order = (np.argsort(synth.splitmix64(V + n, n), kind="stable") % DISTINCT).astype(np.int64)      # every triple all over the query tiles
    return F, C, fb, cb, i, j, Z, zt, order


def _check(got, want, zt, what):
    rank, score, s = got
    assert rank.dtype == np.int32 and score.dtype == np.float32
    bad = np.flatnonzero(rank != want)
    assert bad.size == 0, (what, "%d pairs differ; pair %d: rank %d, want %d" % (bad.size, bad[0], rank[bad[0]], want[bad[0]]))
    assert score.tobytes() == zt.tobytes(), (what, "score bits")
    assert s == R.summary(want), (what, s)


@pytest.mark.parametrize("tables", ["integer", "floats"])
@pytest.mark.parametrize("V,D,n", SHAPES)
def test_ranges_of_several_tiles(gpu, V, D, n, tables):
    F, C, fb, cb, i, j, Z, zt, order = _case(V, D, n, tables)
    I, J = i[order], j[order]
    tiles = (V + TC - 1) // TC
    h = _handle(V, D)
    try:
        _set(h, F, C, fb, cb)
        plain = R.ranks(Z, j)
        got, info = _run(h, I, J, None, V, D)
        _check(got, plain[order], zt[order], ("plain", info))
        # the sixth kind of list is placed by the grid the plain run had, not by a copy of the library's rule
        range_tiles = (tiles + info["ranges"] - 1) // info["ranges"]
        lists = _tile_filters(7 * V + D, j, V, range_tiles)
        filtered = R.ranks(Z, j, R.csr(lists))
        changed = np.mean(plain != filtered)
        print("    %d ranges of %d tiles; the filter lists change %.0f %% of the ranks" % (info["ranges"], range_tiles, 100 * changed))
        assert changed > 0.5, "the filter lists change too few ranks to test anything"
        got, again = _run(h, I, J, _expand(lists, order), V, D)
        assert again == info                                       # the same grid: the lists sit where they were meant to
        _check(got, filtered[order], zt[order], ("filtered", info))
    finally:
        h.close()

"""Non-finite scores in ranking and prediction (ge_glove_rank_*, ge_glove_predict_*; csrc/rank.hip, csrc/predict.hip), stated by hand.
include/geglove.h: "A NaN z ranks, and is reported, as -inf", the order is "as fp32 compares" with equal scores by ascending
column id, "A real candidate whose z is -inf comes before the fill", and a predicted column handed to ge_glove_rank_run returns rank
t + 1.  Both kernels start their thresholds at (-inf, INT_MAX) and tell a real -inf candidate from the fill by the id alone; a
diverged table is where the metrics have to be the documented ones.

Tables of small floats with designed columns, each with a twin m = V / 2 columns on (another tile, at V = 1100 another range):
  NAN_ENTRY    a NaN element;
  INF_D0       +inf at d = 0, met by focus rows whose element 0 is positive (+inf), zero (0 * inf = NaN) and negative (-inf);
  CB_PINF, CB_NINF, CB_NAN     cBias +inf, -inf, NaN;
  INF_CB_NINF  +inf at d = 0 AND cBias -inf: where the chain reaches +inf, inf - inf = NaN;
  OVERFLOW     the header's case (2^100, 2^100) . (2^100, -2^100) with the focus row BIG: the fused chain holds fmaf(2^100, 2^100, 0)
               = +inf and then fmaf(2^100, -2^100, +inf) = +inf, where a product rounded on its own would give inf - inf = NaN;
and one focus row that holds a NaN, so that every z of that query is -inf.  CLASS below states what every (kind of query, designed
column) must give; it is first asserted against the fmaf chain in numpy (kernel_model.fma32 under np.errstate: chain_ref.chain
asserts its small-product condition and is used for the finite part only), and only then is the device asked.

-0 as a z is unreachable and has no case here: a chain from +0 never holds -0 (an exact cancellation gives +0 under round to
nearest), and s + cBias is -0 only where both are."""
import functools

import numpy as np
import pytest

from geglove import capi, synth
import chain_ref as CH
import predict_ref as P
import rank_ref as R
from kernel_model import fma32
from test_rank_gpu import _handle, _set
from test_predict_gpu import _same

pytestmark = pytest.mark.gpu

F32 = np.float32
INF = F32(np.inf)
NEG_INF_BITS = 0xFF800000

NAN_ENTRY, INF_D0, CB_PINF, CB_NINF, CB_NAN, INF_CB_NINF, OVERFLOW = 3, 5, 7, 9, 11, 13, 15
DESIGNED = {"NAN_ENTRY": NAN_ENTRY, "INF_D0": INF_D0, "CB_PINF": CB_PINF, "CB_NINF": CB_NINF, "CB_NAN": CB_NAN, "INF_CB_NINF": INF_CB_NINF,
            "OVERFLOW": OVERFLOW}
ZERO_ROWS, BIG, NANROW = (2, 4), 6, 8

# what z is BEFORE the NaN map, per kind of focus row: element 0 positive, zero, negative; (2^100, 2^100, ..); a row with a NaN.
# "nan" ranks, and is reported, as -inf.
CLASS = {
    #            NAN_ENTRY  INF_D0   CB_PINF  CB_NINF  CB_NAN  INF_CB_NINF  OVERFLOW
    "pos":      ("nan",     "+inf",  "+inf",  "-inf",  "nan",  "nan",       "fin"),
    "zero":     ("nan",     "nan",   "+inf",  "-inf",  "nan",  "nan",       "fin"),
    "neg":      ("nan",     "-inf",  "+inf",  "-inf",  "nan",  "-inf",      "fin"),
    "big":      ("nan",     "+inf",  "+inf",  "-inf",  "nan",  "nan",       "+inf"),
    "nanrow":   ("nan",     "nan",   "nan",   "nan",   "nan",  "nan",       "nan"),
}


def _is(z, cls):
    return {"nan": np.isnan(z), "+inf": z == np.inf, "-inf": z == -np.inf, "fin": np.isfinite(z)}[cls]


def _raw_chain(A, B):
    """chain_ref.chain without its condition: the fmaf chain over the zero-padded rows, whatever the values."""
    A, B = CH._pad4(A), CH._pad4(B)
    s = np.zeros((A.shape[0], B.shape[0]), F32)
    with np.errstate(all="ignore"):
        for d in range(A.shape[1]):
            s = fma32(A[:, d, None], B[None, :, d], s)
    return s


@functools.lru_cache(maxsize=None)
def _tables(V, D):
    """(F, C, fb, cb, special columns, {query row: kind}); the arrays are shared between the tests and not written to."""
    m = V // 2
    assert D >= 3 and OVERFLOW < m and NANROW < V
    F, C, fb, cb = P.float_tables(5000 * V + D, V, D)
    for r in ZERO_ROWS:
        F[r, 0] = 0.0
    F[BIG, :2] = 2.0 ** 100
    F[NANROW, 2] = np.nan
    C[NAN_ENTRY, 1] = np.nan
    C[INF_D0, 0] = np.inf
    cb[CB_PINF], cb[CB_NINF], cb[CB_NAN] = np.inf, -np.inf, np.nan
    C[INF_CB_NINF, 0] = np.inf; cb[INF_CB_NINF] = -np.inf
    C[OVERFLOW, :2] = (2.0 ** 100, -(2.0 ** 100))
    more = np.arange(100, m, 128)                                    # a cBias of -inf in (nearly) every tile: real -inf candidates in many ranges
    cb[more] = -np.inf
    designed = np.concatenate([np.array(sorted(DESIGNED.values())), more])
    C[designed + m] = C[designed]; cb[designed + m] = cb[designed]   # the twins
    special = np.concatenate([designed, designed + m])
    plain_rows = [r for r in range(V) if r not in ZERO_ROWS + (BIG, NANROW)]
    kinds = {r: "pos" for r in [r for r in plain_rows if F[r, 0] > 0][:3]}
    kinds.update({r: "neg" for r in [r for r in plain_rows if F[r, 0] < 0][:3]})
    kinds.update({r: "zero" for r in ZERO_ROWS})
    kinds[BIG] = "big"; kinds[NANROW] = "nanrow"
    assert len(kinds) == 10 and max(kinds) < 40
    for a in (F, C, fb, cb):
        a.setflags(write=False)
    return F, C, fb, cb, special, kinds


@functools.lru_cache(maxsize=None)
def _model(V, D):
    """(query rows, z before the NaN map as fp32 [10][V]).  The finite part is chain_ref.chain; the special columns and the NaN row
    are the plain fmaf chain; CLASS is asserted on the result, and the OVERFLOW entry is shown to tell a fused chain from a
    product rounded on its own."""
    F, C, fb, cb, special, kinds = _tables(V, D)
    rows = np.array(sorted(kinds), np.int32)
    Ff, Cf = F.copy(), C.copy()
    Ff[NANROW] = 0; Cf[special] = 0
    S = CH.chain(Ff[rows], Cf)
    assert np.all(np.isfinite(S))
    S[:, special] = _raw_chain(F[rows], C[special])
    nanq = np.flatnonzero(rows == NANROW)
    S[nanq] = _raw_chain(F[rows[nanq]], C)
    with np.errstate(all="ignore"):
        Z = (S + cb[None, :]).astype(F32)
    m = V // 2
    for q, r in enumerate(rows):
        for name, cls in zip(DESIGNED, CLASS[kinds[r]]):
            for c in (DESIGNED[name], DESIGNED[name] + m):
                assert _is(Z[q, c], cls), ("row %d (%s) column %d (%s): %r is not %s" % (r, kinds[r], c, name, Z[q, c], cls))
    ordinary = np.setdiff1d(np.arange(V), special)
    assert np.all(np.isfinite(Z[np.ix_(rows != NANROW, ordinary)])) and np.all(np.isnan(Z[nanq]))
    with np.errstate(all="ignore"):
        a, b = F[BIG, :2], C[OVERFLOW, :2]
        assert np.isnan(F32(F32(a[0] * b[0]) + F32(a[1] * b[1])))           # the unfused sum is inf - inf
        assert fma32(a[1], b[1], fma32(a[0], b[0], F32(0))) == INF           # the header's chain is +inf
    return rows, Z


def _csr_or_none(lists):
    return None if lists is None else R.csr(lists)


# ------------------------------------------------------------------ rank
@pytest.mark.parametrize("D", [8, 40])
def test_ranks_at_non_finite_scores(gpu, D):
    V = 300
    m = V // 2
    F, C, fb, cb, special, kinds = _tables(V, D)
    rows, Z = _model(V, D)
    targets = np.concatenate([special, [0, 1, 127, 128, 149, 150, 299]]).astype(np.int32)
    q = np.repeat(np.arange(len(rows)), len(targets))
    I, J = rows[q], np.tile(targets, len(rows)).astype(np.int32)
    n = len(I)
    quarter = [np.flatnonzero(synth.splitmix64(40 + k, V) % np.uint64(4) == 0) for k in range(n)]
    lists = [[[], [INF_D0, CB_PINF + m], [NAN_ENTRY, CB_PINF, OVERFLOW, INF_D0 + m], quarter[k]][(k + k // len(targets)) % 4] for k in range(n)]
    h = _handle(V, D)
    try:
        _set(h, F, C, fb, cb)
        for filters in (None, lists):
            want = R.ranks(Z[q], J, _csr_or_none(filters))
            rk = capi.Ranking(h._h, I, J, *(_csr_or_none(filters) or (None, None)))
            try:
                rank, score, s = rk.run()
            finally:
                rk.close()
            bad = np.flatnonzero(rank != want)
            assert bad.size == 0, ("filtered" if filters else "plain", "row %d (%s) column %d: rank %d, want %d" %
                                   (I[bad[0]], kinds[I[bad[0]]], J[bad[0]], rank[bad[0]], want[bad[0]]))
            zt = Z[q, J]
            assert score.tobytes() == CH.ranked(zt).tobytes()
            assert np.isnan(zt).sum() > n // 4 and np.all(score.view(np.uint32)[np.isnan(zt)] == NEG_INF_BITS)   # a NaN is reported with the bytes of -inf
            assert s == R.summary(want) and np.isfinite(s["mrr"]) and np.isfinite(s["mean_rank"]) and 1 <= s["mean_rank"] <= V
            for k in range(n):
                gone = set(np.asarray(filters[k]).tolist()) if filters else set()
                if kinds[I[k]] == "nanrow":                          # every z is -inf: the order is the ids'
                    assert rank[k] == 1 + len([c for c in range(J[k]) if c not in gone]), (k, J[k])
                if kinds[I[k]] == "pos" and J[k] in (INF_D0, CB_PINF, INF_D0 + m, CB_PINF + m):
                    # the row's four +inf columns, equal as fp32 compares: ordered by id across the tiles
                    ahead = [c for c in (INF_D0, CB_PINF, INF_D0 + m, CB_PINF + m) if c < J[k] and c not in gone]
                    assert rank[k] == 1 + len(ahead), (k, J[k], rank[k])
    finally:
        h.close()


# ------------------------------------------------------------------ predict
def _keep_lists(V, special, rows, kept, extra):
    """Per query a filter list of every ordinary column but `kept` of them, spread over the table and shifted by the query
    (kept None: no such list), plus, for every other query, two of the +inf columns."""
    m = V // 2
    ordinary = np.setdiff1d(np.arange(V), special)
    lists = []
    for k in range(len(rows)):
        gone = np.zeros(0, np.int64)
        if kept is not None:
            gone = np.setdiff1d(ordinary, ordinary[((np.arange(kept) * len(ordinary)) // kept + k) % len(ordinary)])
        if k % 2 == extra:
            gone = np.union1d(gone, [INF_D0, CB_PINF + m])
        lists.append(gone.astype(np.int32))
    return lists


# kept ordinary columns per (V, K): none filtered; few enough that |C_k| < K; and so many that |C_k| > K with fewer than K of
# them finite, so that K cuts the run of real -inf candidates (V = 40 has fewer than K = 64 columns: there every list is short)
KEPT = {40: (None, 10, 26), 300: (None, 60, 120), 1100: (None, 90, 115)}


@pytest.mark.parametrize("V,K,D", [(40, 64, 8), (40, 64, 40), (300, 128, 8), (300, 128, 40), (1100, 128, 8), (1100, 128, 40)])
def test_predictions_at_non_finite_scores(gpu, V, K, D):
    """K is larger than the number of finite candidates, and in most variants larger than |C_k|: the real -inf candidates follow the
    finite ones in ascending id and the (-1, -inf) fill comes after them; out_count = min(K, |C_k|).  At V = 1100 the ten queries
    make nine ranges of one tile, so the -inf candidates of different ranges meet in k_predict_merge.  Every list goes back
    through ge_glove_rank_run: rank t + 1 and the same score bits."""
    F, C, fb, cb, special, kinds = _tables(V, D)
    rows, Z = _model(V, D)
    n = len(rows)
    h = _handle(V, D)
    try:
        _set(h, F, C, fb, cb)
        for kept, own in zip(KEPT[V], (False, True, False)):
            lists = _keep_lists(V, special, rows, kept, int(own))
            filters = R.csr(lists)
            self_col = rows if own else None
            want = P.topk(Z, K, filters, None, self_col)
            keep = P.candidates(n, V, filters, None, self_col)
            finite = (np.isfinite(Z) & keep).sum(axis=1)
            assert np.all(want[2] == np.minimum(K, keep.sum(axis=1)))
            short = int((want[2] < K).sum())
            print("V %d K %d dim %d kept %s: %d of %d lists are shorter than K; finite candidates %d .. %d of %d .. %d" %
                  (V, K, D, kept, short, n, finite.min(), finite.max(), keep.sum(axis=1).min(), keep.sum(axis=1).max()))
            if kept is not None:
                assert np.all(finite < K), "K is not larger than the number of finite candidates"
                above = ((CH.ranked(Z) > -np.inf) & keep).sum(axis=1)
                assert np.all(above < np.minimum(K, keep.sum(axis=1))), "a list would hold no real -inf candidate"
                assert (short == n) if kept == KEPT[V][1] or V == 40 else (short == 0), "the variant is not what it is for"
            pr = capi.Prediction(h._h, rows, filters, None, own)
            try:
                got = pr.run(K)
                info = pr.info()
            finally:
                pr.close()
            assert V < 1100 or info["ranges"] > 1, info
            _same(got, want, (V, K, D, kept, own))
            index, score, count = got
            pairs_i, pairs_j, pairs_f, pairs_z = [], [], [], []
            for k in range(n):
                c = int(count[k])
                assert np.all(index[k, c:] == -1) and np.all(score[k, c:].view(np.uint32) == NEG_INF_BITS)      # the fill comes last
                real = index[k, :c]
                low = np.flatnonzero(score[k, :c] == -np.inf)
                if low.size:                                       # the real -inf candidates: after the others, in ascending id
                    assert low[0] + low.size == c and np.all(np.diff(real[low]) > 0), (k, real[low])
                    zk = CH.ranked(Z[k])
                    all_low = np.flatnonzero((zk == -np.inf) & keep[k])
                    assert np.array_equal(real[low], all_low[:low.size]), (k, "not the first real -inf candidates by id")
                gone = np.union1d(lists[k], [rows[k]] if own else []).astype(np.int32)
                for t in range(c):
                    pairs_i.append(rows[k]); pairs_j.append(real[t]); pairs_f.append(gone); pairs_z.append(score[k, t])
            low_count = np.array([int((score[k, :count[k]] == -np.inf).sum()) for k in range(n)])
            kq = int(np.flatnonzero(rows == NANROW)[0])
            assert low_count[kq] == count[kq] and count[kq] > 0                              # the NaN row: nothing but real -inf candidates
            if kept is not None:
                # fewer than K candidates are finite or +inf, so every list, not only the NaN row's, holds real -inf candidates
                assert np.all(low_count >= 1), ("a list without a real -inf candidate", low_count)
            rk = capi.Ranking(h._h, np.array(pairs_i, np.int32), np.array(pairs_j, np.int32), *R.csr(pairs_f))
            try:
                rank, zt, s = rk.run()
            finally:
                rk.close()
            expect = np.concatenate([np.arange(1, int(c) + 1) for c in count])
            bad = np.flatnonzero(rank != expect)
            assert bad.size == 0, "row %d column %d: rank %d, want %d" % (pairs_i[bad[0]], pairs_j[bad[0]], rank[bad[0]], expect[bad[0]])
            assert zt.tobytes() == np.array(pairs_z, F32).tobytes() and np.isfinite(s["mrr"]) and np.isfinite(s["mean_rank"])
    finally:
        h.close()

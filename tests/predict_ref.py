"""The yardstick of the prediction tests (ge_glove_predict_*, include/geglove.h "Prediction"): numpy in fp64 on the same fp32
inputs.  Never the library itself.

Exact tables.  Where focus, context and cBias hold small integers every product, partial sum and the bias add are exact in
fp32, so the fp64 value of z IS the library's z and `topk` gives index, score bits and count with no tolerance, ties included.

The bound is rank_ref.py's: with u = 2^-24, S = sum_d |a_d b_d| and t = s + cb in exact arithmetic, the library's z^ obeys
    |z^ - t| <= E := (D + 2) u (S + |cb|)
(the derivation, and the condition S + |cb| >= 2^-100 that covers subnormal steps, are written down there; `bound` asserts the
condition).  Candidate c is PROVABLY before d when t_c - E_c > t_d + E_d: then z^_c > z^_d whatever the rounding.  From that:
  * a returned score lies within E of the t of its index;
  * no unreturned candidate is provably before a returned one;
  * of two neighbouring returned entries the later is never provably before the earlier;
  * slot s of a query is DECIDED when exactly s candidates are provably before the fp64 model's s-th entry m_s and m_s is
    provably before all the others: a correct library has m_s there.  The other slots are left out of that comparison;
    `decided` reports them so that a test can cap their share before it looks at device output."""
import numpy as np

import nn_ref as N
import rank_ref as R

U = R.U
csr = R.csr


def value_range(dim):
    """|x_d| <= 8 and every partial sum far below 2^24; narrow ranges at the wide dims keep ties frequent."""
    return 8 if dim <= 3 else 2 if dim <= 50 else 1


def integer_tables(seed, V, D):
    """(focus, context, fbias, cbias) of small integers as fp32: every z is exact in fp32 and ties are plentiful."""
    v = value_range(D)
    assert v * v * D + v < 2 ** 24
    return (N.integers(seed, (V, D), -v, v), N.integers(seed + 1, (V, D), -v, v), N.integers(seed + 2, (V,), -9, 9),
            N.integers(seed + 3, (V,), -v, v))


def float_tables(seed, V, D):
    return (N.random_rows(seed, V, D), N.random_rows(seed + 1, V, D), N.uniform(seed + 2, (V,)).astype(np.float32),
            N.uniform(seed + 3, (V,)).astype(np.float32))


def candidates(n, V, filters=None, subset=None, self_col=None):
    """bool[n][V]: True where column c is a candidate of query k -- c in S, c not in F_k, c != self_col[k]."""
    keep = np.zeros((n, V), bool)
    if subset is None:
        keep[:] = True
    else:
        keep[:, np.asarray(subset, np.int64)] = True
    if filters is not None:
        ptr, idx = filters
        for k in range(n):
            keep[k, idx[ptr[k]:ptr[k + 1]]] = False
    if self_col is not None:
        keep[np.arange(n), np.asarray(self_col, np.int64)] = False
    return keep


def _select(Z, K, keep):
    n = Z.shape[0]
    index = np.full((n, K), -1, np.int32)
    score = np.full((n, K), -np.inf, np.float32)
    count = np.zeros(n, np.int32)
    for k in range(n):
        cols = np.flatnonzero(keep[k])
        order = cols[np.argsort(-Z[k, cols], kind="stable")][:K]         # stable: equal z stay in ascending column order
        count[k] = len(order)
        index[k, :len(order)] = order
        score[k, :len(order)] = Z[k, order].astype(np.float32)
    return index, score, count


def topk(Z, K, filters=None, subset=None, self_col=None):
    """(index int32[n][K], score float32[n][K], count int32[n]) of the score matrix Z [n][V] in fp64 under the total order: z
    descending (a NaN counts as -inf, -0 = +0), equal z by ascending column; the slots past count hold (-1, -inf)."""
    Z = np.asarray(Z, np.float64)
    Z = np.where(np.isnan(Z), -np.inf, Z)
    return _select(Z, K, candidates(Z.shape[0], Z.shape[1], filters, subset, self_col))


def bound(focus, context, cbias, I, row_begin=0):
    """(t, E) [n][V] of the docstring."""
    t = R.scores(focus, context, cbias, I, row_begin)
    D = np.asarray(context).shape[1]
    assert D <= 1024
    S = np.abs(np.asarray(focus, np.float64)[np.asarray(I) - row_begin]) @ np.abs(np.asarray(context, np.float64)).T
    S = S + np.abs(np.asarray(cbias, np.float64))[None, :]
    assert S.min() >= 2.0 ** -100, "a score so small that subnormal steps are not covered by the bound"
    return t, (D + 2) * U * S


def decided(t, E, keep, K):
    """(model index int32[n][K], decided bool[n][K]) of the docstring; a slot past the model's count is decided (it holds the
    fill whatever the rounding: the count is a property of the candidate set)."""
    n = t.shape[0]
    model, _, count = _select(t, K, keep)
    ok = np.ones((n, K), bool)
    for k in range(n):
        cols = np.flatnonzero(keep[k])
        lo, hi = t[k, cols] - E[k, cols], t[k, cols] + E[k, cols]
        for s in range(count[k]):
            m = model[k, s]
            before = int((lo > t[k, m] + E[k, m]).sum())                  # provably before m
            after = int((hi < t[k, m] - E[k, m]).sum())                   # m provably before them
            ok[k, s] = before == s and after == len(cols) - s - 1
    return model, ok


def check_within_bound(index, score, count, t, E, keep, model, ok):
    """Every check of the docstring on a result over generic floats.  Returns the largest |score - t| / E seen."""
    n, K = index.shape
    worst = 0.0
    for k in range(n):
        c = int(count[k])
        want = min(K, int(keep[k].sum()))
        assert c == want, "query %d: count %d, want %d" % (k, c, want)
        assert np.all(index[k, c:] == -1) and np.all(np.isneginf(score[k, c:])), "query %d: the slots past the count are not the fill" % k
        if c == 0:
            continue
        got = index[k, :c].astype(np.int64)
        assert got.min() >= 0 and got.max() < t.shape[1] and np.all(keep[k, got]), "query %d lists a column that is no candidate" % k
        assert len(set(got.tolist())) == c, "query %d lists a column twice" % k
        z = score[k, :c].astype(np.float64)
        err = np.abs(z - t[k, got])
        assert np.all(err <= E[k, got]), "query %d: a score is %.3g E from the fp64 value" % (k, (err / E[k, got]).max())
        worst = max(worst, float((err / E[k, got]).max()))
        assert np.all(z[1:] <= z[:-1]), "query %d: scores increase along the list" % k
        tie = score[k, 1:c] == score[k, :c - 1]
        assert np.all(got[1:][tie] > got[:-1][tie]), "query %d: equal scores out of column order" % k
        lo, hi = t[k, got] - E[k, got], t[k, got] + E[k, got]
        assert not np.any(lo[1:] > hi[:-1]), "query %d: two neighbouring entries are provably in the wrong order" % k
        rest = keep[k].copy()
        rest[got] = False
        if rest.any():
            assert (t[k, rest] - E[k, rest]).max() <= hi[-1], "query %d: an unreturned candidate is provably before the last entry" % k
        sel = ok[k, :c]
        assert np.array_equal(got[sel], model[k, :c][sel]), "query %d: a decided slot holds another column" % k
    return worst

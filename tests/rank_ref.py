"""The yardstick of the ranking tests (ge_glove_rank_*, include/geglove.h "Ranking"): numpy in fp64 on the same fp32 inputs.
Never the library itself.

Exact tables.  Where focus, context and cBias hold small integers every product, partial sum and the bias add are exact in fp32,
so the fp64 value of z IS the library's z and `ranks` gives the ranks with no tolerance, ties included.

The bound.  u = 2^-24 is the unit roundoff of fp32, D = dim, S = sum_d |a_d b_d|.  The library's s^ is an fmaf chain of length
D: one rounding per step and none of the product, so |s^ - s| <= gamma_D S with gamma_D = D u / (1 - D u).  z^ = fl(s^ + cb) adds
one rounding: |z^ - (s + cb)| <= (1 + u) gamma_D S + u (|s^| + |cb|) <= ((1 + 2 u) gamma_D + u) S + u |cb|.  At D <= 1024,
D^2 u + 2 D u <= 1/16 + 2^-13 < 1, hence (1 + 2 u) gamma_D + u <= (D + 2) u, and
    |z^ - t| <= E := (D + 2) u (S + |cb|),          t = s + cb in exact arithmetic.
The chain's bound counts relative roundings only; a step whose result is subnormal errs by at most 2^-150 absolutely instead.
D of those stay below 2^-140, which the slack left above (more than u (S + |cb|) / 2) covers as soon as S + |cb| >= 2^-100:
`bracket` asserts that.  t and S themselves are fp64 quantities whose own error (~2^-53 relative) is not counted.

Two columns whose t differ by more than the sum of their E keep their order under any scores within E of the truth; closer
ones may come out either way.  So with the target j and the unfiltered columns c != j:
    lo = 1 + #{c : t_c - E_c >  t_j + E_j}   (these precede j whatever the rounding)
    hi = 1 + #{c : t_c + E_c >= t_j - E_j}   (only these can)
and lo <= rank <= hi is what a correct library must give -- and all that can be asked on generic floats."""
import numpy as np

U = 2.0 ** -24


def csr(lists):
    """(filter_ptr int64[n + 1], filter_idx int32) of a list of id lists."""
    ptr = np.zeros(len(lists) + 1, np.int64)
    ptr[1:] = np.cumsum([len(l) for l in lists])
    idx = np.concatenate([np.asarray(l, np.int32).reshape(-1) for l in lists]) if len(lists) else np.zeros(0, np.int32)
    return ptr, idx.astype(np.int32)


def _mask(n, V, J, filters):
    """True where column c counts for pair k: c != J[k] and c not in F_k."""
    keep = np.ones((n, V), bool)
    keep[np.arange(n), J] = False
    if filters is not None:
        ptr, idx = filters
        for k in range(n):
            keep[k, idx[ptr[k]:ptr[k + 1]]] = False
    return keep


def scores(focus, context, cbias, I, row_begin=0):
    """t[k][c] in fp64: focus[I[k] - row_begin] . context[c] + cbias[c]."""
    F = np.asarray(focus, np.float64)[np.asarray(I) - row_begin]
    return F @ np.asarray(context, np.float64).T + np.asarray(cbias, np.float64)[None, :]


def ranks(Z, J, filters=None):
    """rank[k] = 1 + #{c counted : Z[k][c] > Z[k][J[k]], or equal and c < J[k]}; a NaN ranks as -inf.  Z: [n][V]."""
    Z = np.where(np.isnan(Z), -np.inf, np.asarray(Z, np.float64))
    n, V = Z.shape
    J = np.asarray(J, np.int64)
    zt = Z[np.arange(n), J][:, None]
    before = (Z > zt) | ((Z == zt) & (np.arange(V)[None, :] < J[:, None]))
    return (1 + (before & _mask(n, V, J, filters)).sum(axis=1)).astype(np.int32)


def bracket(focus, context, cbias, I, J, filters=None, row_begin=0):
    """(lo, hi, t_target, E_target) of the docstring, every pair."""
    t = scores(focus, context, cbias, I, row_begin)
    D = np.asarray(context).shape[1]
    assert D <= 1024
    S = np.abs(np.asarray(focus, np.float64)[np.asarray(I) - row_begin]) @ np.abs(np.asarray(context, np.float64)).T
    S = S + np.abs(np.asarray(cbias, np.float64))[None, :]
    assert S.min() >= 2.0 ** -100, "a score so small that subnormal steps are not covered by the bound"
    E = (D + 2) * U * S
    n, V = t.shape
    J = np.asarray(J, np.int64)
    rows = np.arange(n)
    tj, Ej = t[rows, J][:, None], E[rows, J][:, None]
    keep = _mask(n, V, J, filters)
    lo = 1 + ((t - E > tj + Ej) & keep).sum(axis=1)
    hi = 1 + ((t + E >= tj - Ej) & keep).sum(axis=1)
    return lo, hi, tj[:, 0], Ej[:, 0]


def summary(rank):
    """ge_rank_summary from the ranks: fp64 sums in ascending k from 0.0 (numpy's cumsum adds in that order), then / n."""
    r = np.asarray(rank, np.float64)
    n = len(r)
    return {"n": n, "mrr": float(np.cumsum(1.0 / r)[-1] / n), "mean_rank": float(np.cumsum(r)[-1] / n),
            "hits1": int((r <= 1).sum()), "hits10": int((r <= 10).sum()), "hits100": int((r <= 100).sum())}

"""The yardstick of the nearest-neighbour tests: numpy in fp64 on the same fp32 input, the inputs, and the derived bound.
Never the library itself.

The bound.  u = 2^-24 is the unit roundoff of fp32.  The library scores prepared rows xh = fl(x / n): every component is rounded
once, |xh_d - x_d / n| <= u |x_d / n| (n itself is an fp64 quantity whose error, ~2^-53, is not counted), so xh = y + e with y the
exact unit vector and ||e|| <= u.  Then
    |xh_q . xh_c - y_q . y_c| <= ||e_q|| ||y_c|| + ||y_q|| ||e_c|| + ||e_q|| ||e_c|| <= 2 u + u^2,
and the fp32 fmaf chain of length dim adds at most gamma_dim ||xh_q|| ||xh_c|| with gamma_dim = dim u / (1 - dim u) and
||xh|| <= 1 + u.  At dim <= 1024 the sum is below (dim + 4) u =: B.  The chain's bound needs every product and partial sum to
be normal or zero-free of underflow; `cosines` asserts the inputs are scaled so that no component of a prepared row is subnormal.

Two candidates whose true cosines differ by more than 2 B keep their order under any scores within B of the truth; closer
ones may come out either way, which is what the checks below allow -- and nothing else."""
import numpy as np

from geglove import synth

U = 2.0 ** -24
TINY = float(np.finfo(np.float32).tiny)


def bound(dim):
    return (dim + 4) * U


def uniform(seed, shape):
    """Uniform on [-1, 1) from SplitMix64."""
    n = int(np.prod(shape))
    u = (synth.splitmix64(seed, n) >> np.uint64(11)).astype(np.float64) * (1.0 / 9007199254740992.0)
    return (2.0 * u - 1.0).reshape(shape)


def integers(seed, shape, lo, hi):
    """Integers of [lo, hi] as fp32."""
    n = int(np.prod(shape))
    v = (synth.splitmix64(seed, n) >> np.uint64(33)).astype(np.int64) % (hi - lo + 1) + lo
    return v.reshape(shape).astype(np.float32)


def random_rows(seed, n, dim):
    """Rows of uniform components, scaled per row by 2^e, e in [-3, 3]: norms differ, nothing is near the subnormal range."""
    X = uniform(seed, (n, dim)) * np.exp2(integers(seed ^ 0xABCD, (n, 1), -3, 3).astype(np.float64))
    return X.astype(np.float32)


def unit_rows(X):
    """x / ||x|| in fp64 (a zero row stays zero); asserts that the fp32 image of no nonzero component is subnormal."""
    X = np.asarray(X, dtype=np.float64)
    n = np.sqrt((X * X).sum(axis=1, keepdims=True))
    Y = np.divide(X, n, out=np.zeros_like(X), where=n > 0)
    nz = np.abs(Y[Y != 0])
    assert nz.size == 0 or nz.min() >= TINY, "a prepared component is subnormal: rescale the input"
    return Y


def planted(seed, clusters, size, dim, noise):
    """`clusters` centres on the unit sphere, `size` near-duplicates of each (centre + noise * uniform / sqrt(dim)), shuffled."""
    C = uniform(seed, (clusters, dim))
    C /= np.linalg.norm(C, axis=1, keepdims=True)
    X = np.repeat(C, size, axis=0) + noise / np.sqrt(dim) * uniform(seed + 1, (clusters * size, dim))
    label = np.repeat(np.arange(clusters), size)
    order = np.argsort(synth.splitmix64(seed + 2, clusters * size), kind="stable")
    return X[order].astype(np.float32), label[order]


def exact_topk(S, k, self_pos=None):
    """The first k columns of every row of the integer-valued score matrix S in the order (score descending, column ascending):
    what a stable sort of -S gives.  Computed through the key -S * ncols + column, which orders the same way and lets numpy
    select instead of sorting whole rows (test_nn_abi.py holds the two routes against each other)."""
    S = np.asarray(S)
    nq, n = S.shape
    assert np.array_equal(S, np.rint(S)) and np.abs(S).max() < 2 ** 24
    key = -S.astype(np.int64) * n + np.arange(n, dtype=np.int64)[None, :]
    if self_pos is not None:
        key[np.arange(nq), self_pos] = np.iinfo(np.int64).max
    part = np.partition(key, k - 1, axis=1)[:, :k]
    part.sort(axis=1)
    idx = (part % n).astype(np.int32)
    return idx, np.take_along_axis(S, idx.astype(np.int64), axis=1).astype(np.float32)


def stable_topk(S, k, self_pos=None):
    """The same by the definition: numpy's stable sort by (-score, id), the query's own column removed first."""
    S = np.asarray(S)
    idx = np.empty((S.shape[0], k), np.int32)
    for q in range(S.shape[0]):
        order = np.argsort(-S[q], kind="stable")
        if self_pos is not None:
            order = order[order != self_pos[q]]
        idx[q] = order[:k]
    return idx, np.take_along_axis(S, idx.astype(np.int64), axis=1).astype(np.float32)


def check_against_cosines(Yq, Yc, idx, score, B, self_pos=None, ids=None, q_block=1024, c_block=1 << 18):
    """Every check of a cosine result against fp64 cosines t = Yq @ Yc.T (Yq, Yc: unit rows in fp64), for every query and every
    element.  idx holds ORIGINAL ids when `ids` (ascending original id of every candidate row) is given, positions otherwise;
    self_pos[q] is the candidate position a query must not return (or None).  Returns the largest |score - t| / B seen."""
    nq, k = idx.shape
    n = Yc.shape[0]
    pos = idx.astype(np.int64)
    if ids is not None:
        ids = np.asarray(ids, dtype=np.int64)
        pos = np.searchsorted(ids, pos)
        assert np.all(pos < n) and np.array_equal(ids[pos], idx), "an index that is not a candidate's id"
    assert pos.min() >= 0 and pos.max() < n, "index out of range"
    srt = np.sort(pos, axis=1)
    assert np.all(srt[:, 1:] != srt[:, :-1]), "a query lists a candidate twice"
    if self_pos is not None:
        assert not np.any(pos == np.asarray(self_pos)[:, None]), "a query lists itself"
    s = score.astype(np.float64)
    assert np.all(s[:, 1:] <= s[:, :-1]), "scores increase along a list"
    tie = score[:, 1:] == score[:, :-1]
    assert np.all(pos[:, 1:][tie] > pos[:, :-1][tie]), "equal scores out of id order"
    worst = 0.0
    for q0 in range(0, nq, q_block):
        q1 = min(nq, q0 + q_block)
        t_ret = np.einsum("qd,qkd->qk", Yq[q0:q1], Yc[pos[q0:q1]])
        err = np.abs(s[q0:q1] - t_ret)
        worst = max(worst, float(err.max()) / B)
        assert np.all(err <= B), "a score is %.3g B from the fp64 cosine of its index" % (err.max() / B)
        # wherever two returned rows differ in t by more than 2 B, the larger comes first
        run_min = np.minimum.accumulate(t_ret, axis=1)
        assert np.all(t_ret[:, 1:] - run_min[:, :-1] <= 2 * B), "two returned rows more than 2 B apart are in the wrong order"
        # no unreturned candidate has t greater than the smallest returned t plus 2 B
        floor = t_ret.min(axis=1)
        rows = np.arange(q1 - q0)
        for c0 in range(0, n, c_block):
            c1 = min(n, c0 + c_block)
            T = Yq[q0:q1] @ Yc[c0:c1].T
            p = pos[q0:q1]
            inside = (p >= c0) & (p < c1)
            T[np.repeat(rows, k)[inside.ravel()], (p - c0).ravel()[inside.ravel()]] = -np.inf
            if self_pos is not None:
                sp = np.asarray(self_pos)[q0:q1]
                m = (sp >= c0) & (sp < c1)
                T[rows[m], sp[m] - c0] = -np.inf
            assert np.all(T.max(axis=1) <= floor + 2 * B), "an unreturned candidate beats a returned one by more than 2 B"
    return worst

"""The score that include/geglove.h promises for the five matrix-core score kernels (k_nn_score_select, k_pca_project,
k_km_assign, k_predict_select, k_rank_count), in numpy: "an fp32 fmaf chain from 0 in ascending d".  Never the library itself.

`chain` is that sentence and nothing else: s = +0.0f, then s = fmaf(a[d], b[d], s) for d = 0, 1, ... with one rounding per step
(kernel_model.fma32).  The kernels read rows padded with zeros to a multiple of four floats, so the chain runs over the padded
length too (fmaf(0, 0, s) = s for every s a chain can reach: a chain from +0 never holds -0, an exact cancellation gives +0).

Conditions under which the header's sentence is held to the bit: no nonzero product below 2^-100 in magnitude (nothing pins how
the matrix cores treat subnormal products or sums; `chain` asserts it, as nn_ref / kmeans_ref keep clear of the subnormal range),
and, for the general-float tests, finite partial sums (the overflow tests state what they expect by hand).

`topk` is the header's total order on float scores; labels come from kmeans_ref.assign and ranks from `ranks` below."""
import numpy as np

from kernel_model import fma32

F32 = np.float32
SMALLEST_PRODUCT = 2.0 ** -100


def _pad4(A):
    A = np.ascontiguousarray(A, F32)
    assert A.ndim == 2
    D4 = (A.shape[1] + 3) // 4 * 4
    out = np.zeros((A.shape[0], D4), F32)
    out[:, :A.shape[1]] = A
    return out


def assert_no_small_product(A, B):
    """No nonzero |a_d b_d| below 2^-100: per d, the smallest nonzero |a_d| times the smallest nonzero |b_d|."""
    A, B = np.abs(np.asarray(A, F32).astype(np.float64)), np.abs(np.asarray(B, F32).astype(np.float64))
    A[A == 0] = np.inf
    B[B == 0] = np.inf
    lo = A.min(axis=0) * B.min(axis=0)
    assert np.all(lo >= SMALLEST_PRODUCT), "a nonzero product is below 2^-100 (column %d): rescale the input" % int(np.argmin(lo))


def chain(A, B, order=None, fused=True):
    """fp32 [m][n]: s = fma32(A[:, d], B[:, d], s) from +0.0f over ascending d, A fp32 [m][D], B fp32 [n][D].
    `order` (a sequence of column indices of the padded rows) and `fused=False` (the product rounded on its own, then added)
    exist for the rivals that test_chain_ref.py holds the model apart from; the header's chain is the default."""
    A, B = _pad4(A), _pad4(B)
    assert A.shape[1] == B.shape[1], "rows of different lengths"
    assert_no_small_product(A, B)
    s = np.zeros((A.shape[0], B.shape[0]), F32)
    with np.errstate(over="ignore", invalid="ignore"):
        for d in (range(A.shape[1]) if order is None else order):
            a, b = A[:, d, None], B[None, :, d]
            s = fma32(a, b, s) if fused else ((a * b).astype(F32) + s).astype(F32)
    return s


def dot64(A, B):
    """fp32(fp64 dot): the correctly rounded score, up to fp64's own error."""
    return (_pad4(A).astype(np.float64) @ _pad4(B).astype(np.float64).T).astype(F32)


def descending(A, B):
    D4 = (np.asarray(A).shape[1] + 3) // 4 * 4
    return chain(A, B, order=range(D4 - 1, -1, -1))


def unfused(A, B):
    return chain(A, B, fused=False)


def ranked(S):
    """S as the header's order sees it: fp32, a NaN counting as -inf."""
    S = np.array(S, F32)
    S[np.isnan(S)] = -np.inf
    return S


def topk(S, k, self_pos=None):
    """Per row of the score matrix S the first k columns of the header's total order: score descending as fp32 compares (so
    -0 = +0), a NaN counting (and reported) as -inf, equal scores by ascending column; column self_pos[q] is no candidate of
    row q.  Returns (int32 columns, fp32 scores)."""
    S = ranked(S)
    nq, n = S.shape
    order = np.argsort(-S, axis=1, kind="stable")               # -(-0.0) == -(+0.0) under <, and the sort is stable
    if self_pos is not None:
        order = order[order != np.asarray(self_pos, np.int64)[:, None]].reshape(nq, n - 1)
    assert k <= order.shape[1]
    idx = order[:, :k]
    return idx.astype(np.int32), np.take_along_axis(S, idx, axis=1)


def ranks(S, target, excluded=None):
    """1 + the number of columns c != target[q] with S[q, c] > S[q, target[q]] under fp32 compare (NaN as -inf), columns with
    excluded[q, c] set left out: the rank of the target among the columns, ties in the target's favour."""
    S = ranked(S)
    rows = np.arange(S.shape[0])
    above = S > S[rows, np.asarray(target, np.int64)][:, None]
    if excluded is not None:
        above &= ~np.asarray(excluded, bool)
    above[rows, target] = False
    return 1 + above.sum(axis=1).astype(np.int64)

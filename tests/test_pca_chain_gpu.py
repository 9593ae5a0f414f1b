"""k_pca_project held to the header's transform bit for bit -- centred in fp64, rounded to fp32 once, then "an fmaf chain on the
fp32 matrix cores" in ascending d, in numpy (tests/chain_ref.py) -- at (dim, k) pairs that launch every instance <CT> of the kernel
with one and with several column groups; a selection tier that needs no model (W a permutation); and the moments of k_pca_gram
exact on integer rows, at dims where the column of ones of [x | 1] meets a 16-column tile or a 64-column block.

Every comparison is of bytes.  Models with a k of our choosing come from ge_pca_from_moments (host only) with variance 1 and
max_components = k."""
import functools

import numpy as np
import pytest

from geglove import capi, synth
import chain_ref as CH
import nn_ref as NR
import pca_ref as R

pytestmark = pytest.mark.gpu

# transform_impl's rule: CT = the widest of 2, 3, 4 with D4 * proj_w_stride(ct) <= 16128 (strides 48, 48, 80) and ct <= KW / 16,
# else 1; groups = ceil(KW / 16 / CT).  (dim, k, CT, column groups):
SHAPES = [(200, 17, 2, 1), (200, 32, 2, 1), (200, 33, 3, 1), (200, 64, 4, 1),
          (200, 65, 4, 2),          # the second group with one live tile of its four
          (204, 64, 3, 2),          # 204 * 80 > 16128: W no longer fits four tiles wide
          (336, 40, 3, 1),          # 336 * 48 = 16128: the last dim at which it fits three wide
          (340, 40, 1, 3),          # 340 * 48 > 16128: one tile wide, three groups
          (1024, 100, 1, 7), (16, 16, 1, 1), (17, 17, 2, 1), (1, 1, 1, 1)]
ROWS = 130                          # two full row tiles of 64 and two rows
ROW_COUNTS = (1, 63, 64, 65)        # at dim 200, besides ROWS


def _launch(dim, k):
    """(CT, column groups) by transform_impl's rule, restated."""
    D4, KW = (dim + 3) // 4 * 4, (k + 15) // 16 * 16
    stride = {2: 48, 3: 48, 4: 80}
    CT = 1
    for ct in (2, 3, 4):
        if D4 * stride[ct] <= 16128 and ct <= KW // 16:
            CT = ct
    return CT, (KW // 16 + CT - 1) // CT


assert all(_launch(d, k) == (ct, g) for d, k, ct, g in SHAPES)
assert {_launch(d, k)[0] for d, k, _, _ in SHAPES} == {1, 2, 3, 4}


def _mean(dim):
    """General fp64 means in [-2, 2): no fp32 numbers, so the centring has to happen in fp64."""
    return 2.0 * NR.uniform(900 + dim, (dim,))


def _rows(dim, n, mean, seed=0):
    return (NR.random_rows(1234 + dim + seed, n, dim).astype(np.float64) + mean).astype(np.float32)


def _model(p, X):
    """The header's transform of the rows X by the model p, from p's own mean and components."""
    dim, k, _, mean, _, _, W = p.get()
    xc = (X.astype(np.float64) - mean).astype(np.float32)
    W32 = W[:, :k].astype(np.float32)
    return CH.chain(xc, np.ascontiguousarray(W32.T))


def _same_bytes(got, want, what):
    assert got.dtype == np.float32 and got.shape == want.shape, what
    if got.tobytes() != want.tobytes():
        bad = got.view(np.uint32) != want.view(np.uint32)
        r, c = np.argwhere(bad)[0]
        raise AssertionError("%s: %d of %d elements differ from the model (columns %s); first at [%d][%d]: got %r, want %r"
                             % (what, bad.sum(), bad.size, np.flatnonzero(bad.any(axis=0))[:8].tolist(), r, c, got[r, c], want[r, c]))


@functools.lru_cache(maxsize=None)
def _dense(dim, k):
    p = capi.Pca.from_moments(_mean(dim), R.spd(dim), 1000, variance=1.0, max_components=k)
    assert p.k == k
    return p


@pytest.mark.parametrize("dim,k,CT,groups", SHAPES)
def test_projection_is_the_chain_bit_for_bit(gpu, dim, k, CT, groups):
    p = _dense(dim, k)
    X = _rows(dim, ROWS, p.get()[3])
    want = _model(p, X)
    assert want.shape == (ROWS, k) and np.all(np.isfinite(want))
    _same_bytes(p.transform(X), want, "dim %d k %d <%d> x %d groups" % (dim, k, CT, groups))
    if dim == 200:
        for n in ROW_COUNTS:                                     # a projected row does not depend on the rows beside it
            _same_bytes(p.transform(X[:n]), want[:n], "dim %d k %d rows %d" % (dim, k, n))


def test_projection_past_the_grid_of_512_row_tiles(gpu):
    """512 * 64 + 65 rows: 514 row tiles on a grid of 512, so two workgroups walk a second tile, the last one of one row."""
    dim = k = 8
    p = _dense(dim, k)
    X = _rows(dim, 512 * 64 + 65, p.get()[3])
    _same_bytes(p.transform(X), _model(p, X), "rows %d" % X.shape[0])


def test_a_capped_model_gives_the_leading_columns(gpu):
    """A projected column does not depend on its neighbours: capped at j the model takes another instance, another slab of W and
    another column group for the same column, and gives the same bytes."""
    dim, k = 200, 65
    p = _dense(dim, k)
    mean, full = p.get()[3], None
    X = _rows(dim, ROWS, mean)
    full = p.transform(X)
    _same_bytes(full, _model(p, X), "uncapped")
    for j in (1, 16, 17, 32, 33, 48, 49, 64):
        q = capi.Pca.from_moments(mean, R.spd(dim), 1000, variance=1.0, max_components=j)
        assert q.k == j and q.get()[6].tobytes() == p.get()[6].tobytes()
        _same_bytes(q.transform(X), np.ascontiguousarray(full[:, :j]), "capped at %d, <%d> x %d" % ((j,) + _launch(dim, j)))


@functools.lru_cache(maxsize=None)
def _permuting(dim, k):
    """A diagonal covariance with distinct entries: the components are unit vectors, component c = e_perm[c]."""
    order = np.argsort(synth.splitmix64(77 + dim, dim), kind="stable")
    var = np.empty(dim)
    var[order] = 2.0 - np.arange(dim) / dim                      # order[c] holds the c-th largest variance
    p = capi.Pca.from_moments(_mean(dim), np.diag(var), 1000, variance=1.0, max_components=k)
    W = p.get()[6]
    assert p.k == k and np.array_equal(W, np.eye(dim)[:, order]), "the solver did not return the permutation"
    return p, order


@pytest.mark.parametrize("dim,k,CT,groups", SHAPES)
def test_a_permutation_selects_the_centred_columns(gpu, dim, k, CT, groups):
    """No model: with W a permutation, out[r][c] = fl32(x[r][perm[c]] - mean[perm[c]]) exactly (every other product is a zero,
    and a chain from +0 never holds -0): a wrong column, a wrong row or a wrong slab of W cannot hide behind rounding."""
    p, perm = _permuting(dim, k)
    mean = p.get()[3]
    for n in ((ROWS,) + ROW_COUNTS if dim == 200 else (ROWS,)):
        X = _rows(dim, n, mean, seed=n)
        want = (X.astype(np.float64) - mean).astype(np.float32)[:, perm[:k]]
        _same_bytes(p.transform(X), np.ascontiguousarray(want), "permutation dim %d k %d rows %d" % (dim, k, n))


# ---------------------------------------------------------------------------------------------------------------------
# Moments, exact.
# ---------------------------------------------------------------------------------------------------------------------
def _integer_rows(n, dim):
    X = NR.integers(31 * dim + n, (n, dim), -3, 3)
    if dim >= 3:
        X[:, 1] = X[:, 0]                                        # a duplicated column
        X[:, 2] = 3                                              # a constant column
    return X


def _closing_formula(X):
    """fit_impl's closing formula on the exact Gram matrix of [x - x0 | 1], x0 = row 0, in its operation order.  With integer rows
    of |x| <= 3 every entry of the Gram matrix is an integer below 2^53 and exact in fp64 in any order of summation."""
    X64 = X.astype(np.float64)
    n = np.float64(X.shape[0])
    Y = X64 - X64[0]
    s, S = Y.sum(axis=0), Y.T @ Y
    assert np.abs(S).max() < 2 ** 53 and np.array_equal(S, np.rint(S))
    return X64[0] + s / n, (S - s[:, None] * s[None, :] / n) / (n - np.float64(1.0))


def _moments_case(n, dim):
    X = _integer_rows(n, dim)
    want_mean, want_cov = _closing_formula(X)
    _, _, rows, mean, cov, _, _ = capi.Pca.fit(X).get()
    assert rows == n
    assert mean.tobytes() == want_mean.tobytes(), "n %d dim %d: the mean differs in %d entries" % (n, dim, np.sum(mean != want_mean))
    if cov.tobytes() != want_cov.tobytes():
        bad = np.argwhere(cov.view(np.uint64) != want_cov.view(np.uint64))
        raise AssertionError("n %d dim %d: %d covariance entries differ, first [%d][%d]: got %r, want %r"
                             % (n, dim, len(bad), bad[0][0], bad[0][1], cov[tuple(bad[0])], want_cov[tuple(bad[0])]))
    if dim >= 3:
        assert not cov[2].any() and not cov[:, 2].any() and mean[2] == 3.0
        assert cov[0].tobytes() == cov[1].tobytes() and cov[:, 0].tobytes() == cov[:, 1].tobytes()


@pytest.mark.parametrize("dim", [15, 16, 63, 64, 65, 127, 128, 129])
def test_moments_are_exact_on_integer_rows(gpu, dim):
    """The column of ones of [x | 1] is column `dim`: at 15 the last of a 16-column tile, at 16 alone in a tile, at 63 the last of
    a full 64-column block, at 64 alone in a block of its own, and so on at 127 / 128.  Rows: below, at and above a 32-row panel;
    289 rows are ten row ranges of one panel, which the reduction adds in eight runs of two."""
    for n in (2, 31, 32, 33, 289):
        _moments_case(n, dim)


def test_moments_are_exact_with_sixteen_full_blocks(gpu):
    """dim 1023: [x | 1] fills sixteen blocks exactly, 136 block pairs; 1000 rows are 16 ranges of two panels."""
    _moments_case(1000, 1023)

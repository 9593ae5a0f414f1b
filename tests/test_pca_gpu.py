"""PCA on the device against numpy in fp64 on the same fp32 input (tests/pca_ref.py): moments, k, projection, within bounds
derived from the number formats; reproducibility; and the trainer-handle entry points against the host-rows ones, bit for bit.
Every test runs under the per-test timeout of pytest.ini, in this one process."""
import functools

import numpy as np
import pytest

import geglove
from geglove import capi, synth
from helpers import make_config
import pca_ref as R

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=None)
def _designed(i):
    X = R.designed_input(*R.DESIGNED[i])
    return X, R.numpy_pca(X)


def _check_against_numpy(X, ref=None, what=""):
    """Moments, k and every element of the projection of X against numpy; returns the model and its projection."""
    ref = ref or R.numpy_pca(X)
    n, D = X.shape
    p = capi.Pca.fit(X)
    dim, k, rows, mean, cov, lam, W = p.get()
    assert (dim, rows) == (D, n)
    mean_use = np.max(np.abs(mean - ref["mean"]) / np.maximum(R.mean_bound(X), np.finfo(float).tiny))
    cov_use = np.max(np.abs(cov - ref["cov"]) / np.maximum(R.cov_bound(X), np.finfo(float).tiny))
    margin = R.share_margin(ref["lam"], ref["k"])
    print("%s n %d D %d: mean error %.3g of its bound, covariance error %.3g of its bound, k %d (numpy %d, share margin %.3g)"
          % (what, n, D, mean_use, cov_use, k, ref["k"], margin))
    assert np.all(np.abs(mean - ref["mean"]) <= R.mean_bound(X))
    assert np.all(np.abs(cov - ref["cov"]) <= R.cov_bound(X))
    assert np.array_equal(cov, cov.T)
    assert margin >= 1e-4, "the input does not decide k: 0.95 is %.3g from a cumulative share" % margin
    assert k == ref["k"]
    out = p.transform(X)
    assert out.shape == (n, k) and out.dtype == np.float32
    bound = R.transform_bound(ref, cov)
    err = np.abs(out.astype(np.float64) - ref["out"])
    print("%s n %d D %d: projection error at most %.3g of its bound" % (what, n, D, np.max(err / np.maximum(bound, np.finfo(float).tiny))))
    assert np.all(err <= bound)                                    # every element
    return p, out, ref


@pytest.mark.parametrize("i", range(len(R.DESIGNED)))
def test_designed_inputs_against_numpy(gpu, i):
    X, ref = _designed(i)
    _check_against_numpy(X, ref, "designed")


@pytest.mark.parametrize("D", [1, 3, 8, 50, 200, 300, 1024])
def test_every_width(gpu, D):
    _check_against_numpy(R.designed_input(4096, D, 0.8, 0.25, seed=100 + D), what="width")


@pytest.mark.parametrize("n", [2, 17, 20011])
def test_row_counts_off_the_panel_height(gpu, n):
    _check_against_numpy(R.designed_input(n, 50, 0.8, 0.25, seed=200 + n), what="rows")


def test_more_than_one_slab(gpu):
    """1.4 M x 48 floats are a little more than one upload slab of 2^26 floats: the second slab's moments are added to the first's."""
    n, D = 1400000, 48
    X = R.designed_input(n, D, 0.8, 0.5, seed=31)
    assert X.size > 2 ** 26
    _check_against_numpy(X, what="slabs")


def test_constant_input(gpu):
    X = np.full((1000, 20), np.float32(0.1))
    p = capi.Pca.fit(X)
    _, k, _, mean, cov, lam, W = p.get()
    assert k == 1 and np.array_equal(mean, np.full(20, float(np.float32(0.1)))) and not cov.any() and not lam.any()
    out = p.transform(X)
    assert out.shape == (1000, 1) and not out.any()


def test_non_finite_input_is_refused(gpu):
    X = R.designed_input(500, 6, 0.8, 0.0).copy()
    X[123, 4] = np.nan
    with pytest.raises(capi.GeError) as e:
        capi.Pca.fit(X)
    assert e.value.status == capi.GE_ERR_ARG and "non-finite input" in str(e.value)
    X[123, 4] = np.inf
    with pytest.raises(capi.GeError) as e:
        capi.Pca.fit(X)
    assert e.value.status == capi.GE_ERR_ARG and "non-finite input" in str(e.value)


def test_same_input_same_bytes(gpu):
    X, _ = _designed(2)
    a, b = capi.Pca.fit(X), capi.Pca.fit(X)
    for ta, tb in zip(a.get()[3:], b.get()[3:]):
        assert ta.tobytes() == tb.tobytes()
    assert a.get()[:3] == b.get()[:3]
    o1, o2, o3 = a.transform(X), a.transform(X), b.transform(X)
    assert o1.tobytes() == o2.tobytes() == o3.tobytes()
    capped = capi.Pca.fit(X, max_components=5)
    assert capped.k == 5 and capped.transform(X).tobytes() == np.ascontiguousarray(o1[:, :5]).tobytes()     # a column does not depend on its neighbours


def test_projected_rows_have_the_leading_eigenvalues_as_covariance(gpu):
    """cov(out) = diag(lambda[:k]).  With out = ref + E, |E[r][c]| <= t_r (the projection bound), and ref centred, the difference
    of the two sample covariances is at most sum_r ((|ref_ra| + |ref_rb|) 2 t_r + 4 t_r^2) / (n - 1) (E - mean(E) is at most 2 t),
    plus what numpy's own fp64 sums of ref may carry (the covariance bound on ref)."""
    for i in (0, 1, 2):
        X, ref = _designed(i)
        p = capi.Pca.fit(X)
        cov = p.get()[4]
        out = p.transform(X).astype(np.float64)
        n, k = out.shape
        t = R.transform_bound(ref, cov)[:, 0]
        a = np.abs(ref["out"])
        s1 = (a * (2 * t)[:, None]).sum(axis=0)
        bound = (s1[:, None] + s1[None, :] + (4 * t * t).sum()) / (n - 1) + R.cov_bound(ref["out"])
        got = np.cov(out, rowvar=False).reshape(k, k)
        err = np.abs(got - np.diag(ref["lam"][:k]))
        print("designed %d: covariance of the projection off diag(lambda) by at most %.3g of its bound" % (i, np.max(err / bound)))
        assert np.all(err <= bound)


@pytest.mark.parametrize("mode,dtype,dim", [("hogwild", "f32", 50), ("hogwild", "bf16", 40), ("deterministic", "f32", 24)])
def test_trainer_handle_entry_points_equal_the_host_rows_ones(gpu, mode, dtype, dim):
    V, N = 3000, 40000
    I, J, Xc, xmax = synth.synthetic_coo(V, N, seed=77)
    m = geglove.CooMatrix(V, I, J, Xc, xmax)
    cfg = make_config(dim, method="pglove", mode=mode, shuffle="java" if mode == "deterministic" else "device", dtype=dtype, seed=5)
    opt = geglove.Adagrad(m, cfg, cfg.costFunction())
    for it in range(3):
        opt.epoch(it)
    before = opt.state()
    rows = opt.extractResultF32().reshape(V, dim)
    on_handle = capi.Pca.fit_glove(opt._h)
    on_rows = capi.Pca.fit(rows)
    ga, gb = on_handle.get(), on_rows.get()
    assert ga[:3] == gb[:3] == (dim, ga[1], V)
    for ta, tb in zip(ga[3:], gb[3:]):
        assert ta.tobytes() == tb.tobytes()
    oa = on_handle.transform_glove(opt._h, V)
    ob = on_rows.transform(rows)
    assert oa.shape == ob.shape == (V, ga[1]) and oa.tobytes() == ob.tobytes()
    assert np.array_equal(on_rows.transform_glove(opt._h, V), ob)
    after = opt.state()
    for name in before:
        assert before[name].tobytes() == after[name].tobytes(), name
    assert rows.tobytes() == opt.extractResultF32().tobytes()
    # and the model is the PCA of those rows
    ref = R.numpy_pca(rows)
    assert np.all(np.abs(ga[4] - ref["cov"]) <= R.cov_bound(rows)) and np.all(np.abs(ga[3] - ref["mean"]) <= R.mean_bound(rows))
    fit_ms, tr_ms = on_handle.kernel_ms()
    assert fit_ms > 0 and tr_ms > 0
    opt.close()

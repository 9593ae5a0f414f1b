"""Top-k nearest neighbours on the device against numpy (tests/nn_ref.py): exact on integer-valued rows -- indices and scores,
no tolerance, ties included -- and within the bound B = (dim + 4) 2^-24 derived there on cosines, every query and every element;
planted neighbours, determinism, independence of the batch, subsets, the trainer-handle entry point bit for bit, non-finite input,
and one size with several upload slabs and candidate ranges."""
import numpy as np
import pytest

import geglove
from geglove import capi, synth
from helpers import make_config
import nn_ref as R

pytestmark = pytest.mark.gpu

WIDTHS = [1, 3, 50, 200, 300, 1024]
TILE = 64                                   # queries per workgroup


def _value_range(dim):
    """|x_d| <= 8 and every partial sum <= 64 dim <= 65536 < 2^24; narrow ranges at the wide dims keep ties frequent."""
    return 8 if dim <= 3 else 2 if dim <= 50 else 1


def _exact(X, nn, query_pos, k, exclude_self, block=2048):
    """One call on the device for all the queries; numpy block by block.  Returns the share of queries whose k-th score is tied
    with the next candidate's (the tie rule decided the result there)."""
    got_i, got_s = nn.query_rows(query_pos, k, exclude_self=exclude_self)
    assert got_i.dtype == np.int32 and got_s.dtype == np.float32 and got_i.shape == got_s.shape == (len(query_pos), k)
    more = min(k + 1, X.shape[0] - int(exclude_self))
    tied = 0
    for q0 in range(0, len(query_pos), block):
        qp = np.asarray(query_pos[q0:q0 + block])
        want_i, want_s = R.exact_topk(X[qp] @ X.T, more, qp if exclude_self else None)
        gi, gs = got_i[q0:q0 + block], got_s[q0:q0 + block]
        bad = np.flatnonzero((gi != want_i[:, :k]).any(axis=1) | (gs != want_s[:, :k]).any(axis=1))
        assert bad.size == 0, "query %d: got %s %s, want %s %s" % (qp[bad[0]], gi[bad[0]], gs[bad[0]], want_i[bad[0], :k], want_s[bad[0], :k])
        if more > k:
            tied += int(np.sum(want_s[:, k - 1] == want_s[:, k]))
    return tied / len(query_pos)


@pytest.mark.parametrize("dim", WIDTHS)
def test_exact_on_integer_rows(gpu, dim):
    """DOT on integer-valued rows: fp32 arithmetic is exact, so indices AND scores equal the stable sort by (-score, id)."""
    v = _value_range(dim)
    assert 64 * dim <= 65536 and v * v * dim < 2 ** 24
    n = 20011
    X = R.integers(10 + dim, (n, dim), -v, v)
    nn = capi.Neighbors.create(X, metric="dot")
    assert nn.get() == (n, dim, capi.GE_NN_DOT)
    every = np.arange(n, dtype=np.int32)
    some = (synth.splitmix64(dim, TILE + 1) % np.uint64(n)).astype(np.int32)
    for k, queries in ((10, every), (1, some[:TILE - 1]), (128, some), (10, some[:1]), (128, every[:4 * TILE + 5])):
        for exclude_self in (False, True):
            tied = _exact(X, nn, queries, k, exclude_self)
            print("exact dim %d n %d k %d nq %d exclude_self %d: k-th score tied with the next in %.0f %% of the queries" % (dim, n, k, len(queries), exclude_self, 100 * tied))
    # None = every indexed row, in order
    a = nn.query_rows(None, 10, exclude_self=True)
    b = nn.query_rows(every, 10, exclude_self=True)
    assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes()
    if dim == 50:
        # 20 011 queries at k = 128 are more partial entries than one launch takes: two batches of queries, by id, in order and by value
        for exclude_self in (False, True):
            _exact(X, nn, every, 128, exclude_self)
            b = nn.query_rows(every, 128, exclude_self=exclude_self)
            a = nn.query_rows(None, 128, exclude_self=exclude_self)
            assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes()
        a = nn.query_vectors(X, 128)
        b = nn.query_rows(every, 128)
        assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes()


@pytest.mark.parametrize("dim", [1, 3, 50, 1024])
def test_exact_on_a_table_smaller_than_a_tile(gpu, dim):
    """17 rows: one candidate range, one short tile; k up to every other row."""
    v = _value_range(dim)
    X = R.integers(90 + dim, (17, dim), -v, v)
    nn = capi.Neighbors.create(X, metric="dot")
    every = np.arange(17, dtype=np.int32)
    for k in (1, 10, 16):
        for exclude_self in (False, True):
            _exact(X, nn, every, k, exclude_self)
            _exact(X, nn, every[5:6], k, exclude_self)
    _exact(X, nn, every, 17, False)
    with pytest.raises(capi.GeError) as e:
        nn.query_rows(every, 17, exclude_self=True)                 # k <= candidates - 1
    assert e.value.status == capi.GE_ERR_ARG
    for bad in ([17], [-1]):
        with pytest.raises(capi.GeError) as e:
            nn.query_rows(bad, 1)
        assert e.value.status == capi.GE_ERR_ARG and "not a row of the index" in str(e.value)
    for k in (0, 129):
        with pytest.raises(capi.GeError) as e:
            nn.query_rows(every, k)
        assert e.value.status == capi.GE_ERR_ARG


def _cosine_case(X, query_pos, k, exclude_self, what):
    nn = capi.Neighbors.create(X)
    idx, score = nn.query_rows(query_pos, k, exclude_self=exclude_self)
    Y = R.unit_rows(X)
    qp = np.arange(X.shape[0]) if query_pos is None else np.asarray(query_pos)
    worst = R.check_against_cosines(Y[qp], Y, idx, score, R.bound(X.shape[1]), qp if exclude_self else None)
    print("%s n %d dim %d k %d nq %d: scores within %.3g of the bound" % (what, X.shape[0], X.shape[1], k, len(qp), worst))
    return nn, idx, score


@pytest.mark.parametrize("dim", WIDTHS)
def test_cosine_within_the_bound(gpu, dim):
    n = 20011
    X = R.random_rows(300 + dim, n, dim)
    some = np.unique((synth.splitmix64(7 * dim, 2 * TILE + 1) % np.uint64(n)).astype(np.int32))
    _cosine_case(X, None, 10, True, "cosine")
    _cosine_case(X, np.arange(0, n, 5, dtype=np.int32), 10, False, "cosine")
    _cosine_case(X, some, 128, False, "cosine")
    _cosine_case(X, some[:1], 1, True, "cosine")
    _cosine_case(X[:17], None, 10, True, "cosine")


@pytest.mark.parametrize("dim", [50, 200])
def test_planted_neighbours(gpu, dim):
    k, clusters = 7, 512
    X, label = R.planted(40 + dim, clusters, k + 1, dim, noise=0.3)
    n = X.shape[0]
    assert n >= 4096
    Y = R.unit_rows(X)
    T = Y @ Y.T
    np.fill_diagonal(T, -np.inf)
    srt = -np.sort(-T, axis=1)
    gap = srt[:, k - 1] - srt[:, k]
    B = R.bound(dim)
    print("planted dim %d: smallest gap between the k-th and (k+1)-th cosine %.3g = %.3g B" % (dim, gap.min(), gap.min() / B))
    assert gap.min() >= 4 * B
    true = np.sort(np.argsort(-T, axis=1, kind="stable")[:, :k], axis=1)
    assert np.all(label[true] == label[:, None])                   # and the true sets are the clusters
    idx, _ = capi.Neighbors.create(X).query_rows(None, k, exclude_self=True)
    assert np.array_equal(np.sort(idx, axis=1), true)


def test_same_bytes_alone_in_a_batch_by_id_or_by_value(gpu):
    n, dim, k = 5003, 200, 10
    X = R.random_rows(77, n, dim)
    a, b = capi.Neighbors.create(X), capi.Neighbors.create(X)
    every = a.query_rows(None, k)
    for other in (a.query_rows(None, k), b.query_rows(None, k), a.query_rows(np.arange(n, dtype=np.int32), k), a.query_vectors(X, k)):
        assert other[0].tobytes() == every[0].tobytes() and other[1].tobytes() == every[1].tobytes()
    excl = a.query_rows(None, k, exclude_self=True)
    for q in (0, 63, 64, 2500, n - 1):
        alone = a.query_rows([q], k)
        by_value = a.query_vectors(X[q:q + 1], k)
        batch = a.query_rows([n - 1 - q, q, 17], k)
        assert alone[0].tobytes() == by_value[0].tobytes() == every[0][q].tobytes() == batch[0][1].tobytes()
        assert alone[1].tobytes() == by_value[1].tobytes() == every[1][q].tobytes() == batch[1][1].tobytes()
        alone = a.query_rows([q], k, exclude_self=True)
        assert alone[0].tobytes() == excl[0][q].tobytes() and alone[1].tobytes() == excl[1][q].tobytes()
    # a vector that is no row of the index: cosine does not see its length
    v = R.random_rows(78, 3, dim)
    r1, r2 = a.query_vectors(v, k), a.query_vectors(v * np.float32(4.0), k)
    assert r1[0].tobytes() == r2[0].tobytes() and r1[1].tobytes() == r2[1].tobytes()
    Y = R.unit_rows(X)
    R.check_against_cosines(R.unit_rows(v), Y, r1[0], r1[1], R.bound(dim))


@pytest.mark.parametrize("metric", ["dot", "cosine"])
def test_an_index_over_a_subset(gpu, metric):
    n, dim, k = 6000, 50, 10
    keep = np.flatnonzero(synth.splitmix64(5, n) % np.uint64(3) != 0).astype(np.int32)          # about two rows in three
    queries = keep[:: 7]
    if metric == "dot":
        X = R.integers(55, (n, dim), -2, 2)
        nn = capi.Neighbors.create(X, subset=keep, metric="dot")
        assert nn.get() == (len(keep), dim, capi.GE_NN_DOT)
        for exclude_self in (False, True):
            sub = X[keep]
            qp = np.searchsorted(keep, queries)
            want_i, want_s = R.exact_topk(sub[qp] @ sub.T, k, qp if exclude_self else None)
            got_i, got_s = nn.query_rows(queries, k, exclude_self=exclude_self)
            assert np.array_equal(got_i, keep[want_i]) and np.array_equal(got_s, want_s)         # original row ids
    else:
        X = R.random_rows(56, n, dim)
        nn = capi.Neighbors.create(X, subset=keep)
        idx, score = nn.query_rows(queries, k, exclude_self=True)
        Y = R.unit_rows(X[keep])
        qp = np.searchsorted(keep, queries)
        R.check_against_cosines(Y[qp], Y, idx, score, R.bound(dim), qp, ids=keep)
        full = capi.Neighbors.create(np.ascontiguousarray(X[keep]))                             # the same rows as a table of their own
        fi, fs = full.query_rows(qp.astype(np.int32), k, exclude_self=True)
        assert np.array_equal(keep[fi], idx) and fs.tobytes() == score.tobytes()
    missing = np.setdiff1d(np.arange(n, dtype=np.int32), keep)[:1]
    with pytest.raises(capi.GeError) as e:
        nn.query_rows(missing, k)
    assert e.value.status == capi.GE_ERR_ARG and "not a row of the index" in str(e.value)


@pytest.mark.parametrize("mode,dtype,dim", [("hogwild", "f32", 50), ("hogwild", "bf16", 40), ("deterministic", "f32", 24)])
def test_trainer_handle_entry_point_equals_the_host_rows_one(gpu, mode, dtype, dim):
    V, N, k = 3000, 40000, 10
    I, J, Xc, xmax = synth.synthetic_coo(V, N, seed=77)
    m = geglove.CooMatrix(V, I, J, Xc, xmax)
    cfg = make_config(dim, method="pglove", mode=mode, shuffle="java" if mode == "deterministic" else "device", dtype=dtype, seed=5)
    opt = geglove.Adagrad(m, cfg, cfg.costFunction())
    for it in range(3):
        opt.epoch(it)
    before = opt.state()
    rows = opt.extractResultF32().reshape(V, dim)
    keep = np.arange(1, V, 3, dtype=np.int32)
    for subset in (None, keep):
        for metric in ("cosine", "dot"):
            on_handle = capi.Neighbors.create_glove(opt._h, subset=subset, metric=metric)
            on_rows = capi.Neighbors.create(rows, subset=subset, metric=metric)
            assert on_handle.get() == on_rows.get() == (V if subset is None else len(keep), dim, capi.NN_METRICS[metric])
            a, b = on_handle.query_rows(None, k, exclude_self=True), on_rows.query_rows(None, k, exclude_self=True)
            assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes()
            prep_ms, query_ms = on_handle.kernel_ms()
            assert prep_ms > 0 and query_ms > 0
            if metric == "cosine":
                ids = np.arange(V) if subset is None else keep
                Y = R.unit_rows(rows[ids])
                R.check_against_cosines(Y, Y, a[0], a[1], R.bound(dim), np.arange(len(ids)), ids=ids)
    after = opt.state()
    for name in before:
        assert before[name].tobytes() == after[name].tobytes(), name
    assert rows.tobytes() == opt.extractResultF32().tobytes()
    opt.close()


def test_non_finite_input_is_refused_and_a_zero_row_is_harmless(gpu):
    X = R.random_rows(9, 500, 6)
    for bad in (np.nan, np.inf, -np.inf):
        for metric in ("cosine", "dot"):
            Z = X.copy(); Z[123, 4] = bad
            with pytest.raises(capi.GeError) as e:
                capi.Neighbors.create(Z, metric=metric)
            assert e.value.status == capi.GE_ERR_ARG and "non-finite input" in str(e.value)
            nn = capi.Neighbors.create(X, metric=metric)
            with pytest.raises(capi.GeError) as e:
                nn.query_vectors(Z[120:125], 3)
            assert e.value.status == capi.GE_ERR_ARG and "non-finite input" in str(e.value)
    Z = X[:100].copy(); Z[20] = 0
    nn = capi.Neighbors.create(Z)
    idx, score = nn.query_rows(None, 99, exclude_self=True)
    others = np.delete(np.arange(100), 20)
    assert np.all(np.isfinite(score))
    assert not score[20].any() and np.array_equal(idx[20], others)                              # 0 against everything, in id order
    at = np.argmax(idx == 20, axis=1)
    assert np.all((idx[others] == 20).any(axis=1)) and not score[others, at[others]].any()
    Y = R.unit_rows(Z)
    R.check_against_cosines(Y, Y, idx, score, R.bound(6), np.arange(100))                       # and the other rows are not poisoned


def test_more_than_one_slab_and_many_candidate_ranges(gpu):
    """1.4 M x 48 floats are a little more than one upload slab of 2^26 floats; 4096 queries leave the grid to the candidate ranges."""
    n, dim, nq, k = 1400000, 48, 4096, 10
    X = R.random_rows(31, n, dim)
    assert X.size > 2 ** 26
    queries = np.unique((synth.splitmix64(32, nq) % np.uint64(n)).astype(np.int32))
    queries = np.union1d(queries, np.arange(n - (nq - len(queries)), n, dtype=np.int32)).astype(np.int32)[:nq]
    nn = capi.Neighbors.create(X)
    idx, score = nn.query_rows(queries, k, exclude_self=True)
    Y = R.unit_rows(X)
    worst = R.check_against_cosines(Y[queries], Y, idx, score, R.bound(dim), queries, q_block=512, c_block=1 << 17)
    prep_ms, query_ms = nn.kernel_ms()
    print("n %d dim %d nq %d: scores within %.3g of the bound; prepare %.2f ms, query %.2f ms" % (n, dim, len(queries), worst, prep_ms, query_ms))

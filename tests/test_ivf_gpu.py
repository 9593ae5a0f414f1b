"""The inverted-file index on the device against the header in numpy (tests/ivf_ref.py): indices, scores, counts, candidate
counts, labels, sizes and centroids are compared AS BYTES -- no bound, no slot left out.  Given centroids at the edges of the
32-column panel and of D4, of the 128-row candidate tile, of the 64-query tile and of the four list capacities; ties inside a list
and across lists; duplicate centroids and empty lists; a list longer than the scan's chunk; two batches of queries; equality with
the exact index at nprobe = L on every one of these families, by id with and without exclude_self and by value; the trained path
against ge_kmeans_*; the trainer-handle entry point.
Every table, centroid set and query-vector set compared with the model comes from ivf_ref.case(name); test_ivf_ref.py walks the
same list and holds each to what it is designed for, without a device."""
import numpy as np
import pytest

import geglove
from geglove import capi, synth
from helpers import make_config
import ivf_ref as IR
import nn_ref as R

pytestmark = pytest.mark.gpu

KS = (1, 16, 17, 32, 33, 64, 65, 128)               # both sides of every edge of ivf_cap_of: CAP 32 | 64 | 128 | 256
DIMS = IR.DIMS
NAMES = ("index", "score", "count", "candidates")


def _same(got, want, what):
    for name, g, w in zip(NAMES, got, want):
        assert g.dtype == w.dtype and g.shape == w.shape, (what, name, g.dtype, g.shape, w.dtype, w.shape)
        if g.tobytes() != w.tobytes():
            bad = np.argwhere(g.view(np.uint32) != w.view(np.uint32))
            at = tuple(bad[0])
            raise AssertionError("%s: %d of %d %s entries differ from the model; first at %s: got %r, want %r (row got %s want %s)"
                                 % (what, len(bad), g.size, name, at, g[at], w[at], g[at[0]], w[at[0]]))


def _same_build(ivf, m, what):
    assert ivf.labels.tobytes() == m.label.tobytes(), what + ": labels"
    assert ivf.sizes.tobytes() == m.sizes.tobytes(), what + ": sizes"
    assert ivf.centroids.tobytes() == m.cen.tobytes(), what + ": centroids"


def _same_as_exact(got, exact, what):
    """nprobe = L: every row is a candidate, and out_index / out_score are the exact index's bytes."""
    assert got[0].tobytes() == exact[0].tobytes() and got[1].tobytes() == exact[1].tobytes(), what + ": differs from ge_nn_*"


def _every_list_probed_is_the_exact_index(ivf, nn, n, L, vector_sets, ks, what, ids=None):
    """nprobe = L against ge_nn_query_rows (every row, or `ids`; with and without exclude_self) and ge_nn_query_vectors (every
    set of vectors), out_index and out_score byte for byte; k is cut to what ge_nn_* accepts."""
    for k in ks:
        for ex in (False, True):
            kk = min(k, n - int(ex))
            got = ivf.query_rows(ids, kk, L, exclude_self=ex)
            _same_as_exact(got, nn.query_rows(ids, kk, exclude_self=ex), "%s: rows k %d exclude_self %d" % (what, kk, ex))
            assert np.all(got[2] == kk) and np.all(got[3] == n - int(ex))
        for name, V in vector_sets.items():
            kk = min(k, n)
            _same_as_exact(ivf.query_vectors(V, kk, L), nn.query_vectors(V, kk), "%s: vectors %s k %d" % (what, name, kk))


def _create(c, **kw):
    return capi.IvfNeighbors.create(c.X, c.L, subset=c.subset, centroids=c.C, **kw)


# ---- given centroids: every dim, every k, nprobe 1 / 2 / L ---------------------------------------------------------------

@pytest.mark.parametrize("dim", DIMS)
def test_given_centroids_bit_for_bit(gpu, dim):
    """300 rows whose second half doubles the first (identical prepared rows: same list, tied scores), five centroids.  Every k of
    KS with one of nprobe 1 / 2 / L and one way of asking, rotating; then nprobe = L against the exact index."""
    c = IR.case("twin_%d" % dim)
    m, S = c.model()
    n, L = m.XH.shape[0], c.L
    ivf = _create(c)
    assert ivf.get() == {"n": n, "dim": dim, "lists": L, "train_steps": 0, "converged": False}
    _same_build(ivf, m, c.name)
    every = np.arange(n)
    V = c.vectors["mixed"]
    tied = False
    for i, k in enumerate(KS):
        nprobe = (1, 2, L)[(i + dim) % 3]
        mode = (i + dim) % 4
        what = "dim %d k %d nprobe %d mode %d" % (dim, k, nprobe, mode)
        if mode < 2:                                                  # every row by id, without and with exclude_self
            ex = mode == 1
            got = ivf.query_rows(m.ids, k, nprobe, exclude_self=ex)
            want = m.query_rows(every, k, nprobe, ex, S)
            none = ivf.query_rows(None, k, nprobe, exclude_self=ex)
            assert all(a.tobytes() == b.tobytes() for a, b in zip(got, none)), what + ": query_ids None differs"
        elif mode == 2:                                               # 65 rows by id, in no order
            pos = (synth.splitmix64(dim * 100 + k, 65) % np.uint64(n)).astype(np.int64)
            got = ivf.query_rows(m.ids[pos], k, nprobe, exclude_self=True)
            want = m.query_rows(pos, k, nprobe, True, S)
        else:                                                         # by value: 60 vectors that are no rows, three that are
            got = ivf.query_vectors(V, k, nprobe)
            want = m.query_vectors(V, k, nprobe)
        _same(got, want, what)
        tied |= k >= 2 and bool(np.any((want[1][:, 1:] == want[1][:, :-1]) & (want[0][:, 1:] >= 0)))
    assert tied, "no case held a tie"
    nn = capi.Neighbors.create(c.X, subset=c.subset)
    _every_list_probed_is_the_exact_index(ivf, nn, n, L, c.vectors, KS if dim == 50 else (KS[dim % 8], 128), c.name)


# ---- list lengths, query tiles, duplicate centroids, empty lists -----------------------------------------------------------

def test_list_lengths_0_1_127_128_129_and_duplicate_centroids(gpu):
    c = IR.case("axis")
    m, S = c.model()
    assert m.sizes.tolist() == [129, 1, 127, 128, 0, 0]
    ivf = _create(c)
    _same_build(ivf, m, "axis table")
    every = np.arange(c.X.shape[0])
    for k, nprobe, ex in ((1, 1, False), (16, 1, True), (33, 2, False), (128, 1, True), (128, 1, False), (65, 6, True), (128, 6, False), (17, 2, True)):
        got = ivf.query_rows(every, k, nprobe, exclude_self=ex)
        want = m.query_rows(every, k, nprobe, ex, S)
        _same(got, want, "axis table k %d nprobe %d exclude_self %d" % (k, nprobe, ex))
    # the one member of list 1, alone with exclude_self: nothing is left
    lone = np.flatnonzero(m.label == 1)
    got = ivf.query_rows(lone, 16, 1, exclude_self=True)
    assert got[2].tolist() == [0] and got[3].tolist() == [0] and np.all(got[0] == -1) and np.all(np.isneginf(got[1]))
    # all six lists probed, two of them empty: the exact index
    _every_list_probed_is_the_exact_index(ivf, capi.Neighbors.create(c.X), len(every), 6, c.vectors, (1, 17, 65, 128), "axis table")


@pytest.mark.parametrize("nq", [1, 63, 64, 65])
def test_query_tiles_of_1_63_64_65_on_one_list(gpu, nq):
    c = IR.case("axis")
    m, S = c.model()
    ivf = _create(c)
    V = c.vectors["near3_%d" % nq]
    for k in (16, 128):
        got = ivf.query_vectors(V, k, 1)
        assert np.all(got[3] == 128)                                  # every query probes list 3 alone
        _same(got, m.query_vectors(V, k, 1), "nq %d k %d" % (nq, k))
    members = np.flatnonzero(m.label == 3)[:nq]
    _same(ivf.query_rows(members, 33, 1, exclude_self=True), m.query_rows(members, 33, 1, True, S), "nq %d by id" % nq)


def test_duplicate_centroid_and_a_query_that_probes_only_empty_lists(gpu):
    c = IR.case("axis")
    m, S = c.model()
    ivf = _create(c)
    V = c.vectors["dup_and_empty"]
    probed = m.probe(IR.given(V), 2)
    assert probed[:3].tolist() == [[0, 4]] * 3                        # the duplicate: lower id first
    assert np.all(probed[3:, 0] == 5)                                 # -e0: the empty list first
    for k in (1, 17, 128):
        got = ivf.query_vectors(V, k, 1)
        _same(got, m.query_vectors(V, k, 1), "empty lists k %d" % k)
        assert got[3][:3].tolist() == [129] * 3                       # nprobe = 1 picked list 0, not its empty copy
        assert got[2][3:].tolist() == [0, 0, 0] and np.all(got[0][3:] == -1) and np.all(np.isneginf(got[1][3:]))
        _same(ivf.query_vectors(V, k, 2), m.query_vectors(V, k, 2), "empty lists k %d nprobe 2" % k)


# ---- ties across lists ----------------------------------------------------------------------------------------------------

def test_ties_across_lists_are_broken_by_original_id(gpu):
    c = IR.case("ties")
    m, S = c.model()
    q = c.vectors["e0"]
    ivf = _create(c)
    _same_build(ivf, m, "cross-list ties")
    for k in (1, 16, 17, 48, 64, 128):
        got = ivf.query_vectors(q, k, 2)
        _same(got, m.query_vectors(q, k, 2), "cross-list ties k %d" % k)
        kk = min(k, 48)
        assert got[0][0, :kk].tolist() == list(range(kk))             # all scores equal: ids ascending, lists interleaved
    for ex in (False, True):
        _same(ivf.query_rows(None, 33, 2, exclude_self=ex), m.query_rows(np.arange(48), 33, 2, ex, S), "cross-list ties by id exclude_self %d" % ex)
    _every_list_probed_is_the_exact_index(ivf, capi.Neighbors.create(c.X), 48, 2, c.vectors, (1, 17, 33, 48), "cross-list ties")
    # over a subset ids differ from positions: still by ORIGINAL id
    cs = IR.case("ties_subset")
    ms, Ss = cs.model()
    keep = cs.subset
    sub = _create(cs)
    got = sub.query_vectors(q, 33, 2)
    _same(got, ms.query_vectors(q, 33, 2), "cross-list ties over a subset")
    assert got[0][0].tolist() == keep[:33].tolist()
    pos = np.arange(0, len(keep), 3)
    _same(sub.query_rows(keep[pos], 17, 2, exclude_self=True), ms.query_rows(pos, 17, 2, True, Ss), "subset by id")
    _every_list_probed_is_the_exact_index(sub, capi.Neighbors.create(cs.X, subset=keep), len(keep), 2, cs.vectors, (17, 38), "cross-list ties over a subset")


# ---- a list longer than a chunk, and two batches ----------------------------------------------------------------------------

def test_a_list_one_row_longer_than_the_chunk(gpu):
    """THIS TEST DEPENDS ON IVF_CHUNK = 4096 in csrc/ivf.hip (ivf_ref.CHUNK): list 0 holds 4097 rows, so it is scanned as two chunks
    whose partial lists the merge joins; the last row of the list sits alone in the second chunk."""
    c = IR.case("long")
    m, S = c.model()
    X = c.X
    assert m.sizes.tolist() == [IR.CHUNK + 1, 50]
    ivf = _create(c)
    _same_build(ivf, m, "long list")
    last = np.flatnonzero(m.label == 0)[-1:]
    pos = np.concatenate([last, (synth.splitmix64(5, 69) % np.uint64(X.shape[0])).astype(np.int64)])
    V = c.vectors["mixed"]
    for k, nprobe in ((1, 1), (17, 2), (128, 1), (128, 2)):
        _same(ivf.query_rows(pos, k, nprobe, exclude_self=True), m.query_rows(pos, k, nprobe, True, S), "long list k %d nprobe %d" % (k, nprobe))
        got = ivf.query_vectors(V, k, nprobe)
        _same(got, m.query_vectors(V, k, nprobe), "long list by value k %d nprobe %d" % (k, nprobe))
        assert got[0][0, 0] == last[0]                                 # the row alone in the second chunk is found
    _every_list_probed_is_the_exact_index(ivf, capi.Neighbors.create(X), X.shape[0], 2, c.vectors, (1, 33, 128), "long list")


def test_two_batches_of_queries(gpu):
    """k = 128 and nprobe = 8 are 1024 partial entries per query (every list is one chunk), so 2^24 / 1024 = 16384 queries fill a
    batch (ivf_ref.BATCH_ENTRIES): 20 000 queries are two.  By id and by value; the model answers the 2000 distinct rows once.
    At nprobe = 16 = L a batch holds 8192 queries, 20 000 are three, and the result is the exact index's."""
    c = IR.case("batches")
    n, L, k, nprobe, nq = 2000, 16, 128, 8, 20000
    assert nq * nprobe * k > IR.BATCH_ENTRIES and c.X.shape[0] == n and c.L == L
    m, S = c.model()
    assert m.sizes.max() <= IR.CHUNK
    ivf = _create(c)
    _same_build(ivf, m, "batches")
    ids = (synth.splitmix64(4006, nq) % np.uint64(n)).astype(np.int32)
    ids[:n] = np.arange(n)
    for ex in (False, True):
        once = m.query_rows(np.arange(n), k, nprobe, ex, S)
        _same(ivf.query_rows(ids, k, nprobe, exclude_self=ex), tuple(a[ids] for a in once), "two batches by id exclude_self %d" % ex)
    once = m.query_rows(np.arange(n), k, nprobe, False, S)
    _same(ivf.query_vectors(c.X[ids], k, nprobe), tuple(a[ids] for a in once), "two batches by value")
    _every_list_probed_is_the_exact_index(ivf, capi.Neighbors.create(c.X), n, L, {"its own rows": c.X[ids]}, (k,), "batches", ids=ids)


# ---- the trained path -----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("kind", ["integers", "general"])
@pytest.mark.parametrize("T", IR.TRAIN_STEPS)
def test_trained_equals_kmeans_then_given(gpu, kind, T):
    """ge_ivf_create with T steps against ge_kmeans_create + ge_kmeans_run(T) -> ge_ivf_create(centroids = those): centroids as
    ge_kmeans_get returns them -- and as the numpy run of the same steps gives them --, labels, sizes and results, byte for byte.
    (Giving centroids by value prepares them; test_ivf_ref.py asserts that these are fixed points of the preparation, the condition
    the header names.)"""
    c = IR.case("trained_" + kind)
    X, L, seed = c.X, c.L, IR.TRAIN_SEED
    want_cen, want_steps, want_conv = c.centroids(T)
    km = capi.Clustering.create(X, L, seed=seed)
    steps, conv = km.run(T) if T > 0 else (0, False)
    cen = km.centroids
    assert cen.tobytes() == want_cen.tobytes() and (steps, conv) == (want_steps, want_conv)
    assert IR.given(cen).tobytes() == cen.tobytes(), "a k-means centroid is no fixed point of the preparation: choose another table"
    if T == 50:
        assert conv and 1 < steps < 50, (steps, conv)
    a = capi.IvfNeighbors.create(X, L, train_iterations=T, seed=seed)
    b = capi.IvfNeighbors.create(X, L, centroids=cen)
    ga, gb = a.get(), b.get()
    assert (ga["train_steps"], ga["converged"]) == (steps, conv) and (gb["train_steps"], gb["converged"]) == (0, False)
    assert a.centroids.tobytes() == cen.tobytes() == b.centroids.tobytes()
    assert a.labels.tobytes() == b.labels.tobytes() and a.sizes.tobytes() == b.sizes.tobytes()
    if T > 0 and conv:
        assert a.labels.tobytes() == km.labels.tobytes()               # converged: the last assign is the index's
    m, S = c.model(T)
    _same_build(a, m, "trained %s T %d" % (kind, T))
    V = c.vectors["forty"]
    for k, nprobe, ex in ((10, 1, True), (33, 3, False), (128, L, True)):
        ra, rb = a.query_rows(None, k, nprobe, exclude_self=ex), b.query_rows(None, k, nprobe, exclude_self=ex)
        assert all(x.tobytes() == y.tobytes() for x, y in zip(ra, rb))
        _same(ra, m.query_rows(np.arange(X.shape[0]), k, nprobe, ex, S), "trained %s T %d by id k %d nprobe %d" % (kind, T, k, nprobe))
        ra, rb = a.query_vectors(V, k, nprobe), b.query_vectors(V, k, nprobe)
        assert all(x.tobytes() == y.tobytes() for x, y in zip(ra, rb))
        _same(ra, m.query_vectors(V, k, nprobe), "trained %s T %d k %d nprobe %d" % (kind, T, k, nprobe))
    _every_list_probed_is_the_exact_index(a, capi.Neighbors.create(X), X.shape[0], L, c.vectors, (10, 128), "trained %s T %d" % (kind, T))
    other = capi.IvfNeighbors.create(X, L, train_iterations=T, seed=seed + 1)
    assert other.centroids.tobytes() != cen.tobytes()                 # the seed keys the sample


# ---- the trainer handle ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("mode,dtype,dim", [("hogwild", "f32", 50), ("hogwild", "bf16", 40), ("deterministic", "f32", 24)])
def test_trainer_handle_entry_point_equals_the_host_rows_one(gpu, mode, dtype, dim):
    """The vectors of a trained handle exist on a device only, so nothing here is compared with the numpy model (ivf_ref.cases()
    says so too): the handle entry point against the host-rows one, and nprobe = L against the exact index on the same handle."""
    V, N, k, L = 3000, 40000, 10, 16
    I, J, Xc, xmax = synth.synthetic_coo(V, N, seed=77)
    mat = geglove.CooMatrix(V, I, J, Xc, xmax)
    cfg = make_config(dim, method="pglove", mode=mode, shuffle="java" if mode == "deterministic" else "device", dtype=dtype, seed=5)
    opt = geglove.Adagrad(mat, cfg, cfg.costFunction())
    for it in range(3):
        opt.epoch(it)
    before = opt.state()
    rows = opt.extractResultF32().reshape(V, dim)
    keep = np.arange(1, V, 3, dtype=np.int32)
    given = R.random_rows(88, L, dim)
    for subset in (None, keep):
        for centroids in (None, given):
            on_handle = capi.IvfNeighbors.create_glove(opt._h, L, subset=subset, train_iterations=3, seed=9, centroids=centroids)
            on_rows = capi.IvfNeighbors.create(rows, L, subset=subset, train_iterations=3, seed=9, centroids=centroids)
            assert on_handle.get() == on_rows.get() and on_handle.get()["n"] == (V if subset is None else len(keep))
            assert on_handle.labels.tobytes() == on_rows.labels.tobytes() and on_handle.centroids.tobytes() == on_rows.centroids.tobytes()
            a, b = on_handle.query_rows(None, k, 4, exclude_self=True), on_rows.query_rows(None, k, 4, exclude_self=True)
            assert all(x.tobytes() == y.tobytes() for x, y in zip(a, b))
            build_ms, probe_ms, scan_ms, merge_ms = on_handle.kernel_ms()
            assert build_ms > 0 and probe_ms > 0 and scan_ms > 0 and merge_ms > 0
            exact = capi.Neighbors.create_glove(opt._h, subset=subset)         # every list probed: the exact index on the same handle
            n = V if subset is None else len(keep)
            _every_list_probed_is_the_exact_index(on_handle, exact, n, L, {"eighty-eight": given}, (k,), "trainer handle")
    after = opt.state()
    for name in before:
        assert before[name].tobytes() == after[name].tobytes(), name
    assert rows.tobytes() == opt.extractResultF32().tobytes()
    opt.close()


def test_bad_queries_are_refused(gpu):
    X = R.random_rows(9, 500, 6)
    ivf = capi.IvfNeighbors.create(X, 4, train_iterations=2)
    for bad in ([500], [-1]):
        with pytest.raises(capi.GeError) as e:
            ivf.query_rows(bad, 1, 1)
        assert e.value.status == capi.GE_ERR_ARG and "not a row of the index" in str(e.value)
    for k, nprobe in ((0, 1), (129, 1), (1, 0), (1, 5)):
        with pytest.raises(capi.GeError) as e:
            ivf.query_rows([0], k, nprobe)
        assert e.value.status == capi.GE_ERR_ARG
    Z = X[:5].copy(); Z[2, 3] = np.nan
    with pytest.raises(capi.GeError) as e:
        ivf.query_vectors(Z, 3, 1)
    assert e.value.status == capi.GE_ERR_ARG and "non-finite input" in str(e.value)

"""ge_match_* against the numpy model (tests/match_ref.py): a[], b[], score[], label[] and the summary are compared as bytes, with
no tolerance and no slot left out.  test_match_ref.py asserts, without a device, that every family used here has the structure
it is named for and that the general-float tables tell the fmaf chain from a correctly rounded dot product."""
import ctypes as C
import importlib.util
import os

import numpy as np
import pytest

from geglove import capi
import match_ref as M

pytestmark = pytest.mark.gpu


def _same(got, want, what):
    names = ("a", "b", "score", "label")
    dtypes = (np.int32, np.int32, np.float32, np.int32)
    assert got[4] == want[4], (what, got[4], want[4])
    for name, dt, g, w in zip(names, dtypes, got[:4], want[:4]):
        assert g.dtype == dt and g.shape == w.shape, (what, name, g.dtype, g.shape, w.shape)
        if g.tobytes() != w.tobytes():
            at = int(np.flatnonzero(g.view(np.uint32) != w.view(np.uint32))[0])
            raise AssertionError("%s: %s differs from the model in %d of %d entries; first at %d: got %r, want %r"
                                 % (what, name, int((g.view(np.uint32) != w.view(np.uint32)).sum()), g.size, at, g[at], w[at]))


@pytest.mark.parametrize("metric", M.METRICS)
@pytest.mark.parametrize("dim", M.TILE_DIMS)
@pytest.mark.parametrize("n", M.TILE_SIZES)
def test_tile_edges_on_general_floats(gpu, n, dim, metric):
    X, S, T, share = M.tile_case(dim, n, metric)
    assert M.SHARE[0] <= share <= M.SHARE[1], share
    want = M.match_scores(S, np.arange(n), T)
    assert want[4]["pairs"] == round(share * (n * (n - 1) // 2))
    m = capi.Matching.from_rows(X, metric=metric)
    _same(m.run(float(T), want[4]["pairs"] + 5), want, (n, dim, metric))
    assert m.found() == want[4]["pairs"]


def test_exactly_at_the_threshold(gpu):
    X, S, T = M.threshold_case()
    n = X.shape[0]
    m = capi.Matching.from_rows(X, metric="dot")
    want = M.match_scores(S, np.arange(n), T)
    got = m.run(float(T))
    _same(got, want, "at T")
    assert np.any(got[2] == T) and not np.any(got[2] == M.below(T))            # the pairs at T are in, the pairs one below are out
    lower = M.match_scores(S, np.arange(n), M.below(T))
    assert lower[4]["pairs"] > want[4]["pairs"]
    _same(m.run(float(M.below(T))), lower, "one ulp below T")


def test_extremes_nothing_and_everything(gpu):
    X, S, _, _ = M.tile_case(33, 300, "cosine")
    n = 300
    m = capi.Matching.from_rows(X)
    hi = np.nextafter(S.max(), np.float32(np.inf))
    got = m.run(float(hi))
    _same(got, M.match_scores(S, np.arange(n), hi), "above every score")
    assert got[0].size == 0 and np.array_equal(got[3], np.arange(n)) and got[4] == {"pairs": 0, "components": n, "groups": 0, "grouped_rows": 0, "largest": 1}
    lo = np.nextafter(S.min(), np.float32(-np.inf))
    got = m.run(float(lo), 44850)
    _same(got, M.match_scores(S, np.arange(n), lo), "below every score")
    assert got[4] == {"pairs": 44850, "components": 1, "groups": 1, "grouped_rows": n, "largest": n}


def test_two_million_pairs_fill_the_cap_exactly(gpu):
    n, dim = 2000, 8
    X = M.NR.random_rows(4242, n, dim)
    _, S = M.scores(X, "dot")
    lo = np.nextafter(S.min(), np.float32(-np.inf))
    want = M.match_scores(S, np.arange(n), lo)
    assert want[4]["pairs"] == 1999000
    m = capi.Matching.from_rows(X, metric="dot")
    _same(m.run(float(lo), 1999000), want, "2000 rows, every pair")
    prepare_ms, join_ms, sort_ms, components_ms = m.kernel_ms()
    assert prepare_ms > 0 and join_ms > 0 and sort_ms > 0 and components_ms > 0


def test_overflow_reports_the_exact_count_and_the_handle_recovers(gpu):
    X, S, T, _ = M.tile_case(200, 300, "cosine")
    want = M.match_scores(S, np.arange(300), T)
    count = want[4]["pairs"]
    m = capi.Matching.from_rows(X)
    with pytest.raises(capi.GeError) as e:
        m.run(float(T), count - 1)
    assert e.value.status == capi.GE_ERR_OVERFLOW and ("%d pairs" % count) in str(e.value) and "max_pairs" in str(e.value)
    assert m.found() == count
    L = capi.lib()
    a, label, summary = C.POINTER(C.c_int32)(), C.POINTER(C.c_int32)(), capi.MatchSummary()
    assert L.ge_match_get(m._h, None, None, C.byref(a), None, None, C.byref(label), C.byref(summary)) == capi.GE_OK
    assert not a and not label and (summary.pairs, summary.components, summary.groups) == (count, 0, 0)      # no pairs and no groups are held
    _same(m.run(float(T), count), want, "after the overflow")
    # far past the cap: the counter keeps counting
    lo = np.nextafter(S.min(), np.float32(-np.inf))
    with pytest.raises(capi.GeError) as e:
        m.run(float(lo), 1)
    assert e.value.status == capi.GE_ERR_OVERFLOW and m.found() == 44850
    _same(m.run(float(T), count), want, "after the second overflow")


def test_components_path(gpu):
    X, S, perm = M.path_case()
    want = M.match_scores(S, np.arange(511), 1.0)
    got = capi.Matching.from_rows(X, metric="dot").run(1.0)
    _same(got, want, "path")
    assert got[4] == {"pairs": 510, "components": 1, "groups": 1, "grouped_rows": 511, "largest": 511} and np.all(got[3] == 0)


def test_components_star_joined_paths_isolated_rows_and_a_cutting_subset(gpu):
    X, S, perm, edges, _ = M.forest_case()
    n = X.shape[0]
    want = M.match_scores(S, np.arange(n), 1.0)
    got = capi.Matching.from_rows(X, metric="dot").run(1.0)
    _same(got, want, "forest")
    assert got[4] == {"pairs": 399, "components": 32, "groups": 2, "grouped_rows": 401, "largest": 300}
    subset = np.setdiff1d(np.arange(n), [perm[40]]).astype(np.int32)
    want = M.match_scores(S[np.ix_(subset, subset)], subset, 1.0)
    got = capi.Matching.from_rows(X, subset=subset, metric="dot").run(1.0)
    _same(got, want, "forest without one path vertex")
    assert got[4]["groups"] == 3 and got[3].size == n - 1
    # the same rows under cosine, general floats, with a subset: original ids come back
    Xt, St, T, _ = M.tile_case(32, 193, "cosine")
    keep = np.arange(1, 193, 3, dtype=np.int32)
    _same(capi.Matching.from_rows(Xt, subset=keep).run(float(T)), M.match_scores(St[np.ix_(keep, keep)], keep, T), "subset, cosine")


def _hip_runtime():
    """The HIP runtime the library uses: the copy capi maps first where torch is installed, else the system's."""
    capi.lib()
    spec = importlib.util.find_spec("torch")
    path = os.path.join(os.path.dirname(spec.origin), "lib", "libamdhip64.so") if spec is not None and spec.origin else ""
    return C.CDLL(path if os.path.exists(path) else "libamdhip64.so")


def test_same_bytes_twice_and_on_two_streams(gpu):
    X, S, T, _ = M.tile_case(200, 300, "dot")
    want = M.match_scores(S, np.arange(300), T)
    m = capi.Matching.from_rows(X, metric="dot")
    first, second = m.run(float(T)), m.run(float(T))
    _same(first, want, "first run")
    _same(second, want, "second run")
    hip = _hip_runtime()
    streams = [C.c_void_p(), C.c_void_p()]
    for s in streams:
        assert hip.hipStreamCreate(C.byref(s)) == 0 and s.value
    handles = [capi.Matching.from_rows(X, metric="dot", stream=s) for s in streams]
    for h in handles:
        _same(h.run(float(T)), want, "on a stream of its own")
    for h in handles:
        h.close()
    for s in streams:
        assert hip.hipStreamDestroy(s) == 0


def test_non_finite_rows_are_refused(gpu):
    X = M.NR.random_rows(9, 200, 6)
    for bad in (np.nan, np.inf, -np.inf):
        Z = X.copy(); Z[123, 4] = bad
        with pytest.raises(capi.GeError) as e:
            capi.Matching.from_rows(Z)
        assert e.value.status == capi.GE_ERR_ARG and "non-finite input" in str(e.value)
    # one row matches nothing and labels itself
    got = capi.Matching.from_rows(X[:1]).run(0.0)
    assert got[0].size == 0 and got[3].tolist() == [0] and got[4] == {"pairs": 0, "components": 1, "groups": 0, "grouped_rows": 0, "largest": 1}


def test_trainer_handle_entry_point_equals_the_host_rows_one(gpu):
    import geglove
    from geglove import synth
    from helpers import make_config
    V, N, dim = 1500, 20000, 24
    I, J, Xc, xmax = synth.synthetic_coo(V, N, seed=77)
    cfg = make_config(dim, method="pglove", mode="hogwild", shuffle="device", dtype="f32", seed=5)
    opt = geglove.Adagrad(geglove.CooMatrix(V, I, J, Xc, xmax), cfg, cfg.costFunction())
    for it in range(3):
        opt.epoch(it)
    before = opt.state()
    rows = opt.extractResultF32().reshape(V, dim)
    keep = np.arange(1, V, 3, dtype=np.int32)
    for subset in (None, keep):
        for metric in ("cosine", "dot"):
            on_rows = capi.Matching.from_rows(rows, subset=subset, metric=metric)
            on_handle = capi.Matching.from_glove(opt._h, subset=subset, metric=metric)
            ids = np.arange(V) if subset is None else keep
            _, S = M.scores(rows[ids], metric)
            p, q = np.triu_indices(ids.size, 1)
            T = np.sort(S[p, q])[-2000]                                         # about two thousand pairs
            want = M.match_scores(S, ids, T)
            got_rows, got_handle = on_rows.run(float(T)), on_handle.run(float(T))
            _same(got_rows, want, ("rows", metric))
            _same(got_handle, want, ("handle", metric))
    after = opt.state()
    for name in before:
        assert before[name].tobytes() == after[name].tobytes(), name           # no trainer table is written
    assert rows.tobytes() == opt.extractResultF32().tobytes()
    opt.close()

"""ge_align_* against the model (tests/align_ref.py): the candidates, target_of[], target_score[], flags[], source_of[] and the
summary are compared as bytes, with no tolerance and no slot left out.  test_align_ref.py asserts, without a device, that every
family used here has the structure it is named for, that the model's two assignments agree, and that the general-float tables
tell the fmaf chain from a correctly rounded dot product."""
import ctypes as C

import numpy as np
import pytest

from geglove import capi
import align_ref as A
import match_ref as M
from test_match_gpu import _hip_runtime

pytestmark = pytest.mark.gpu
NAMES = ("a", "b", "score", "target_of", "target_score", "flags", "source_of")
DTYPES = (np.int32, np.int32, np.float32, np.int32, np.float32, np.uint8, np.int32)


def _same(got, want, what):
    assert got[7] == want[7], (what, got[7], want[7])
    for name, dt, g, w in zip(NAMES, DTYPES, got[:7], want[:7]):
        assert g.dtype == dt and w.dtype == dt and g.shape == w.shape, (what, name, g.dtype, w.dtype, g.shape, w.shape)
        if g.tobytes() != w.tobytes():
            raw = np.uint8 if dt == np.uint8 else np.uint32
            differ = np.flatnonzero(g.view(raw) != w.view(raw))
            at = int(differ[0])
            raise AssertionError("%s: %s differs from the model in %d of %d entries; first at %d: got %r, want %r"
                                 % (what, name, differ.size, g.size, at, g[at], w[at]))


@pytest.mark.parametrize("metric", A.METRICS)
@pytest.mark.parametrize("shape", A.TILE_SHAPES)
def test_tile_edges_on_general_floats(gpu, shape, metric):
    nA, nB, dim = shape
    X, source, target, S, T, share = A.tile_case(nA, nB, dim, metric)
    assert A.SHARE[0] <= share <= A.SHARE[1], share
    want = A.align_scores(S, source, target, T)
    al = capi.Alignment.from_rows(X, source, target, metric=metric)
    _same(al.run(float(T), want[7]["candidates"] + 5), want, (shape, metric))
    assert al.found() == want[7]["candidates"] == round(share * nA * nB)


def test_exactly_at_the_threshold(gpu):
    X, source, target, S, T = A.threshold_case()
    al = capi.Alignment.from_rows(X, source, target, metric="dot")
    want = A.align_scores(S, source, target, T)
    got = al.run(float(T))
    _same(got, want, "at T")
    assert np.any(got[2] == T) and not np.any(got[2] == M.below(T))            # the pairs at T are in, the pairs one below are out
    lower = A.align_scores(S, source, target, M.below(T))
    assert lower[7]["candidates"] > want[7]["candidates"]
    _same(al.run(float(M.below(T))), lower, "one ulp below T")


def test_all_ties_pair_in_id_order(gpu):
    X, source, target, S, T = A.ties_case()
    want = A.align_scores(S, source, target, T)
    al = capi.Alignment.from_rows(X, source, target, metric="dot")
    got = al.run(float(T))
    _same(got, want, "ties")
    assert np.array_equal(got[3], 64 + np.arange(64)) and got[7]["assigned"] == 64 and got[7]["mutual"] == 1
    assert al.kernel_ms()[4] >= 1                                              # a diagnostic: the model's 64 rounds are not held against it


def test_weighted_chain_of_three_hundred_rounds(gpu):
    X, source, target, S, T, _ = A.chain_case()
    want = A.align_scores(S, source, target, T)
    al = capi.Alignment.from_rows(X, source, target, metric="dot")
    got = al.run(float(T))
    _same(got, want, "chain")
    assert got[7]["assigned"] == 300 and got[7]["mutual"] == 1
    prepare_ms, join_ms, sort_ms, assign_ms, rounds = al.kernel_ms()
    assert prepare_ms > 0 and join_ms > 0 and sort_ms > 0 and assign_ms > 0 and rounds >= 1


def test_star_one_source_gets_the_hub(gpu):
    X, source, target, S, T, perm = A.star_case()
    want = A.align_scores(S, source, target, T)
    got = capi.Alignment.from_rows(X, source, target, metric="dot").run(float(T))
    _same(got, want, "star")
    assert got[7]["assigned"] == 41 and int((got[3] == perm[300]).sum()) == 1 and np.all(got[6] >= 0)


def test_extremes_nothing_and_everything(gpu):
    X, source, target, S, _, _ = A.tile_case(65, 129, 33, "cosine")
    al = capi.Alignment.from_rows(X, source, target)
    hi = np.nextafter(S.max(), np.float32(np.inf))
    got = al.run(float(hi))
    _same(got, A.align_scores(S, source, target, hi), "above every score")
    assert got[0].size == 0 and np.all(got[3] == -1) and np.all(got[6] == -1) and got[7]["candidates"] == got[7]["assigned"] == 0
    lo = np.nextafter(S.min(), np.float32(-np.inf))
    got = al.run(float(lo), 65 * 129)
    _same(got, A.align_scores(S, source, target, lo), "below every score")
    assert got[7]["candidates"] == 65 * 129 and got[7]["assigned"] == 65


@pytest.mark.parametrize("metric", A.METRICS)
def test_candidates_are_the_matching_pairs_across_the_two_sets(gpu, metric):
    X, source, target, S, T, _ = A.tile_case(193, 300, 200, metric)
    a, b, s = capi.Alignment.from_rows(X, source, target, metric=metric).run(float(T))[:3]
    ma, mb, ms, _, _ = capi.Matching.from_rows(X, metric=metric).run(float(T))
    is_source = np.zeros(X.shape[0], bool)
    is_source[source] = True
    cross = is_source[ma] != is_source[mb]
    ua = np.where(is_source[ma], ma, mb)[cross]                                # the pair as (source, target)
    ub = np.where(is_source[ma], mb, ma)[cross]
    us = ms[cross]
    at = np.lexsort((ub, ua))
    assert a.size == int(cross.sum()) > 0
    assert a.tobytes() == ua[at].astype(np.int32).tobytes() and b.tobytes() == ub[at].astype(np.int32).tobytes() and s.tobytes() == us[at].tobytes()


@pytest.mark.parametrize("metric", A.METRICS)
def test_mutual_pairs_are_each_others_nearest_neighbours(gpu, metric):
    X, source, target, S, _, _ = A.tile_case(129, 65, 31, metric)
    lo = np.nextafter(S.min(), np.float32(-np.inf))
    got = capi.Alignment.from_rows(X, source, target, metric=metric).run(float(lo))
    to_target = capi.Neighbors.create(X, subset=target, metric=metric).query_vectors(X[source], 1)[0][:, 0]
    to_source = capi.Neighbors.create(X, subset=source, metric=metric).query_vectors(X[target], 1)[0][:, 0]
    back = dict(zip(target.tolist(), to_source.tolist()))
    want = [(int(x), int(y)) for x, y in zip(source, to_target) if back[int(y)] == int(x)]
    mutual = got[5] & 2 != 0
    assert len(want) >= 1 and list(zip(source[mutual].tolist(), got[3][mutual].tolist())) == want
    assert np.all(got[5][mutual] & 1)


def test_overflow_reports_the_exact_count_and_the_handle_recovers(gpu):
    X, source, target, S, T, _ = A.tile_case(193, 300, 200, "cosine")
    want = A.align_scores(S, source, target, T)
    count = want[7]["candidates"]
    al = capi.Alignment.from_rows(X, source, target)
    with pytest.raises(capi.GeError) as e:
        al.run(float(T), count - 1)
    assert e.value.status == capi.GE_ERR_OVERFLOW and ("%d candidates" % count) in str(e.value) and "max_pairs" in str(e.value)
    assert al.found() == count
    L = capi.lib()
    a, target_of, flags, source_of, summary = C.POINTER(C.c_int32)(), C.POINTER(C.c_int32)(), C.POINTER(C.c_uint8)(), C.POINTER(C.c_int32)(), capi.AlignSummary()
    assert L.ge_align_get(al._h, None, None, None, C.byref(a), None, None, C.byref(target_of), None, C.byref(flags), C.byref(source_of),
                          C.byref(summary)) == capi.GE_OK
    assert not a and not target_of and not flags and not source_of                                             # nothing is held
    assert [getattr(summary, k) for k, _ in capi.AlignSummary._fields_] == [count, 0, 0, 0, 0, 0]
    _same(al.run(float(T), count), want, "after the overflow: exactly max_pairs is none")
    # far past the cap: the counter keeps counting
    lo = np.nextafter(S.min(), np.float32(-np.inf))
    with pytest.raises(capi.GeError) as e:
        al.run(float(lo), 1)
    assert e.value.status == capi.GE_ERR_OVERFLOW and al.found() == 193 * 300
    _same(al.run(float(T), count), want, "after the second overflow")


def test_same_bytes_twice_and_on_two_streams(gpu):
    X, source, target, S, T, _ = A.tile_case(193, 300, 200, "dot")
    want = A.align_scores(S, source, target, T)
    al = capi.Alignment.from_rows(X, source, target, metric="dot")
    first, second = al.run(float(T)), al.run(float(T))
    _same(first, want, "first run")
    _same(second, want, "second run")
    hip = _hip_runtime()
    streams = [C.c_void_p(), C.c_void_p()]
    for s in streams:
        assert hip.hipStreamCreate(C.byref(s)) == 0 and s.value
    handles = [capi.Alignment.from_rows(X, source, target, metric="dot", stream=s) for s in streams]
    for h in handles:
        _same(h.run(float(T)), want, "on a stream of its own")
    for h in handles:
        h.close()
    for s in streams:
        assert hip.hipStreamDestroy(s) == 0


def test_non_finite_rows_and_overlapping_sets_are_refused(gpu):
    X = M.NR.random_rows(9, 200, 6)
    source, target = np.arange(0, 200, 2, dtype=np.int32), np.arange(1, 200, 2, dtype=np.int32)
    for bad in (np.nan, np.inf, -np.inf):
        for row in (122, 123):                                                 # once in each set
            Z = X.copy(); Z[row, 4] = bad
            with pytest.raises(capi.GeError) as e:
                capi.Alignment.from_rows(Z, source, target)
            assert e.value.status == capi.GE_ERR_ARG and "non-finite input" in str(e.value)
    Z = X.copy(); Z[5, 1] = np.nan                                             # a row of neither set is never read
    capi.Alignment.from_rows(Z, source[3:], target[3:]).run(0.5)
    with pytest.raises(capi.GeError) as e:
        capi.Alignment.from_rows(X, source, np.sort(np.append(target, 10)).astype(np.int32))
    assert e.value.status == capi.GE_ERR_ARG and "the source and target sets share row 10" in str(e.value)
    # one row on each side
    got = capi.Alignment.from_rows(X, [7], [3], metric="dot").run(-3.0e38)
    assert got[0].tolist() == [7] and got[1].tolist() == [3] and got[3].tolist() == [3] and got[6].tolist() == [7] and got[5].tolist() == [3]


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
    source, target = np.arange(1, V, 3, dtype=np.int32), np.arange(2, V, 3, dtype=np.int32)
    for metric in ("cosine", "dot"):
        on_rows = capi.Alignment.from_rows(rows, source, target, metric=metric)
        on_handle = capi.Alignment.from_glove(opt._h, source, target, metric=metric)
        S = A.scores(rows, source, target, metric)
        T = np.sort(S.ravel())[-2000]                                          # about two thousand candidates
        want = A.align_scores(S, source, target, T)
        _same(on_rows.run(float(T)), want, ("rows", metric))
        _same(on_handle.run(float(T)), want, ("handle", metric))
    after = opt.state()
    for name in before:
        assert before[name].tobytes() == after[name].tobytes(), name           # no trainer table is written
    assert rows.tobytes() == opt.extractResultF32().tobytes()
    opt.close()

"""CPU-only checks of the prediction section of include/geglove.h: the exported symbols, the argument errors that need no
device, the `device.predict` key of the C++ host's bean, and the numpy yardstick (tests/predict_ref.py) against a brute-force
double loop and against the ranking yardstick."""
import ctypes as C
import os
import re

import numpy as np

from geglove import capi
import predict_ref as P
import rank_ref as R

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
i32p, i64p, f32p = C.POINTER(C.c_int32), C.POINTER(C.c_int64), C.POINTER(C.c_float)


def test_header_symbols_are_exported():
    header = open(os.path.join(REPO, "include", "geglove.h")).read()
    declared = set(re.findall(r"\b(ge_glove_predict_\w+|ge_predict_\w+)\s*\(", header))
    assert declared == {"ge_glove_predict_create", "ge_glove_predict_run", "ge_predict_last_kernel_ms", "ge_predict_get", "ge_predict_destroy"}
    L = capi.lib()
    for name in declared:
        assert name in capi.SYMBOLS and getattr(L, name) is not None


def _create(h, I, n, ptr, idx, subset=None, n_subset=0, exclude_self=0, out=True):
    L = capi.lib()
    arr = lambda a, t: None if a is None else np.asarray(a, t)
    I, ptr, idx, subset = arr(I, np.int32), arr(ptr, np.int64), arr(idx, np.int32), arr(subset, np.int32)
    p = lambda a, t: None if a is None else a.ctypes.data_as(t)
    r = C.c_void_p()
    st = L.ge_glove_predict_create(h, p(I, i32p), n, p(ptr, i64p), p(idx, i32p), p(subset, i32p), n_subset, exclude_self, C.byref(r) if out else None)
    assert r.value is None
    return st, L.ge_last_error().decode()


def test_limits_are_refused_without_a_device():
    """Everything that needs no handle is checked before the handle is looked at, so a null handle reaches each message."""
    ARG = capi.GE_ERR_ARG
    I = [0, 1, 2]
    ptr, idx = [0, 2, 2, 3], [0, 5, 1]
    sub = [0, 2, 5]
    # a well-formed set gets as far as the handle
    assert _create(None, I, 3, ptr, idx, sub, 3, 1) == (ARG, "null ge_glove handle")
    assert _create(None, I, 3, None, None) == (ARG, "null ge_glove handle")
    assert _create(None, I, 3, None, None, None, -7) == (ARG, "null ge_glove handle")        # n_subset is ignored without a subset
    # null arguments
    assert _create(None, I, 3, ptr, idx, out=False) == (ARG, "out is null")
    assert _create(None, None, 3, ptr, idx) == (ARG, "null query rows")
    assert _create(None, I, 3, ptr, None) == (ARG, "filter_idx is null")
    # n
    for n in (0, -1, 2 ** 31):
        st, msg = _create(None, I, n, None, None)
        assert st == ARG and "1 <= n < 2^31" in msg, (n, msg)
    # ids below zero
    st, msg = _create(None, [0, -1, 2], 3, ptr, idx)
    assert st == ARG and "query 1: focus row -1 out of range" in msg
    st, msg = _create(None, I, 3, ptr, [-1, 5, 1])
    assert st == ARG and "query 0: filter id -1 out of range" in msg
    # a descending and a repeated filter id
    for bad in ([5, 0, 1], [5, 5, 1]):
        st, msg = _create(None, I, 3, ptr, bad)
        assert st == ARG and "query 0: the filter list is not strictly ascending at entry 1" in msg, (bad, msg)
    # the offsets
    st, msg = _create(None, I, 3, [1, 2, 2, 3], idx)
    assert st == ARG and "filter_ptr[0] is 1, not 0" in msg
    st, msg = _create(None, I, 3, [0, 2, 1, 3], idx)
    assert st == ARG and "filter_ptr decreases at [2]" in msg
    # the subset: empty, an id below zero, descending, repeated
    for ns in (0, -1):
        st, msg = _create(None, I, 3, ptr, idx, sub, ns)
        assert st == ARG and "a subset of %d columns" % ns in msg, (ns, msg)
    st, msg = _create(None, I, 3, ptr, idx, [-2, 2, 5], 3)
    assert st == ARG and "subset[0] = -2 out of range" in msg
    for bad in ([0, 5, 2], [0, 2, 2]):
        st, msg = _create(None, I, 3, ptr, idx, bad, 3)
        assert st == ARG and "the subset is not strictly ascending at [2]" in msg, (bad, msg)
    # K at run, before the set is looked at
    L = capi.lib()
    for K in (0, -1, 129):
        assert L.ge_glove_predict_run(None, K, None, None, None) == ARG
        assert L.ge_last_error().decode() == "predict: K %d outside [1, 128]" % K
    # the other entry points
    assert L.ge_glove_predict_run(None, 10, None, None, None) == ARG and L.ge_last_error().decode() == "null ge_predict handle"
    assert L.ge_predict_last_kernel_ms(None, None, None, None) == ARG
    assert L.ge_predict_get(None, None, None, None, None) == ARG
    L.ge_predict_destroy(None)                                        # harmless


def test_host_configuration_key(tmp_path):
    """`device: { predict: K }` in the C++ host's bean: an integer 0 .. 128, 0 = off; one rank only; the banner gains its line
    only when the key is set."""
    capi._share_hip_runtime_with_torch()
    host = C.CDLL(os.path.join(REPO, "graph-embeddings_amd", "lib", "libgehost.so"))
    host.geh_config_summary.restype = C.c_char_p
    base = "graph: g.nt\nmethod: glove\ndim: 4\nbca:\n  alpha: 0.1\n  epsilon: 0.001\noutput:\n  uri: []\n"
    bad = "ERR\nInvalid configuration: Invalid device.predict, choose a number of links to predict per vertex from 1 to 128 (0 = off)"
    ranks = "ERR\nInvalid configuration: device.predict runs on one rank only, set device.gpus: 1"
    line = lambda k: "# Predict: the %d best missing links of every kept vertex, known nonzeros filtered" % k
    cases = {"": (None, None), "device:\n  predict: 0\n": (None, None), "device:\n  predict: 1\n": (None, line(1)),
             "device:\n  predict: 128\n": (None, line(128)), "device:\n  holdout: 0.2\n  predict: 10\n": (None, line(10)),
             "device:\n  predict: 129\n": (bad, None), "device:\n  predict: -1\n": (bad, None), "device:\n  predict: 1.5\n": (bad, None),
             "device:\n  predict: many\n": (bad, None), "device:\n  predict: 99999999999\n": (bad, None),
             "device:\n  predict: 5\n  gpus: 2\n": (ranks, None), "device:\n  predict: 0\n  gpus: 2\n": (None, None)}
    for i, (extra, (err, want)) in enumerate(cases.items()):
        p = tmp_path / ("c%d.yml" % i)
        p.write_text(base + extra)
        out = host.geh_config_summary(str(p).encode(), 1).decode()
        if err:
            assert out == err, (extra, out)
        else:
            assert out.startswith("OK\n") and ("# Predict" in out) == (want is not None) and (want is None or want in out.splitlines()), (extra, out)


Z7 = np.array([[1, 1, 1, 1, 1],
               [3, 2, 2, 5, 2],
               [0.0, -0.0, 0.0, -1, 0.0],
               [np.nan, 4, np.nan, -np.inf, 4],
               [2, 9, 9, 9, 1],
               [5, 4, 3, 2, 1],
               [1, 2, 3, 4, 5]], np.float64)
LISTS7 = [[], [1, 4], [0, 1, 2, 3, 4], [3, 4], [1], [0, 2, 4], [4]]


def test_the_yardstick_against_a_double_loop():
    """7 queries x 5 columns with ties, -0 beside +0, NaNs beside a real -inf, and filters: empty, every column, ending at V - 1;
    with and without a subset and the query's own column."""
    self_col = np.array([0, 3, 1, 1, 4, 2, 4])
    for K in (1, 3, 5, 7):
        for filters in (None, P.csr(LISTS7)):
            for subset in (None, [0, 2, 3], [4]):
                for own in (None, self_col):
                    index, score, count = P.topk(Z7, K, filters, subset, own)
                    assert index.dtype == np.int32 and score.dtype == np.float32 and count.dtype == np.int32
                    for k in range(7):
                        z = [(-np.inf if np.isnan(v) else v) for v in Z7[k]]
                        cand = [c for c in range(5) if (subset is None or c in subset) and (filters is None or c not in LISTS7[k])
                                and (own is None or c != own[k])]
                        order = []
                        while cand:                                        # selection by the definition: nobody precedes the pick
                            best = [c for c in cand if not any(z[d] > z[c] or (z[d] == z[c] and d < c) for d in cand if d != c)]
                            assert len(best) == 1
                            order.append(best[0]); cand.remove(best[0])
                        order = order[:K]
                        assert count[k] == len(order) and index[k, :len(order)].tolist() == order, (K, k, subset, index[k], order)
                        assert score[k, :len(order)].tolist() == [np.float32(z[c]) for c in order]
                        assert np.all(index[k, len(order):] == -1) and np.all(np.isneginf(score[k, len(order):]))
    index, score, count = P.topk(Z7, 3, P.csr(LISTS7))
    assert index.tolist() == [[0, 1, 2], [3, 0, 2], [-1, -1, -1], [1, 0, 2], [2, 3, 0], [1, 3, -1], [3, 2, 1]] and count.tolist() == [3, 3, 0, 3, 3, 2, 3]
    assert np.isneginf(score[3, 1:]).all() and score[3, 0] == 4                    # NaN columns 0 and 2 come before the fill, as -inf


def test_the_yardstick_agrees_with_the_ranking_yardstick():
    """The t-th prediction of a query has rank t + 1 under the same filter: the two numpy models state one order."""
    n, V, K = 40, 60, 17
    F, Cx, fb, cb = P.integer_tables(5, V, 8)
    I = (np.arange(n) * 7 % V).astype(np.int32)
    Z = R.scores(F, Cx, cb, I)
    lists = [np.flatnonzero((np.arange(V) * 3 + k) % 5 == 0) for k in range(n)]
    index, _, count = P.topk(Z, K, P.csr(lists), None, I)
    assert np.all(count == K)
    with_self = P.csr([np.union1d(l, [i]) for l, i in zip(lists, I)])
    for t in range(K):
        assert np.all(R.ranks(Z, index[:, t], with_self) == t + 1), t


def test_decided_slots_of_the_yardstick():
    """Three columns far apart and two within each other's bound: the pair's two slots are undecided, the others decided."""
    t = np.array([[5.0, 1.0, 1.0 + 1e-9, -3.0, 9.0]])
    E = np.full((1, 5), 1e-6)
    keep = np.ones((1, 5), bool)
    model, ok = P.decided(t, E, keep, 5)
    assert model.tolist() == [[4, 0, 2, 1, 3]] and ok.tolist() == [[True, True, False, False, True]]
    keep[0, 2] = False
    model, ok = P.decided(t, E, keep, 5)
    assert model.tolist() == [[4, 0, 1, 3, -1]] and ok.all()
    # a result that swaps the undecided pair passes, one that swaps a decided pair does not
    keep[0, 2] = True
    model, ok = P.decided(t, E, keep, 4)
    good = (np.array([[4, 0, 1, 2]], np.int32), np.array([[9, 5, 1, 1]], np.float32), np.array([4], np.int32))
    P.check_within_bound(*good, t, E, keep, model, ok)
    wrong = (np.array([[0, 4, 1, 2]], np.int32), np.array([[5, 9, 1, 1]], np.float32), np.array([4], np.int32))
    try:
        P.check_within_bound(*wrong, t, E, keep, model, ok)
    except AssertionError:
        pass
    else:
        raise AssertionError("a provably wrong order passed")

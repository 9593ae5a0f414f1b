"""k_similarity (csrc/similarity.hip) on the designed label families of tests/sim_ref.py, through the C ABI: vertex ids,
string positions and job ranges are set independently.  The reference is the oracle's double similarity of every pair
(one table per family and method, computed once), filtered in double at each threshold, in job order.  Every comparison
is on positions and on the float's bits.  tests/test_sim_designed.py shows that the families hold what they are for."""
import ctypes as C

import numpy as np
import pytest

import oracle as O
import sim_ref as R
from geglove import capi

pytestmark = pytest.mark.gpu

_TABLES = {}


def _ptr(a, ct):
    return a.ctypes.data_as(C.POINTER(ct))


def run(labels, method, source, target, source_vertex=None, target_vertex=None, upper=False, threshold=0.0, ngram=3,
        smooth=1.0, distance=0.0, job_range=None):
    """ge_similarity_pairs -> (i, j, float32 similarity); vertices default to the string positions."""
    key = id(labels)
    if key not in _TABLES or _TABLES[key][0] is not labels:
        _TABLES[key] = (labels,) + O.string_table(labels)
    _, off, units = _TABLES[key]
    L = capi.lib()
    table = capi.Strings(len(labels), _ptr(off, C.c_int64), _ptr(units, C.c_uint16))
    sp = np.ascontiguousarray(source, dtype=np.int32); tp = np.ascontiguousarray(target, dtype=np.int32)
    sv = np.ascontiguousarray(source if source_vertex is None else source_vertex, dtype=np.int32)
    tv = np.ascontiguousarray(target if target_vertex is None else target_vertex, dtype=np.int32)
    cfg = capi.SimCfg(); L.ge_sim_cfg_default(C.byref(cfg))
    cfg.method = O.SIM_METHODS.index(method); cfg.threshold = threshold; cfg.ngram = ngram; cfg.smooth = smooth; cfg.distance = distance
    cfg.upper_triangle = int(upper)
    if job_range is not None:
        cfg.job_begin, cfg.job_end = job_range
    h = C.c_void_p()
    status = L.ge_similarity_pairs(C.byref(table), _ptr(sp, C.c_int32), _ptr(sv, C.c_int32), len(sp), _ptr(tp, C.c_int32), _ptr(tv, C.c_int32),
                                   len(tp), C.byref(cfg), C.byref(h))
    assert status == capi.GE_OK, L.ge_last_error().decode()
    try:
        n = C.c_int64(-1); pi = C.POINTER(C.c_int32)(); pj = C.POINTER(C.c_int32)(); ps = C.POINTER(C.c_float)()
        assert L.ge_sim_pairs_get(h, C.byref(n), C.byref(pi), C.byref(pj), C.byref(ps)) == capi.GE_OK
        k = n.value
        if k == 0:
            return np.zeros(0, np.int32), np.zeros(0, np.int32), np.zeros(0, np.float32)
        return np.ctypeslib.as_array(pi, (k,)).copy(), np.ctypeslib.as_array(pj, (k,)).copy(), np.ctypeslib.as_array(ps, (k,)).copy()
    finally:
        L.ge_sim_pairs_destroy(h)


def assert_same(ref, got, what=""):
    np.testing.assert_array_equal(got[0], ref[0], err_msg=what + " source positions")
    np.testing.assert_array_equal(got[1], ref[1], err_msg=what + " target positions")
    np.testing.assert_array_equal(got[2].view(np.uint32), ref[2].view(np.uint32), err_msg=what + " similarities (bits)")


def check(tab, method, ngram, threshold, form, src, tgt, upper):
    exp = R.expected(tab, threshold, src, tgt, upper=upper)
    got = run(tab.labels, method, src, tgt, upper=upper, threshold=threshold, ngram=ngram)
    assert_same(exp, got, "%s %s at %r" % (method, form, threshold))
    return got


CASES = ([("jw_sparse%d" % L, "jarowinkler", 3) for L in R.LENGTH_CLASSES] + [("jw_gate", "jarowinkler", 3)]
         + [("lev_edges%d" % L, "levenshtein", 3) for L in R.LENGTH_CLASSES] + [("jw_sparse%d" % L, "levenshtein", 3) for L in R.LENGTH_CLASSES]
         + [("profile_edges", m, k) for m in ("ngram_cosine", "ngram_jaccard") for k in (1, 2, 3, 4)]
         + [("profile_edges", "token_cosine", 3), ("profile_edges", "token_jaccard", 3)])


@pytest.mark.parametrize("name,method,ngram", CASES)
def test_every_pair_of_every_family(gpu, name, method, ngram):
    """Thresholds 0 and -1 keep every pair the reference keeps; a NaN (two empty profiles) is kept by neither."""
    tab = R.table(name, method, ngram)
    for threshold in (0.0, -1.0):
        for form, src, tgt, upper in R.splits(len(tab.labels)):
            got = check(tab, method, ngram, threshold, form, src, tgt, upper)
            assert not np.isnan(got[2]).any()
            if form == "square":
                nan = int(np.isnan(tab.sim[tab.have & np.triu(np.ones_like(tab.have), 1)]).sum())
                assert len(got[0]) == len(src) * (len(src) - 1) // 2 - nan


@pytest.mark.parametrize("name,method,ngram", CASES)
def test_thresholds_on_attained_values(gpu, name, method, ngram):
    """Each threshold is a similarity some pair attains, and its two neighbouring doubles: v keeps that pair, the double
    above drops it.  Then 1, the double above 1, and 1.5."""
    tab = R.table(name, method, ngram)
    values = R.attained(tab, 8)
    assert len(values) >= 8 and len(set(values)) == len(values)
    # one lane walks one pair: a run over 1 024-unit labels takes 0.14 s, so that class keeps to the square form here
    forms = R.splits(len(tab.labels))[:1 if name.endswith("1024") else 2]
    for v in values:
        for form, src, tgt, upper in forms:
            at = check(tab, method, ngram, v, form, src, tgt, upper)
            above = check(tab, method, ngram, float(np.nextafter(v, 2)), form, src, tgt, upper)
            check(tab, method, ngram, float(np.nextafter(v, 0)), form, src, tgt, upper)
            if form == "square":
                assert set(zip(at[0], at[1])) - set(zip(above[0], above[1])), "no pair sits on %r" % v
    for threshold in (1.0, float(np.nextafter(1.0, 2)), 1.5):
        for form, src, tgt, upper in forms:
            check(tab, method, ngram, threshold, form, src, tgt, upper)


def test_jaro_winkler_thresholds_on_the_length_bound(gpu):
    """Every prefix pair of jw_gate attains the most its lengths allow, so a threshold on its value sits on the prune."""
    tab = R.table("jw_gate", "jarowinkler"); info = R.jw_gate_info()
    n = len(tab.labels); everyone = list(range(n))
    values = sorted({float(tab.sim[i, j]) for i, j in info["prefix"]} | {float(tab.sim[j, i]) for i, j in info["prefix"]})
    assert len(values) > 250
    for v in values:
        at = check(tab, "jarowinkler", 3, v, "square", everyone, everyone, True)
        above = check(tab, "jarowinkler", 3, float(np.nextafter(v, 2)), "square", everyone, everyone, True)
        assert len(at[0]) > len(above[0])
    # the other order of every pair: sources are the longer labels
    back = everyone[::-1]
    for v in values[::8]:
        exp = R.expected(tab, v, back, back, upper=True)
        assert_same(exp, run(tab.labels, "jarowinkler", back, back, upper=True, threshold=v), "reversed at %r" % v)


def give_up(threshold, m):
    lim = (1.0 - threshold) * m
    return m if lim >= m else 0 if lim < 0 else int(lim) + 1


@pytest.mark.parametrize("L", R.LENGTH_CLASSES)
def test_levenshtein_thresholds_one_minus_d_over_m(gpu, L):
    """threshold = 1 - d/m as a double, for the designed (m, d): the distance budget (1 - threshold) * m then lies on d or
    just below it ((1 - 0.9) * 10 < 1), and the group holds partners whose length difference is the budget and its
    neighbours."""
    name = "lev_edges%d" % L
    tab = R.table(name, "levenshtein"); cases = R.lev_edges_cases(L)
    md = {(m, d) for m, d, _, _, place in cases if place != "cut"} if L == 64 else {(L, d) for d in (0, 1, L // 2, L - 1, L)}
    assert len(md) >= (20 if L == 64 else 5) and all(m <= 64 or m == L for m, _ in md)
    if L == 64:
        assert (10, 1) in md and any((1.0 - (1.0 - d / m)) * m < d for m, d in md)
    cuts = {}
    for m, k, _, _, place in cases:
        if place == "cut":
            cuts.setdefault(m, {0}).add(k)
    n = len(tab.labels)
    for m, d in sorted(md):
        threshold = 1.0 - d / m
        g = give_up(threshold, m)
        assert {k for k in (g - 1, g, g + 1) if 0 <= k <= m} <= cuts[m], (m, d, g)
        for form, src, tgt, upper in R.splits(n):
            got = check(tab, "levenshtein", 3, threshold, "%s m=%d d=%d" % (form, m, d), src, tgt, upper)
            if form == "square":                                                # the designed pairs sit on the threshold
                kept = set(zip(got[0], got[1]))
                assert all((min(b, p), max(b, p)) in kept for m_, d_, b, p, _ in cases if (m_, d_) == (m, d))


def short_labels(n):
    return ["n%03d" % (k * 7 % 1000) for k in range(n)]


@pytest.mark.parametrize("n", [255, 256, 257, 513])
def test_square_groups_around_the_tile_size(gpu, n):
    labels = short_labels(n); everyone = list(range(n))
    ref = O.compare_group(O.sim_cfg("jarowinkler", 0.0), labels, everyone, everyone, upper_triangle=True)
    got = run(labels, "jarowinkler", everyone, everyone, upper=True, threshold=0.0)
    want = [(i, j) for i in range(n) for j in range(i + 1, n)]
    assert list(zip(got[0], got[1])) == want                                   # every (i, j > i) once, in job order
    assert_same(ref, got)
    for i in (r for r in (254, 255, 256, 511, 512) if r < n):                    # one row of tiles at a time
        row = run(labels, "jarowinkler", everyone, everyone, upper=True, threshold=0.0, job_range=(i, i + 1))
        keep = ref[0] == i
        assert keep.sum() == n - 1 - i
        assert_same(tuple(a[keep] for a in ref), row, "row %d" % i)


@pytest.mark.parametrize("n", [257, 513])
def test_own_vertex_at_tile_edges(gpu, n):
    labels = short_labels(n + 3)
    src = [n, n + 1, n + 2]; sv = [9000, 9001, 9002]
    tgt = list(range(n)); tv = list(range(n))
    for pos in (0, 255, 256, n - 1):
        tv[pos] = 9000
    tv[1] = tv[254] = 9001
    ref = O.compare_group(O.sim_cfg("jarowinkler", 0.0), labels, src, tgt, sv, tv)
    got = run(labels, "jarowinkler", src, tgt, sv, tv, threshold=0.0)
    assert len(ref[0]) == 3 * n - len({0, 255, 256, n - 1}) - 2                 # at 257 the last target is 256
    assert not {(0, 0), (0, 255), (0, 256), (0, n - 1), (1, 1), (1, 254)} & set(zip(got[0], got[1]))
    assert_same(ref, got)
    for pos in (0, 255, 256, n - 1):                                             # one at a time
        tv = list(range(n)); tv[pos] = 9002
        got = run(labels, "jarowinkler", src, tgt, sv, tv, threshold=0.0)
        assert_same(O.compare_group(O.sim_cfg("jarowinkler", 0.0), labels, src, tgt, sv, tv), got, "own vertex at %d" % pos)
        assert len(got[0]) == 3 * n - 1 and (2, pos) not in set(zip(got[0], got[1]))


@pytest.mark.parametrize("upper", [True, False])
def test_job_ranges_on_tile_edges(gpu, upper):
    n = 513
    labels = short_labels(n); everyone = list(range(n))
    ref = O.compare_group(O.sim_cfg("jarowinkler", 0.0), labels, everyone, everyone, upper_triangle=upper)
    got = run(labels, "jarowinkler", everyone, everyone, upper=upper, threshold=0.0, job_range=(255, 257))
    keep = (ref[0] >= 255) & (ref[0] < 257)
    assert keep.sum() == ((n - 256) + (n - 257) if upper else 2 * (n - 1))
    assert_same(tuple(a[keep] for a in ref), got)
    empty = run(labels, "jarowinkler", everyone, everyone, upper=upper, threshold=0.0, job_range=(256, 256))     # GE_OK, no pair
    assert len(empty[0]) == 0


def test_numeric_jobs_skip_their_own_vertex_before_they_can_die(gpu):
    for c in R.numeric_own_vertex():
        ref = O.compare_group(O.sim_cfg("numeric", **R.NUMERIC_CFG), c["labels"], c["source"], c["target"], c["source_vertex"],
                              c["target_vertex"], upper_triangle=c["upper"])
        got = run(c["labels"], "numeric", c["source"], c["target"], c["source_vertex"], c["target_vertex"], upper=c["upper"], **R.NUMERIC_CFG)
        assert list(zip(ref[0], ref[1])) == c["pairs"]
        assert_same(ref, got, c["name"])

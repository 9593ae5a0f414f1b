"""CPU-only checks of the clustering section of include/geglove.h: the exported symbols, the configuration struct, every limit
(an argument error with a message, before any device is touched), and the numpy yardstick (tests/kmeans_ref.py) against an
independent brute-force statement of itself."""
import ctypes as C
import math
import os
import re
import subprocess

import numpy as np
import pytest

from geglove import capi, synth
import kmeans_ref as R
import nn_ref

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32p, i32p = C.POINTER(C.c_float), C.POINTER(C.c_int32)


def _cfg(**kw):
    cfg = capi.KmeansCfg(); capi.lib().ge_kmeans_cfg_default(C.byref(cfg))
    cfg.k = 2
    for k, v in kw.items():
        setattr(cfg, k, v)
    return cfg


def test_header_symbols_are_exported():
    header = open(os.path.join(REPO, "include", "geglove.h")).read()
    declared = set(re.findall(r"\b(ge_(?:glove_)?kmeans_\w+)\s*\(", header))
    assert declared == {"ge_kmeans_cfg_default", "ge_kmeans_cfg_size", "ge_kmeans_create", "ge_glove_kmeans_create", "ge_kmeans_set_centroids",
                        "ge_kmeans_step", "ge_kmeans_run", "ge_kmeans_get", "ge_kmeans_last_kernel_ms", "ge_kmeans_destroy"}
    L = capi.lib()
    for name in declared:
        assert name in capi.SYMBOLS and getattr(L, name) is not None
    out = subprocess.check_output(["nm", "-D", "--defined-only", capi.LIB_PATH]).decode()
    assert declared <= set(re.findall(r" T (ge_[a-z0-9_]+)", out))
    assert re.search(r"enum \{ GE_KM_COSINE = 0, GE_KM_EUCLID = 1 \}", header) and (capi.GE_KM_COSINE, capi.GE_KM_EUCLID) == (0, 1)
    assert re.search(r"#define GE_KM_INIT_KEY 0x4B4D45414E53ull", header) and capi.GE_KM_INIT_KEY == R.INIT_KEY == 0x4B4D45414E53


def test_cfg_size_and_defaults(tmp_path):
    src = '#include <stdio.h>\n#include "geglove.h"\nint main(){printf("%zu", sizeof(ge_kmeans_cfg));return 0;}'
    exe = str(tmp_path / "probe_size_kmeans")
    subprocess.run(["gcc", "-x", "c", "-", "-I", os.path.join(REPO, "include"), "-o", exe], input=src.encode(), check=True)
    size = int(subprocess.check_output([exe]))
    assert size == C.sizeof(capi.KmeansCfg) == capi.lib().ge_kmeans_cfg_size() == 32
    assert [n for n, _ in capi.KmeansCfg._fields_] == ["metric", "k", "seed", "device", "stream"]
    cfg = capi.KmeansCfg(); capi.lib().ge_kmeans_cfg_default(C.byref(cfg))
    assert (cfg.metric, cfg.k, cfg.seed, cfg.device, cfg.stream) == (capi.GE_KM_COSINE, 0, 0, 0, None)


def test_argument_errors_come_before_any_device_work():
    L = capi.lib()
    ARG = capi.GE_ERR_ARG
    rows = np.ones((6, 3), np.float32); rp = rows.ctypes.data_as(f32p)
    h = C.c_void_p()
    good = _cfg()

    def create(n_rows=6, dim=3, subset=None, cfg=good, rows_p=rp, out=C.byref(h)):
        sub = np.ascontiguousarray(subset, np.int32) if subset is not None else None
        st = L.ge_kmeans_create(rows_p, n_rows, dim, sub.ctypes.data_as(i32p) if sub is not None else None, len(sub) if sub is not None else 0,
                                C.byref(cfg) if cfg is not None else None, out)
        return st, L.ge_last_error()

    for st, msg in (create(rows_p=None), create(cfg=None), create(out=None)):
        assert st == ARG and b"null" in msg
    for dim in (0, -1, 1025):
        st, msg = create(dim=dim)
        assert st == ARG and b"dim" in msg
    for k in (0, -3, 65537, 2 ** 31 - 1):
        st, msg = create(cfg=_cfg(k=k))
        assert st == ARG and b"k %d outside [1, 65536]" % k in msg, msg
    st, msg = create(cfg=_cfg(k=7))                                   # more clusters than rows
    assert st == ARG and b"k 7 exceeds the 6 indexed rows" in msg
    st, msg = create(cfg=_cfg(k=3), subset=[1, 4])                    # ... than the rows of the subset
    assert st == ARG and b"k 3 exceeds the 2 indexed rows" in msg
    for n in (0, -5, 2 ** 31 - 1, 2 ** 40):
        st, msg = create(n_rows=n)
        assert st == ARG and b"rows" in msg
    st, msg = create(n_rows=2 ** 26, dim=1024)                        # 2^36 floats
    assert st == ARG and b"more than one handle holds" in msg
    for metric in (-1, 2, 77):
        st, msg = create(cfg=_cfg(metric=metric))
        assert st == ARG and b"unknown metric" in msg
    for subset, word in (([2, 2], b"ascending"), ([3, 1], b"ascending"), ([0, 6], b"outside"), ([-1, 2], b"outside"), ([], b"subset"),
                         (list(range(6)) + [5], b"subset")):
        st, msg = create(subset=subset)
        assert st == ARG and word in msg, (subset, msg)
    assert h.value is None
    # the handle-taking calls
    assert L.ge_glove_kmeans_create(None, None, 0, C.byref(good), C.byref(h)) == ARG and b"null" in L.ge_last_error()
    assert L.ge_kmeans_set_centroids(None, rp) == ARG
    assert L.ge_kmeans_step(None, None, None) == ARG
    for max_iter in (0, -1):
        assert L.ge_kmeans_run(None, max_iter, None, None) == ARG and b"max_iter %d is below 1" % max_iter in L.ge_last_error()
    assert L.ge_kmeans_run(None, 1, None, None) == ARG and b"null" in L.ge_last_error()
    assert L.ge_kmeans_get(None, *([None] * 11)) == ARG
    assert L.ge_kmeans_last_kernel_ms(None, None, None) == ARG
    L.ge_kmeans_destroy(None)                                         # harmless


@pytest.mark.skipif(capi.lib().ge_device_count() > 0, reason="only meaningful on a box without a GPU")
def test_no_cpu_fallback_without_a_device():
    for metric in ("cosine", "euclid"):
        with pytest.raises(capi.GeError) as e:
            capi.Clustering.create(np.ones((6, 3), np.float32), 2, metric=metric)
        assert e.value.status == capi.GE_ERR_HIP


def test_host_configuration_keys(tmp_path):
    """`device: { clusters: K, clusters_metric, clusters_iterations }` in the C++ host's bean: the banner gains its line only when
    K > 0, and invalid values are refused in the wording of the other keys."""
    capi._share_hip_runtime_with_torch()
    host = C.CDLL(os.path.join(REPO, "graph-embeddings_amd", "lib", "libgehost.so"))
    host.geh_config_summary.restype = C.c_char_p
    base = "graph: g.nt\nmethod: glove\ndim: 4\nbca:\n  alpha: 0.1\n  epsilon: 0.001\noutput:\n  uri: []\n"
    number = "ERR\nInvalid configuration: Invalid device.clusters, choose a number from 1 to 65536 (0 = off)"
    metric = "ERR\nInvalid configuration: Invalid device.clusters_metric, choose one of: cosine, euclid"
    iters = "ERR\nInvalid configuration: Invalid device.clusters_iterations, choose a number from 1 up"
    line = lambda k, m, n: "# Clusters: %d (%s, at most %d iterations)" % (k, m, n)
    cases = {"": (None, None), "device:\n  clusters: 0\n": (None, None), "device:\n  clusters_metric: euclid\n": (None, None),
             "device:\n  clusters: 7\n": (None, line(7, "cosine", 50)), "device:\n  clusters: 65536\n  clusters_metric: euclid\n": (None, line(65536, "euclid", 50)),
             "device:\n  clusters: 2\n  clusters_iterations: 1\n": (None, line(2, "cosine", 1)),
             "device:\n  clusters: 65537\n": (number, None), "device:\n  clusters: -1\n": (number, None), "device:\n  clusters: 1.5\n": (number, None),
             "device:\n  clusters: few\n": (number, None), "device:\n  clusters: 3\n  clusters_metric: dot\n": (metric, None),
             "device:\n  clusters: 3\n  clusters_iterations: 0\n": (iters, None), "device:\n  clusters: 3\n  clusters_iterations: -2\n": (iters, None)}
    for i, (extra, (err, want)) in enumerate(cases.items()):
        p = tmp_path / ("c%d.yml" % i)
        p.write_text(base + extra)
        out = host.geh_config_summary(str(p).encode(), 1).decode()
        if err:
            assert out == err, (extra, out)
        else:
            assert out.startswith("OK\n") and ("# Clusters" in out) == (want is not None) and (want is None or want in out.splitlines()), (extra, out)


# ---- the yardstick against a brute-force statement of itself ------------------------------------------------------------

def test_prepare_and_bias_against_scalar_loops():
    X = nn_ref.random_rows(5, 9, 7)
    X[3] = 0
    XH = R.prepare(X, R.COSINE)
    for p in range(9):
        s = 0.0
        for d in range(7):
            s += float(X[p, d]) * float(X[p, d])
        n = math.sqrt(s)
        want = [np.float32(float(X[p, d]) / n) if n > 0 else np.float32(0) for d in range(7)]
        assert XH[p].tolist() == want
    assert np.array_equal(R.prepare(X, R.EUCLID), X)
    h = R.bias(X, R.EUCLID)
    for c in range(9):
        q = 0.0
        for d in range(7):
            q += float(X[c, d]) * float(X[c, d])
        assert h[c] == np.float32(-0.5 * q)
    assert not R.bias(X, R.COSINE).any()


def test_assign_against_a_double_loop():
    """Ties, -0 beside +0, a NaN (as -inf), a row of NaNs, -inf everywhere: the first centroid in (z descending, id ascending)."""
    Z = np.array([[1, 1, 1, 1], [3, 2, 5, 5], [-0.0, 0.0, -1, 0.0], [np.nan, 4, np.nan, 4], [np.nan] * 4, [-np.inf] * 4, [2, np.inf, np.inf, 1]],
                 np.float32)
    label, best = R.assign(Z)
    want = []
    for p in range(Z.shape[0]):
        z = [(-np.inf if np.isnan(v) else v) for v in Z[p]]
        w = 0
        for c in range(1, 4):
            if z[c] > z[w]:
                w = c
        want.append(w)
    assert label.tolist() == want == [0, 2, 0, 1, 0, 0, 1]
    assert np.array_equal(best, np.array([1, 5, 0, 4, -np.inf, -np.inf, np.inf], np.float32))


def test_exact_scores_hold_what_they_assert():
    X = nn_ref.integers(1, (5, 3), -4, 4)
    Cn = nn_ref.integers(2, (4, 3), -4, 4)
    Z = R.exact_scores(X, Cn, R.EUCLID)
    for p in range(5):
        for c in range(4):
            s = np.float32(0)
            for d in range(3):
                s = np.float32(float(X[p, d]) * float(Cn[c, d]) + float(s))          # exact: small integers
            assert Z[p, c] == np.float32(s + R.bias(Cn, R.EUCLID)[c])
    with pytest.raises(AssertionError):
        R.exact_scores(X + np.float32(0.5), Cn, R.EUCLID)


def test_update_and_objective_against_scalar_loops():
    n, dim, K = 2100, 3, 4
    XH = R.prepare(nn_ref.random_rows(7, n, dim), R.COSINE)
    XH[:2] = [[1, 0, 0], [-1, 0, 0]]
    labels = (synth.splitmix64(9, n) % np.uint64(2)).astype(np.int32)              # clusters 0 and 1: more than a piece each
    labels[:2] = 3                                                                    # cluster 3: two members that cancel; 2 is empty
    cen = nn_ref.random_rows(8, K, dim)
    for metric in (R.COSINE, R.EUCLID):
        got = R.update(XH, labels, cen, metric)
        for c in range(K):
            members = [p for p in range(n) if labels[p] == c]
            S = []
            for d in range(dim):
                total = 0.0
                for i in range(0, len(members), 1024):
                    piece = 0.0
                    for p in members[i:i + 1024]:
                        piece += float(XH[p, d])
                    total += piece
                S.append(total)
            if not members:
                want = cen[c].tolist()
            elif metric == R.EUCLID:
                want = [np.float32(s / float(len(members))) for s in S]
            else:
                m = math.sqrt(sum([s * s for s in S], 0.0))
                want = cen[c].tolist() if m == 0 else [np.float32(s / m) for s in S]
            assert got[c].tolist() == want, (metric, c)
        assert np.array_equal(got[2], cen[2])                                         # the empty cluster keeps its centroid
    assert np.array_equal(R.update(XH, labels, cen, R.COSINE)[3], cen[3])             # and so does the one whose members cancel
    assert np.array_equal(R.update(XH, labels, cen, R.EUCLID)[3], np.zeros(3, np.float32))
    best = nn_ref.random_rows(3, 1, 2500)[0]
    total = 0.0
    for i in range(0, 2500, 1024):
        blk = 0.0
        for v in best[i:i + 1024]:
            blk += float(v)
        total += blk
    assert R.objective(best) == total
    assert R.seq_sum(np.array([-0.0, -0.0]), 0) == 0 and not np.signbit(R.seq_sum(np.array([-0.0, -0.0]), 0))   # from +0.0


def test_the_keyed_sample():
    M = 2 ** 64 - 1
    for seed, n, K in ((0, 10, 10), (42, 1000, 17), (0xC0FFEE, 5000, 257), (2 ** 64 - 1, 64, 1)):
        pos = R.initial_positions(seed, n, K)
        assert len(pos) == K == len(set(pos.tolist())) and pos.min() >= 0 and pos.max() < n
        key = [(int(synth.splitmix64((seed ^ R.INIT_KEY) & M, 1, offset=p)[0]), p) for p in range(n)]
        assert pos.tolist() == [p for _, p in sorted(key)[:K]]
        assert np.array_equal(pos, R.initial_positions(seed, n, K))                  # a function of (seed, n, K)
        if K > 1:
            assert np.array_equal(pos[:K - 1], R.initial_positions(seed, n, K - 1))
    assert not np.array_equal(R.initial_positions(1, 1000, 17), R.initial_positions(2, 1000, 17))


def test_bound_refuses_inputs_near_the_subnormal_range():
    X = np.full((2, 3), 1e-30, np.float32)
    with pytest.raises(AssertionError):
        R.bound(X, X, R.COSINE)
    B = R.bound(np.ones((2, 4), np.float32), 2 * np.ones((3, 4), np.float32), R.EUCLID)
    assert np.allclose(B, (6 * 2 * 4 + 1.5 * 16) * R.U)

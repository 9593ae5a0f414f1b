"""CPU-only checks of the nearest-neighbour section of include/geglove.h: the exported symbols, the configuration struct, every
limit (an argument error with a message, before any device is touched), and the reference's own two routes to an exact top-k."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from geglove import capi
import nn_ref as R

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32p, i32p = C.POINTER(C.c_float), C.POINTER(C.c_int32)


def _cfg(**kw):
    cfg = capi.NnCfg(); capi.lib().ge_nn_cfg_default(C.byref(cfg))
    for k, v in kw.items():
        setattr(cfg, k, v)
    return cfg


def test_header_symbols_are_exported():
    header = open(os.path.join(REPO, "include", "geglove.h")).read()
    declared = set(re.findall(r"\b(ge_(?:glove_)?nn_\w+)\s*\(", header))
    assert declared == {"ge_nn_cfg_default", "ge_nn_cfg_size", "ge_nn_create", "ge_glove_nn_create", "ge_nn_query_rows", "ge_nn_query_vectors",
                        "ge_nn_get", "ge_nn_last_kernel_ms", "ge_nn_destroy"}
    L = capi.lib()
    for name in declared:
        assert name in capi.SYMBOLS and getattr(L, name) is not None
    assert re.search(r"enum \{ GE_NN_COSINE = 0, GE_NN_DOT = 1 \}", header) and (capi.GE_NN_COSINE, capi.GE_NN_DOT) == (0, 1)


def test_cfg_size_and_defaults():
    src = '#include <stdio.h>\n#include "geglove.h"\nint main(){printf("%zu", sizeof(ge_nn_cfg));return 0;}'
    exe = os.path.join(REPO, "tests", ".probe_sizes_nn")
    subprocess.run(["gcc", "-x", "c", "-", "-I", os.path.join(REPO, "include"), "-o", exe], input=src.encode(), check=True)
    try:
        size = int(subprocess.check_output([exe]))
    finally:
        os.remove(exe)
    assert size == C.sizeof(capi.NnCfg) == capi.lib().ge_nn_cfg_size()
    cfg = _cfg()
    assert (cfg.metric, cfg.device, cfg.stream) == (capi.GE_NN_COSINE, 0, None)


def test_argument_errors_come_before_any_device_work():
    L = capi.lib()
    ARG = capi.GE_ERR_ARG
    rows = np.ones((6, 3), np.float32); rp = rows.ctypes.data_as(f32p)
    h = C.c_void_p()
    good = _cfg()

    def create(n_rows=6, dim=3, subset=None, cfg=good, rows_p=rp, out=C.byref(h)):
        sub = np.ascontiguousarray(subset, np.int32) if subset is not None else None
        st = L.ge_nn_create(rows_p, n_rows, dim, sub.ctypes.data_as(i32p) if sub is not None else None, len(sub) if sub is not None else 0,
                            C.byref(cfg) if cfg is not None else None, out)
        return st, L.ge_last_error()

    assert create(rows_p=None)[0] == ARG and create(cfg=None)[0] == ARG and create(out=None)[0] == ARG
    for dim in (0, -1, 1025):
        st, msg = create(dim=dim)
        assert st == ARG and b"dim" in msg
    for n in (0, -5, 2 ** 31 - 1, 2 ** 40):
        st, msg = create(n_rows=n)
        assert st == ARG and b"rows" in msg
    st, msg = create(n_rows=2 ** 26, dim=1024)                       # 2^36 floats: more than one index holds
    assert st == ARG and b"more than one index holds" in msg
    for metric in (-1, 2, 77):
        st, msg = create(cfg=_cfg(metric=metric))
        assert st == ARG and b"metric" in msg
    for subset, word in (([2, 2], b"ascending"), ([3, 1], b"ascending"), ([0, 6], b"outside"), ([-1, 2], b"outside"), ([], b"subset"),
                         (list(range(6)) + [5], b"subset")):
        st, msg = create(subset=subset)
        assert st == ARG and word in msg, (subset, msg)
    assert h.value is None
    # the handle-taking calls
    out_i = np.zeros(8, np.int32); out_s = np.zeros(8, np.float32)
    pi, ps = out_i.ctypes.data_as(i32p), out_s.ctypes.data_as(f32p)
    assert L.ge_glove_nn_create(None, None, 0, C.byref(good), C.byref(h)) == ARG
    assert L.ge_nn_query_rows(None, None, 1, 1, 0, pi, ps) == ARG
    assert L.ge_nn_query_vectors(None, rp, 1, 1, pi, ps) == ARG
    assert L.ge_nn_get(None, None, None, None) == ARG
    assert L.ge_nn_last_kernel_ms(None, None, None) == ARG
    L.ge_nn_destroy(None)                                             # harmless


@pytest.mark.skipif(capi.lib().ge_device_count() > 0, reason="only meaningful on a box without a GPU")
def test_no_cpu_fallback_without_a_device():
    with pytest.raises(capi.GeError) as e:
        capi.Neighbors.create(np.ones((6, 3), np.float32))
    assert e.value.status == capi.GE_ERR_HIP
    with pytest.raises(capi.GeError) as e:
        capi.Neighbors.create(np.ones((6, 3), np.float32), subset=[1, 4], metric="dot")
    assert e.value.status == capi.GE_ERR_HIP


def test_the_reference_selects_what_a_stable_sort_gives():
    for seed, n, dim, lo, hi in ((1, 300, 3, -8, 8), (2, 257, 50, -1, 1), (3, 40, 1, -2, 2)):
        X = R.integers(seed, (n, dim), lo, hi)
        S = X @ X.T
        for k in (1, 10, 39):
            for self_pos in (None, np.arange(n)):
                a = R.exact_topk(S, k, self_pos)
                b = R.stable_topk(S, k, self_pos)
                assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
        assert np.mean([len(np.unique(row)) for row in S]) < 0.8 * n      # ties are frequent in every row


def test_the_bound_covers_its_derivation():
    for dim in (1, 3, 50, 200, 300, 1024):
        gamma = dim * R.U / (1 - dim * R.U)
        assert 2 * R.U + R.U ** 2 + gamma * (1 + R.U) ** 2 <= R.bound(dim)


def test_host_configuration_keys(tmp_path):
    """`device: { neighbors: K, neighbors_metric: cosine | dot }` in the C++ host's bean, checked where the other errors are; the
    banner gains its line only when the key is set."""
    capi._share_hip_runtime_with_torch()
    host = C.CDLL(os.path.join(REPO, "graph-embeddings_amd", "lib", "libgehost.so"))
    host.geh_config_summary.restype = C.c_char_p
    base = "graph: g.nt\nmethod: glove\ndim: 4\nbca:\n  alpha: 0.1\n  epsilon: 0.001\noutput:\n  uri: []\n"
    bad_k = "ERR\nInvalid configuration: Invalid device.neighbors, choose a number from 1 to 128 (0 = off)"
    bad_metric = "ERR\nInvalid configuration: Invalid device.neighbors_metric, choose one of: cosine, dot"
    cases = {"": (None, None), "device:\n  neighbors: 0\n": (None, None), "device:\n  neighbors: 5\n": (None, "# Nearest neighbours: 5 (cosine)"),
             "device:\n  neighbors: 128\n  neighbors_metric: dot\n": (None, "# Nearest neighbours: 128 (dot)"),
             "device:\n  neighbors: 129\n": (bad_k, None), "device:\n  neighbors: -1\n": (bad_k, None),
             "device:\n  neighbors: 5\n  neighbors_metric: euclid\n": (bad_metric, None)}
    for i, (extra, (err, line)) in enumerate(cases.items()):
        p = tmp_path / ("c%d.yml" % i)
        p.write_text(base + extra)
        out = host.geh_config_summary(str(p).encode(), 1).decode()
        if err:
            assert out == err, (extra, out)
        else:
            assert out.startswith("OK\n") and ("# Nearest neighbours" in out) == (line is not None) and (line is None or line in out.splitlines()), (extra, out)

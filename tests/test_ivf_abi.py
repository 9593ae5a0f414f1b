"""CPU-only checks of the inverted-file section of include/geglove.h: the exported symbols, the configuration struct, and every
limit of creation refused as an argument error with a message before any device is touched (the limits of a query -- k, nprobe,
member ids -- need an index and are in test_ivf_gpu.py; here the query calls refuse a null handle)."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from geglove import capi

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32p, i32p = C.POINTER(C.c_float), C.POINTER(C.c_int32)


def _cfg(**kw):
    cfg = capi.IvfCfg(); capi.lib().ge_ivf_cfg_default(C.byref(cfg))
    cfg.lists = 2
    for k, v in kw.items():
        setattr(cfg, k, v)
    return cfg


def test_header_symbols_are_exported():
    header = open(os.path.join(REPO, "include", "geglove.h")).read()
    declared = set(re.findall(r"\b(ge_(?:glove_)?ivf_\w+)\s*\(", header))
    assert declared == {"ge_ivf_cfg_default", "ge_ivf_cfg_size", "ge_ivf_create", "ge_glove_ivf_create", "ge_ivf_query_rows", "ge_ivf_query_vectors",
                        "ge_ivf_get", "ge_ivf_last_kernel_ms", "ge_ivf_destroy"}
    L = capi.lib()
    for name in declared:
        assert name in capi.SYMBOLS and getattr(L, name) is not None


def test_cfg_size_and_defaults():
    src = '#include <stdio.h>\n#include "geglove.h"\nint main(){printf("%zu", sizeof(ge_ivf_cfg));return 0;}'
    exe = os.path.join(REPO, "tests", ".probe_sizes_ivf")
    subprocess.run(["gcc", "-x", "c", "-", "-I", os.path.join(REPO, "include"), "-o", exe], input=src.encode(), check=True)
    try:
        size = int(subprocess.check_output([exe]))
    finally:
        os.remove(exe)
    assert size == C.sizeof(capi.IvfCfg) == capi.lib().ge_ivf_cfg_size()
    cfg = capi.IvfCfg(); capi.lib().ge_ivf_cfg_default(C.byref(cfg))
    assert (cfg.metric, cfg.lists, cfg.train_iterations, cfg.seed, bool(cfg.centroids), cfg.device, cfg.stream) == (capi.GE_NN_COSINE, 0, 10, 0, False, 0, None)


def test_argument_errors_come_before_any_device_work():
    L = capi.lib()
    ARG = capi.GE_ERR_ARG
    rows = np.arange(1, 19, dtype=np.float32).reshape(6, 3); rp = rows.ctypes.data_as(f32p)
    h = C.c_void_p()
    good = _cfg()

    def create(n_rows=6, dim=3, subset=None, cfg=good, rows_p=rp, out=C.byref(h)):
        sub = np.ascontiguousarray(subset, np.int32) if subset is not None else None
        st = L.ge_ivf_create(rows_p, n_rows, dim, sub.ctypes.data_as(i32p) if sub is not None else None, len(sub) if sub is not None else 0,
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
    st, msg = create(cfg=_cfg(metric=capi.GE_NN_DOT))
    assert st == ARG and b"no quantiser for dot" in msg
    for metric in (-1, 2, 77):
        st, msg = create(cfg=_cfg(metric=metric))
        assert st == ARG and b"metric" in msg
    for subset, word in (([2, 2], b"ascending"), ([3, 1], b"ascending"), ([0, 6], b"outside"), ([-1, 2], b"outside"), ([], b"subset"),
                         (list(range(6)) + [5], b"subset")):
        st, msg = create(subset=subset)
        assert st == ARG and word in msg, (subset, msg)
    for lists in (0, -1, 65537, 7):                                  # 1 <= L <= min(n, 65536): six rows hold no seven lists
        st, msg = create(cfg=_cfg(lists=lists))
        assert st == ARG and b"lists" in msg, (lists, msg)
    st, msg = create(subset=[1, 4], cfg=_cfg(lists=3))               # n is the subset's size
    assert st == ARG and b"lists" in msg
    for T in (-1, 1025):
        st, msg = create(cfg=_cfg(train_iterations=T))
        assert st == ARG and b"train_iterations" in msg
    # non-finite rows and centroids, found on the host
    for bad in (np.nan, np.inf, -np.inf):
        Z = rows.copy(); Z[4, 1] = bad
        st, msg = create(rows_p=Z.ctypes.data_as(f32p))
        assert st == ARG and b"non-finite input (rows)" in msg
        st, msg = create(rows_p=Z.ctypes.data_as(f32p), subset=[0, 4])
        assert st == ARG and b"non-finite input (rows)" in msg
        cen = np.ones((2, 3), np.float32); cen[1, 2] = bad
        st, msg = create(cfg=_cfg(centroids=cen.ctypes.data_as(f32p)))
        assert st == ARG and b"non-finite input (centroids)" in msg
    assert h.value is None
    # the handle-taking calls
    out_i = np.zeros(8, np.int32); out_s = np.zeros(8, np.float32)
    pi, ps = out_i.ctypes.data_as(i32p), out_s.ctypes.data_as(f32p)
    assert L.ge_glove_ivf_create(None, None, 0, C.byref(good), C.byref(h)) == ARG
    assert L.ge_ivf_query_rows(None, None, 1, 1, 1, 0, pi, ps, None, None) == ARG
    assert L.ge_ivf_query_vectors(None, rp, 1, 1, 1, pi, ps, None, None) == ARG
    assert L.ge_ivf_get(None, None, None, None, None, None, None, None, None) == ARG
    assert L.ge_ivf_last_kernel_ms(None, None, None, None, None) == ARG
    L.ge_ivf_destroy(None)                                            # harmless


@pytest.mark.skipif(capi.lib().ge_device_count() > 0, reason="only meaningful on a box without a GPU")
def test_no_cpu_fallback_without_a_device():
    rows = np.arange(1, 19, dtype=np.float32).reshape(6, 3)
    with pytest.raises(capi.GeError) as e:
        capi.IvfNeighbors.create(rows, 2)
    assert e.value.status == capi.GE_ERR_HIP
    with pytest.raises(capi.GeError) as e:
        capi.IvfNeighbors.create(rows, 2, subset=[1, 4], centroids=np.ones((2, 3), np.float32))
    assert e.value.status == capi.GE_ERR_HIP


def test_host_configuration_keys(tmp_path):
    """`device: { neighbors_lists: L, neighbors_probes: P, neighbors_iterations: T }` in the C++ host's bean, checked where the other
    errors are; the banner gains its line only when the key is set."""
    capi._share_hip_runtime_with_torch()
    host = C.CDLL(os.path.join(REPO, "graph-embeddings_amd", "lib", "libgehost.so"))
    host.geh_config_summary.restype = C.c_char_p
    base = "graph: g.nt\nmethod: glove\ndim: 4\nbca:\n  alpha: 0.1\n  epsilon: 0.001\noutput:\n  uri: []\n"
    err = "ERR\nInvalid configuration: "
    bad_l = err + "Invalid device.neighbors_lists, choose a number from 1 to 65536 (0 = off)"
    bad_p = err + "Invalid device.neighbors_probes, choose a number from 1 to the smaller of device.neighbors_lists and 128"
    bad_t = err + "Invalid device.neighbors_iterations, choose a number from 0 to 1024"
    alone = err + "device.neighbors_probes and device.neighbors_iterations need device.neighbors_lists"
    cases = {"device:\n  neighbors: 5\n": (None, None), "device:\n  neighbors: 5\n  neighbors_lists: 0\n": (None, None),
             "device:\n  neighbors: 5\n  neighbors_lists: 2048\n": (None, "# Neighbour lists: 2048 (16 probed, at most 10 iterations)"),
             "device:\n  neighbors: 5\n  neighbors_lists: 8\n": (None, "# Neighbour lists: 8 (8 probed, at most 10 iterations)"),
             "device:\n  neighbors: 5\n  neighbors_lists: 64\n  neighbors_probes: 4\n  neighbors_iterations: 0\n": (None, "# Neighbour lists: 64 (4 probed, at most 0 iterations)"),
             "device:\n  neighbors_lists: 8\n": (err + "device.neighbors_lists needs device.neighbors", None),
             "device:\n  neighbors: 5\n  neighbors_metric: dot\n  neighbors_lists: 8\n": (err + "device.neighbors_lists needs device.neighbors_metric: cosine", None),
             "device:\n  neighbors: 5\n  neighbors_probes: 4\n": (alone, None), "device:\n  neighbors: 5\n  neighbors_iterations: 4\n": (alone, None),
             "device:\n  neighbors: 5\n  neighbors_lists: 65537\n": (bad_l, None), "device:\n  neighbors: 5\n  neighbors_lists: -1\n": (bad_l, None),
             "device:\n  neighbors: 5\n  neighbors_lists: 8\n  neighbors_probes: 9\n": (bad_p, None),
             "device:\n  neighbors: 5\n  neighbors_lists: 8\n  neighbors_probes: 0\n": (bad_p, None),
             "device:\n  neighbors: 5\n  neighbors_lists: 1000\n  neighbors_probes: 129\n": (bad_p, None),
             "device:\n  neighbors: 5\n  neighbors_lists: 8\n  neighbors_iterations: 1025\n": (bad_t, None)}
    for i, (extra, (bad, line)) in enumerate(cases.items()):
        p = tmp_path / ("c%d.yml" % i)
        p.write_text(base + extra)
        out = host.geh_config_summary(str(p).encode(), 1).decode()
        if bad:
            assert out == bad, (extra, out)
        else:
            assert out.startswith("OK\n") and ("# Neighbour lists" in out) == (line is not None) and (line is None or line in out.splitlines()), (extra, out)

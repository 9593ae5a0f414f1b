"""CPU-only checks of the alignment section of include/geglove.h: the exported symbols, the two structs, and every limit refused
as an argument error with a message before any device is touched (ge_align_run looks at the threshold and the cap before the
handle, so those limits are checked here too); a valid call without a device is GE_ERR_HIP; the host's configuration keys."""
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
    cfg = capi.AlignCfg(); capi.lib().ge_align_cfg_default(C.byref(cfg))
    for k, v in kw.items():
        setattr(cfg, k, v)
    return cfg


def test_header_symbols_are_exported():
    header = open(os.path.join(REPO, "include", "geglove.h")).read()
    declared = set(re.findall(r"\b(ge_(?:glove_)?align_\w+)\s*\(", header))
    assert declared == {"ge_align_cfg_default", "ge_align_cfg_size", "ge_align_summary_size", "ge_align_create", "ge_glove_align_create", "ge_align_run",
                        "ge_align_get", "ge_align_last_kernel_ms", "ge_align_destroy"}
    L = capi.lib()
    for name in declared:
        assert name in capi.SYMBOLS and getattr(L, name) is not None


def test_struct_sizes_and_defaults():
    src = '#include <stdio.h>\n#include "geglove.h"\nint main(){printf("%zu %zu", sizeof(ge_align_cfg), sizeof(ge_align_summary));return 0;}'
    exe = os.path.join(REPO, "tests", ".probe_sizes_align")
    subprocess.run(["gcc", "-x", "c", "-", "-I", os.path.join(REPO, "include"), "-o", exe], input=src.encode(), check=True)
    try:
        cfg_size, summary_size = (int(v) for v in subprocess.check_output([exe]).split())
    finally:
        os.remove(exe)
    assert cfg_size == C.sizeof(capi.AlignCfg) == capi.lib().ge_align_cfg_size()
    assert summary_size == C.sizeof(capi.AlignSummary) == capi.lib().ge_align_summary_size() == 48
    assert all(t is C.c_int64 for _, t in capi.AlignSummary._fields_)                # integer throughout
    cfg = _cfg()
    assert (cfg.metric, cfg.device, cfg.stream) == (capi.GE_NN_COSINE, 0, None)


def test_argument_errors_come_before_any_device_work():
    L = capi.lib()
    ARG = capi.GE_ERR_ARG
    rows = np.arange(1, 19, dtype=np.float32).reshape(6, 3); rp = rows.ctypes.data_as(f32p)
    h = C.c_void_p()
    good = _cfg()

    def create(n_rows=6, dim=3, source=(0, 2), target=(1, 4, 5), cfg=good, rows_p=rp, out=C.byref(h)):
        s = np.ascontiguousarray(source, np.int32) if source is not None else None
        t = np.ascontiguousarray(target, np.int32) if target is not None else None
        st = L.ge_align_create(rows_p, n_rows, dim, s.ctypes.data_as(i32p) if s is not None else None, len(s) if s is not None else 0,
                               t.ctypes.data_as(i32p) if t is not None else None, len(t) if t is not None else 0,
                               C.byref(cfg) if cfg is not None else None, out)
        return st, L.ge_last_error()

    for st, msg in (create(rows_p=None), create(cfg=None), create(out=None), create(source=None), create(target=None)):
        assert st == ARG and b"null" in msg
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
    for ids, word in (([2, 2], b"ascending"), ([3, 1], b"ascending"), ([0, 6], b"outside"), ([-1, 2], b"outside"), ([], b"set of 0"),
                      (list(range(6)) + [5], b"set of 7")):
        st, msg = create(source=ids, target=[1] if 1 not in ids else [4])
        assert st == ARG and word in msg and b"source" in msg, (ids, msg)
        st, msg = create(target=ids, source=[1] if 1 not in ids else [4])
        assert st == ARG and word in msg and b"target" in msg, (ids, msg)
    for source, target, shared in (([0, 2], [2, 3], 2), ([1, 3, 5], [0, 5], 5), ([4], [4], 4), ([0, 1, 2], [0, 3], 0)):
        st, msg = create(source=source, target=target)
        assert st == ARG and (b"the source and target sets share row %d" % shared) in msg, (source, target, msg)
    assert h.value is None
    # the run: the threshold and the cap are looked at before the handle
    for T in (float("nan"), float("inf"), float("-inf")):
        assert L.ge_align_run(None, T, 10) == ARG and b"threshold must be finite" in L.ge_last_error()
    for cap in (0, -1, 2 ** 28 + 1, 2 ** 40):
        assert L.ge_align_run(None, 0.5, cap) == ARG and b"max_pairs" in L.ge_last_error()
    assert L.ge_align_run(None, 0.5, 2 ** 28) == ARG and b"null ge_align handle" in L.ge_last_error()
    assert L.ge_align_run(None, 0.5, 1) == ARG and b"null ge_align handle" in L.ge_last_error()
    # the other handle-taking calls
    one = np.zeros(1, np.int32).ctypes.data_as(i32p)
    assert L.ge_glove_align_create(None, one, 1, one, 1, C.byref(good), C.byref(h)) == ARG and b"null" in L.ge_last_error()
    assert L.ge_align_get(None, None, None, None, None, None, None, None, None, None, None, None) == ARG and b"null" in L.ge_last_error()
    assert L.ge_align_last_kernel_ms(None, None, None, None, None, None) == ARG and b"null" in L.ge_last_error()
    L.ge_align_destroy(None)                                          # harmless


@pytest.mark.skipif(capi.lib().ge_device_count() > 0, reason="only meaningful on a box without a GPU")
def test_no_cpu_fallback_without_a_device():
    rows = np.arange(1, 19, dtype=np.float32).reshape(6, 3)
    for kw in ({}, {"metric": "dot"}):
        with pytest.raises(capi.GeError) as e:
            capi.Alignment.from_rows(rows, [0, 2], [1, 4, 5], **kw)
        assert e.value.status == capi.GE_ERR_HIP


def test_host_configuration_keys(tmp_path):
    """`device: { align: T, align_source: P, align_target: Q, align_metric: cosine | dot, align_max_pairs: M }` in the C++ host's
    bean, checked where the other errors are; the banner gains its line only when the key is set."""
    capi._share_hip_runtime_with_torch()
    host = C.CDLL(os.path.join(REPO, "graph-embeddings_amd", "lib", "libgehost.so"))
    host.geh_config_summary.restype = C.c_char_p
    base = "graph: g.nt\nmethod: glove\ndim: 4\nbca:\n  alpha: 0.1\n  epsilon: 0.001\noutput:\n  uri: []\n"
    err = "ERR\nInvalid configuration: "
    bad_t = err + "Invalid device.align, choose a finite score threshold"
    bad_m = err + "Invalid device.align_metric, choose one of: cosine, dot"
    bad_p = err + "Invalid device.align_max_pairs, choose a number from 1 to 268435456"
    alone = err + "device.align_source, device.align_target, device.align_metric and device.align_max_pairs need device.align"
    sets = err + "device.align needs device.align_source and device.align_target, the key prefixes of the two sets"
    over = err + "device.align_source and device.align_target overlap: one prefix begins with the other"
    st = "  align_source: http://a/p\n  align_target: http://b/p\n"
    line = "# Align: http://a/p to http://b/p, pairs scoring at least %s (%s, at most %d pairs)"
    cases = {"": (None, None), "device:\n  neighbors: 5\n": (None, None), "device:\n  match: 0.9\n": (None, None),
             "device:\n  align: 0.9\n" + st: (None, line % ("0.9", "cosine", 16777216)),
             "device:\n  align: -2.5\n" + st + "  align_metric: dot\n  align_max_pairs: 1\n": (None, line % ("-2.5", "dot", 1)),
             "device:\n  align: 0\n" + st + "  align_max_pairs: 268435456\n": (None, line % ("0.0", "cosine", 268435456)),
             "device:\n" + st: (alone, None), "device:\n  align_source: x\n": (alone, None), "device:\n  align_target: x\n": (alone, None),
             "device:\n  align_metric: dot\n": (alone, None), "device:\n  align_max_pairs: 100\n": (alone, None),
             "device:\n  match: 0.5\n  align_metric: cosine\n": (alone, None),
             "device:\n  align: 0.9\n": (sets, None), "device:\n  align: 0.9\n  align_source: x\n": (sets, None),
             "device:\n  align: 0.9\n  align_target: x\n": (sets, None),
             "device:\n  align: 0.9\n  align_source: http://a/p\n  align_target: http://a/person\n": (over, None),
             "device:\n  align: 0.9\n  align_source: http://a/person\n  align_target: http://a/p\n": (over, None),
             "device:\n  align: 0.9\n  align_source: same\n  align_target: same\n": (over, None),
             "device:\n  align: nan\n" + st: (bad_t, None), "device:\n  align: inf\n" + st: (bad_t, None), "device:\n  align: -inf\n" + st: (bad_t, None),
             "device:\n  align: 1e39\n" + st: (bad_t, None), "device:\n  align: high\n" + st: (bad_t, None), "device:\n  align: 0.9x\n" + st: (bad_t, None),
             "device:\n  align: 0.9\n" + st + "  align_metric: euclid\n": (bad_m, None),
             "device:\n  align: 0.9\n" + st + "  align_max_pairs: 0\n": (bad_p, None),
             "device:\n  align: 0.9\n" + st + "  align_max_pairs: 268435457\n": (bad_p, None),
             "device:\n  align: 0.9\n" + st + "  align_max_pairs: -3\n": (bad_p, None),
             "device:\n  align: 0.9\n" + st + "  align_max_pairs: 2.5\n": (bad_p, None),
             "device:\n  align: 0.9\n" + st + "  align_max_pairs: many\n": (bad_p, None)}
    for i, (extra, (bad, want)) in enumerate(cases.items()):
        p = tmp_path / ("c%d.yml" % i)
        p.write_text(base + extra)
        out = host.geh_config_summary(str(p).encode(), 1).decode()
        if bad:
            assert out == bad, (extra, out)
        else:
            assert out.startswith("OK\n") and ("# Align" in out) == (want is not None) and (want is None or want in out.splitlines()), (extra, out)

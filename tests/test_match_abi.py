"""CPU-only checks of the matching section of include/geglove.h: the exported symbols, the two structs, and every limit refused
as an argument error with a message before any device is touched (ge_match_run looks at the threshold and the cap before the
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
    cfg = capi.MatchCfg(); capi.lib().ge_match_cfg_default(C.byref(cfg))
    for k, v in kw.items():
        setattr(cfg, k, v)
    return cfg


def test_header_symbols_are_exported():
    header = open(os.path.join(REPO, "include", "geglove.h")).read()
    declared = set(re.findall(r"\b(ge_(?:glove_)?match_\w+)\s*\(", header))
    assert declared == {"ge_match_cfg_default", "ge_match_cfg_size", "ge_match_summary_size", "ge_match_create", "ge_glove_match_create", "ge_match_run",
                        "ge_match_get", "ge_match_last_kernel_ms", "ge_match_destroy"}
    L = capi.lib()
    for name in declared:
        assert name in capi.SYMBOLS and getattr(L, name) is not None


def test_struct_sizes_and_defaults():
    src = '#include <stdio.h>\n#include "geglove.h"\nint main(){printf("%zu %zu", sizeof(ge_match_cfg), sizeof(ge_match_summary));return 0;}'
    exe = os.path.join(REPO, "tests", ".probe_sizes_match")
    subprocess.run(["gcc", "-x", "c", "-", "-I", os.path.join(REPO, "include"), "-o", exe], input=src.encode(), check=True)
    try:
        cfg_size, summary_size = (int(v) for v in subprocess.check_output([exe]).split())
    finally:
        os.remove(exe)
    assert cfg_size == C.sizeof(capi.MatchCfg) == capi.lib().ge_match_cfg_size()
    assert summary_size == C.sizeof(capi.MatchSummary) == capi.lib().ge_match_summary_size() == 40
    cfg = _cfg()
    assert (cfg.metric, cfg.device, cfg.stream) == (capi.GE_NN_COSINE, 0, None)


def test_argument_errors_come_before_any_device_work():
    L = capi.lib()
    ARG = capi.GE_ERR_ARG
    rows = np.arange(1, 19, dtype=np.float32).reshape(6, 3); rp = rows.ctypes.data_as(f32p)
    h = C.c_void_p()
    good = _cfg()

    def create(n_rows=6, dim=3, subset=None, cfg=good, rows_p=rp, out=C.byref(h)):
        sub = np.ascontiguousarray(subset, np.int32) if subset is not None else None
        st = L.ge_match_create(rows_p, n_rows, dim, sub.ctypes.data_as(i32p) if sub is not None else None, len(sub) if sub is not None else 0,
                               C.byref(cfg) if cfg is not None else None, out)
        return st, L.ge_last_error()

    for st, msg in (create(rows_p=None), create(cfg=None), create(out=None)):
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
    for subset, word in (([2, 2], b"ascending"), ([3, 1], b"ascending"), ([0, 6], b"outside"), ([-1, 2], b"outside"), ([], b"subset"),
                         (list(range(6)) + [5], b"subset")):
        st, msg = create(subset=subset)
        assert st == ARG and word in msg, (subset, msg)
    assert h.value is None
    # the run: the threshold and the cap are looked at before the handle
    for T in (float("nan"), float("inf"), float("-inf")):
        assert L.ge_match_run(None, T, 10) == ARG and b"threshold must be finite" in L.ge_last_error()
    for cap in (0, -1, 2 ** 28 + 1, 2 ** 40):
        assert L.ge_match_run(None, 0.5, cap) == ARG and b"max_pairs" in L.ge_last_error()
    assert L.ge_match_run(None, 0.5, 2 ** 28) == ARG and b"null ge_match handle" in L.ge_last_error()
    assert L.ge_match_run(None, 0.5, 1) == ARG and b"null ge_match handle" in L.ge_last_error()
    # the other handle-taking calls
    assert L.ge_glove_match_create(None, None, 0, C.byref(good), C.byref(h)) == ARG and b"null" in L.ge_last_error()
    assert L.ge_match_get(None, None, None, None, None, None, None, None) == ARG and b"null" in L.ge_last_error()
    assert L.ge_match_last_kernel_ms(None, None, None, None, None) == ARG and b"null" in L.ge_last_error()
    L.ge_match_destroy(None)                                          # harmless


@pytest.mark.skipif(capi.lib().ge_device_count() > 0, reason="only meaningful on a box without a GPU")
def test_no_cpu_fallback_without_a_device():
    rows = np.arange(1, 19, dtype=np.float32).reshape(6, 3)
    for kw in ({}, {"subset": [1, 4]}, {"metric": "dot"}):
        with pytest.raises(capi.GeError) as e:
            capi.Matching.from_rows(rows, **kw)
        assert e.value.status == capi.GE_ERR_HIP


def test_host_configuration_keys(tmp_path):
    """`device: { match: T, match_metric: cosine | dot, match_max_pairs: M }` in the C++ host's bean, checked where the other errors
    are; the banner gains its line only when the key is set."""
    capi._share_hip_runtime_with_torch()
    host = C.CDLL(os.path.join(REPO, "graph-embeddings_amd", "lib", "libgehost.so"))
    host.geh_config_summary.restype = C.c_char_p
    base = "graph: g.nt\nmethod: glove\ndim: 4\nbca:\n  alpha: 0.1\n  epsilon: 0.001\noutput:\n  uri: []\n"
    err = "ERR\nInvalid configuration: "
    bad_t = err + "Invalid device.match, choose a finite score threshold"
    bad_m = err + "Invalid device.match_metric, choose one of: cosine, dot"
    bad_p = err + "Invalid device.match_max_pairs, choose a number from 1 to 268435456"
    alone = err + "device.match_metric and device.match_max_pairs need device.match"
    cases = {"": (None, None), "device:\n  neighbors: 5\n": (None, None),
             "device:\n  match: 0.9\n": (None, "# Match: pairs scoring at least 0.9 (cosine, at most 16777216 pairs)"),
             "device:\n  match: -2.5\n  match_metric: dot\n  match_max_pairs: 1\n": (None, "# Match: pairs scoring at least -2.5 (dot, at most 1 pairs)"),
             "device:\n  match: 0\n  match_max_pairs: 268435456\n": (None, "# Match: pairs scoring at least 0.0 (cosine, at most 268435456 pairs)"),
             "device:\n  match_metric: dot\n": (alone, None), "device:\n  match_max_pairs: 100\n": (alone, None),
             "device:\n  match_metric: cosine\n  match_max_pairs: 100\n": (alone, None),
             "device:\n  match: nan\n": (bad_t, None), "device:\n  match: inf\n": (bad_t, None), "device:\n  match: -inf\n": (bad_t, None),
             "device:\n  match: 1e39\n": (bad_t, None), "device:\n  match: high\n": (bad_t, None), "device:\n  match: 0.9x\n": (bad_t, None),
             "device:\n  match: 0.9\n  match_metric: euclid\n": (bad_m, None),
             "device:\n  match: 0.9\n  match_max_pairs: 0\n": (bad_p, None), "device:\n  match: 0.9\n  match_max_pairs: 268435457\n": (bad_p, None),
             "device:\n  match: 0.9\n  match_max_pairs: -3\n": (bad_p, None), "device:\n  match: 0.9\n  match_max_pairs: 2.5\n": (bad_p, None),
             "device:\n  match: 0.9\n  match_max_pairs: many\n": (bad_p, None)}
    for i, (extra, (bad, line)) in enumerate(cases.items()):
        p = tmp_path / ("c%d.yml" % i)
        p.write_text(base + extra)
        out = host.geh_config_summary(str(p).encode(), 1).decode()
        if bad:
            assert out == bad, (extra, out)
        else:
            assert out.startswith("OK\n") and ("# Match" in out) == (line is not None) and (line is None or line in out.splitlines()), (extra, out)

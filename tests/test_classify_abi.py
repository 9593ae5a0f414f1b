"""CPU-only checks of the classification section of include/geglove.h: the exported symbols, the configuration struct and its
defaults, and every limit (an argument error with a message, before any device is touched)."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from geglove import capi

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32p, i32p, u8p = C.POINTER(C.c_float), C.POINTER(C.c_int32), C.POINTER(C.c_uint8)


def _cfg(**kw):
    cfg = capi.ClassifyCfg(); capi.lib().ge_classify_cfg_default(C.byref(cfg))
    cfg.classes = 3
    for k, v in kw.items():
        setattr(cfg, k, v)
    return cfg


def test_header_symbols_are_exported():
    header = open(os.path.join(REPO, "include", "geglove.h")).read()
    declared = set(re.findall(r"\b(ge_(?:glove_)?classify_\w+)\s*\(", header))
    assert declared == {"ge_classify_cfg_default", "ge_classify_cfg_size", "ge_classify_create", "ge_glove_classify_create", "ge_classify_set_weights",
                        "ge_classify_eval", "ge_classify_run", "ge_classify_predict", "ge_classify_score", "ge_classify_get",
                        "ge_classify_last_kernel_ms", "ge_classify_destroy"}
    L = capi.lib()
    for name in declared:
        assert name in capi.SYMBOLS and getattr(L, name) is not None
    out = subprocess.check_output(["nm", "-D", "--defined-only", capi.LIB_PATH]).decode()
    assert declared <= set(re.findall(r" T (ge_[a-z0-9_]+)", out))
    assert re.search(r"enum \{ GE_CLS_COSINE = 0, GE_CLS_RAW = 1 \}", header) and (capi.GE_CLS_COSINE, capi.GE_CLS_RAW) == (0, 1)
    assert re.search(r"enum \{ GE_CLS_STOP_NONE = 0, GE_CLS_STOP_GRADIENT = 1, GE_CLS_STOP_MAXITER = 2, GE_CLS_STOP_LINESEARCH = 3 \}", header)
    assert capi.CLS_STOPS == ("none", "gradient", "maxiter", "linesearch")


def test_cfg_size_and_defaults(tmp_path):
    src = ('#include <stdio.h>\n#include "geglove.h"\nint main(){printf("%zu %zu", sizeof(ge_classify_cfg), sizeof(ge_classify_summary));return 0;}')
    exe = str(tmp_path / "probe_size_classify")
    subprocess.run(["gcc", "-x", "c", "-", "-I", os.path.join(REPO, "include"), "-o", exe], input=src.encode(), check=True)
    size, summary = (int(v) for v in subprocess.check_output([exe]).split())
    assert size == C.sizeof(capi.ClassifyCfg) == capi.lib().ge_classify_cfg_size() == 40
    assert summary == C.sizeof(capi.ClassifySummary) == 56
    assert [n for n, _ in capi.ClassifyCfg._fields_] == ["normalize", "classes", "l2", "tolerance", "device", "stream"]
    cfg = capi.ClassifyCfg(); capi.lib().ge_classify_cfg_default(C.byref(cfg))
    assert (cfg.normalize, cfg.classes, cfg.l2, cfg.tolerance, cfg.device, cfg.stream) == (capi.GE_CLS_COSINE, 0, 1e-4, 1e-4, 0, None)


def test_argument_errors_come_before_any_device_work():
    L = capi.lib()
    ARG = capi.GE_ERR_ARG
    rows = np.ones((6, 3), np.float32); rp = rows.ctypes.data_as(f32p)
    h = C.c_void_p()
    good = _cfg()
    fine = [0, 1, 2, -1, 1, 0]

    def create(n_rows=6, dim=3, subset=None, labels=fine, train=None, cfg=good, rows_p=rp, out=C.byref(h)):
        sub = np.ascontiguousarray(subset, np.int32) if subset is not None else None
        lab = np.ascontiguousarray(labels, np.int32) if labels is not None else None
        tr = np.ascontiguousarray(train, np.uint8) if train is not None else None
        st = L.ge_classify_create(rows_p, n_rows, dim, sub.ctypes.data_as(i32p) if sub is not None else None, len(sub) if sub is not None else 0,
                                  lab.ctypes.data_as(i32p) if lab is not None else None, tr.ctypes.data_as(u8p) if tr is not None else None,
                                  C.byref(cfg) if cfg is not None else None, out)
        return st, L.ge_last_error()

    for st, msg in (create(rows_p=None), create(cfg=None), create(out=None), create(labels=None)):
        assert st == ARG and b"null" in msg
    for dim in (0, -1, 1025):
        st, msg = create(dim=dim)
        assert st == ARG and b"dim" in msg
    for classes in (0, 1, -3, 1025, 2 ** 31 - 1):
        st, msg = create(cfg=_cfg(classes=classes))
        assert st == ARG and b"classes %d outside [2, 1024]" % classes in msg, msg
    for labels, word in (([0, 1, 3, -1, 1, 0], b"labels[2] = 3 outside [-1, 3)"), ([0, -2, 1, 0, 1, 0], b"labels[1] = -2 outside [-1, 3)")):
        st, msg = create(labels=labels)
        assert st == ARG and word in msg, msg
    for labels, train in (([-1] * 6, None), (fine, [0] * 6), (fine, [0, 0, 0, 1, 0, 0])):      # nothing labelled; nothing trains; only an unlabelled one
        st, msg = create(labels=labels, train=train)
        assert st == ARG and b"no training member" in msg, msg
    for l2 in (-1e-9, float("inf"), float("nan")):
        st, msg = create(cfg=_cfg(l2=l2))
        assert st == ARG and b"l2" in msg
    for tolerance in (-1e-9, float("nan")):
        st, msg = create(cfg=_cfg(tolerance=tolerance))
        assert st == ARG and b"tolerance" in msg
    for normalize in (-1, 2, 77):
        st, msg = create(cfg=_cfg(normalize=normalize))
        assert st == ARG and b"unknown normalize" in msg
    for n in (0, -5, 2 ** 31 - 1, 2 ** 40):
        st, msg = create(n_rows=n)
        assert st == ARG and b"rows" in msg
    st, msg = create(n_rows=2 ** 26, dim=1024)                        # 2^36 floats
    assert st == ARG and b"more than one handle holds" in msg
    st, msg = create(n_rows=2 ** 23 + 1, dim=1, cfg=_cfg(classes=1024))               # n * C = 2^33 + 1024
    assert st == ARG and b"more than 2^33 logits" in msg
    for subset, word in (([2, 2], b"ascending"), ([3, 1], b"ascending"), ([0, 6], b"outside"), ([-1, 2], b"outside"), ([], b"subset"),
                         (list(range(6)) + [5], b"subset")):
        st, msg = create(subset=subset)
        assert st == ARG and word in msg, (subset, msg)
    st, msg = create(subset=[1, 3], labels=[-1, -1])                  # the labels belong to the positions of the subset
    assert st == ARG and b"no training member" in msg
    assert h.value is None
    # the handle-taking calls
    assert L.ge_glove_classify_create(None, None, 0, None, None, C.byref(good), C.byref(h)) == ARG and b"null" in L.ge_last_error()
    assert L.ge_classify_set_weights(None, rp) == ARG
    assert L.ge_classify_eval(None, None, None) == ARG
    for max_iter in (0, -1):
        assert L.ge_classify_run(None, max_iter, None, None) == ARG and b"max_iter %d is below 1" % max_iter in L.ge_last_error()
    assert L.ge_classify_run(None, 1, None, None) == ARG and b"null" in L.ge_last_error()
    assert L.ge_classify_predict(None, None, None) == ARG
    assert L.ge_classify_score(None, None, None, None) == ARG
    assert L.ge_classify_get(None, *([None] * 9)) == ARG
    assert L.ge_classify_last_kernel_ms(None, None, None, None) == ARG
    L.ge_classify_destroy(None)                                       # harmless


@pytest.mark.skipif(capi.lib().ge_device_count() > 0, reason="only meaningful on a box without a GPU")
def test_no_cpu_fallback_without_a_device():
    for normalize in ("cosine", "none"):
        with pytest.raises(capi.GeError) as e:
            capi.Classifier.create(np.ones((6, 3), np.float32), [0, 1, 0, 1, -1, 0], 2, normalize=normalize)
        assert e.value.status == capi.GE_ERR_HIP


def test_host_configuration_keys(tmp_path):
    """`device: { classify: <labels.tsv>, classify_test, classify_l2, classify_iterations, classify_normalize }` in the C++ host's
    bean: the banner gains its line only with a labels file, and invalid values are refused in the wording of the other keys."""
    capi._share_hip_runtime_with_torch()
    host = C.CDLL(os.path.join(REPO, "graph-embeddings_amd", "lib", "libgehost.so"))
    host.geh_config_summary.restype = C.c_char_p
    base = "graph: g.nt\nmethod: glove\ndim: 4\nbca:\n  alpha: 0.1\n  epsilon: 0.001\noutput:\n  uri: []\n"
    test = "ERR\nInvalid configuration: Invalid device.classify_test, choose a fraction from 0 to 0.9"
    l2 = "ERR\nInvalid configuration: Invalid device.classify_l2, choose a number from 0 up"
    iters = "ERR\nInvalid configuration: Invalid device.classify_iterations, choose a number from 1 up"
    norm = "ERR\nInvalid configuration: Invalid device.classify_normalize, choose one of: cosine, none"
    line = lambda f, t, l, m, n: "# Classify: %s (test %s, l2 %s, %s, at most %d iterations)" % (f, t, l, m, n)
    cases = {"": (None, None), "device:\n  classify_test: 0.5\n": (None, None), "device:\n  classify_normalize: none\n": (None, None),
             "device:\n  classify: labels.tsv\n": (None, line("labels.tsv", "0.2", "1.0E-4", "cosine", 200)),
             "device:\n  classify: l.tsv\n  classify_test: 0\n  classify_l2: 0.01\n  classify_iterations: 3\n  classify_normalize: none\n":
                 (None, line("l.tsv", "0.0", "0.01", "none", 3)),
             "device:\n  classify: l.tsv\n  classify_test: 0.9\n  classify_l2: 0\n": (None, line("l.tsv", "0.9", "0.0", "cosine", 200)),
             "device:\n  classify: l.tsv\n  classify_test: 0.95\n": (test, None), "device:\n  classify_test: -0.1\n": (test, None),
             "device:\n  classify_test: half\n": (test, None), "device:\n  classify_test: nan\n": (test, None),
             "device:\n  classify_l2: -1\n": (l2, None), "device:\n  classify_l2: inf\n": (l2, None), "device:\n  classify_l2: small\n": (l2, None),
             "device:\n  classify_iterations: 0\n": (iters, None), "device:\n  classify_iterations: 2.5\n": (iters, None),
             "device:\n  classify_iterations: soon\n": (iters, None), "device:\n  classify_normalize: euclid\n": (norm, None)}
    for i, (extra, (err, want)) in enumerate(cases.items()):
        p = tmp_path / ("c%d.yml" % i)
        p.write_text(base + extra)
        out = host.geh_config_summary(str(p).encode(), 1).decode()
        if err:
            assert out == err, (extra, out)
        else:
            assert out.startswith("OK\n") and ("# Classify" in out) == (want is not None) and (want is None or want in out.splitlines()), (extra, out)

"""CPU-only checks of the fold-in section of include/geglove.h: the exported symbols, the struct and its defaults, every limit
that needs no handle (refused with a message before the handle is looked at, so without a device), and the late-vertex rule
ge_foldin_mask against a Python SplitMix64."""
import ctypes as C
import os
import re

import numpy as np

from geglove import capi

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
i32p, i64p, f32p = C.POINTER(C.c_int32), C.POINTER(C.c_int64), C.POINTER(C.c_float)
M64 = (1 << 64) - 1


def test_header_symbols_are_exported():
    header = open(os.path.join(REPO, "include", "geglove.h")).read()
    declared = set(re.findall(r"\b(ge_glove_fold_\w+|ge_fold_\w+|ge_foldin_\w+)\s*\(", header))
    assert declared == {"ge_fold_cfg_default", "ge_fold_cfg_size", "ge_glove_fold_create", "ge_glove_fold_run", "ge_fold_last_kernel_ms",
                        "ge_fold_get", "ge_fold_destroy", "ge_foldin_mask"}
    L = capi.lib()
    for name in declared:
        assert name in capi.SYMBOLS and getattr(L, name) is not None


def test_struct_size_and_defaults():
    L = capi.lib()
    assert C.sizeof(capi.FoldCfg) == 24 == L.ge_fold_cfg_size()
    cfg = capi.FoldCfg(side=7, epochs=7, shuffle=7, learning_rate=7.0, seed=7)
    L.ge_fold_cfg_default(C.byref(cfg))
    assert (cfg.side, cfg.epochs, cfg.shuffle, cfg.learning_rate, cfg.seed) == (capi.GE_FOLD_FOCUS, 10, capi.GE_SHUFFLE_DEVICE, 0.0, 0)
    assert (capi.GE_FOLD_FOCUS, capi.GE_FOLD_CONTEXT) == (0, 1)
    L.ge_fold_cfg_default(None)                                        # harmless


def _create(h, row_ptr, idx, X, n_rows, out=True, cfg=True, **fields):
    L = capi.lib()
    c = capi.FoldCfg()
    L.ge_fold_cfg_default(C.byref(c))
    for k, v in fields.items():
        setattr(c, k, v)
    arr = lambda a, t: None if a is None else np.asarray(a, t)
    row_ptr, idx, X = arr(row_ptr, np.int64), arr(idx, np.int32), arr(X, np.float32)
    p = lambda a, t: None if a is None else a.ctypes.data_as(t)
    r = C.c_void_p()
    st = L.ge_glove_fold_create(h, p(row_ptr, i64p), p(idx, i32p), p(X, f32p), n_rows, C.byref(c) if cfg else None, C.byref(r) if out else None)
    assert r.value is None
    return st, L.ge_last_error().decode()


def test_limits_are_refused_without_a_device():
    """Everything that needs no handle is checked before the handle is looked at, so a null handle reaches each message."""
    ARG = capi.GE_ERR_ARG
    ptr, idx, X = [0, 2, 2, 3], [0, 5, 5], [0.5, 0.25, 2.0]            # an empty row and a repeated id are legal
    ok = (ARG, "null ge_glove handle")
    assert _create(None, ptr, idx, X, 3) == ok
    assert _create(None, ptr, idx, X, 3, side=capi.GE_FOLD_CONTEXT, shuffle=capi.GE_SHUFFLE_NONE, epochs=1024, learning_rate=0.5, seed=-3) == ok
    # null arguments
    assert _create(None, ptr, idx, X, 3, out=False) == (ARG, "out is null")
    for a in ((None, idx, X), (ptr, None, X), (ptr, idx, None)):
        assert _create(None, *a, 3) == (ARG, "null fold-in arrays")
    assert _create(None, ptr, idx, X, 3, cfg=False) == (ARG, "null ge_fold_cfg")
    # n_rows
    for n in (0, -1, 2 ** 31):
        st, msg = _create(None, ptr, idx, X, n)
        assert st == ARG and "1 <= n_rows < 2^31" in msg, (n, msg)
    # the configuration
    for side in (-1, 2):
        assert _create(None, ptr, idx, X, 3, side=side) == (ARG, "fold: unknown side %d" % side)
    st, msg = _create(None, ptr, idx, X, 3, shuffle=capi.GE_SHUFFLE_JAVA)
    assert st == ARG and "GE_SHUFFLE_JAVA" in msg
    for sh in (-1, 3):
        assert _create(None, ptr, idx, X, 3, shuffle=sh) == (ARG, "fold: unknown shuffle %d" % sh)
    for e in (0, -1, 1025):
        assert _create(None, ptr, idx, X, 3, epochs=e) == (ARG, "fold: %d epochs outside [1, 1024]" % e)
    for lr in (-0.1, float("inf"), float("nan")):
        st, msg = _create(None, ptr, idx, X, 3, learning_rate=lr)
        assert st == ARG and "learning rate" in msg, (lr, msg)
    # n_rows * E: only row_ptr[0 .. n_rows] is read, and the product is refused before that
    st, msg = _create(None, ptr, idx, X, 2 ** 21, epochs=1024)
    assert st == ARG and "not below 2^31" in msg
    # the offsets
    assert _create(None, [1, 2, 2, 3], idx, X, 3) == (ARG, "row_ptr[0] is 1, not 0")
    assert _create(None, [0, 2, 1, 3], idx, X, 3) == (ARG, "row_ptr decreases at [2]")
    st, msg = _create(None, [0, 2 ** 31], idx, X, 1)
    assert st == ARG and "below 2^31" in msg
    # ids below zero, values that are not finite and positive
    st, msg = _create(None, ptr, [0, -1, 5], X, 3)
    assert st == ARG and "row 0: id -1 out of range" in msg
    for x in (0.0, -0.5, float("inf"), float("nan")):
        st, msg = _create(None, ptr, idx, [0.5, 0.25, x], 3)
        assert st == ARG and "row 2: value" in msg and "not finite and positive" in msg, (x, msg)
    # the other entry points
    L = capi.lib()
    assert L.ge_glove_fold_run(None, None, None, None, None, None, None) == ARG and L.ge_last_error().decode() == "null ge_fold handle"
    assert L.ge_fold_last_kernel_ms(None, None) == ARG
    assert L.ge_fold_get(None, None, None, None, None) == ARG
    L.ge_fold_destroy(None)                                            # harmless


def test_host_configuration_keys(tmp_path):
    """`device: { foldin: F, foldin_epochs: E }` in the C++ host's bean: F in (0, 0.5], 0 = off; E from 1 to 1024, 50 by default;
    not beside holdout, one rank only; the banner gains its line only when the key is set."""
    capi._share_hip_runtime_with_torch()
    host = C.CDLL(os.path.join(REPO, "graph-embeddings_amd", "lib", "libgehost.so"))
    host.geh_config_summary.restype = C.c_char_p
    base = "graph: g.nt\nmethod: glove\ndim: 4\nbca:\n  alpha: 0.1\n  epsilon: 0.001\noutput:\n  uri: []\n"
    bad = "ERR\nInvalid configuration: Invalid device.foldin, choose a fraction from 0 to 0.5 (0 = off)"
    bad_e = "ERR\nInvalid configuration: Invalid device.foldin_epochs, choose a number from 1 to 1024"
    both = "ERR\nInvalid configuration: device.foldin and device.holdout split the matrix differently, set one of them"
    ranks = "ERR\nInvalid configuration: device.foldin runs on one rank only, set device.gpus: 1"
    line = lambda f, e: "# Foldin: %s, %d epochs" % (f, e)
    cases = {"": (None, None), "device:\n  foldin: 0\n": (None, None), "device:\n  foldin: 0.2\n": (None, line("0.2", 50)),
             "device:\n  foldin: 0.5\n  foldin_epochs: 1024\n": (None, line("0.5", 1024)), "device:\n  foldin: 0.001\n  foldin_epochs: 1\n": (None, line("0.001", 1)),
             "device:\n  foldin: 0.5000001\n": (bad, None), "device:\n  foldin: -0.1\n": (bad, None), "device:\n  foldin: 1\n": (bad, None),
             "device:\n  foldin: some\n": (bad, None), "device:\n  foldin: 0.2x\n": (bad, None),
             "device:\n  foldin: 0.2\n  foldin_epochs: 0\n": (bad_e, None), "device:\n  foldin: 0.2\n  foldin_epochs: 1025\n": (bad_e, None),
             "device:\n  foldin: 0.2\n  foldin_epochs: 2.5\n": (bad_e, None), "device:\n  foldin: 0.2\n  foldin_epochs: -1\n": (bad_e, None),
             "device:\n  foldin: 0.2\n  holdout: 0.2\n": (both, None), "device:\n  foldin: 0.2\n  gpus: 2\n": (ranks, None),
             "device:\n  foldin: 0\n  gpus: 2\n": (None, None), "device:\n  foldin: 0\n  holdout: 0.2\n": (None, None)}
    for i, (extra, (err, want)) in enumerate(cases.items()):
        p = tmp_path / ("c%d.yml" % i)
        p.write_text(base + extra)
        out = host.geh_config_summary(str(p).encode(), 1).decode()
        if err:
            assert out == err, (extra, out)
        else:
            assert out.startswith("OK\n") and ("# Foldin" in out) == (want is not None) and (want is None or want in out.splitlines()), (extra, out)


def _splitmix_at(seed, n):
    z = (seed + (n + 1) * 0x9E3779B97F4A7C15) & M64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
    return z ^ (z >> 31)


def test_foldin_mask_is_the_stated_rule():
    for seed, fraction in ((0, 0.5), (42, 0.2), (2 ** 64 - 1, 1e-3), (0xC0FFEE, 0.333)):
        n = 3000
        T = int(np.floor(fraction * 4294967296.0))
        want = np.array([(_splitmix_at(seed ^ 0x464F4C44494E, v) >> 32) < T for v in range(n)], np.uint8)
        got = capi.foldin_mask(seed, n, fraction)
        assert np.array_equal(got, want)
        assert abs(int(got.sum()) - fraction * n) < 5 * np.sqrt(n)     # about the asked share
        assert np.array_equal(capi.foldin_mask(seed, 100, fraction), want[:100])          # a function of (seed, v, fraction) alone
    assert not np.array_equal(capi.foldin_mask(1, 3000, 0.2), capi.holdout_mask(1, 3000, 0.2))     # its own key
    assert capi.foldin_mask(5, 0, 0.2).shape == (0,)


def test_foldin_fractions_outside_the_range_are_refused():
    L = capi.lib()
    mask = np.zeros(4, np.uint8)
    for f in (0.0, -0.1, 0.5000001, 1.0, float("nan"), float("inf")):
        assert L.ge_foldin_mask(1, 4, f, mask.ctypes.data_as(C.POINTER(C.c_uint8))) == capi.GE_ERR_ARG, f
        assert "outside (0, 0.5]" in L.ge_last_error().decode()
    assert L.ge_foldin_mask(1, 4, 0.5, None) == capi.GE_ERR_ARG
    assert L.ge_foldin_mask(1, -1, 0.5, mask.ctypes.data_as(C.POINTER(C.c_uint8))) == capi.GE_ERR_ARG

"""CPU-only checks of the generator section of include/geglove.h: the exported symbols, the configuration struct, every limit (an
argument error with its message, before any device is touched), and the properties of the recipe's numpy model (tests/synth_ref.py)
that the device output is then held to bit for bit (tests/test_synth_gpu.py)."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from geglove import capi
import synth_ref as R

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _cfg(**kw):
    cfg = capi.SynthCfg(); capi.lib().ge_synth_cfg_default(C.byref(cfg))
    for k, v in kw.items():
        setattr(cfg, k, v)
    return cfg


def test_header_symbols_are_exported():
    header = open(os.path.join(REPO, "include", "geglove.h")).read()
    declared = set(re.findall(r"\b(ge_synth_\w+|ge_coo_device|ge_coo_synth_stats|ge_glove_create_coo)\s*\(", header))
    assert declared == {"ge_synth_cfg_default", "ge_synth_cfg_size", "ge_synth_coo", "ge_coo_device", "ge_coo_synth_stats", "ge_glove_create_coo"}
    L = capi.lib()
    for name in declared:
        assert name in capi.SYMBOLS and getattr(L, name) is not None


def test_cfg_size_and_defaults(tmp_path):
    src = '#include <stdio.h>\n#include "geglove.h"\nint main(){printf("%zu", sizeof(ge_synth_cfg));return 0;}'
    exe = str(tmp_path / "probe_size_synth")
    subprocess.run(["gcc", "-x", "c", "-", "-I", os.path.join(REPO, "include"), "-o", exe], input=src.encode(), check=True)
    size = int(subprocess.check_output([exe]))
    assert size == C.sizeof(capi.SynthCfg) == capi.lib().ge_synth_cfg_size()
    cfg = _cfg()
    assert (cfg.vocab_size, cfg.row_begin, cfg.row_end, cfg.nnz, cfg.seed, cfg.device, cfg.stream) == (0, 0, 0, 0, 0xC0FFEE, 0, None)


def test_argument_errors_come_before_any_device_work():
    L = capi.lib()
    h = C.c_void_p()

    def call(out=C.byref(h), null_cfg=False, **kw):
        st = L.ge_synth_coo(None if null_cfg else C.byref(_cfg(**kw)), out)
        return st, L.ge_last_error().decode()

    cases = [
        (dict(vocab_size=0, nnz=1), "vocab_size must be >= 1"),
        (dict(vocab_size=-5, nnz=1), "vocab_size must be >= 1"),
        (dict(vocab_size=10, nnz=20, row_begin=5, row_end=5), "invalid row range [5,5)"),
        (dict(vocab_size=10, nnz=20, row_begin=-1, row_end=5), "invalid row range [-1,5)"),
        (dict(vocab_size=10, nnz=20, row_begin=3, row_end=11), "invalid row range [3,11)"),
        (dict(vocab_size=10, nnz=20, row_begin=7, row_end=3), "invalid row range [7,3)"),
        (dict(vocab_size=10, nnz=9), "nnz out of range: 9"),                      # less than the diagonal
        (dict(vocab_size=10, nnz=2, row_begin=2, row_end=5), "nnz out of range: 2"),
        (dict(vocab_size=10, nnz=2 ** 31), "nnz out of range: 2147483648"),
        (dict(vocab_size=10, nnz=-1), "nnz out of range: -1"),
        (dict(vocab_size=10, nnz=101), "nnz 101 exceeds the 100 cells"),
        (dict(vocab_size=10, nnz=31, row_begin=2, row_end=5), "nnz 31 exceeds the 30 cells"),
        (dict(vocab_size=1, nnz=2), "nnz 2 exceeds the 1 cells"),
    ]
    for kw, msg in cases:
        st, err = call(**kw)
        assert st == capi.GE_ERR_ARG and msg in err, (kw, st, err)
        assert not h.value
        rb, re_ = kw.get("row_begin", 0), kw.get("row_end", 0)
        with pytest.raises(ValueError):                                           # the model draws the same lines
            R.check_args(kw["vocab_size"], rb, re_, kw["nnz"])
    st, err = call(null_cfg=True)
    assert st == capi.GE_ERR_ARG and "cfg is null" in err
    st, err = call(out=None, vocab_size=10, nnz=20)
    assert st == capi.GE_ERR_ARG and "out is null" in err
    # a request inside the limits gets as far as the device (and no further on a machine without one)
    st, err = call(vocab_size=10, nnz=20)
    assert st in (capi.GE_OK, capi.GE_ERR_HIP), (st, err)
    if st == capi.GE_OK:
        L.ge_coo_destroy(h)
    # the views and the statistics of a null handle, the trainer on one
    assert L.ge_coo_device(None, None, None, None, None) == capi.GE_ERR_ARG
    assert L.ge_coo_synth_stats(None, None, None, None) == capi.GE_ERR_ARG
    g = capi.GloveCfg(); L.ge_glove_cfg_default(C.byref(g))
    assert L.ge_glove_create_coo(C.byref(g), None, C.byref(h)) == capi.GE_ERR_ARG and b"null ge_coo" in L.ge_last_error()
    assert L.ge_glove_create_coo(None, None, C.byref(h)) == capi.GE_ERR_ARG


SHAPES = [(64, 0, 64, 2000), (1000, 250, 500, 30000)]


@pytest.mark.parametrize("V,rb,re_,nnz", SHAPES)
def test_model_properties(V, rb, re_, nnz):
    I, J, X, draws = R.model(V, rb, re_, nnz)
    rows = re_ - rb
    assert I.dtype == np.int32 and J.dtype == np.int32 and X.dtype == np.float32
    assert len(I) == len(J) == len(X) == nnz                                     # exactly the named size
    key = I.astype(np.int64) * V + J
    assert np.all(np.diff(key) > 0)                                              # strictly ascending (i, j): sorted, no duplicates
    assert I.min() >= rb and I.max() < re_ and J.min() >= 0 and J.max() < V
    diag = I == J
    assert np.array_equal(I[diag], np.arange(rb, re_)) and np.all(X[diag] == np.float32(0.2))      # the whole diagonal
    assert np.all(X > 0) and np.all(X <= np.float32(0.2))
    M = nnz - rows
    assert M <= draws <= 8 * M + 1024
    print("V %d rows [%d,%d) nnz %d: %d draws, %.2f per key" % (V, rb, re_, nnz, draws, draws / M))
    # every entry is what its own draw says, and no valid key drawn before the cut is missing
    i, j, ok, c = R.draws(V, rb, re_, 0xC0FFEE, 0, draws)
    assert ok[-1]                                                                # the last draw delivered the last key
    dk = (i * V + j)[ok]
    uk, first = np.unique(dk, return_index=True)
    assert np.array_equal(uk, key[~diag])
    assert np.array_equal(R.value(c[ok][first]), X[~diag])


def test_model_hub_column_is_full():
    V, nnz = 64, 2000
    I, J, X, draws = R.model(V, 0, V, nnz)
    hub, count, most = R.hub_column(J, V)
    assert count == most == V                                                    # rank 0's column is the busiest: present in every row
    assert draws > 1.25 * (nnz - V) + 1024                                       # past a first range sized from M: later ranges merge


def test_model_does_not_depend_on_the_step():
    for V, rb, re_, nnz in SHAPES:
        a = R.model(V, rb, re_, nnz)
        for step in (1000, 777):
            b = R.model(V, rb, re_, nnz, 0xC0FFEE, step)
            assert a[3] == b[3] and all(x.tobytes() == y.tobytes() for x, y in zip(a[:3], b[:3]))


def test_model_refuses_what_the_budget_cannot_hold():
    with pytest.raises(R.TooDense):
        R.model(64, 0, 64, 4096)
    I, J, X, draws = R.model(64, 0, 64, 64)                                      # M = 0: the diagonal, no draw
    assert draws == 0 and np.array_equal(I, np.arange(64)) and np.array_equal(I, J) and np.all(X == np.float32(0.2))


def test_shards_share_the_relabelling():
    V = 1000
    a = R.model(V, 250, 500, 30000)
    b = R.model(V, 500, 750, 30000)
    for I, J, X, draws in (a, b):                                                # one relabelling: the same column is the hub of both
        hub, count, most = R.hub_column(J, V)
        assert count == most == 250
    assert R.sigma(0xC0FFEE, 250) != R.sigma(0xC0FFEE, 500)

"""CPU-only checks of the held-out evaluation section of include/geglove.h: the exported symbols, the split rule against a numpy
SplitMix64 model, the argument errors that need no device, the `device.holdout` key of the C++ host's bean, and the numpy model
of the evaluation (tests/eval_ref.py) against the oracle it restates."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest

from geglove import capi, synth
import oracle as O
import eval_ref as R

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32p, i32p, u8p = C.POINTER(C.c_float), C.POINTER(C.c_int32), C.POINTER(C.c_uint8)
T1 = 1.5 * 2.0 ** -32          # T = floor(1.5) = 1: only a zero high word is held out


def test_header_symbols_are_exported():
    header = open(os.path.join(REPO, "include", "geglove.h")).read()
    declared = set(re.findall(r"\b(ge_glove_eval_\w+|ge_eval_\w+|ge_holdout_\w+)\s*\(", header))
    assert declared == {"ge_glove_eval_create", "ge_glove_eval_run", "ge_eval_last_kernel_ms", "ge_eval_get", "ge_eval_destroy", "ge_holdout_mask"}
    L = capi.lib()
    for name in declared:
        assert name in capi.SYMBOLS and getattr(L, name) is not None


@pytest.mark.parametrize("fraction", [T1, 0.1, 0.5])
@pytest.mark.parametrize("n", [1, 1000, 100003])
def test_holdout_mask_equals_the_splitmix_model(n, fraction):
    for seed in (0, 42, 0xC0FFEE, 2 ** 64 - 1, -7):
        got = capi.holdout_mask(seed, n, fraction)
        want = R.holdout_mask(seed & 0xFFFFFFFFFFFFFFFF, n, fraction)
        assert got.dtype == np.uint8 and np.array_equal(got, want), (seed, n, fraction)
        assert set(np.unique(got)) <= {0, 1}


def test_holdout_threshold_is_the_floor_in_fp64():
    """T = floor(fraction * 2^32): with T = 1 exactly the draws whose high word is 0 are held; 0.5 holds the draws below 2^31."""
    n = 100003
    hi = synth.splitmix64(42 ^ R.HOLDOUT_SALT, n, 0) >> np.uint64(32)
    assert np.array_equal(capi.holdout_mask(42, n, T1), (hi == 0).astype(np.uint8))
    assert np.array_equal(capi.holdout_mask(42, n, 0.5), (hi < 2 ** 31).astype(np.uint8))
    assert math.floor(0.1 * 2.0 ** 32) == 429496729
    assert np.array_equal(capi.holdout_mask(42, n, 0.1), (hi < 429496729).astype(np.uint8))


def test_held_share_lies_within_five_sigma():
    n, F = 100003, 0.1
    p = math.floor(F * 2.0 ** 32) / 2.0 ** 32
    for seed in (1, 42, 0xC0FFEE):
        held = int(capi.holdout_mask(seed, n, F).sum())
        assert abs(held - n * p) <= 5.0 * math.sqrt(n * p * (1 - p)), (seed, held)


def test_a_nonzero_keeps_its_side_when_the_set_grows():
    """A function of (seed, k, fraction) alone: the first 1000 entries of a longer mask are the mask of 1000."""
    assert np.array_equal(capi.holdout_mask(9, 100003, 0.1)[:1000], capi.holdout_mask(9, 1000, 0.1))


def test_holdout_fraction_outside_its_range_is_refused():
    L = capi.lib()
    mask = np.full(8, 7, np.uint8)
    for bad in (0.0, 0.5000001, float("nan"), -0.1, 1.0, float("inf")):
        assert L.ge_holdout_mask(1, 8, bad, mask.ctypes.data_as(u8p)) == capi.GE_ERR_ARG, bad
        assert b"fraction" in L.ge_last_error()
        with pytest.raises(capi.GeError):
            capi.holdout_mask(1, 8, bad)
    assert np.all(mask == 7)                                          # nothing written
    assert L.ge_holdout_mask(1, 8, 0.25, None) == capi.GE_ERR_ARG
    assert L.ge_holdout_mask(1, -1, 0.25, mask.ctypes.data_as(u8p)) == capi.GE_ERR_ARG


def test_null_arguments_are_refused_without_a_device():
    L = capi.lib()
    ARG = capi.GE_ERR_ARG
    I = np.zeros(4, np.int32); J = np.zeros(4, np.int32); X = np.full(4, 0.1, np.float32)
    pI, pJ, pX = I.ctypes.data_as(i32p), J.ctypes.data_as(i32p), X.ctypes.data_as(f32p)
    h = C.c_void_p()
    assert L.ge_glove_eval_create(None, pI, pJ, pX, 4, C.byref(h)) == ARG and b"handle" in L.ge_last_error()
    assert L.ge_glove_eval_create(None, None, None, None, 4, C.byref(h)) == ARG
    assert L.ge_glove_eval_create(None, pI, pJ, pX, 4, None) == ARG
    assert h.value is None
    out = C.c_double(); ms = C.c_float()
    assert L.ge_glove_eval_run(None, None, None, C.byref(out)) == ARG
    assert L.ge_eval_last_kernel_ms(None, C.byref(ms)) == ARG
    assert L.ge_eval_get(None, None, None) == ARG
    L.ge_eval_destroy(None)                                           # harmless


def test_host_configuration_key(tmp_path):
    """`device: { holdout: F }` in the C++ host's bean, checked where the other errors are; the banner gains its line only when
    the key is set, and a multi-rank run refuses it."""
    capi._share_hip_runtime_with_torch()
    host = C.CDLL(os.path.join(REPO, "graph-embeddings_amd", "lib", "libgehost.so"))
    host.geh_config_summary.restype = C.c_char_p
    base = "graph: g.nt\nmethod: glove\ndim: 4\nbca:\n  alpha: 0.1\n  epsilon: 0.001\noutput:\n  uri: []\n"
    bad = "ERR\nInvalid configuration: Invalid device.holdout, choose a fraction from 0 to 0.5 (0 = off)"
    cases = {"": (None, None), "device:\n  holdout: 0\n": (None, None), "device:\n  holdout: 0.2\n": (None, "# Holdout: 0.2"),
             "device:\n  holdout: 0.5\n": (None, "# Holdout: 0.5"),
             "device:\n  holdout: 0.6\n": (bad, None), "device:\n  holdout: -0.1\n": (bad, None), "device:\n  holdout: 0.5000001\n": (bad, None),
             "device:\n  holdout: .nan\n": (bad, None),
             "device:\n  holdout: 0.2\n  gpus: 2\n": ("ERR\nInvalid configuration: device.holdout runs on one rank only, set device.gpus: 1", None)}
    for i, (extra, (err, line)) in enumerate(cases.items()):
        p = tmp_path / ("c%d.yml" % i)
        p.write_text(base + extra)
        out = host.geh_config_summary(str(p).encode(), 1).decode()
        if err:
            assert out == err, (extra, out)
        else:
            assert out.startswith("OK\n") and ("# Holdout" in out) == (line is not None) and (line is None or line in out.splitlines()), (extra, out)


# ------------------------------------------------------------------ the numpy model against the oracle it restates
def _trained_state(V, D, cost, opt, epochs=2):
    I, J, X, xmax = synth.synthetic_coo(V, 6 * V, seed=11)
    m = O.Glove(V, D, I, J, X, xmax, cost, seed=42, threads=1, opt=opt)
    for _ in range(epochs):
        m.epoch()
    return {k: np.array(v, np.float32) for k, v in m.state(full=opt != O.OPT_ADAGRAD).items()}, xmax


def eval_set(V, n, seed, rows=None):
    """Repeated rows and columns, one pair repeated 65 times (as far as n goes), X drawn as the parity tests draw it plus values
    past xmax (GloVe's w = 1 branch; still < 1 for pGloVe)."""
    lo, hi = rows if rows else (0, V)
    u = synth.splitmix64(seed, 3 * n)
    I = (lo + (u[:n] >> np.uint64(33)) % np.uint64(hi - lo)).astype(np.int32)
    J = ((u[n:2 * n] >> np.uint64(33)) % np.uint64(V)).astype(np.int32)
    I[5:70] = I[0]; J[5:70] = J[0]
    X = np.clip(np.power(10.0, -3.5 + synth._u01(u[2 * n:]) * 2.8), 1.0001e-4, 0.2).astype(np.float32)
    X[3::17] = np.float32(0.75)
    return I, J, X


@pytest.mark.parametrize("cost", [O.COST_GLOVE, O.COST_PGLOVE])
@pytest.mark.parametrize("D", [1, 3, 32, 33, 200])
def test_the_model_agrees_with_the_oracle(D, cost):
    V = 37
    state, xmax = _trained_state(V, D, cost, O.OPT_ADAGRAD)
    I, J, X = eval_set(V, 300, seed=D)
    _, term = R.model(state, D, I, J, X, xmax, cost)
    want = R.oracle_terms(state, V, D, I, J, X, xmax, cost)
    assert np.array_equal(R.bits32(term.astype(np.float32)), R.bits32(want))
    assert np.all(term >= 0) and np.any(term > 0)


def test_the_model_agrees_with_the_oracle_on_adam_states():
    V, D = 37, 31
    state, xmax = _trained_state(V, D, O.COST_GLOVE, O.OPT_ADAM)
    I, J, X = eval_set(V, 200, seed=5)
    _, term = R.model(state, D, I, J, X, xmax, O.COST_GLOVE)
    want = R.oracle_terms(state, V, D, I, J, X, xmax, O.COST_GLOVE, opt=O.OPT_ADAM, iteration=2)
    assert np.array_equal(R.bits32(term.astype(np.float32)), R.bits32(want))


def test_the_partitioned_sum_follows_its_partition():
    """S_b over [1024 b, 1024 (b + 1)) in ascending k, then the S_b in ascending b: at 2049 terms of mixed magnitude that is neither
    the plain left-to-right sum nor numpy's pairwise one, so the partition shows in the bits."""
    rng = np.random.default_rng(3)
    t = rng.random(2049) * 10.0 ** rng.integers(-8, 3, 2049)
    want, flat = 0.0, 0.0
    for b in range(3):
        sb = 0.0
        for v in t[1024 * b:1024 * (b + 1)]:
            sb += float(v)
            flat += float(v)
        want += sb
    assert R.partitioned_sum(t) == want
    assert R.partitioned_sum(t[:1]) == float(t[0]) and R.partitioned_sum(t[:1024]) == sum(float(v) for v in t[:1024])
    assert want != flat

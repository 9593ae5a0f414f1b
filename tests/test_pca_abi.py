"""CPU-only checks of the PCA section of include/geglove.h: the configuration struct, every argument error (before any device
work), and ge_pca_from_moments -- the host eigen solver, the sign rule, the k rule -- against numpy.linalg.eigh."""
import ctypes as C
import os
import subprocess
import time

import numpy as np
import pytest

from geglove import capi
import pca_ref as R

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32p, f64p = C.POINTER(C.c_float), C.POINTER(C.c_double)


def _cfg(**kw):
    cfg = capi.PcaCfg(); capi.lib().ge_pca_cfg_default(C.byref(cfg))
    for k, v in kw.items():
        setattr(cfg, k, v)
    return cfg


def test_cfg_size_and_defaults():
    src = '#include <stdio.h>\n#include "geglove.h"\nint main(){printf("%zu", sizeof(ge_pca_cfg));return 0;}'
    exe = os.path.join(REPO, "tests", ".probe_sizes_pca")
    subprocess.run(["gcc", "-x", "c", "-", "-I", os.path.join(REPO, "include"), "-o", exe], input=src.encode(), check=True)
    try:
        size = int(subprocess.check_output([exe]))
    finally:
        os.remove(exe)
    assert size == C.sizeof(capi.PcaCfg) == capi.lib().ge_pca_cfg_size()
    cfg = _cfg()
    assert (cfg.variance, cfg.max_components, cfg.device, cfg.stream) == (0.95, 0, 0, None)


def test_argument_errors_come_before_any_device_work():
    L = capi.lib()
    ARG = capi.GE_ERR_ARG
    rows = np.zeros((4, 3), np.float32); rp = rows.ctypes.data_as(f32p)
    mean = np.zeros(3); cov = np.eye(3)
    mp, cp = mean.ctypes.data_as(f64p), cov.ctypes.data_as(f64p)
    h = C.c_void_p()
    good = _cfg()
    # ge_pca_fit: null pointers, limits of n_rows / dim, variance outside (0, 1], a negative cap
    assert L.ge_pca_fit(None, 4, 3, C.byref(good), C.byref(h)) == ARG
    assert L.ge_pca_fit(rp, 4, 3, None, C.byref(h)) == ARG
    assert L.ge_pca_fit(rp, 4, 3, C.byref(good), None) == ARG
    assert L.ge_pca_fit(rp, 1, 3, C.byref(good), C.byref(h)) == ARG and b"at least 2" in L.ge_last_error()
    for dim in (0, -1, 1025):
        assert L.ge_pca_fit(rp, 4, dim, C.byref(good), C.byref(h)) == ARG and b"dim" in L.ge_last_error()
    for variance in (0.0, -0.5, 1.0000001, float("nan"), float("inf")):
        assert L.ge_pca_fit(rp, 4, 3, C.byref(_cfg(variance=variance)), C.byref(h)) == ARG and b"variance" in L.ge_last_error()
        assert L.ge_pca_from_moments(mp, cp, 3, 4, C.byref(_cfg(variance=variance)), C.byref(h)) == ARG
    assert L.ge_pca_fit(rp, 4, 3, C.byref(_cfg(max_components=-1)), C.byref(h)) == ARG
    # ge_pca_from_moments
    assert L.ge_pca_from_moments(None, cp, 3, 4, C.byref(good), C.byref(h)) == ARG
    assert L.ge_pca_from_moments(mp, None, 3, 4, C.byref(good), C.byref(h)) == ARG
    assert L.ge_pca_from_moments(mp, cp, 3, 4, None, C.byref(h)) == ARG
    assert L.ge_pca_from_moments(mp, cp, 3, 4, C.byref(good), None) == ARG
    assert L.ge_pca_from_moments(mp, cp, 3, 1, C.byref(good), C.byref(h)) == ARG
    assert L.ge_pca_from_moments(mp, cp, 0, 4, C.byref(good), C.byref(h)) == ARG
    assert L.ge_pca_from_moments(mp, cp, 1025, 4, C.byref(good), C.byref(h)) == ARG
    bad = cov.copy(); bad[1, 2] = np.nan
    assert L.ge_pca_from_moments(mp, bad.ctypes.data_as(f64p), 3, 4, C.byref(good), C.byref(h)) == ARG and b"non-finite input" in L.ge_last_error()
    badm = mean.copy(); badm[0] = np.inf
    assert L.ge_pca_from_moments(badm.ctypes.data_as(f64p), cp, 3, 4, C.byref(good), C.byref(h)) == ARG and b"non-finite input" in L.ge_last_error()
    assert h.value is None
    # the handle-taking calls
    assert L.ge_glove_pca_fit(None, C.byref(good), C.byref(h)) == ARG
    assert L.ge_pca_get(None, None, None, None, None, None, None, None) == ARG
    assert L.ge_pca_transform(None, rp, 4, rp) == ARG
    assert L.ge_glove_pca_transform(None, None, rp) == ARG
    assert L.ge_pca_last_kernel_ms(None, None, None) == ARG
    p = capi.Pca.from_moments(mean, cov, 4)
    assert L.ge_pca_transform(p._h, None, 4, rp) == ARG and L.ge_pca_transform(p._h, rp, 4, None) == ARG
    assert L.ge_pca_transform(p._h, rp, 0, rp) == ARG
    assert L.ge_glove_pca_transform(p._h, None, rp) == ARG
    assert L.ge_pca_get(p._h, None, None, None, None, None, None, None) == capi.GE_OK        # every out pointer may be NULL
    L.ge_pca_destroy(None)                                                                     # harmless


@pytest.mark.skipif(capi.lib().ge_device_count() > 0, reason="only meaningful on a box without a GPU")
def test_no_cpu_fallback_without_a_device():
    rows = np.arange(12, dtype=np.float32).reshape(4, 3) ** 2
    with pytest.raises(capi.GeError) as e:
        capi.Pca.fit(rows)
    assert e.value.status == capi.GE_ERR_HIP
    p = capi.Pca.from_moments(np.zeros(3), np.eye(3), 4)            # the host-only entry point needs no device ...
    with pytest.raises(capi.GeError) as e:
        p.transform(rows)                                           # ... the projection does
    assert e.value.status == capi.GE_ERR_HIP


def test_hand_cases():
    # identity: every direction is an eigenvector; eigenvalues 1, an orthonormal basis, largest entries positive
    D, k, n, mean, cov, lam, W = capi.Pca.from_moments(np.arange(4.0), np.eye(4), 9).get()
    assert (D, n) == (4, 9) and np.array_equal(lam, np.ones(4)) and np.array_equal(mean, np.arange(4.0)) and np.array_equal(cov, np.eye(4))
    assert np.allclose(W.T @ W, np.eye(4), atol=1e-15) and k == 4                       # 0.95 of 4 needs all four
    # diag(3, 1, 2): sorted descending, unit vectors e0, e2, e1
    D, k, n, mean, cov, lam, W = capi.Pca.from_moments(np.zeros(3), np.diag([3.0, 1.0, 2.0]), 5).get()
    assert np.array_equal(lam, [3.0, 2.0, 1.0]) and np.array_equal(W, np.eye(3)[:, [0, 2, 1]]) and k == 3
    # [[2, 1], [1, 2]]: 3 and 1, w0 = (1, 1) / sqrt 2, w1 = (1, -1) / sqrt 2 with the FIRST of the two equal magnitudes positive
    D, k, n, mean, cov, lam, W = capi.Pca.from_moments(np.zeros(2), np.array([[2.0, 1.0], [1.0, 2.0]]), 5, variance=0.7).get()
    assert np.allclose(lam, [3.0, 1.0], rtol=0, atol=4 * R.U64 * 3) and k == 1
    assert np.allclose(W, np.array([[1.0, 1.0], [1.0, -1.0]]) / np.sqrt(2), rtol=0, atol=4 * R.U64)
    # lambda = (2, 1, 1), variance 0.5: 2 >= 0.5 * 4, equality counts
    assert capi.Pca.from_moments(np.zeros(3), np.diag([1.0, 2.0, 1.0]), 5, variance=0.5).k == 1
    assert capi.Pca.from_moments(np.zeros(3), np.diag([1.0, 2.0, 1.0]), 5, variance=0.5000001).k == 2
    # variance 1 keeps everything; max_components caps; no variance at all keeps one
    assert capi.Pca.from_moments(np.zeros(3), np.diag([1.0, 2.0, 1.0]), 5, variance=1.0).k == 3
    assert capi.Pca.from_moments(np.zeros(3), np.diag([1.0, 2.0, 1.0]), 5, variance=1.0, max_components=2).k == 2
    assert capi.Pca.from_moments(np.zeros(3), np.diag([1.0, 2.0, 1.0]), 5, variance=0.5, max_components=2).k == 1
    D, k, n, mean, cov, lam, W = capi.Pca.from_moments(np.ones(3), np.zeros((3, 3)), 5).get()
    assert k == 1 and np.array_equal(lam, np.zeros(3)) and np.allclose(W.T @ W, np.eye(3), atol=1e-15)
    # negative rounding residue is clamped: a rank-1 matrix has eigenvalues (|v|^2, ~0, ~0), none below zero
    v = np.array([1.0, 1e-3, 1e-6, 0.3])
    lam = capi.Pca.from_moments(np.zeros(4), np.outer(v, v), 5).get()[5]
    assert np.all(lam >= 0) and lam[1] <= 4 * 2 * R.U64 * lam[0]


def test_sign_rule():
    for D in (2, 3, 50):
        C_ = R.spd(D)
        W = capi.Pca.from_moments(np.zeros(D), C_, 10).get()[6]
        big = np.argmax(np.abs(W), axis=0)                      # argmax returns the lowest index on a tie
        assert np.all(W[big, np.arange(D)] > 0)
    # a tie: columns (1, -1)/sqrt 2 and (1, 1)/sqrt 2 -- index 0 decides in both
    W = capi.Pca.from_moments(np.zeros(2), np.array([[2.0, -1.0], [-1.0, 2.0]]), 5).get()[6]
    assert W[0, 0] > 0 and W[1, 0] < 0 and W[0, 1] > 0 and W[1, 1] > 0


@pytest.mark.parametrize("D", [1, 2, 3, 50, 300, 1024])
def test_solver_against_lapack(D):
    """Residual and orthogonality, scaled by D * 2 u64 (* lambda_max): the library may use 8 x the larger of numpy's ratio and 1.
    Observed (library / numpy): residual 0.33 / 0.17 at D = 3, 0.0012 / 0.0014 at D = 1024; orthogonality 0.73 / 0.67 at D = 3,
    0.056 / 0.014 at D = 1024; the D = 1024 solve takes about 1.3 s on the host."""
    C_ = R.spd(D)
    t0 = time.time()
    p = capi.Pca.from_moments(np.zeros(D), C_, 10, variance=0.95)
    seconds = time.time() - t0
    _, k, _, _, cov, lam, W = p.get()
    assert np.array_equal(cov, C_)
    lam_np, W_np = R.eig_desc(C_)
    res, orth = R.solver_ratios(C_, lam, W)
    res_np, orth_np = R.solver_ratios(C_, lam_np, W_np)
    print("D %d: residual ratio %.4g (numpy %.4g), orthogonality ratio %.4g (numpy %.4g), host time %.3f s" % (D, res, res_np, orth, orth_np, seconds))
    assert np.all(np.diff(lam) <= 0) and np.all(lam >= 0)
    assert res <= 8 * max(res_np, 1.0) and orth <= 8 * max(orth_np, 1.0)
    assert np.max(np.abs(lam - lam_np)) <= 8 * D * 2 * R.U64 * lam_np[0]            # Weyl: a backward-stable solver moves no eigenvalue further
    assert R.share_margin(lam_np, R.k_rule(lam_np, 0.95)) >= 1e-4
    assert k == R.k_rule(lam_np, 0.95)


def test_host_views_are_per_handle():
    A, B = R.spd(5), R.spd(7)
    pa = capi.Pca.from_moments(np.arange(5.0), A, 10)
    f64pp = C.POINTER(C.c_double)
    comp = f64pp(); mean = f64pp()
    capi.check(capi.lib().ge_pca_get(pa._h, None, None, None, C.byref(mean), None, None, C.byref(comp)))
    before = np.ctypeslib.as_array(comp, shape=(5, 5)).copy()
    pb = capi.Pca.from_moments(np.zeros(7), B, 10)
    pb.get()
    assert np.array_equal(np.ctypeslib.as_array(comp, shape=(5, 5)), before)        # the same memory, unchanged
    assert np.array_equal(np.ctypeslib.as_array(mean, shape=(5,)), np.arange(5.0))
    assert np.array_equal(pa.get()[6], before)


def test_host_configuration_key(tmp_path):
    """`device: { pca: off | apply }` in the C++ host's bean: apply needs the `pca:` block, checked where the other errors are."""
    capi._share_hip_runtime_with_torch()
    host = C.CDLL(os.path.join(REPO, "graph-embeddings_amd", "lib", "libgehost.so"))
    host.geh_config_summary.restype = C.c_char_p
    base = "graph: g.nt\nmethod: glove\ndim: 4\nbca:\n  alpha: 0.1\n  epsilon: 0.001\noutput:\n  uri: []\n"
    cases = {"device:\n  pca: apply\n": "ERR\nInvalid configuration: device.pca: apply needs a pca block with a variance",
             "pca:\n  variance: 0.9\ndevice:\n  pca: apply\n": "OK",
             "pca:\n  variance: 0.9\ndevice:\n  pca: off\n": "OK",
             "pca:\n  variance: 0.9\n": "OK",
             "pca:\n  variance: 1.5\ndevice:\n  pca: apply\n": "ERR\nInvalid configuration: Invalid PCA parameters, variance must lie in (0, 1]",
             "pca:\n  variance: 1.5\n": "OK",                       # a block nobody applies stays as tolerated as it was
             "pca:\n  variance: 0.9\ndevice:\n  pca: whiten\n": "ERR\nInvalid configuration: Invalid device.pca, choose one of: off, apply"}
    for k, (extra, want) in enumerate(cases.items()):
        p = tmp_path / ("c%d.yml" % k)
        p.write_text(base + extra)
        out = host.geh_config_summary(str(p).encode(), 1).decode()
        assert out == want or (want == "OK" and out.startswith("OK\n")), (extra, out)
        if want == "OK":
            assert "name=g_glove_exact_undirected_0.1_0.001_adagrad_pca_4" in out.splitlines()      # the file name does not know the key

"""CPU-only checks of GE_MODE_STRATIFIED: the ABI (struct sizes, argument errors before any device work), the numpy model of the
schedule (tests/strata_ref.py) on the matrices the GPU tests use, and the two hosts' YAML keys."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import geglove
from geglove import capi, synth
import strata_ref as S

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(REPO, "tests", "golden")
PS = [1, 2, 7, 16, 64]
# synthetic_coo(300, 4000, seed=9): 3 366 nonzeros after de-duplication, busiest column 258 -- wider than N / 64
PATHS_300 = {7: (617, 480, 49, 7), 16: (392, 210, 256, 16), 64: (317, 52, 1914, 52)}      # P -> (path, N // P, tiles used, column blocks used)


def _matrices():
    return {"zipf300": synth.synthetic_coo(300, 4000, seed=9), "zipf90": synth.synthetic_coo(90, 2500, seed=17)}


def test_struct_sizes_match_their_mirrors():
    L = capi.lib()
    assert L.ge_glove_cfg_size() == C.sizeof(capi.GloveCfg)
    assert L.ge_glove_info_size() == C.sizeof(capi.GloveInfo)
    # and the header itself (a C compiler is the authority on its layout)
    src = ('#include <stdio.h>\n#include <stddef.h>\n#include "geglove.h"\nint main(){printf("%zu %zu %zu %zu %zu %d", sizeof(ge_glove_cfg), '
           'sizeof(ge_glove_info), offsetof(ge_glove_cfg, strata), offsetof(ge_glove_info, strata), offsetof(ge_glove_info, strata_path), '
           '(int)GE_MODE_STRATIFIED);return 0;}')
    exe = os.path.join(REPO, "tests", ".probe_sizes_strata")
    subprocess.run(["gcc", "-x", "c", "-", "-I", os.path.join(REPO, "include"), "-o", exe], input=src.encode(), check=True)
    try:
        got = [int(x) for x in subprocess.check_output([exe]).split()]
    finally:
        os.remove(exe)
    assert got == [C.sizeof(capi.GloveCfg), C.sizeof(capi.GloveInfo), capi.GloveCfg.strata.offset, capi.GloveInfo.strata.offset,
                   capi.GloveInfo.strata_path.offset, capi.GE_MODE_STRATIFIED]
    # appended: every older field keeps its place
    assert capi.GloveCfg._fields_[-1][0] == "strata" and [f for f, _ in capi.GloveInfo._fields_[-2:]] == ["strata", "strata_path"]
    cfg = capi.GloveCfg(); cfg.strata = 7
    L.ge_glove_cfg_default(C.byref(cfg))
    assert cfg.strata == 0 and cfg.mode == capi.GE_MODE_HOGWILD


def _create_status(**fields):
    I = np.array([0, 1, 2], np.int32); J = np.array([1, 2, 0], np.int32); X = np.array([0.1, 0.15, 0.05], np.float32)
    cfg = capi.GloveCfg(); capi.lib().ge_glove_cfg_default(C.byref(cfg))
    cfg.vocab_size, cfg.dim, cfg.nnz, cfg.xmax = 3, 4, 3, 0.2
    cfg.device = 1 << 20                      # no such device: a call that got past the argument checks fails at selecting it
    for k, v in fields.items():
        setattr(cfg, k, v)
    h = C.c_void_p()
    i32p, f32p = C.POINTER(C.c_int32), C.POINTER(C.c_float)
    st = capi.lib().ge_glove_create(C.byref(cfg), I.ctypes.data_as(i32p), J.ctypes.data_as(i32p), X.ctypes.data_as(f32p), C.byref(h))
    assert not h.value
    return st, capi.lib().ge_last_error().decode()


def test_argument_errors_come_before_any_device_work():
    strat = dict(mode=capi.GE_MODE_STRATIFIED, shuffle=capi.GE_SHUFFLE_DEVICE)
    for bad in (-1, 2049, 1 << 20):
        st, msg = _create_status(strata=bad, **strat)
        assert st == capi.GE_ERR_ARG and "strata" in msg, (bad, st, msg)
    for mode, shuffle in ((capi.GE_MODE_HOGWILD, capi.GE_SHUFFLE_DEVICE), (capi.GE_MODE_DETERMINISTIC, capi.GE_SHUFFLE_JAVA)):
        st, msg = _create_status(strata=4, mode=mode, shuffle=shuffle)
        assert st == capi.GE_ERR_ARG and "GE_MODE_STRATIFIED" in msg, (mode, st, msg)
    st, msg = _create_status(strata=4, mode=capi.GE_MODE_STRATIFIED, shuffle=capi.GE_SHUFFLE_JAVA)
    assert st == capi.GE_ERR_ARG and "Fisher-Yates" in msg, (st, msg)
    st, msg = _create_status(strata=4, emb_dtype=capi.GE_DTYPE_BF16, **strat)
    assert st == capi.GE_ERR_ARG and "bf16" in msg, (st, msg)
    st, msg = _create_status(mode=3, shuffle=capi.GE_SHUFFLE_DEVICE)
    assert st == capi.GE_ERR_ARG and "invalid mode" in msg
    # the valid forms pass the argument checks and fail only for want of the device
    for P in (0, 1, 4, 2048):
        for shuffle in (capi.GE_SHUFFLE_DEVICE, capi.GE_SHUFFLE_NONE):
            st, msg = _create_status(strata=P, mode=capi.GE_MODE_STRATIFIED, shuffle=shuffle)
            assert _no_such_device(st, msg), (P, shuffle, st, msg)


def _no_such_device(status, message):
    """Without a GPU every device is GE_ERR_HIP; with one, ordinal 2^20 is out of range."""
    return status == capi.GE_ERR_HIP or (status == capi.GE_ERR_ARG and "out of range [0," in message)


@pytest.mark.parametrize("name", ["zipf300", "zipf90"])
@pytest.mark.parametrize("P", PS)
def test_model_sub_epochs_are_conflict_free_and_cover_the_matrix(name, P):
    I, J, X, xmax = _matrices()[name]
    m = S.Model(I, J, P)
    seen = np.zeros(len(I), np.int64)
    for s in range(P):
        rows, cols = [], []
        for T, nz in m.sub_epoch(s):
            seen[nz] += 1
            assert np.all(np.diff(nz) > 0)                               # matrix order inside a tile
            rows.append(np.unique(I[nz])); cols.append(np.unique(J[nz]))
        allr, allc = np.concatenate(rows), np.concatenate(cols)
        assert len(np.unique(allr)) == len(allr), (s, "two tiles of a sub-epoch share a focus row")
        assert len(np.unique(allc)) == len(allc), (s, "two tiles of a sub-epoch share a context row")
    assert np.all(seen == 1)
    # blocks are contiguous id ranges, balanced by nonzero count
    rb, cb = S.partition(I, J, P)
    for ids, blk in ((I, rb), (J, cb)):
        order = np.argsort(ids, kind="stable")
        assert np.all(np.diff(blk[order]) >= 0)
    for shuffle in (S.SHUFFLE_NONE, S.SHUFFLE_DEVICE):
        for it in range(2):
            assert np.array_equal(np.sort(m.epoch_order(11, it, shuffle)), np.arange(len(I)))
    assert not np.array_equal(m.epoch_order(11, 0, S.SHUFFLE_DEVICE), m.epoch_order(11, 1, S.SHUFFLE_DEVICE)) or len(I) < 2
    assert m.path >= max(m.counts.sum(axis=0).max(), m.counts.sum(axis=1).max())      # the busiest column block / row block


def test_model_reproduces_the_quoted_schedule():
    I, J, X, xmax = _matrices()["zipf300"]
    assert len(I) == 3366 and np.bincount(J).max() == 258
    for P, (path, ideal, used, colblocks) in PATHS_300.items():
        m = S.Model(I, J, P)
        assert (m.path, len(I) // P, int((m.counts > 0).sum()), len(np.unique(S.partition(I, J, P)[1]))) == (path, ideal, used, colblocks)
    assert S.Model(I, J, 1).path == len(I)
    assert np.bincount(J).max() > len(I) // 64          # the hub column is wider than a block at P = 64: it sets the floor by itself
    assert S.Model(I, J, 64).path >= 258


def test_bijections_are_bijections_and_keyed():
    for n in (1, 2, 3, 7, 64, 65, 1000):
        a = S.bijection(n, S.keys(5, 0, 3)); b = S.bijection(n, S.keys(5, 1, 3)); c = S.bijection(n, S.keys(5, 0, 4))
        for x in (a, b, c):
            assert np.array_equal(np.sort(x), np.arange(n))
        if n >= 64:
            assert not np.array_equal(a, b) and not np.array_equal(a, c)


def test_default_p_is_a_function_of_rows_and_nnz():
    assert S.default_p(300, 3366) == 16 and S.default_p(10, 3366) == 8 and S.default_p(1, 0) == 1 and S.default_p(300, 0) == 1
    assert S.default_p(100000, 10_000_000) == 1024 and S.default_p(1 << 20, 1 << 31) == 2048


# ---------------------------------------------------------------- YAML keys in both hosts
YAML = ("graph: g.nt\nmethod: glove\ndim: 4\nbca:\n  alpha: 0.1\n  epsilon: 0.001\noutput:\n  uri: []\n"
        "device:\n  mode: stratified\n  strata: %d\n  shuffle: %s\n")


@pytest.fixture(scope="module")
def host():
    capi._share_hip_runtime_with_torch()
    L = C.CDLL(os.environ.get("GE_HOST_LIB") or os.path.join(REPO, "graph-embeddings_amd", "lib", "libgehost.so"))
    L.geh_config_summary.restype = C.c_char_p
    return L


def test_yaml_keys_parse_in_both_hosts(host, tmp_path):
    good = tmp_path / "strat.yml"; good.write_text(YAML % (4, "device"))
    out = host.geh_config_summary(str(good).encode(), 1).decode().splitlines()
    assert out[0] == "OK" and "# Stratified trainer: 4 strata" in out
    auto = tmp_path / "auto.yml"; auto.write_text(YAML % (0, "none"))
    out = host.geh_config_summary(str(auto).encode(), 1).decode().splitlines()
    assert out[0] == "OK" and "# Stratified trainer: strata chosen from the matrix" in out
    java = tmp_path / "java.yml"; java.write_text(YAML % (4, "java"))
    out = host.geh_config_summary(str(java).encode(), 1).decode()
    assert out.startswith("ERR\nInvalid configuration:") and "stratified" in out and "java" in out
    wide = tmp_path / "wide.yml"; wide.write_text(YAML % (4096, "device"))
    assert host.geh_config_summary(str(wide).encode(), 1).decode().startswith("ERR\nInvalid configuration: Invalid device.strata")
    other = tmp_path / "other.yml"; other.write_text((YAML % (4, "device")).replace("stratified", "hogwild"))
    assert "device.strata needs device.mode: stratified" in host.geh_config_summary(str(other).encode(), 1).decode()
    # a configuration without the block keeps its banner
    tiny = host.geh_config_summary(os.path.join(GOLD, "tiny.config.yml").encode(), 1).decode()
    assert tiny.startswith("OK") and "Stratified" not in tiny
    # the Python host: the same two keys reach ge_glove_cfg
    py = geglove.Configuration.load(str(good))
    assert py.device["mode"] == "stratified" and py.device["strata"] == 4
    assert geglove.host._MODES["stratified"] == capi.GE_MODE_STRATIFIED
    m = geglove.CooMatrix(3, [0, 1], [1, 2], [0.1, 0.1], 0.2)
    for dev, what in ((dict(py.device, id=1 << 20), None), (dict(py.device, id=1 << 20, strata=4096), "strata must lie in"),
                      (dict(py.device, id=1 << 20, shuffle="java"), "Fisher-Yates")):
        cfg = geglove.Configuration(dict(graph="g", method="glove", dim=4, threads=1, bca={"alpha": .1, "epsilon": 1e-3},
                                         opt={"maxiter": 1}, output={"uri": []}, device=dev))
        with pytest.raises(geglove.GeError) as e:
            geglove.Adagrad(m, cfg, cfg.costFunction())
        if what is None:
            assert _no_such_device(e.value.status, str(e.value)), (dev, str(e.value))
        else:
            assert e.value.status == capi.GE_ERR_ARG and what in str(e.value), (dev, str(e.value))

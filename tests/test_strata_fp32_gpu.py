"""GE_ARITH_FP32 on the device: k_strata_fp32 held word for word to the numpy model of the arithmetic (tests/strata_fp32_ref.py)
walking the sequential order the header defines (tests/strata_ref.py).

Every comparison is exact: np.array_equal on all tables (8, or 12 with moments) and == on the cost, after every epoch.  The
model's only transcendental steps are the fp64 log / pow of the cost terms, and tests/test_strata_gpu.py shows the device's equal
glibc's bit for bit on these matrices, so there is no tolerance to state.  The matrices are the hub-heavy ones of that file: any
overlap between concurrent tiles loses an update and breaks the equality, so the exactness test is the race test; and a prefetched
row that missed a store, or a forwarded row that was loaded again too early, breaks it inside one tile."""
import os
import subprocess

import numpy as np
import pytest

import geglove
from geglove import capi, synth
import kernel_model as KM
import oracle as O
import strata_ref as S
import strata_fp32_ref as R
from helpers import make_config, cost_kind

pytestmark = pytest.mark.gpu
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(REPO, "graph-embeddings_amd", "bin", "geglove")
SEED = 5

_MATRICES = {}


def _matrix(name):
    if name not in _MATRICES:
        V, N, seed = {"zipf300": (300, 4000, 9), "zipf90": (90, 2500, 17)}[name]
        I, J, X, xmax = synth.synthetic_coo(V, N, seed=seed)
        _MATRICES[name] = (V, I, J, X, xmax)
    return _MATRICES[name]


def _create(V, I, J, X, xmax, D, method="glove", opt="adagrad", **device):
    cfg = make_config(D, method, opt=opt, **device)
    return geglove.createOptimizer(cfg, geglove.CooMatrix(V, I, J, X, xmax))


def _as2d(st, V, D):
    return {k: np.ascontiguousarray(v if "bias" in k else v.reshape(V, D), np.float32) for k, v in st.items()}


def _same_tables(got, ref, what):
    assert set(got) == set(ref)
    for name in ref:
        bad = np.count_nonzero(got[name].view(np.uint32) != ref[name].view(np.uint32))
        assert np.array_equal(got[name], ref[name]) and bad == 0, "%s: table %s differs in %d words" % (what, name, bad)


def _replay(V, I, J, X, xmax, D, method, P, shuffle, epochs=2, opt="adagrad", seed=SEED):
    """`epochs` fp32 stratified epochs against the model walking the tiles one after another: order, all tables, cost."""
    dev = _create(V, I, J, X, xmax, D, method, opt=opt, mode="stratified", arith="fp32", strata=P, shuffle=shuffle, seed=seed)
    try:
        assert dev.get_arith() == capi.GE_ARITH_FP32
        model = S.Model(I, J, P)
        info = dev.info()
        assert (info["strata"], info["strata_path"]) == (P, model.path)
        ref = _as2d(dev.state(), V, D)
        assert len(ref) == (8 if opt == "adagrad" else 12)
        for it in range(epochs):
            assert np.array_equal(dev.epoch_order(it).astype(np.int64), model.epoch_order(seed, it, shuffle)), (it, "epoch_order")
            cost = dev.epoch(it)
            assert dev.last_kernel_ms()[1] == model.launches() <= P
            want = R.epoch(model, seed, it, shuffle, opt, D, I, J, X, xmax, ref, pglove=method == "pglove")
            _same_tables(_as2d(dev.state(), V, D), ref, "P=%d %s D=%d %s %s epoch %d" % (P, shuffle, D, method, opt, it))
            assert cost == want, ("cost_sum", it, cost, want)
    finally:
        dev.close()


# ------------------------------------------------------------------ 1. race and replay
@pytest.mark.parametrize("shuffle", ["none", "device"])
@pytest.mark.parametrize("P", [1, 7, 64])
@pytest.mark.parametrize("D", [3, 50, 200, 300])
@pytest.mark.parametrize("method", ["glove", "pglove"])
@pytest.mark.parametrize("name", ["zipf300", "zipf90"])
def test_fp32_epochs_equal_the_model_word_for_word(gpu, name, method, D, P, shuffle):
    V, I, J, X, xmax = _matrix(name)
    if name == "zipf300":
        assert np.bincount(J).max() == 258           # the hub column: wider than a block at P = 64
    _replay(V, I, J, X, xmax, D, method, P, shuffle)


# ------------------------------------------------------------------ 2. Adam and AMSGrad
@pytest.mark.parametrize("D", [52, 300])
@pytest.mark.parametrize("opt", ["adam", "amsgrad"])
def test_fp32_adam_amsgrad_equal_the_model(gpu, opt, D):
    V, I, J, X, xmax = _matrix("zipf90")
    _replay(V, I, J, X, xmax, D, "pglove", 7, "device", opt=opt)


# ------------------------------------------------------------------ 3. every lane shape
@pytest.mark.parametrize("D", KM.SHAPE_TABLE_DIMS)
def test_every_lane_shape_equals_the_model(gpu, D):
    V, I, J, X, xmax = _matrix("zipf90")
    _replay(V, I, J, X, xmax, D, "glove", 7, "device", epochs=1)


# ------------------------------------------------------------------ 4. forwarding and prefetch: designed orders
def _values(n, seed):
    return (0.01 + 0.19 * np.random.default_rng(seed).random(n)).astype(np.float32)        # 0 < x <= 0.2: valid for both costs


def _coo(V, pairs, seed, keep_order=True):
    """The nonzeros in the caller's order (a tile keeps it: matrix order inside a tile), or sorted as tests/test_strata_gpu.py has them."""
    pairs = list(dict.fromkeys(pairs)) if keep_order else sorted(set(pairs))
    I = np.array([p[0] for p in pairs], np.int32); J = np.array([p[1] for p in pairs], np.int32)
    return V, I, J, _values(len(pairs), seed), float(np.float32(0.2))


def _hub_column():
    """one column holds half of the nonzeros"""
    rng = np.random.default_rng(3)
    rest = {(int(a), int(b)) for a, b in zip(rng.integers(0, 220, 400), rng.integers(0, 220, 400)) if b != 5}
    rest = sorted(rest)[:200]
    return _coo(220, [(i, 5) for i in range(200)] + rest, 1, keep_order=False)


def _interleave():
    """(A,1),(B,1),(A,2),(B,2),...: the column repeats at once, the row returns two steps back -- after its store, before the
    prefetch that follows it has been consumed"""
    A, B = 2, 7
    return _coo(24, [(r, c) for c in range(1, 21) for r in (A, B)], 12)


DESIGNED = {
    # name: (matrix, the P values it runs at)
    "one_row_40_columns": (lambda: _coo(40, [(3, (7 * j) % 40) for j in range(40)], 10), (1, 4)),
    "one_column_40_rows": (lambda: _coo(40, [((11 * i) % 40, 5) for i in range(40)], 11), (1, 4)),
    "interleave": (_interleave, (1, 4)),
    "diagonal": (lambda: _coo(30, [((7 * i) % 30, (7 * i) % 30) for i in range(30)], 6), (1, 4)),
    "N_is_1": (lambda: _coo(9, [(4, 6)], 13), (1, 4)),
    "tile_of_exactly_2": (lambda: _coo(9, [(4, 6), (2, 6)], 14), (1, 4)),
    "N_below_P": (lambda: _coo(30, [(1, 2), (4, 9), (9, 4), (20, 20), (29, 0)], 3, keep_order=False), (16,)),
    "empty_ends": (lambda: _coo(50, [(10 + (7 * k) % 30, 10 + (11 * k) % 30) for k in range(120)], 5, keep_order=False), (7,)),
    "hub_column_half_P16": (_hub_column, (16,)),
}


@pytest.mark.parametrize("shuffle", ["none", "device"])
@pytest.mark.parametrize("D", [6, 200])
@pytest.mark.parametrize("name", sorted(DESIGNED))
def test_designed_orders_equal_the_model(gpu, name, D, shuffle):
    make, Ps = DESIGNED[name]
    V, I, J, X, xmax = make()
    if name == "one_row_40_columns":
        assert len(I) == 40 and len(set(I)) == 1 and not np.all(np.diff(J) > 0)        # caller order, not sorted
    if name == "one_column_40_rows":
        assert len(I) == 40 and len(set(J)) == 1 and not np.all(np.diff(I) > 0)
    if name == "interleave":
        assert np.array_equal(I[:4], [2, 7, 2, 7]) and np.array_equal(J[:4], [1, 1, 2, 2])
    if name == "tile_of_exactly_2":
        assert S.Model(I, J, 1).counts.max() == 2
    if name == "N_below_P":
        assert len(I) < Ps[0]
    if name == "hub_column_half_P16":
        assert np.bincount(J).max() * 2 == len(I)
    for P in Ps:
        for method in ("glove", "pglove"):
            _replay(V, I, J, X, xmax, D, method, P, shuffle)


def test_without_prefetch_and_without_forwarding_the_bytes_are_the_same(gpu, monkeypatch):
    """GE_STRATA_FP32_ABLATE (what the measuring tool switches): neither the prefetch nor the forwarding is part of the result."""
    V, I, J, X, xmax = _interleave()
    runs = []
    for ablate in (None, "1", "2"):
        if ablate is None:
            monkeypatch.delenv("GE_STRATA_FP32_ABLATE", raising=False)
        else:
            monkeypatch.setenv("GE_STRATA_FP32_ABLATE", ablate)
        dev = _create(V, I, J, X, xmax, 200, "glove", mode="stratified", arith="fp32", strata=1, shuffle="none", seed=SEED)
        costs = [dev.epoch(it) for it in range(2)]
        runs.append((costs, dev.state()))
        dev.close()
    for costs, st in runs[1:]:
        assert costs == runs[0][0]
        for name in st:
            assert st[name].tobytes() == runs[0][1][name].tobytes(), name


# ------------------------------------------------------------------ 5. switching and repeatability
def test_switching_between_epochs_chains_oracle_model_oracle(gpu):
    V, I, J, X, xmax = _matrix("zipf90")
    D, P, method = 50, 7, "glove"
    dev = _create(V, I, J, X, xmax, D, method, mode="stratified", strata=P, shuffle="device", seed=SEED)
    model = S.Model(I, J, P)
    ref = _as2d(dev.state(), V, D)
    assert dev.get_arith() == capi.GE_ARITH_JAVA                  # the default
    for it, arith in enumerate(("java", "fp32", "java")):
        dev.set_arith(arith)
        assert dev.get_arith() == geglove.host._ARITH[arith]
        cost = dev.epoch(it)
        if arith == "java":
            want = 0.0
            for nz in model.jobs(SEED, it, "device"):
                if len(nz):
                    want += float(O.adagrad_job(D, I[nz], J[nz], X[nz], xmax, cost_kind(method), ref))
        else:
            want = R.epoch(model, SEED, it, "device", "adagrad", D, I, J, X, xmax, ref)
        _same_tables(_as2d(dev.state(), V, D), ref, "epoch %d (%s)" % (it, arith))
        assert cost == want, (it, arith, cost, want)
    dev.close()


def test_two_fresh_fp32_handles_give_equal_bytes(gpu):
    V, I, J, X, xmax = _matrix("zipf300")
    runs = []
    for _ in range(2):
        dev = _create(V, I, J, X, xmax, 50, "glove", mode="stratified", arith="fp32", strata=16, shuffle="device", seed=SEED)
        assert dev.get_arith() == capi.GE_ARITH_FP32
        costs = [dev.epoch(it) for it in range(3)]
        runs.append((costs, dev.state(), dev.extractResultF32()))
        dev.close()
    (c0, s0, x0), (c1, s1, x1) = runs
    assert c0 == c1 and x0.tobytes() == x1.tobytes()
    for name in s0:
        assert s0[name].tobytes() == s1[name].tobytes(), name
    # and the java arithmetic is another function of the same input
    dev = _create(V, I, J, X, xmax, 50, "glove", mode="stratified", strata=16, shuffle="device", seed=SEED)
    assert dev.get_arith() == capi.GE_ARITH_JAVA
    assert [dev.epoch(it) for it in range(3)] != c0
    dev.close()


# ------------------------------------------------------------------ 6. errors
def test_set_arith_is_for_stratified_handles_and_known_values(gpu):
    V, I, J, X, xmax = _matrix("zipf90")
    for device in (dict(mode="hogwild", shuffle="device"), dict(mode="deterministic", shuffle="none")):
        dev = _create(V, I, J, X, xmax, 8, "glove", seed=SEED, **device)
        for arith in (capi.GE_ARITH_FP32, capi.GE_ARITH_JAVA):
            with pytest.raises(capi.GeError) as e:
                dev.set_arith(arith)
            assert e.value.status == capi.GE_ERR_STATE, str(e.value)
        assert dev.get_arith() == capi.GE_ARITH_JAVA
        dev.close()
    dev = _create(V, I, J, X, xmax, 8, "glove", mode="stratified", strata=4, shuffle="device", seed=SEED)
    for bad in (2, -1, 7):
        with pytest.raises(capi.GeError) as e:
            dev.set_arith(bad)
        assert e.value.status == capi.GE_ERR_ARG and "arith" in str(e.value)
    assert dev.get_arith() == capi.GE_ARITH_JAVA
    dev.close()
    # a dim without a lane shape: five chunks of 64 lanes
    dev = _create(V, I, J, X, xmax, 1028, "glove", mode="stratified", strata=4, shuffle="device", seed=SEED)
    with pytest.raises(capi.GeError) as e:
        dev.set_arith("fp32")
    assert e.value.status == capi.GE_ERR_ARG and "dim = 1028" in str(e.value)
    assert dev.get_arith() == capi.GE_ARITH_JAVA
    dev.close()


def test_the_empty_matrix_costs_nothing_and_launches_nothing(gpu):
    V, D = 12, 5
    e = np.zeros(0, np.int32)
    dev = _create(V, e, e, np.zeros(0, np.float32), 0.2, D, "glove", mode="stratified", arith="fp32", strata=4, shuffle="device", seed=SEED)
    before = dev.state()
    assert dev.get_arith() == capi.GE_ARITH_FP32
    assert dev.epoch(0) == 0.0 and dev.last_kernel_ms()[1] == 0
    after = dev.state()
    for name in before:
        assert before[name].tobytes() == after[name].tobytes(), name
    dev.close()


# ------------------------------------------------------------------ 7. shards
def test_a_row_sharded_handle_equals_the_model_on_its_shard(gpu):
    V, I, J, X, xmax = _matrix("zipf300")
    rb, re = 100, 220
    keep = (I >= rb) & (I < re)
    Ik, Jk, Xk = I[keep], J[keep], X[keep]
    D, P = 6, 7
    dev = _create(V, Ik, Jk, Xk, xmax, D, "glove", mode="stratified", arith="fp32", strata=P, shuffle="device", seed=SEED, row_range=(rb, re))
    model = S.Model(Ik, Jk, P)
    assert dev.info()["strata_path"] == model.path
    st = dev.state()
    ref = {}
    for k, v in st.items():                            # the model indexes by global row id: rows outside the shard are never touched
        wide = v.size in (V * D, (re - rb) * D)
        full = np.ones((V, D) if wide else V, np.float32)
        if k in R.FOCUS_SIDE:
            full[rb:re] = v.reshape(re - rb, -1) if wide else v
        else:
            full = v.reshape(full.shape).copy()
        ref[k] = np.ascontiguousarray(full, np.float32)
    cost = dev.epoch(0)
    assert np.array_equal(dev.epoch_order(0), model.epoch_order(SEED, 0, "device"))
    want = R.epoch(model, SEED, 0, "device", "adagrad", D, Ik, Jk, Xk, xmax, ref)
    for k, v in dev.state().items():
        w = ref[k][rb:re] if k in R.FOCUS_SIDE else ref[k]
        assert np.array_equal(v.reshape(w.shape), w), k
    assert cost == want
    dev.close()


# ------------------------------------------------------------------ 8. CLI
def test_cli_fp32_runs_are_byte_identical_and_differ_from_java(gpu, tmp_path):
    assert os.path.exists(EXE), "host CLI not built"
    base = open(os.path.join(REPO, "tests", "golden", "tiny.config.yml")).read()
    old = "  mode: deterministic\n  shuffle: java\n"
    assert old in base
    name = "tiny_pglove_partial_directed_0.1_0.001_adagrad_pca_8"
    outs = {}
    for run, arith in (("a", "fp32"), ("b", "fp32"), ("j", "java")):
        cwd = tmp_path / run
        os.makedirs(cwd / "tests" / "golden")
        (cwd / "tests" / "golden" / "tiny.nt").write_bytes(open(os.path.join(REPO, "tests", "golden", "tiny.nt"), "rb").read())
        (cwd / "strat.yml").write_text(base.replace(old, "  mode: stratified\n  arith: %s\n  strata: 4\n  shuffle: device\n" % arith))
        r = subprocess.run([EXE, "-c", "strat.yml"], cwd=cwd, capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, r.stderr + r.stdout
        assert ("stratified: P = 4, strata_path / N = " in r.stdout) and (", arithmetic: %s" % arith in r.stdout)
        outs[run] = (cwd / "out" / (name + ".vectors.tsv")).read_bytes()
    assert outs["a"] == outs["b"]
    for run in "abj":
        assert b"# Stratified trainer: 4 strata\n" in outs[run]
        assert (b"# Stratified arithmetic: fp32\n" in outs[run]) == (run != "j")
    # the java run's file is another file: it lacks the arithmetic's line.  (Its three vectors read the same at the seven digits
    # the writer prints: three epochs on this graph move the two arithmetics apart by fp32 round-off only.  That the fp32 kernel ran
    # is what the handle reports in the log line above.)
    assert outs["a"] != outs["j"]
    body = [l for l in outs["a"].decode().splitlines() if not l.startswith("#") and "\t" in l]
    assert len(body) == 3 and all(np.isfinite([float(x) for x in l.split("\t")]).all() for l in body)
    # fp32 outside the stratified mode is refused by the bean check
    bad = tmp_path / "bad.yml"; bad.write_text(base.replace(old, old + "  arith: fp32\n"))
    r = subprocess.run([EXE, "-c", str(bad)], cwd=tmp_path, capture_output=True, text=True, timeout=120)
    assert r.returncode == 1 and "Invalid configuration: device.arith: fp32 needs device.mode: stratified" in r.stderr

"""GE_MODE_STRATIFIED on the device: P wavefronts at once, held bit for bit to the oracle replaying the sequential order the
header defines (tests/strata_ref.py restates it in numpy).

The matrices are small and hub-heavy (synthetic_coo(300, 4000, seed=9): 3 366 nonzeros, one column with 258 of them; at P = 64
that column is wider than a block), so any overlap between concurrent tiles -- a shared focus row or context row -- loses an
update and breaks the bit equality: the exactness test is the race test.  Every comparison here is exact (np.array_equal on
all tables, == on the cost); there is no tolerance to state."""
import os
import subprocess

import numpy as np
import pytest

import geglove
from geglove import capi, synth
import oracle as O
import strata_ref as S
from helpers import make_config, cost_kind, OPT_KIND

pytestmark = pytest.mark.gpu
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(REPO, "graph-embeddings_amd", "bin", "geglove")
SEED = 5
PS = [1, 2, 7, 16, 64]
DIMS = [3, 50, 200, 300]

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
    return {k: np.ascontiguousarray(v.reshape(V, -1) if v.size == V * D else v, np.float32) for k, v in st.items()}


def _replay_exact(V, I, J, X, xmax, D, method, P, shuffle, epochs=3, opt="adagrad", seed=SEED):
    """`epochs` stratified epochs against the oracle walking the model's tiles one after another: order, tables, cost."""
    dev = _create(V, I, J, X, xmax, D, method, opt=opt, mode="stratified", strata=P, shuffle=shuffle, seed=seed)
    model = S.Model(I, J, P)
    info = dev.info()
    assert (info["strata"], info["strata_path"]) == (P, model.path)
    ref = _as2d(dev.state(), V, D)
    N = len(I)
    for it in range(epochs):
        order = dev.epoch_order(it).astype(np.int64)
        assert np.array_equal(order, model.epoch_order(seed, it, shuffle)), (it, "epoch_order differs from the header's rule")
        assert np.array_equal(np.sort(order), np.arange(N))
        cost = dev.epoch(it)
        ms, launches = dev.last_kernel_ms()
        assert launches == model.launches() <= P
        total, at = 0.0, 0
        for nz in model.jobs(seed, it, shuffle):                 # every tile is a job with its own fp32 cost
            assert np.array_equal(order[at:at + len(nz)], nz)
            at += len(nz)
            if len(nz) == 0:
                continue
            if opt == "adagrad":
                job = O.adagrad_job(D, I[nz], J[nz], X[nz], xmax, cost_kind(method), ref)
            else:
                job = O.opt_job(OPT_KIND[opt], it, D, I[nz], J[nz], X[nz], xmax, cost_kind(method), ref)
            total += float(job)                                   # fp64 sum of fp32 job costs, in epoch order
        got = _as2d(dev.state(), V, D)
        assert set(got) == set(ref)
        for name in ref:
            bad = np.nonzero(got[name].view(np.uint32) != ref[name].view(np.uint32))
            assert np.array_equal(got[name], ref[name]) and bad[0].size == 0, \
                "P=%d %s D=%d %s epoch %d: table %s differs in %d words" % (P, shuffle, D, method, it, name, bad[0].size)
        assert cost == total, ("cost_sum", it, cost, total)
    dev.close()


# ------------------------------------------------------------------ 1. exact to the oracle (and therefore race-free)
@pytest.mark.parametrize("shuffle", ["none", "device"])
@pytest.mark.parametrize("P", PS)
@pytest.mark.parametrize("D", DIMS)
@pytest.mark.parametrize("method", ["glove", "pglove"])
@pytest.mark.parametrize("name", ["zipf300", "zipf90"])
def test_stratified_epochs_bit_exact(gpu, name, method, D, P, shuffle):
    V, I, J, X, xmax = _matrix(name)
    _replay_exact(V, I, J, X, xmax, D, method, P, shuffle)


# ------------------------------------------------------------------ 2. Adam and AMSGrad
@pytest.mark.parametrize("P", [7, 64])
@pytest.mark.parametrize("opt", ["adam", "amsgrad"])
def test_stratified_adam_amsgrad_bit_exact(gpu, opt, P):
    V, I, J, X, xmax = _matrix("zipf300")
    _replay_exact(V, I, J, X, xmax, 50, "pglove", P, "device", epochs=2, opt=opt)


# ------------------------------------------------------------------ 3. designed edges
def _values(n, seed):
    return (0.01 + 0.19 * np.random.default_rng(seed).random(n)).astype(np.float32)        # 0 < x <= 0.2: valid for both costs


def _coo(V, pairs, seed):
    pairs = sorted(set(pairs))
    I = np.array([p[0] for p in pairs], np.int32); J = np.array([p[1] for p in pairs], np.int32)
    return V, I, J, _values(len(pairs), seed), float(np.float32(0.2))


def _hub_column():
    """one column holds half of the nonzeros"""
    rng = np.random.default_rng(3)
    rest = {(int(a), int(b)) for a, b in zip(rng.integers(0, 220, 400), rng.integers(0, 220, 400)) if b != 5}
    rest = sorted(rest)[:200]
    return _coo(220, [(i, 5) for i in range(200)] + rest, 1)


EDGES = {
    "hub_column_half_P16": (_hub_column, 16),
    "one_row": (lambda: _coo(40, [(3, j) for j in range(40)], 2), 4),
    "N_below_P": (lambda: _coo(30, [(1, 2), (4, 9), (9, 4), (20, 20), (29, 0)], 3), 16),
    "P_above_nonempty_rows": (lambda: _coo(40, [(r, j) for r in (2, 17, 33) for j in range(0, 40, 4)], 4), 8),
    "empty_ends": (lambda: _coo(50, [(10 + (7 * k) % 30, 10 + (11 * k) % 30) for k in range(120)], 5), 7),
    "diagonal": (lambda: _coo(30, [(i, i) for i in range(30)], 6), 4),
}


@pytest.mark.parametrize("shuffle", ["none", "device"])
@pytest.mark.parametrize("name", sorted(EDGES))
def test_designed_edges_bit_exact(gpu, name, shuffle):
    make, P = EDGES[name]
    V, I, J, X, xmax = make()
    m = S.Model(I, J, P)
    if name == "hub_column_half_P16":
        assert np.bincount(J).max() * 2 == len(I) and m.path >= len(I) // 2           # the column is the floor
    if name == "N_below_P":
        assert len(I) < P
    if name == "P_above_nonempty_rows":
        assert len(np.unique(I)) < P and (m.counts.sum(axis=1) == 0).any()           # empty row blocks are legal
    if name == "diagonal":
        assert m.launches() == 1 and m.path == int(m.counts.max())                   # only sub-epoch 0 holds anything
    for method in ("glove", "pglove"):
        _replay_exact(V, I, J, X, xmax, 6, method, P, shuffle, epochs=2)


def test_empty_matrix_costs_nothing_and_launches_nothing(gpu):
    V, D = 12, 5
    e = np.zeros(0, np.int32)
    for P in (0, 4):
        dev = _create(V, e, e, np.zeros(0, np.float32), 0.2, D, "glove", mode="stratified", strata=P, shuffle="device", seed=SEED)
        before = dev.state()
        assert dev.epoch(0) == 0.0 and dev.last_kernel_ms()[1] == 0
        assert dev.epoch_order(0).size == 0
        after = dev.state()
        for name in before:
            assert before[name].tobytes() == after[name].tobytes(), name
        assert dev.info()["strata_path"] == 0 and dev.info()["strata"] == (P or S.default_p(V, 0))
        dev.close()


# ------------------------------------------------------------------ 4. P = 1 is the one-wave mode
@pytest.mark.parametrize("opt", ["adagrad", "adam"])
def test_one_stratum_equals_the_deterministic_mode(gpu, opt):
    V, I, J, X, xmax = _matrix("zipf90")
    a = _create(V, I, J, X, xmax, 50, "pglove", opt=opt, mode="stratified", strata=1, shuffle="none", seed=SEED)
    b = _create(V, I, J, X, xmax, 50, "pglove", opt=opt, threads=1, mode="deterministic", shuffle="none", seed=SEED)
    for it in range(2):
        assert a.epoch(it) == b.epoch(it)
        sa, sb = a.state(), b.state()
        for name in sa:
            assert sa[name].tobytes() == sb[name].tobytes(), (it, name)
    a.close(); b.close()


# ------------------------------------------------------------------ 5. repeatability
def test_two_handles_give_equal_bytes_and_orders_change_per_iteration(gpu):
    V, I, J, X, xmax = _matrix("zipf300")
    runs = []
    for _ in range(2):
        dev = _create(V, I, J, X, xmax, 50, "glove", mode="stratified", strata=16, shuffle="device", seed=SEED)
        costs = [dev.epoch(it) for it in range(3)]
        runs.append((costs, dev.state(), dev.extractResultF32(), [dev.epoch_order(it) for it in range(3)]))
        dev.close()
    (c0, s0, x0, o0), (c1, s1, x1, o1) = runs
    assert c0 == c1 and x0.tobytes() == x1.tobytes()
    for name in s0:
        assert s0[name].tobytes() == s1[name].tobytes(), name
    for it in range(3):
        assert np.array_equal(o0[it], o1[it])
    assert not np.array_equal(o0[0], o0[1]) and not np.array_equal(o0[1], o0[2])
    # another seed is another order
    dev = _create(V, I, J, X, xmax, 50, "glove", mode="stratified", strata=16, shuffle="device", seed=SEED + 1)
    assert not np.array_equal(dev.epoch_order(0), o0[0])
    dev.close()


# ------------------------------------------------------------------ 6. info
@pytest.mark.parametrize("P", [0, 1, 7, 64])
def test_info_reports_the_schedule(gpu, P):
    for name in ("zipf300", "zipf90"):
        V, I, J, X, xmax = _matrix(name)
        dev = _create(V, I, J, X, xmax, 8, "glove", mode="stratified", strata=P, shuffle="device", seed=SEED)
        used = P or S.default_p(V, len(I))
        m = S.Model(I, J, used)
        info = dev.info()
        assert (info["strata"], info["strata_path"]) == (used, m.path)
        dev.epoch(0)
        ms, launches = dev.last_kernel_ms()
        assert ms > 0 and launches == m.launches() and launches <= used
        dev.close()
    other = _create(V, I, J, X, xmax, 8, "glove", mode="hogwild", shuffle="device", seed=SEED)
    assert other.info()["strata"] == 0 and other.info()["strata_path"] == 0
    other.close()


def test_sharded_rows_are_accepted_as_in_the_deterministic_mode(gpu):
    """row_begin / row_end: a handle that owns rows [rb, re) stratifies ITS nonzeros; exact against the oracle on the full tables."""
    V, I, J, X, xmax = _matrix("zipf300")
    rb, re = 100, 220
    keep = (I >= rb) & (I < re)
    Ik, Jk, Xk = I[keep], J[keep], X[keep]
    D, P = 6, 7
    dev = _create(V, Ik, Jk, Xk, xmax, D, "glove", mode="stratified", strata=P, shuffle="device", seed=SEED, row_range=(rb, re))
    model = S.Model(Ik, Jk, P)
    assert dev.info()["strata_path"] == model.path
    st = dev.state()
    ref = {k: np.zeros((V, D) if v.size in (V * D, (re - rb) * D) else V, np.float32) + 1 for k, v in st.items()}
    for k, v in st.items():
        focus_side = k in ("focus", "fbias", "gsq_focus", "gsq_fbias")
        if focus_side:
            ref[k][rb:re] = v.reshape(re - rb, -1) if ref[k].ndim == 2 else v
        else:
            ref[k] = np.ascontiguousarray(v.reshape(ref[k].shape))
    ref = {k: np.ascontiguousarray(v, np.float32) for k, v in ref.items()}
    cost = dev.epoch(0)
    assert np.array_equal(dev.epoch_order(0), model.epoch_order(SEED, 0, "device"))
    total = 0.0
    for nz in model.jobs(SEED, 0, "device"):
        if len(nz):
            total += float(O.adagrad_job(D, Ik[nz], Jk[nz], Xk[nz], xmax, O.COST_GLOVE, ref))
    got = dev.state()
    for k, v in got.items():
        want = ref[k][rb:re] if k in ("focus", "fbias", "gsq_focus", "gsq_fbias") else ref[k]
        assert np.array_equal(v.reshape(want.shape), want), k
    assert cost == total
    dev.close()


# ------------------------------------------------------------------ 7. downstream entry points
def test_downstream_entry_points_equal_the_host_rows_ones(gpu):
    V, I, J, X, xmax = _matrix("zipf300")
    dim, k = 24, 10
    dev = _create(V, I, J, X, xmax, dim, "pglove", mode="stratified", strata=16, shuffle="device", seed=SEED)
    for it in range(3):
        dev.epoch(it)
    before = dev.state()
    rows = dev.extractResultF32().reshape(V, dim)
    want = (before["focus"] + before["context"]) / np.float32(2.0)
    assert rows.tobytes() == want.astype(np.float32).tobytes()
    assert np.array_equal(dev.extractResult(), rows.reshape(-1).astype(np.float64))
    on_handle, on_rows = capi.Pca.fit_glove(dev._h), capi.Pca.fit(rows)
    ga, gb = on_handle.get(), on_rows.get()
    assert ga[:3] == gb[:3] == (dim, ga[1], V)
    for ta, tb in zip(ga[3:], gb[3:]):
        assert ta.tobytes() == tb.tobytes()
    assert on_handle.transform_glove(dev._h, V).tobytes() == on_rows.transform(rows).tobytes()
    for metric in ("cosine", "dot"):
        na, nb = capi.Neighbors.create_glove(dev._h, metric=metric), capi.Neighbors.create(rows, metric=metric)
        a, b = na.query_rows(None, k, exclude_self=True), nb.query_rows(None, k, exclude_self=True)
        assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes()
    # set_state / get_state / device_ptr as for DETERMINISTIC handles: plain dense tables
    ptr, count = dev.device_ptr("context")
    assert ptr and count == V * dim
    dev.set_state("context", before["focus"])
    assert dev.get_state("context").tobytes() == before["focus"].tobytes()
    dev.set_state("context", before["context"])
    after = dev.state()
    for name in before:
        assert before[name].tobytes() == after[name].tobytes(), name
    with pytest.raises(capi.GeError) as e:
        dev.perm()
    assert e.value.status == capi.GE_ERR_STATE
    dev.close()


def test_create_from_a_device_resident_coo_takes_the_host_route(gpu):
    coo = capi.synth_coo(200, 3000, seed=7)
    m = geglove.DeviceCooMatrix(coo)
    cfg = make_config(8, "pglove", mode="stratified", strata=7, shuffle="device", seed=SEED)
    a = geglove.Adagrad(m, cfg, cfg.costFunction())
    I, J, X = m.I, m.J, m.X
    b = geglove.Adagrad(geglove.CooMatrix(200, I, J, X, m.max()), cfg, cfg.costFunction())
    assert a.info()["strata_path"] == b.info()["strata_path"] == S.Model(I, J, 7).path
    for it in range(2):
        assert a.epoch(it) == b.epoch(it)
    sa, sb = a.state(), b.state()
    for name in sa:
        assert sa[name].tobytes() == sb[name].tobytes(), name
    a.close(); b.close()


# ------------------------------------------------------------------ 8. CLI
def test_cli_stratified_runs_are_byte_identical(gpu, tmp_path):
    assert os.path.exists(EXE), "host CLI not built"
    base = open(os.path.join(REPO, "tests", "golden", "tiny.config.yml")).read()
    text = base.replace("  mode: deterministic\n  shuffle: java\n", "  mode: stratified\n  strata: 4\n  shuffle: device\n")
    assert "stratified" in text
    name = "tiny_pglove_partial_directed_0.1_0.001_adagrad_pca_8"
    outs = []
    for run in ("a", "b"):
        cwd = tmp_path / run
        os.makedirs(cwd / "tests" / "golden")
        (cwd / "tests" / "golden" / "tiny.nt").write_bytes(open(os.path.join(REPO, "tests", "golden", "tiny.nt"), "rb").read())
        (cwd / "strat.yml").write_text(text)
        r = subprocess.run([EXE, "-c", "strat.yml"], cwd=cwd, capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, r.stderr + r.stdout
        assert "stratified: P = 4, strata_path / N = " in r.stdout
        outs.append((cwd / "out" / (name + ".vectors.tsv")).read_bytes())
    assert outs[0] == outs[1] and b"# Stratified trainer: 4 strata" in outs[0]
    body = [l for l in outs[0].decode().splitlines() if not l.startswith("#") and "\t" in l]
    assert len(body) == 3 and all(np.isfinite([float(x) for x in l.split("\t")]).all() for l in body)
    # shuffle: java is refused by the bean check, in check()'s words
    bad = tmp_path / "bad.yml"; bad.write_text(base.replace("  mode: deterministic\n", "  mode: stratified\n"))
    r = subprocess.run([EXE, "-c", str(bad)], cwd=tmp_path, capture_output=True, text=True, timeout=120)
    assert r.returncode == 1 and "Invalid configuration: device.mode: stratified cannot follow shuffle: java" in r.stderr

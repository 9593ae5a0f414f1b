"""Every Hogwild kernel instance held to a sequential reference.

k_adagrad_runs<VW, NCH, OPT, EMB16, FAT> (csrc/glove.hip) is picked from `dim` alone (kernel_model.lane_shape): 16 fp32 lane
shapes x 3 optimisers + 8 bf16 shapes = 56 instances, each with its own register chunking, per-row resource bounds, bias lane and
record stride.  The dims of kernel_model.SHAPE_DIMS reach all of them (tests/test_kernel_resources.py checks that on the CPU); here
each one runs through the C ABI against the oracle (fp64 Java arithmetic) or kernel_model (the kernel's own fp32 arithmetic):
  * dispatch and refusals: info() reports lane_shape(dim); dims past the largest shape of their vector width are refused;
  * initial state: the Java draw order through every record layout, bit for bit; set_state / get_state round trips;
  * AdaGrad: one-worker replays of the blocked order, and conflict-free batches with many workers (fp32 and bf16 rows);
  * Adam / AMSGrad: one-worker replays against kernel_model (tight) and the oracle (loose);
  * long rows: focus rows cut into pieces that publish by delta, replayed with one worker;
  * the deterministic kernel across its whole width (up to the 64 KiB LDS bound), bit for bit.
Tolerances are those of the tests in test_glove_parity_gpu.py that make the same comparison at fewer dims."""
import numpy as np
import pytest

import geglove
from geglove import capi, synth
import oracle as O
import kernel_model as K
from helpers import make_config, cost_kind, assert_state_equal, OPT_KIND

pytestmark = pytest.mark.gpu

FP32_DIMS = K.SHAPE_TABLE_DIMS


def _as2d(st, V, D):
    return {k: np.ascontiguousarray(v.reshape(V, -1) if v.size == V * D else v, np.float32) for k, v in st.items()}


def _bf16_rne(a):
    u = np.ascontiguousarray(a, np.float32).view(np.uint32)
    return (((u + 0x7FFF + ((u >> 16) & 1)) >> 16) << 16).astype(np.uint32).view(np.float32)


def _create(V, I, J, X, xmax, D, method="glove", opt="adagrad", **device):
    cfg = make_config(D, method, opt=opt, **device)
    return geglove.createOptimizer(cfg, geglove.CooMatrix(V, I, J, X, xmax))


# ------------------------------------------------------------------ dispatch and refusals
def test_dispatch_follows_the_lane_shape(gpu):
    """For every dim of the shape table, every optimiser and (dim % 4 == 0) bf16 rows: the handle runs the lane shape of
    kernel_model.lane_shape."""
    V = 40
    I, J, X, xmax = synth.synthetic_coo(V, 200, seed=3)
    for D in FP32_DIMS:
        vw, nch, _ = K.lane_shape(D)
        kinds = [("adagrad", "f32"), ("adam", "f32"), ("amsgrad", "f32")] + ([("adagrad", "bf16")] if D % 4 == 0 else [])
        for opt, dtype in kinds:
            h = _create(V, I, J, X, xmax, D, opt=opt, mode="hogwild", shuffle="device", seed=1, dtype=dtype)
            info = h.info()
            assert (info["vector_width"], info["chunks_per_lane"]) == (vw, nch), (D, opt, dtype, info["vector_width"], info["chunks_per_lane"])
            h.close()


@pytest.mark.parametrize("D,dtype", [(257, "f32"), (259, "f32"), (1025, "f32"), (514, "f32"), (1022, "f32"), (1028, "f32"),
                                     (50, "bf16"), (255, "bf16")])
def test_hogwild_refuses_dims_without_an_instance(gpu, D, dtype):
    """Odd dims past 256, even non-multiples of 4 past 510 and multiples of 4 past 1024 have no lane shape; bf16 rows need
    dim % 4 == 0."""
    V = 40
    I, J, X, xmax = synth.synthetic_coo(V, 200, seed=3)
    assert dtype == "bf16" or K.lane_shape(D) is None
    with pytest.raises(geglove.GeError) as e:
        _create(V, I, J, X, xmax, D, mode="hogwild", shuffle="device", seed=1, dtype=dtype)
    assert e.value.status == capi.GE_ERR_ARG


@pytest.mark.parametrize("D", [255, 510, 1024])
def test_hogwild_accepts_the_largest_dim_of_each_width(gpu, D):
    V = 40
    I, J, X, xmax = synth.synthetic_coo(V, 200, seed=3)
    h = _create(V, I, J, X, xmax, D, mode="hogwild", shuffle="device", seed=1)
    assert (h.info()["vector_width"], h.info()["chunks_per_lane"]) == K.lane_shape(D)[:2]


# ------------------------------------------------------------------ initial state and state access
@pytest.mark.parametrize("opt", ["adagrad", "adam"])
@pytest.mark.parametrize("layout", [[], ["separate_tables"]])
@pytest.mark.parametrize("D", FP32_DIMS)
def test_hogwild_init_and_state_round_trip(gpu, D, layout, opt):
    """Right after ge_glove_create every table equals the oracle's initial state (Java draw order, accumulators 1, moments 0) bit
    for bit -- through fat rows, padded records of two or three rows, and separate tables.  Then every table written through
    set_state reads back bit for bit, none disturbing the others."""
    V = 67
    I, J, X, xmax = synth.synthetic_coo(V, 400, seed=5)
    h = _create(V, I, J, X, xmax, D, opt=opt, mode="hogwild", shuffle="device", seed=42, layout=layout)
    ora = O.Glove(V, D, I, J, X, xmax, O.COST_GLOVE, seed=42, threads=1, opt=OPT_KIND[opt])
    assert_state_equal(h.state(), ora, what="init D=%d %s %s" % (D, layout, opt))
    rng = np.random.default_rng(D)
    sent = {}
    for name in h.state():
        sent[name] = rng.standard_normal(h.get_state(name).size).astype(np.float32)
        h.set_state(name, sent[name])
    for name, v in sent.items():
        got = h.get_state(name)
        bad = np.nonzero(got.view(np.uint32) != v.view(np.uint32))[0]
        assert bad.size == 0, (name, D, "first differing element", int(bad[0]), "row", int(bad[0]) // D, "d", int(bad[0]) % D)


@pytest.mark.parametrize("hot", ["none", "all"])
@pytest.mark.parametrize("D", K.BF16_DIMS)
def test_bf16_init_and_state_round_trip(gpu, D, hot):
    """bf16 rows: the Java draw order rounded to nearest-even bf16; hub context rows (hot=all: every column that occurs) keep the
    fp32 value; biases, accumulators exact.  set_state: rows round to nearest-even (hub rows keep fp32), the fp32 tables -- the
    accumulator rows and the scalars behind them in the records -- keep what they are given."""
    V = 67
    I, J, X, xmax = synth.synthetic_coo(V, 400, seed=5)
    h = _create(V, I, J, X, xmax, D, mode="hogwild", shuffle="device", seed=42, hot=hot, dtype="bf16")
    ora = O.Glove(V, D, I, J, X, xmax, O.COST_GLOVE, seed=42, threads=1)
    st = h.state()
    hubs = np.zeros(V, bool)
    if hot == "all":
        hubs[np.unique(J)] = True
    assert np.array_equal(st["focus"].reshape(V, D), _bf16_rne(ora.focus))
    exp_ctx = _bf16_rne(ora.context)
    exp_ctx[hubs] = ora.context[hubs]
    assert np.array_equal(st["context"].reshape(V, D), exp_ctx)
    for k in ("fbias", "cbias", "gsq_focus", "gsq_context", "gsq_fbias", "gsq_cbias"):
        assert np.array_equal(st[k].reshape(-1), np.asarray(ora.state()[k]).reshape(-1)), k
    rng = np.random.default_rng(D)
    new = rng.standard_normal(V * D).astype(np.float32)
    h.set_state("focus", new)
    h.set_state("context", new)
    sent = {}
    for name in capi.STATE_NAMES[2:]:
        sent[name] = rng.standard_normal(h.get_state(name).size).astype(np.float32)
        h.set_state(name, sent[name])
    for name, v in sent.items():
        np.testing.assert_array_equal(h.get_state(name), v, err_msg=name)
    np.testing.assert_array_equal(h.get_state("focus"), _bf16_rne(new))
    exp = _bf16_rne(new).reshape(V, D)
    exp[hubs] = new.reshape(V, D)[hubs]
    np.testing.assert_array_equal(h.get_state("context").reshape(V, D), exp)


# ------------------------------------------------------------------ AdaGrad
@pytest.mark.parametrize("hot", ["none", "auto"])
@pytest.mark.parametrize("method", ["glove", "pglove"])
@pytest.mark.parametrize("D", FP32_DIMS)
def test_adagrad_single_worker_replay(gpu, D, method, hot):
    """One worker walking the blocked order is a sequential program: the oracle replaying the order it reports agrees to fp32
    round-off (tolerances of test_hogwild_blocked_order_single_worker_replays_sequentially)."""
    V, N = 90, 2500
    I, J, X, xmax = synth.synthetic_coo(V, N, seed=17)
    opt = _create(V, I, J, X, xmax, D, method, mode="hogwild", shuffle="device", seed=5, hot=hot, workers=1, hot_theta=0.02)
    if hot == "auto":
        assert 0 < opt.info()["hot_nonzeros"] < len(I)           # resident-focus and hub chunks both run
    ref = _as2d(opt.state(), V, D)
    for it in range(2):
        order = opt.epoch_order(it).astype(np.int64)
        assert np.array_equal(np.sort(order), np.arange(len(I)))
        cost = opt.epoch(it)
        job = O.adagrad_job(D, I[order], J[order], X[order], xmax, cost_kind(method), ref)
        assert cost == pytest.approx(float(job), rel=1e-4)
        assert_state_equal(opt.state(), ref, exact=False, rtol=5e-5, atol=5e-6, what="D=%d epoch %d" % (D, it))


@pytest.mark.parametrize("hot", ["none", "all"])
@pytest.mark.parametrize("method", ["glove", "pglove"])
@pytest.mark.parametrize("D", FP32_DIMS)
def test_adagrad_conflict_free_batch(gpu, D, method, hot):
    """All i distinct, all j distinct, sixteen workers at once: one possible result, through the plain stores (hot=none) and the
    atomic hub flush (hot=all).  Tolerances of test_hogwild_conflict_free_batch."""
    V = 3000
    I, J, X = synth.conflict_free_batch(V, 2048, seed=D)
    xmax = 0.2
    opt = _create(V, I, J, X, xmax, D, method, mode="hogwild", shuffle="device", seed=42, hot=hot, workers=16)
    assert opt.info()["hot_nonzeros"] == (len(I) if hot == "all" else 0)
    ref = _as2d(opt.state(), V, D)
    job_cost = O.adagrad_job(D, I, J, X, xmax, cost_kind(method), ref)
    cost = opt.epoch(0)
    assert cost == pytest.approx(float(job_cost), rel=2e-4)
    assert_state_equal(opt.state(), ref, exact=False, rtol=2e-6, atol=2e-7, what="D=%d" % D)


@pytest.mark.parametrize("hot", ["none", "all"])
@pytest.mark.parametrize("D", K.BF16_DIMS)
def test_bf16_conflict_free_batch(gpu, D, hot):
    """bf16 rows + fp32 accumulators, the assertions of test_bf16_embeddings_conflict_free_batch: fp32 tables to fp32 round-off,
    bf16 rows within one bf16 ulp (stochastic rounding) with zero-mean error, untouched rows untouched."""
    V = 5000
    I, J, X = synth.conflict_free_batch(V, 4096, seed=D)
    opt = _create(V, I, J, X, 0.2, D, mode="hogwild", shuffle="device", seed=42, hot=hot, dtype="bf16")
    st = opt.state()
    ref = {k: (v.reshape(V, -1) if v.size == V * D else v).astype(np.float32, copy=True) for k, v in st.items()}
    O.adagrad_job(D, I, J, X, 0.2, O.COST_GLOVE, ref)
    opt.epoch(0)
    got = opt.state()
    for k in ("fbias", "cbias", "gsq_focus", "gsq_context", "gsq_fbias", "gsq_cbias"):
        np.testing.assert_allclose(got[k], ref[k].reshape(-1), rtol=3e-6, atol=1e-9, err_msg=k)
    tables = ["focus"] if hot == "all" else ["focus", "context"]
    if hot == "all":
        np.testing.assert_allclose(got["context"], ref["context"].reshape(-1), rtol=3e-6, atol=2e-7 * float(np.max(np.abs(ref["context"]))))
    for k in tables:
        g, r = got[k], ref[k].reshape(-1)
        touched = np.zeros(V, bool); touched[I if k == "focus" else J] = True
        m = np.repeat(touched, D)
        ulp = np.maximum(np.abs(r[m]), 1e-30) * 2.0 ** -7
        err = (g[m] - r[m]) / ulp
        slack = 2e-7 * float(np.max(np.abs(r))) / ulp
        assert np.all(np.abs(err) <= 1.0 + slack), (k, float(np.max(np.abs(err) - slack)))
        assert abs(np.mean(err)) < 0.01, (k, float(np.mean(err)))
        assert np.array_equal(g[~m], st[k][~m])


# ------------------------------------------------------------------ Adam / AMSGrad
def _moment_replay(dev, opt, V, D, I, J, X, xmax, epochs=2, long_rows=False):
    """The two checks of test_adam_amsgrad_hogwild_single_worker_replay: the kernel's own arithmetic (kernel_model, every element
    within 1e-5) and the fp64 oracle (bounded in distribution, same bounds).  long_rows: the model publishes the pieces of long
    focus rows by delta, as the kernel does."""
    info = dev.info()
    ref = _as2d(dev.state(), V, D)
    mod = {k: v.copy() for k, v in ref.items()}
    for it in range(epochs):
        order = dev.epoch_order(it).astype(np.int64)
        cost = dev.epoch(it)
        job = O.opt_job(OPT_KIND[opt], it, D, I[order], J[order], X[order], xmax, O.COST_GLOVE, ref)
        runs = K.long_row_pieces(I, order) if long_rows else None
        mcost = K.moment_epoch(opt == "amsgrad", it, D, info["vector_width"], info["chunks_per_lane"], I[order], J[order], X[order], xmax, mod,
                               delta_runs=runs)
        assert cost == pytest.approx(float(mcost), rel=1e-6)
        assert cost == pytest.approx(float(job), rel=2e-2 if (opt == "amsgrad" and D > 64) else 1e-3)
        got = _as2d(dev.state(), V, D)
        for name, g in got.items():
            g, m = g.reshape(-1), mod[name].reshape(-1)
            err = np.abs(g - m) / (np.abs(m) + 1e-3 * np.max(np.abs(m)) + 1e-30)
            k = int(np.argmax(err))
            row, d = (k // D, k % D) if g.size == V * D else (k, D)
            vw, nch = info["vector_width"], info["chunks_per_lane"]
            assert np.max(err) <= 1e-5, ("kernel vs its own arithmetic", name, it, float(np.max(err)),
                                         "row %d d %d lane %d chunk %d" % (row, d, (d // vw) % 64, d // (64 * vw)))
        room = 10.0 if (opt == "amsgrad" and it > 0) else 1.0
        if D > 64:
            room *= 20.0 if opt == "adam" else 100.0
        for name in ("focus", "context", "fbias", "cbias"):
            g, r = got[name].reshape(-1), np.asarray(ref[name]).reshape(-1)
            err = np.abs(g - r) / (np.abs(r) + 1e-3 * np.max(np.abs(r)) + 1e-30)
            assert np.median(err) <= 1e-4 * room and np.quantile(err, 0.95) < 5e-3 * room, (name, it, float(np.median(err)), float(np.quantile(err, 0.95)))


@pytest.mark.parametrize("opt", ["adam", "amsgrad"])
@pytest.mark.parametrize("D", K.LANE63_DIMS)
def test_adam_amsgrad_single_worker_replay(gpu, D, opt):
    """Every fp32 lane shape with its bias in lane 63 of the last chunk (fat shapes) or its lanes full (non-fat shapes), through
    resident-focus and hub chunks (hot=auto).  Half the nonzeros of test_adam_amsgrad_hogwild_single_worker_replay's matrix: the
    numpy model stays under a second per case, and the loose bounds, measured there for dims up to 300, hold for the wider rows
    too (at 2 500 nonzeros AMSGrad's epoch-0 context rows at dim 768 leave them: median 1.8e-2 against the fp64 oracle, with
    the kernel still within 1e-5 of its own arithmetic)."""
    V, N = 90, 1200
    I, J, X, xmax = synth.synthetic_coo(V, N, seed=17)
    dev = _create(V, I, J, X, xmax, D, opt=opt, mode="hogwild", shuffle="device", seed=5, hot="auto", workers=1, hot_theta=0.02)
    assert 0 < dev.info()["hot_nonzeros"] < len(I)
    _moment_replay(dev, opt, V, D, I, J, X, xmax)


# ------------------------------------------------------------------ long rows: pieces that publish by delta
def _long_row_matrix(seed=11):
    """Four focus rows of 300 nonzeros each (past two 128-entry pieces) on distinct columns, plus short rows."""
    rng = np.random.default_rng(seed)
    V = 400
    I, J = [], []
    for r in range(4):
        I += [r] * 300
        J += sorted(rng.choice(V, 300, replace=False).tolist())
    for r in range(4, 60):
        I += [r] * 5
        J += sorted(rng.choice(V, 5, replace=False).tolist())
    I = np.asarray(I, np.int32); J = np.asarray(J, np.int32)
    X = (10 ** rng.uniform(-3.5, -0.7, size=len(I))).astype(np.float32)
    return V, I, J, X, 0.2


@pytest.mark.parametrize("opt", ["adagrad", "adam", "amsgrad"])
@pytest.mark.parametrize("D", [63, 191, 126, 382, 764, 1024])     # VW 1 / VW 2 at one and three chunks, VW 4 at three (fat) and four (full)
def test_long_row_pieces_single_worker_replay(gpu, D, opt):
    """A focus row of more than 128 ordinary nonzeros is cut into pieces that publish the row by delta (float atomics for AdaGrad;
    re-read, add, store for Adam).  With one worker the pieces run one after another, so the walk is still a sequential program:
    AdaGrad against the oracle (tolerances of the single-worker replay), Adam and AMSGrad against kernel_model and the oracle.  A piece adds its
    delta a - a0 to the row it read (a0), which is a in fp32 up to an ulp: inside the oracle's bounds, but Adam's sign-like steps
    carry such an ulp far (a component of a gradient near zero changes sign), so kernel_model restates the delta publish itself."""
    V, I, J, X, xmax = _long_row_matrix()
    dev = _create(V, I, J, X, xmax, D, opt=opt, mode="hogwild", shuffle="device", seed=5, hot="none", workers=1)
    info = dev.info()
    assert info["long_rows"] > 0 and info["shared_chunks"] > 0, (info["long_rows"], info["shared_chunks"])
    if opt != "adagrad":
        _moment_replay(dev, opt, V, D, I, J, X, xmax, long_rows=True)
        return
    ref = _as2d(dev.state(), V, D)
    for it in range(2):
        order = dev.epoch_order(it).astype(np.int64)
        assert np.array_equal(np.sort(order), np.arange(len(I)))
        cost = dev.epoch(it)
        job = O.adagrad_job(D, I[order], J[order], X[order], xmax, O.COST_GLOVE, ref)
        assert cost == pytest.approx(float(job), rel=1e-4)
        assert_state_equal(dev.state(), ref, exact=False, rtol=5e-5, atol=5e-6, what="long rows D=%d epoch %d" % (D, it))


# ------------------------------------------------------------------ deterministic kernel width
@pytest.mark.parametrize("D", [64, 65, 257, 1024, 4097, 16384])
def test_deterministic_width_bit_exact(gpu, D):
    """k_adagrad_exact keeps one product row in LDS: any dim up to 64 KiB of it.  Perm, RNG state, cost and every table bit for bit
    against the oracle, as test_deterministic_epochs_bit_exact does up to dim 300."""
    V, N = 100, 800
    I, J, X, xmax = synth.synthetic_coo(V, N, seed=9)
    opt = _create(V, I, J, X, xmax, D, "pglove", mode="deterministic", shuffle="java", seed=42)
    ora = O.Glove(V, D, I, J, X, xmax, O.COST_PGLOVE, seed=42, threads=1)
    assert_state_equal(opt.state(), ora, what="init")
    n = len(I)
    for it in range(2):
        c_dev = opt.epoch(it) / n
        c_ora = ora.epoch()
        assert np.array_equal(opt.perm(), ora.perm), "Java Fisher-Yates permutation differs at epoch %d" % it
        assert opt.rng_state() == ora.rng_state
        assert c_dev == c_ora, "epoch %d cost %r vs oracle %r" % (it, c_dev, c_ora)
        assert_state_equal(opt.state(), ora, what="D=%d epoch %d" % (D, it))


def test_deterministic_refuses_past_the_lds_bound(gpu):
    V = 40
    I, J, X, xmax = synth.synthetic_coo(V, 200, seed=3)
    with pytest.raises(geglove.GeError) as e:
        _create(V, I, J, X, xmax, 16385, mode="deterministic", shuffle="java", seed=42)
    assert e.value.status == capi.GE_ERR_ARG

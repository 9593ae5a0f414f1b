"""The trainer kernels on designed matrices (tests/designed.py): inputs the synthetic generators never produce, each with a known
right answer.

  1. one-worker replays of every structure matrix, with hub runs cut INSIDE a chunk (flush_every 1, 3, 4, 64, and once through
     stale_budget): with one worker the walk is a sequential program for any flush limit, so the oracle (AdaGrad) or kernel_model
     (Adam, AMSGrad) replaying the reported order must agree -- through the re-read behind a cut, the same streamed row in
     consecutive steps, a new resident row at every step, repeated (i, j);
  2. partial chunks: conflict-free batches of 1 .. 193 nonzeros with sixteen workers;
  3. X on, around and far from xmax, subnormal and huge, pGloVe's X -> 1 and X = 0.5, through all three places that evaluate the
     cost terms (the deterministic kernel, the blocked layout, the general order);
  4. cuts lose nothing with many workers: one hub column of 3000 nonzeros, made countable.
Tolerances are those of the existing tests that make the same comparison on synthetic matrices (named per test); the CPU file
test_designed_matrices.py shows that every single update of a structure matrix is worth at least 10 x the replay tolerance."""
import numpy as np
import pytest

import geglove
import oracle as O
import kernel_model as K
import designed as M
from helpers import make_config, cost_kind, assert_state_equal, OPT_KIND
from test_glove_parity_gpu import _worker_order

pytestmark = pytest.mark.gpu

FLUSH = [0, 1, 3, 4, 64]
ADAGRAD_DIMS = [5, 6, 52, 256, 300]         # VW 1 / 2 / 4 fat rows, full lanes with bias vectors, two register chunks
MOMENT_DIMS = [6, 256]

_MATRICES = {}


def _matrix(name):
    if name not in _MATRICES:
        _MATRICES[name] = M.STRUCTURES[name]()
    return _MATRICES[name]


def _as2d(st, V, D):
    return {k: np.ascontiguousarray(v.reshape(V, -1) if v.size == V * D else v, np.float32) for k, v in st.items()}


def _create(V, I, J, X, xmax, D, method="glove", opt="adagrad", **device):
    cfg = make_config(D, method, opt=opt, **device)
    return geglove.createOptimizer(cfg, geglove.CooMatrix(V, I, J, X, xmax))


def _walk(dev, it, shuffle, J, hot):
    """Runs epoch `it` and returns (cost, the order one worker walked): ge_glove_epoch_order, which for the Java shuffle must also be
    the chunks of the permutation sorted by column (test_hogwild_single_worker_replays_sequentially)."""
    if shuffle == "device":
        order = dev.epoch_order(it).astype(np.int64)
        return dev.epoch(it), order
    cost = dev.epoch(it)
    order = _worker_order(dev.perm().astype(np.int64), J, np.full(int(J.max()) + 1, hot == "all"), 1)[0]
    assert np.array_equal(order, dev.epoch_order(it))
    return cost, order


def _expect_cut(dev, hot, flush_every):
    if hot != "none" and flush_every > 0:
        assert dev.info()["flush_min"] == flush_every          # the cut is active
    assert dev.info()["groups_in_flight"] == 1


# ------------------------------------------------------------------ 1. one-worker replays, hub runs cut inside a chunk
_ADAGRAD_REF = {}       # (matrix, D, method, orders) -> [(job cost, state after the epoch)]: computed once, never modified


def _adagrad_reference(name, D, method, init, orders):
    key = (name, D, method, tuple(o.tobytes() for o in orders))
    if key not in _ADAGRAD_REF:
        V, I, J, X, xmax = _matrix(name)
        ref = {k: v.copy() for k, v in init.items()}
        out = []
        for order in orders:
            job = O.adagrad_job(D, I[order], J[order], X[order], xmax, cost_kind(method), ref)
            out.append((float(job), {k: v.copy() for k, v in ref.items()}))
        _ADAGRAD_REF[key] = (init, out)
    first, out = _ADAGRAD_REF[key]
    for k in init:
        assert np.array_equal(init[k], first[k]), k             # same seed, same initial tables: the cached replay applies
    return out


def _adagrad_replay(name, hot, shuffle, device_extra, flush_every):
    V, I, J, X, xmax = _matrix(name)
    worst = (0.0, "")
    for D in ADAGRAD_DIMS:
        for method in ("glove", "pglove"):
            dev = _create(V, I, J, X, xmax, D, method, mode="hogwild", shuffle=shuffle, seed=5, hot=hot, workers=1, **device_extra)
            _expect_cut(dev, hot, flush_every)
            assert dev.info()["hot_nonzeros"] == (len(I) if hot == "all" else 0)
            init = _as2d(dev.state(), V, D)
            got, orders, costs = [], [], []
            for it in range(2):
                cost, order = _walk(dev, it, shuffle, J, hot)
                assert np.array_equal(np.sort(order), np.arange(len(I)))
                costs.append(cost); orders.append(order); got.append(_as2d(dev.state(), V, D))
            dev.close()
            ref = _adagrad_reference(name, D, method, init, orders)
            for it in range(2):
                job, state = ref[it]
                share, where = M.tolerance_share(got[it], state, 5e-5, 5e-6)
                cshare = abs(costs[it] - job) / (1e-4 * abs(job))
                what = "%s hot=%s %s %s D=%d %s epoch %d" % (name, hot, shuffle, device_extra, D, method, it)
                if max(share, cshare) > worst[0]:
                    worst = (max(share, cshare), what + " " + where)
                assert costs[it] == pytest.approx(job, rel=1e-4), (what, "share of the cost tolerance", cshare)
                assert share <= 1.0, (what, "share of the state tolerance used", share, where)
                assert_state_equal(got[it], state, exact=False, rtol=5e-5, atol=5e-6, what=what)
    print("%s hot=%s %s %s: largest share of the replay tolerance used %.4f (%s)" % (name, hot, shuffle, device_extra, worst[0], worst[1]))


@pytest.mark.parametrize("flush_every", FLUSH)
@pytest.mark.parametrize("shuffle", ["device", "java"])
@pytest.mark.parametrize("hot", ["none", "all"])
@pytest.mark.parametrize("name", sorted(M.STRUCTURES))
def test_adagrad_one_worker_replay_with_cut_hub_runs(gpu, name, hot, shuffle, flush_every):
    """AdaGrad, dims 5 / 6 / 52 / 256 / 300, GloVe and pGloVe, two epochs, against O.adagrad_job replaying the walk: the tolerances of
    test_hogwild_blocked_order_single_worker_replays_sequentially (cost rel 1e-4; state rtol 5e-5, atol 5e-6).  The kernel's
    fp32 arithmetic uses at most 5 % of that tolerance on these matrices (printed per case) and a single lost update at least
    10 x it (test_designed_matrices.py): a miss is not round-off.  A follow-on run that starts from the row as it was BEFORE the
    cut run was published misses by 45 - 1 760 x the cost tolerance."""
    _adagrad_replay(name, hot, shuffle, {"flush_every": flush_every} if flush_every else {}, flush_every)


@pytest.mark.parametrize("shuffle", ["device", "java"])
@pytest.mark.parametrize("name", ["one_column", "repeats"])
def test_adagrad_one_worker_replay_cut_by_the_stale_budget(gpu, name, shuffle):
    """The same cut reached through stale_budget / K_j (K_j = 1 with one worker) instead of flush_every."""
    V, I, J, X, xmax = _matrix(name)
    dev = _create(V, I, J, X, xmax, 8, mode="hogwild", shuffle=shuffle, seed=5, hot="all", workers=1, stale_budget=9.0)
    assert dev.info()["flush_min"] == 9
    dev.close()
    _adagrad_replay(name, "all", shuffle, {"stale_budget": 9.0}, 0)


_MOMENT_REF = {}


def _moment_reference(name, opt, D, vw, nch, init, orders, long_rows):
    """kernel_model and the fp64 oracle replaying the walk, once per (matrix, optimiser, dim, walk, delta publish or not): the
    flush limit changes neither the walk nor, with one worker, the result.  (one_row is walked in the same order as one long row
    and as 300 hub columns; only the former publishes by delta.)"""
    key = (name, opt, D, bool(long_rows), tuple(o.tobytes() for o in orders))
    if key not in _MOMENT_REF:
        V, I, J, X, xmax = _matrix(name)
        ref = {k: v.copy() for k, v in init.items()}
        mod = {k: v.copy() for k, v in init.items()}
        out = []
        for it, order in enumerate(orders):
            job = O.opt_job(OPT_KIND[opt], it, D, I[order], J[order], X[order], xmax, O.COST_GLOVE, ref)
            runs = K.long_row_pieces(I, order) if long_rows else None
            mcost = K.moment_epoch(opt == "amsgrad", it, D, vw, nch, I[order], J[order], X[order], xmax, mod, delta_runs=runs)
            out.append((float(job), float(mcost), {k: v.copy() for k, v in ref.items()}, {k: v.copy() for k, v in mod.items()}))
        _MOMENT_REF[key] = (init, out)
    first, out = _MOMENT_REF[key]
    for k in init:
        assert np.array_equal(init[k], first[k]), k
    return out


@pytest.mark.parametrize("flush_every", FLUSH)
@pytest.mark.parametrize("shuffle", ["device", "java"])
@pytest.mark.parametrize("hot", ["none", "all"])
@pytest.mark.parametrize("name", sorted(M.STRUCTURES))
def test_adam_amsgrad_one_worker_replay_with_cut_hub_runs(gpu, name, hot, shuffle, flush_every):
    """Adam and AMSGrad, dims 6 and 256, GloVe: the checks of test_kernel_shapes_gpu._moment_replay -- every element within 1e-5 of
    kernel_model (the kernel's own fp32 arithmetic), cost rel 1e-6, and the fp64 oracle's bounds in distribution.  Hub columns
    store their rows whole, so a cut run must continue from exactly what it stored; long focus rows (hot=none) publish by delta,
    which kernel_model restates (delta_runs)."""
    V, I, J, X, xmax = _matrix(name)
    extra = {"flush_every": flush_every} if flush_every else {}
    worst = (0.0, "")
    for opt in ("adam", "amsgrad"):
        for D in MOMENT_DIMS:
            dev = _create(V, I, J, X, xmax, D, opt=opt, mode="hogwild", shuffle=shuffle, seed=5, hot=hot, workers=1, **extra)
            _expect_cut(dev, hot, flush_every)
            info = dev.info()
            vw, nch = info["vector_width"], info["chunks_per_lane"]
            long_rows = info["long_rows"] > 0
            init = _as2d(dev.state(), V, D)
            got, orders, costs = [], [], []
            for it in range(2):
                cost, order = _walk(dev, it, shuffle, J, hot)
                costs.append(cost); orders.append(order); got.append(_as2d(dev.state(), V, D))
            dev.close()
            ref = _moment_reference(name, opt, D, vw, nch, init, orders, long_rows)
            for it in range(2):
                job, mcost, rstate, mstate = ref[it]
                what = "%s hot=%s %s flush_every=%d %s D=%d epoch %d" % (name, hot, shuffle, flush_every, opt, D, it)
                assert costs[it] == pytest.approx(mcost, rel=1e-6), what
                assert costs[it] == pytest.approx(job, rel=2e-2 if (opt == "amsgrad" and D > 64) else 1e-3), what
                for tname, g in got[it].items():
                    g, m = g.reshape(-1), mstate[tname].reshape(-1)
                    err = np.abs(g - m) / (np.abs(m) + 1e-3 * np.max(np.abs(m)) + 1e-30)
                    k = int(np.argmax(err))
                    if float(err[k]) / 1e-5 > worst[0]:
                        worst = (float(err[k]) / 1e-5, "%s %s[%d]" % (what, tname, k))
                    assert np.max(err) <= 1e-5, ("kernel vs its own arithmetic", what, tname, k, float(err[k]))
                room = 10.0 if (opt == "amsgrad" and it > 0) else 1.0
                if D > 64:
                    room *= 20.0 if opt == "adam" else 100.0
                for tname in ("focus", "context", "fbias", "cbias"):
                    g, r = got[it][tname].reshape(-1), rstate[tname].reshape(-1)
                    err = np.abs(g - r) / (np.abs(r) + 1e-3 * np.max(np.abs(r)) + 1e-30)
                    assert np.median(err) <= 1e-4 * room and np.quantile(err, 0.95) < 5e-3 * room, \
                        (what, tname, float(np.median(err)), float(np.quantile(err, 0.95)))
    print("%s hot=%s %s flush_every=%d: largest share of the 1e-5 bound against kernel_model %.4f (%s)" % (name, hot, shuffle, flush_every, worst[0], worst[1]))


# ------------------------------------------------------------------ 2. partial chunks
def _untouched_rows_are_untouched(before, after, V, D, I, J, what):
    for name in after:
        rows = I if ("focus" in name or name.endswith("fbias")) else J
        keep = np.ones(V, bool); keep[rows] = False
        a = np.asarray(after[name]).reshape(V, -1)[keep]; b = np.asarray(before[name]).reshape(V, -1)[keep]
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32)), (what, name, "a row that no nonzero touches changed")


@pytest.mark.parametrize("shuffle", ["device", "java"])
@pytest.mark.parametrize("hot", ["none", "all"])
@pytest.mark.parametrize("n", M.PARTIAL_SIZES)
def test_partial_chunks_conflict_free(gpu, n, hot, shuffle):
    """A last chunk of 1, 2, 63, 64, 65, 127 nonzeros (and 128, 129, 193 in all): the odd tail of the two-step loop, the boundary
    between the two 64-lane halves of a chunk.  All i distinct, all j distinct, sixteen workers: one possible result.  AdaGrad at
    dims 5, 52, 256 and Adam at 6, tolerances of test_hogwild_conflict_free_batch (rtol 2e-6, atol 2e-7, cost rel 2e-4); rows
    that no nonzero touches keep their initial bits."""
    V, I, J, X, xmax = M.partial(n)
    worst = (0.0, "")
    for opt, D in (("adagrad", 5), ("adagrad", 52), ("adagrad", 256), ("adam", 6)):
        for method in (("glove", "pglove") if opt == "adagrad" else ("glove",)):
            dev = _create(V, I, J, X, xmax, D, method, opt=opt, mode="hogwild", shuffle=shuffle, seed=42, hot=hot, workers=16)
            assert dev.info()["hot_nonzeros"] == (n if hot == "all" else 0)
            init = _as2d(dev.state(), V, D)
            ref = {k: v.copy() for k, v in init.items()}
            job = O.opt_job(OPT_KIND[opt], 0, D, I, J, X, xmax, cost_kind(method), ref) if opt != "adagrad" \
                else O.adagrad_job(D, I, J, X, xmax, cost_kind(method), ref)
            cost = dev.epoch(0)
            got = _as2d(dev.state(), V, D)
            dev.close()
            what = "n=%d hot=%s %s %s D=%d %s" % (n, hot, shuffle, opt, D, method)
            share, where = M.tolerance_share(got, ref, 2e-6, 2e-7)
            if share > worst[0]:
                worst = (share, what + " " + where)
            assert cost == pytest.approx(float(job), rel=2e-4), what
            assert_state_equal(got, ref, exact=False, rtol=2e-6, atol=2e-7, what=what)
            _untouched_rows_are_untouched(init, got, V, D, I, J, what)
    print("partial n=%d hot=%s %s: largest share of the conflict-free tolerance used %.4f (%s)" % (n, hot, shuffle, worst[0], worst[1]))


def _bf16_rne(a):
    u = np.ascontiguousarray(a, np.float32).view(np.uint32)
    return (((u + 0x7FFF + ((u >> 16) & 1)) >> 16) << 16).astype(np.uint32).view(np.float32)


@pytest.mark.parametrize("hot", ["none", "all"])
@pytest.mark.parametrize("D", [52, 256])
def test_partial_chunks_bf16(gpu, D, hot):
    """bf16 rows on the same partial chunks: the assertions of test_bf16_conflict_free_batch -- fp32 tables to fp32 round-off, bf16
    rows within one bf16 ulp (stochastic rounding), untouched rows untouched -- for every size (bf16 rows exist in the blocked
    order only).  The zero-mean bound on the rounding error (|mean| < 0.01 ulp) is a statement about many samples (there: 4096
    rows): it is applied to the errors of all nine sizes together, 772 rows x dim, where the mean of unbiased roundings has a
    standard deviation of 0.002 ulp or less; one row of 52 elements would miss it by chance."""
    pooled = {"focus": [], "context": []}
    for shuffle in ("device",):
        for n in M.PARTIAL_SIZES:
            V, I, J, X, xmax = M.partial(n)
            dev = _create(V, I, J, X, xmax, D, mode="hogwild", shuffle=shuffle, seed=42, hot=hot, workers=16, dtype="bf16")
            st = dev.state()
            ref = {k: (v.reshape(V, -1) if v.size == V * D else v).astype(np.float32, copy=True) for k, v in st.items()}
            O.adagrad_job(D, I, J, X, xmax, O.COST_GLOVE, ref)
            dev.epoch(0)
            got = dev.state()
            dev.close()
            what = "bf16 n=%d hot=%s %s D=%d" % (n, hot, shuffle, D)
            for k in ("fbias", "cbias", "gsq_focus", "gsq_context", "gsq_fbias", "gsq_cbias"):
                np.testing.assert_allclose(got[k], ref[k].reshape(-1), rtol=3e-6, atol=1e-9, err_msg=what + " " + k)
                touched = np.zeros(V, bool); touched[I if k in ("fbias", "gsq_focus", "gsq_fbias") else J] = True
                m = np.repeat(~touched, got[k].size // V)
                assert np.array_equal(got[k][m], st[k][m]), (what, k)
            tables = ["focus"] if hot == "all" else ["focus", "context"]
            if hot == "all":
                np.testing.assert_allclose(got["context"], ref["context"].reshape(-1), rtol=3e-6,
                                           atol=2e-7 * float(np.max(np.abs(ref["context"]))), err_msg=what)
            for k in tables:
                g, r = got[k], ref[k].reshape(-1)
                touched = np.zeros(V, bool); touched[I if k == "focus" else J] = True
                m = np.repeat(touched, D)
                ulp = np.maximum(np.abs(r[m]), 1e-30) * 2.0 ** -7
                err = (g[m] - r[m]) / ulp
                slack = 2e-7 * float(np.max(np.abs(r))) / ulp
                assert np.all(np.abs(err) <= 1.0 + slack), (what, k, float(np.max(np.abs(err) - slack)))
                assert np.array_equal(g[~m], st[k][~m]), (what, k)
                pooled[k].append(err)
    for k, errs in pooled.items():
        if errs:
            e = np.concatenate(errs)
            print("bf16 D=%d hot=%s %s: mean rounding error %.5f ulp over %d elements" % (D, hot, k, float(np.mean(e)), e.size))
            assert abs(np.mean(e)) < 0.01, (k, float(np.mean(e)))


# ------------------------------------------------------------------ 3. edge X through all three cost_terms sites
EDGE = {"glove": M.glove_edge_x, "pglove": M.pglove_edge_x}


@pytest.mark.parametrize("method", ["glove", "pglove"])
@pytest.mark.parametrize("D", [8, 256])
def test_edge_x_deterministic_bit_exact(gpu, method, D):
    """cost_terms inline in k_adagrad_exact: three epochs bit for bit against O.Glove, as test_deterministic_epochs_bit_exact.  The
    oracle keeps subnormal X (as the JVM does); a device that flushed them would differ here."""
    V, I, J, X, xmax = EDGE[method]()
    cfg = make_config(D, method, threads=1, mode="deterministic", shuffle="java", seed=42)
    opt = geglove.Adagrad(geglove.CooMatrix(V, I, J, X, xmax), cfg, cfg.costFunction())
    ora = O.Glove(V, D, I, J, X, xmax, cost_kind(method), seed=42, threads=1)
    for it in range(3):
        c_dev = opt.epoch(it) / len(I)
        c_ora = ora.epoch()
        assert np.array_equal(opt.perm(), ora.perm)
        assert np.isfinite(c_dev) and c_dev == c_ora, "epoch %d cost %r vs oracle %r" % (it, c_dev, c_ora)
        assert_state_equal(opt.state(), ora, what="edge X %s D=%d epoch %d" % (method, D, it))
        for name, v in opt.state().items():
            assert np.all(np.isfinite(v)), (name, it)


@pytest.mark.parametrize("shuffle", ["device", "java"])         # device: the blocked layout's cost terms; java: k_cost_terms
@pytest.mark.parametrize("hot", ["none", "all"])
@pytest.mark.parametrize("method", ["glove", "pglove"])
@pytest.mark.parametrize("D", [8, 256])
def test_edge_x_hogwild(gpu, D, method, hot, shuffle):
    """The (l, w) the Hogwild kernel reads, computed once per nonzero at create time by the blocked layout (DEVICE shuffle) or by
    k_cost_terms (general order).  Conflict-free, so every X value sits on rows of its own and its (l, w) shows by itself:
    tolerances of test_hogwild_conflict_free_batch.  The weight is 1 for fp32(0.3) > xmax = 0.3 and just under 1 for its lower
    neighbour; everything stays finite."""
    V, I, J, X, xmax = EDGE[method]()
    dev = _create(V, I, J, X, xmax, D, method, mode="hogwild", shuffle=shuffle, seed=42, hot=hot, workers=16)
    init = _as2d(dev.state(), V, D)
    ref = {k: v.copy() for k, v in init.items()}
    job = O.adagrad_job(D, I, J, X, xmax, cost_kind(method), ref)
    cost = dev.epoch(0)
    got = _as2d(dev.state(), V, D)
    what = "edge X %s D=%d hot=%s %s" % (method, D, hot, shuffle)
    share, where = M.tolerance_share(got, ref, 2e-6, 2e-7)
    print("%s: share of the conflict-free tolerance used %.4f (%s); cost %.9g vs %.9g" % (what, share, where, cost, float(job)))
    assert np.isfinite(cost) and all(np.all(np.isfinite(v)) for v in got.values())
    assert cost == pytest.approx(float(job), rel=2e-4), what
    assert_state_equal(got, ref, exact=False, rtol=2e-6, atol=2e-7, what=what)
    _untouched_rows_are_untouched(init, got, V, D, I, J, what)


# ------------------------------------------------------------------ 4. cuts lose nothing with many workers
_HUB_TERMS = {}


@pytest.mark.parametrize("flush_every", [1, 4, 64])
def test_cut_hub_runs_lose_no_update_with_many_workers(gpu, flush_every):
    """One hub column of 3000 nonzeros under the library's own worker count, made countable the way
    test_no_focus_row_is_resident_in_two_workers counts rows: learning rate 0 and the bias accumulators at 1e30, so nothing moves
    and every nonzero's weighted cost wc is a constant.  gradSqContext[j] then grows by the sum over the column of (wc * focus)^2,
    whatever the order, the concurrency and the cuts -- unless a run's delta, or an update behind a cut, is lost.
    Bound (derived, not tuned): the kernel adds positive terms in fp32 -- each fma of a squared gradient onto the row in registers,
    each run's delta formed by one subtraction and published by one atomic add -- at most count_j + 2 runs_j roundings, each at
    most 2^-24 of the running total, which never exceeds the final one: relative error <= (count_j + 2 runs_j) 2^-24.  The terms
    themselves are computed as the kernel computes them (kernel_model: its dot product and cost terms, fp32 products squared
    exactly in fp64), so they carry no error of their own."""
    D = 8
    V, I, J, X, xmax = M.hub_column(3000)
    col = 3000
    cfg = make_config(D, "glove", mode="hogwild", shuffle="device", seed=42, hot="all", flush_every=flush_every, learning_rate=0.0)
    opt = geglove.Adagrad(geglove.CooMatrix(V, I, J, X, xmax), cfg, cfg.costFunction())
    info = opt.info()
    assert info["flush_min"] == flush_every and info["hot_nonzeros"] == len(I)
    assert info["runs"] >= -(-len(I) // flush_every)
    opt.set_state("gsq_fbias", np.full(V, 1e30, np.float32)); opt.set_state("gsq_cbias", np.full(V, 1e30, np.float32))
    before = _as2d(opt.state(), V, D)
    opt.epoch(0)
    after = _as2d(opt.state(), V, D)
    for name in ("focus", "context", "fbias", "cbias"):
        assert np.array_equal(after[name].view(np.uint32), before[name].view(np.uint32)), name       # nothing moves: wc is a constant
    vw, nch = info["vector_width"], info["chunks_per_lane"]
    F32, F64 = np.float32, np.float64
    key = (vw, nch)
    if key not in _HUB_TERMS:                                   # the same for every flush limit
        ctx = before["context"][col]
        total = np.ones(D, F64)                                 # gradSq starts at 1
        rows = np.ones((col, D), F32)
        for k in range(len(I)):
            f = before["focus"][I[k]]
            l, w = K.cost_terms(False, X[k], xmax)
            dot = K.lane_dot(ctx, f, vw, nch)
            ic = F32(F64(dot) + (F64(F32(before["cbias"][col] + before["fbias"][I[k]])) - l))
            wc = F32(w * ic)
            grad = (wc * f).astype(F32)
            total += grad.astype(F64) ** 2
            gf = (wc * ctx).astype(F32)
            rows[I[k]] = K.fma32(gf, gf, rows[I[k]])
        _HUB_TERMS[key] = (before, total, rows)
    first, total, rows = _HUB_TERMS[key]
    for name in before:
        assert np.array_equal(before[name], first[name]), name
    got = after["gsq_context"][col].astype(F64)
    bound = (len(I) + 2 * info["runs"]) * 2.0 ** -24
    rel = np.abs(got - total) / total
    smallest_term_share = 1.0 / len(I)
    print("flush_every %d, %d workers, %d runs: gradSq growth %.4f .. %.4f, relative error %.3g = %.4f of the bound %.3g (one update in %d is %.3g)"
          % (flush_every, info["groups_in_flight"], info["runs"], (got - 1).min(), (got - 1).max(), rel.max(), rel.max() / bound, bound, len(I),
             smallest_term_share))
    assert info["groups_in_flight"] > 1
    assert np.all(rel <= bound), (float(rel.max()), bound)
    # the other side: each focus row took exactly its one update (one fma onto 1), and the row nothing streams took none
    np.testing.assert_allclose(after["gsq_focus"][:col], rows, rtol=1e-6)
    assert np.array_equal(after["gsq_focus"][col], before["gsq_focus"][col])


_FROZEN_TERMS = {}


def _frozen_handle(V, I, J, X, xmax, D, dtype, **device):
    """Learning rate 0 and the bias accumulators at 1e30, under the library's own worker count: nothing but the accumulator rows
    moves, and every nonzero's weighted cost wc is a constant."""
    cfg = make_config(D, "glove", mode="hogwild", shuffle="device", seed=42, learning_rate=0.0, dtype=dtype, **device)
    opt = geglove.Adagrad(geglove.CooMatrix(V, I, J, X, xmax), cfg, cfg.costFunction())
    opt.set_state("gsq_fbias", np.full(V, 1e30, np.float32)); opt.set_state("gsq_cbias", np.full(V, 1e30, np.float32))
    return opt


def _frozen_terms(key, before, I, J, X, xmax, vw, nch, resident_ctx):
    """What the one resident row's accumulator must grow to (fp64 sum of the squared fp32 gradients, from 1) and what each streamed
    row's accumulator becomes after its one fma, with the terms computed as the kernel computes them (kernel_model: its dot
    product and cost terms).  Computed once per key; the tables it was computed from are kept to check that later callers share them."""
    if key not in _FROZEN_TERMS:
        F32, F64 = np.float32, np.float64
        D = before["focus"].shape[1]
        total = np.ones(D, F64)
        streamed = np.ones((before["focus"].shape[0], D), F32)
        for k in range(len(I)):
            f, c = before["focus"][I[k]], before["context"][J[k]]
            res, oth = (c, f) if resident_ctx else (f, c)
            l, w = K.cost_terms(False, X[k], xmax)
            dot = K.lane_dot(res, oth, vw, nch)
            ic = F32(F64(dot) + (F64(F32(before["cbias"][J[k]] + before["fbias"][I[k]])) - l))
            wc = F32(w * ic)
            total += (wc * oth).astype(F32).astype(F64) ** 2
            g = (wc * res).astype(F32)
            o = I[k] if resident_ctx else J[k]
            streamed[o] = K.fma32(g, g, streamed[o])
        _FROZEN_TERMS[key] = (before, total, streamed)
    first, total, streamed = _FROZEN_TERMS[key]
    for name in before:
        assert np.array_equal(before[name], first[name]), name
    return total, streamed


def _nothing_but_accumulators_moved(before, after, what):
    for name in ("focus", "context", "fbias", "cbias", "gsq_fbias", "gsq_cbias"):
        assert np.array_equal(after[name].view(np.uint32), before[name].view(np.uint32)), (what, name)


@pytest.mark.parametrize("flush_every", [1, 4, 64])
def test_cut_hub_runs_lose_no_update_with_many_workers_bf16(gpu, flush_every):
    """test_cut_hub_runs_lose_no_update_with_many_workers with bf16 rows: the hub column lives in its fp32 master row, which the runs
    read and publish into; the streamed focus rows are narrowed with stochastic rounding at every step, which on values bf16 already
    holds (learning rate 0) must change nothing -- rows and biases keep their bits.  Same terms (the hub row is fp32, the focus rows
    are what the bf16 table holds, vw = 4), same derived bound (count_j + 2 runs_j) 2^-24 on gradSqContext[j]; each focus row's
    accumulator took exactly its one fma."""
    D = 8
    V, I, J, X, xmax = M.hub_column(3000)
    col = 3000
    opt = _frozen_handle(V, I, J, X, xmax, D, "bf16", hot="all", flush_every=flush_every)
    info = opt.info()
    assert info["flush_min"] == flush_every and info["hot_nonzeros"] == len(I)
    assert info["runs"] >= -(-len(I) // flush_every)
    assert (info["vector_width"], info["chunks_per_lane"]) == (4, 1)
    before = _as2d(opt.state(), V, D)
    assert np.all(before["focus"].view(np.uint32) & 0xFFFF == 0)                # what the bf16 table holds
    opt.epoch(0)
    after = _as2d(opt.state(), V, D)
    opt.close()
    _nothing_but_accumulators_moved(before, after, "bf16 hub column flush_every %d" % flush_every)
    total, rows = _frozen_terms(("hub", "bf16"), before, I, J, X, xmax, 4, 1, True)
    got = after["gsq_context"][col].astype(np.float64)
    bound = (len(I) + 2 * info["runs"]) * 2.0 ** -24
    rel = np.abs(got - total) / total
    print("bf16 rows, flush_every %d, %d workers, %d runs: gradSq growth %.4f .. %.4f, relative error %.3g = %.4f of the bound %.3g (one update in %d is %.3g)"
          % (flush_every, info["groups_in_flight"], info["runs"], (got - 1).min(), (got - 1).max(), rel.max(), rel.max() / bound, bound, len(I),
             1.0 / len(I)))
    assert info["groups_in_flight"] > 1
    assert np.all(rel <= bound), (float(rel.max()), bound)
    np.testing.assert_allclose(after["gsq_focus"][:col], rows[:col], rtol=1e-6)
    assert np.array_equal(after["gsq_focus"][col:], before["gsq_focus"][col:])
    keep = np.ones(V, bool); keep[col] = False
    assert np.array_equal(after["gsq_context"][keep], before["gsq_context"][keep])


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_long_row_pieces_lose_no_update_with_many_workers(gpu, dtype):
    """The transpose: one focus row of 3000 nonzeros, cut into 24 pieces (23 x 128 + 56) that many workers hold at once.  Each
    piece publishes its accumulator delta with float atomics and the row itself by delta too -- atomics (fp32) or close_run()'s
    read-modify-write (bf16 rows) -- so with learning rate 0 the row must keep its bits whatever the pieces do to each other, and
    gradSqFocus[row] must grow by the sum over the row of (wc * context)^2.
    Bound (derived as above, not tuned): per piece one fma per nonzero onto the accumulator in registers, one subtraction that forms
    the delta, one atomic add that publishes it; every rounding is at most 2^-24 of a running value that never exceeds the final
    total (a piece starts from what the others have published so far, and its own terms are not in that yet): relative error
    <= (count + 2 pieces) 2^-24.  Each context row the row meets took exactly its one fma."""
    D = 8
    V, I, J, X, xmax = M.one_row(3000)
    row = 3000
    opt = _frozen_handle(V, I, J, X, xmax, D, dtype, hot="none")
    info = opt.info()
    pieces = -(-len(I) // 128)
    assert info["hot_nonzeros"] == 0 and info["long_rows"] == 1 and info["shared_chunks"] == pieces
    vw, nch = info["vector_width"], info["chunks_per_lane"]
    before = _as2d(opt.state(), V, D)
    opt.epoch(0)
    after = _as2d(opt.state(), V, D)
    opt.close()
    _nothing_but_accumulators_moved(before, after, "%s long row" % dtype)
    total, rows = _frozen_terms(("row", dtype), before, I, J, X, xmax, vw, nch, False)
    got = after["gsq_focus"][row].astype(np.float64)
    bound = (len(I) + 2 * pieces) * 2.0 ** -24
    rel = np.abs(got - total) / total
    print("%s rows, long row in %d pieces, %d workers: gradSq growth %.4f .. %.4f, relative error %.3g = %.4f of the bound %.3g (one update in %d is %.3g)"
          % (dtype, pieces, info["groups_in_flight"], (got - 1).min(), (got - 1).max(), rel.max(), rel.max() / bound, bound, len(I), 1.0 / len(I)))
    assert info["groups_in_flight"] > 1
    assert np.all(rel <= bound), (float(rel.max()), bound)
    np.testing.assert_allclose(after["gsq_context"][:row], rows[:row], rtol=1e-6)
    assert np.array_equal(after["gsq_context"][row:], before["gsq_context"][row:])
    keep = np.ones(V, bool); keep[row] = False
    assert np.array_equal(after["gsq_focus"][keep], before["gsq_focus"][keep])

"""The depth-2 walk: k_epoch_walk2 is k_epoch_ring with the ordinary walk two nonzeros deep -- the streamed pair
of nonzero p + 2 is requested at the top of step p into the third of three LDS images.  Forced with `deep_walk` on small matrices:

  * with one worker both kernels are the same sequential program on the same layout: after three epochs every state table and every
    epoch cost of a `deep_walk` handle has the bits of the `deep_panels` handle's -- through chunks shorter than the pipeline, the
    same streamed row at distance 1 and 2 (a request made in front of the stores it depends on), hub runs cut on consecutive steps,
    a long focus row in pieces, a chunk that is one run and a chunk of 128 runs;
  * the gate: a small handle without flags is the handle it was, no_deep_walk gives back k_epoch_ring, no_hub_panels wins;
  * many workers: the cost falls and the state stays finite; the convergence of a C2-shaped run, within the recorded margin.

Under a forcing flag every hub column but a last single one goes into tiles and panels, so one hub chunk never holds two columns:
the hub chunk's repeats of a streamed (focus) row are repeated nonzeros of that one column, at distance 1 and (three in a row) 2.
"""
import numpy as np
import pytest

import geglove
from geglove import capi
from helpers import make_config
from test_hub_tiles_gpu import CHUNK, C2_MARGIN, _create, _same_handle
from test_hub_panels_gpu import NO_PANELS, _designed

pytestmark = pytest.mark.gpu

HUB = 16               # the one hub column that stays a column-major hub chunk
SPARSE0 = 32           # first sparse column
BLOCKS = 60            # blocks of five one-nonzero rows


def _matrix(tail):
    """V = 2 048, row-major, with repeats.
      columns 0 .. 15   in all of rows 0 .. 63: one panel.
      column 16         rows 0 .. 59, every fifth of them twice and every seventh three times: the last hub column, alone, a hub
                        chunk whose streamed (focus) row repeats at distance 1 and 2.
      rows 100 .. 399   one nonzero each, in blocks of five rows with the columns a a b c b (three columns of the block's own): two
                        focus rows sharing a context column, adjacent (a a) and one apart (b c b); 300 consecutive runs of one
                        nonzero, so that one chunk holds 128 runs.
      row 500           300 nonzeros: a long row, three pieces (each a chunk of one run, published as a delta).
      rows 2000 .. 2002 129, 130 and 131 nonzeros: long rows whose last pieces are chunks of 1, 2 and 3 nonzeros.
      rows 600 ..       one nonzero each, as many as bring the sparse part to `tail` past a multiple of 128: under fixed_cuts the
                        last chunk holds `tail` nonzeros."""
    rows, cols = [], []
    for r in range(64):
        for c in range(16):
            rows.append(r); cols.append(c)
    for r in range(60):
        for _ in range(3 if r % 7 == 0 else 2 if r % 5 == 0 else 1):
            rows.append(r); cols.append(HUB)
    n_hub = len(rows)
    for k in range(BLOCKS):
        a, b, c = (SPARSE0 + 3 * k + q for q in range(3))
        for q, col in enumerate((a, a, b, c, b)):
            rows.append(100 + 5 * k + q); cols.append(col)
    for c in range(300):
        rows.append(500); cols.append(400 + c)
    for q, n in enumerate((129, 130, 131)):
        for c in range(n):
            rows.append(2000 + q); cols.append(400 + c)
    fill = (tail - (len(rows) - n_hub)) % CHUNK
    for q in range(fill):
        rows.append(600 + q); cols.append(800 + q)
    order = sorted(range(len(rows)), key=lambda k: (rows[k], cols[k]))
    I = np.array([rows[k] for k in order], np.int32); J = np.array([cols[k] for k in order], np.int32)
    rng = np.random.default_rng(17)
    X = (rng.random(len(I)) * 0.95 + 0.01).astype(np.float32)
    assert (len(I) - n_hub) % CHUNK == tail
    return 2048, I, J, X, float(X.max())


def _covered(order, I, J):
    """What the walk order holds of the patterns: (streamed context row at distance 1, at distance 2 with another between, streamed
    focus row of the hub column at distance 1, three times in a row)."""
    i, j = I[order], J[order]
    sp = j >= SPARSE0
    d1 = int(np.sum(sp[:-1] & sp[1:] & (j[:-1] == j[1:]) & (i[:-1] != i[1:])))
    d2 = int(np.sum(sp[:-2] & sp[2:] & (j[:-2] == j[2:]) & (j[:-2] != j[1:-1]) & (i[:-2] != i[2:])))
    hb = j == HUB
    h1 = int(np.sum(hb[:-1] & hb[1:] & (i[:-1] == i[1:])))
    h2 = int(np.sum(hb[:-2] & hb[1:-1] & hb[2:] & (i[:-2] == i[2:]) & (i[:-2] == i[1:-1])))
    return d1, d2, h1, h2


# ---- 1. one worker: the same bits as k_epoch_ring ---------------------------------------------------------------------------------
CASES = [([], 0, 1), ([], 1, 1), ([], 2, 1), ([], 3, 1), (["fixed_cuts"], 1, 1), (["fixed_cuts"], 2, 2), (["fixed_cuts"], 3, 3)]


@pytest.mark.parametrize("D", [8, 200])
@pytest.mark.parametrize("extra,flush,tail", CASES)
def test_deep_walk_and_ring_kernel_compute_the_same_bits(gpu, extra, flush, tail, D):
    V, I, J, X, xmax = _matrix(tail)
    kw = dict(workers=1, hot_theta=0.02, flush_every=flush)
    d = _create(V, I, J, X, xmax, D, layout=["deep_walk"] + extra, **kw)
    p = _create(V, I, J, X, xmax, D, layout=["deep_panels"] + extra, **kw)
    assert d.info() == p.info() and d.panel_info() == p.panel_info() and d.tile_info() == p.tile_info()
    assert d.info()["hot_columns"] == 17 and d.panel_info()["panel_columns"] == 16 and d.info()["hub_chunks"] > 0
    assert d.tile_info()["tile_chunks"] == 0
    if not extra:
        assert d.info()["long_rows"] == 4
    for it in range(3):
        od, op = d.epoch_order(it), p.epoch_order(it)
        assert od.tobytes() == op.tobytes()
        if it == 0:
            order = od.astype(np.int64)
            assert np.array_equal(np.sort(order), np.arange(len(I)))
            d1, d2, h1, h2 = _covered(order, I, J)
            assert d1 >= BLOCKS // 2 and d2 >= BLOCKS // 2 and h1 >= 12 and h2 >= 6, (d1, d2, h1, h2)
        cd, cp = d.epoch(it), p.epoch(it)
        assert np.isfinite(cd) and np.float64(cd).tobytes() == np.float64(cp).tobytes(), (it, cd, cp)
    sd, sp = d.state(), p.state()
    for name in sp:
        assert sd[name].tobytes() == sp[name].tobytes(), name


@pytest.mark.parametrize("flush", [0, 1, 5])
@pytest.mark.parametrize("pattern", ["first", "rotating"])
def test_the_ring_tests_matrices_through_the_deep_walk(gpu, pattern, flush):
    """The designed matrices of the panel and ring tests (35 hub columns: two panels and a tile group of three, 1 200 sparse
    nonzeros in packed row chunks)."""
    V, I, J, X, xmax = _designed(pattern)
    kw = dict(workers=1, hot_theta=0.005, flush_every=flush)
    d = _create(V, I, J, X, xmax, 200, layout=["deep_walk"], **kw)
    p = _create(V, I, J, X, xmax, 200, layout=["deep_panels"], **kw)
    assert d.info() == p.info() and d.panel_info() == p.panel_info() != NO_PANELS and d.tile_info() == p.tile_info()
    for it in range(3):
        assert d.epoch_order(it).tobytes() == p.epoch_order(it).tobytes()
        cd, cp = d.epoch(it), p.epoch(it)
        assert np.float64(cd).tobytes() == np.float64(cp).tobytes(), (it, cd, cp)
    sd, sp = d.state(), p.state()
    for name in sp:
        assert sd[name].tobytes() == sp[name].tobytes(), name


# ---- 2. gate and flags ---------------------------------------------------------------------------------------------------------
def test_small_handles_and_the_flags(gpu):
    V, I, J, X, xmax = _designed("rotating")
    D, kw = 200, dict(workers=1, hot_theta=0.005)
    a = _create(V, I, J, X, xmax, D, **kw)
    b = _create(V, I, J, X, xmax, D, layout=["no_deep_walk"], **kw)
    c = _create(V, I, J, X, xmax, D, layout=["no_hub_panels"], **kw)
    assert a.panel_info() == NO_PANELS == b.panel_info() and a.tile_info() == b.tile_info() == c.tile_info()
    _same_handle(a, b, "default against no_deep_walk")
    a = _create(V, I, J, X, xmax, D, **kw)
    _same_handle(a, c, "default against no_hub_panels")
    e = _create(V, I, J, X, xmax, D, layout=["deep_walk", "no_deep_walk"], **kw)          # everything deep_panels forces, and its kernel
    f = _create(V, I, J, X, xmax, D, layout=["deep_panels"], **kw)
    assert e.panel_info() == f.panel_info() != NO_PANELS and e.tile_info() == f.tile_info()
    _same_handle(e, f, "deep_walk + no_deep_walk against deep_panels")
    g = _create(V, I, J, X, xmax, D, layout=["deep_walk", "no_deep_panels"], **kw)        # no ring kernel: the panel kernel
    h = _create(V, I, J, X, xmax, D, layout=["hub_panels"], **kw)
    assert g.panel_info() == h.panel_info() != NO_PANELS
    _same_handle(g, h, "deep_walk + no_deep_panels against hub_panels")
    k = _create(V, I, J, X, xmax, D, layout=["deep_walk", "no_hub_panels"], **kw)         # never wins
    assert k.panel_info() == NO_PANELS and k.tile_info()["tile_chunks"] == 0 and k.info() == c.info()


# ---- 3. many workers -----------------------------------------------------------------------------------------------------------
def test_all_workers_racing_through_the_deep_walk(gpu):
    V, I, J, X, xmax = _designed("rotating")
    opt = _create(V, I, J, X, xmax, 200, workers=64, hot_theta=0.32, layout=["deep_walk"])     # 64 workers: the same 35 hub columns
    pi = opt.panel_info()
    assert opt.info()["hot_columns"] == 35
    assert pi["panel_columns"] == 32 and 1 <= pi["panel_blocks"] <= opt.info()["blocks"] == 16
    costs = []
    for it in range(3):
        assert np.array_equal(np.sort(opt.epoch_order(it).astype(np.int64)), np.arange(len(I)))      # every nonzero once, every epoch
        costs.append(opt.epoch(it) / len(I))
    print("cost per epoch, 64 workers:", costs, pi)
    assert costs[0] > costs[1] > costs[2] > 0
    for name, v in opt.state().items():
        assert np.all(np.isfinite(v)), name


# ---- 4. convergence at C2's shape ----------------------------------------------------------------------------------------------
def test_the_deep_walk_converges_like_the_column_major_hub_walk(gpu):
    """The run of test_panels_converge_like_the_column_major_hub_walk (100 k rows, 10 M nonzeros, D = 100, every worker, 5 epochs) with
    a deep_walk leg: its mean cost per epoch may exceed the no_hub_tiles leg's by at most that test's recorded margin (C2_MARGIN:
    three times the measured spread of the walk that is replaced)."""
    V, N, D, E = 100000, 10000000, 100, 5
    coo = capi.synth_coo(V, N, seed=2024)
    m = geglove.DeviceCooMatrix(coo)

    def leg(layout):
        cfg = make_config(D, "glove", mode="hogwild", shuffle="device", seed=42, layout=layout)
        opt = geglove.Adagrad(m, cfg, cfg.costFunction())
        pi = opt.panel_info()
        costs = [opt.epoch(it) / N for it in range(E)]
        opt.close()
        return np.array(costs), pi

    n1, p0 = leg(["no_hub_tiles"])
    dl, p1 = leg(["deep_walk"])
    coo.close()
    assert p0 == NO_PANELS and p1["panel_chunks"] > 0
    excess = float(np.max((dl - n1) / n1))
    print("cost per epoch: no_hub_tiles %s, deep_walk %s (%s); recorded margin %.5f, largest excess %.5f"
          % (np.round(n1, 6), np.round(dl, 6), p1, C2_MARGIN, excess))
    assert np.all(dl <= n1 * (1 + C2_MARGIN)), (dl, n1, C2_MARGIN)

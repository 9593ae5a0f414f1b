"""The ring kernel: k_epoch_ring walks hub panels like k_epoch_panels, but stage 0 of the pipeline keeps the focus
pairs of RING_K rows in flight in a ring of RING_K + 1 LDS images instead of one pair in the other of two images.  Forced with
`deep_panels` on small matrices:

  * with one worker both kernels are the same sequential program on the same layout: after three epochs every state table and every
    epoch cost of a `deep_panels` handle has the bits of the `hub_panels` handle's -- through rows with 0 .. 4 nonzeros in a group,
    cuts, chunks shorter than the ring is deep, and panels so sparse that three of the four stages pass nearly every pair through;
  * the oracle replays ge_glove_epoch_order, and the figures follow the rule test_hub_panels_gpu.py restates;
  * the gate: a small handle without flags is the handle it was, no_deep_panels gives back k_epoch_panels, no_hub_panels wins;
  * many workers: the cost falls and the state stays finite; the convergence of a C2-shaped run, within the recorded margin.
"""
import os
import re

import numpy as np
import pytest

import geglove
from geglove import capi
from helpers import make_config
from test_hub_tiles_gpu import CHUNK, C2_MARGIN, _create, _replay, _same_handle
from test_hub_panels_gpu import NO_PANELS, _designed, _finish, _check_figures, _groups

pytestmark = pytest.mark.gpu

_SRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "graph-embeddings_amd", "csrc", "glove.hip")
RING_K = int(re.search(r"#define GE_RING_K (\d+)", open(_SRC).read()).group(1))      # rows stage 0 requests ahead


def _bit_equal_run(V, I, J, X, xmax, D, method, epochs=3, **kw):
    """A deep_panels and a hub_panels handle on the same matrix, one worker each: the same figures, and after `epochs` epochs the
    same bits in every cost and every state table.  Returns the deep_panels handle's twin for the replay (a fresh handle)."""
    d = _create(V, I, J, X, xmax, D, method, layout=["deep_panels"], **kw)
    p = _create(V, I, J, X, xmax, D, method, layout=["hub_panels"], **kw)
    assert d.info() == p.info() and d.panel_info() == p.panel_info() and d.tile_info() == p.tile_info()
    assert p.panel_info()["panel_chunks"] > 0
    for it in range(epochs):
        assert d.epoch_order(it).tobytes() == p.epoch_order(it).tobytes()
        cd, cp = d.epoch(it), p.epoch(it)
        assert np.float64(cd).tobytes() == np.float64(cp).tobytes(), (it, cd, cp)
    sd, sp = d.state(), p.state()
    for name in sp:
        assert sd[name].tobytes() == sp[name].tobytes(), name
    return _create(V, I, J, X, xmax, D, method, layout=["deep_panels"], **kw)


# ---- 1. one worker: the same bits as k_epoch_panels, and the oracle's replay ------------------------------------------------------
@pytest.mark.parametrize("flush", [0, 1, 5])
@pytest.mark.parametrize("D", [4, 200, 252])
@pytest.mark.parametrize("pattern", ["first", "rotating"])
def test_ring_and_panel_kernel_compute_the_same_bits(gpu, pattern, D, flush):
    V, I, J, X, xmax = _designed(pattern)
    kw = dict(workers=1, hot_theta=0.005, flush_every=flush)
    d = _bit_equal_run(V, I, J, X, xmax, D, "glove", **kw)
    t = _create(V, I, J, X, xmax, D, "glove", layout=["hub_tiles", "no_hub_panels"], **kw)
    assert d.info()["hot_columns"] == 35
    _check_figures(d, t, V, D, I, J, flush)
    _replay(d, V, D, I, J, X, xmax, "glove", epochs=3)


@pytest.mark.parametrize("n_last", sorted({1, RING_K - 1, RING_K, RING_K + 1, 32}))
def test_chunks_shorter_than_the_ring(gpu, n_last):
    """16 columns in rows 0 .. 32 + n_last - 1: a chunk of 32 rows and one of n_last -- shorter than the ring is deep, exactly as
    deep, one more (requests against zero-sized resources fill the rest), and a second full chunk."""
    rng = np.random.default_rng(8)
    R = 32 + n_last
    rows = [r for r in range(R) for _ in range(16)]; cols = [c for _ in range(R) for c in range(16)]
    V, I, J, X, xmax = _finish(300, rows, cols, 16, 1200, rng)
    D, kw = 200, dict(workers=1, hot_theta=0.015)
    d = _bit_equal_run(V, I, J, X, xmax, D, "glove", **kw)
    t = _create(V, I, J, X, xmax, D, layout=["hub_tiles", "no_hub_panels"], **kw)
    assert d.info()["hot_columns"] == 16
    fills = _check_figures(d, t, V, D, I, J, 0)
    assert fills == [(CHUNK,) * 4, (4 * n_last,) * 4]
    _replay(d, V, D, I, J, X, xmax, "glove", epochs=3)


def _sparse_panels():
    """V = 1 500, 32 hub columns, column c in the rows r < 1024 with r % 16 == c % 16: a visited row of a panel holds ONE nonzero, in
    one stage, and the other three pass the pair through.  Behind them rows with three stages busy (columns q, 4 + q, 8 + q) and
    with two (q, 4 + q and 8 + q, 12 + q), one of each kind per column so that all counts stay equal and the groups are
    {0 .. 3}, {4 .. 7}, ... in both panels."""
    rng = np.random.default_rng(11)
    rows, cols = [], []
    for r in range(1024):
        for c in (r % 16, 16 + r % 16):
            rows.append(r); cols.append(c)
    r = 1024
    for base in (0, 16):
        for q in range(4):
            for grp_cols in ([q, 4 + q, 8 + q], [12 + q], [q, 4 + q], [8 + q, 12 + q], [12 + q]):
                for c in grp_cols:
                    rows.append(r); cols.append(base + c)
                r += 1
        # (columns 0 .. 11 of the panel: one row of three stages and one of two; columns 12 .. 15: three rows each -- one more)
        for q in range(12):
            rows.append(r); cols.append(base + q)
            r += 1
    return _finish(1500, rows, cols, 40, 3000, rng)


@pytest.mark.parametrize("flush", [0, 5])
def test_a_sparse_panel_passes_most_pairs_through(gpu, flush):
    V, I, J, X, xmax = _sparse_panels()
    D, kw = 200, dict(workers=1, hot_theta=0.005, flush_every=flush)
    d = _bit_equal_run(V, I, J, X, xmax, D, "pglove", **kw)
    t = _create(V, I, J, X, xmax, D, "pglove", layout=["hub_tiles", "no_hub_panels"], **kw)
    assert d.info()["hot_columns"] == 32 and d.panel_info()["panel_columns"] == 32
    _check_figures(d, t, V, D, I, J, flush)
    _, _, pgroups, tgroups, rest = _groups(J, V, d.info()["hot_threshold"])
    assert pgroups == [[4 * g + s for s in range(4)] for g in range(8)] and not tgroups and not rest
    busy = np.zeros((2, V), np.int64)                                        # per panel and row: stages with a nonzero
    for g, grp in enumerate(pgroups):
        busy[g // 4] += np.bincount(I[np.isin(J, grp)], minlength=V) > 0
    for pn in range(2):
        visited = busy[pn][busy[pn] > 0]
        assert (visited == 1).sum() >= 1024 and (visited == 2).sum() >= 4 and (visited == 3).sum() >= 4
    _replay(d, V, D, I, J, X, xmax, "pglove", epochs=3)


# ---- 2. gate and flags ---------------------------------------------------------------------------------------------------------
def test_small_handles_and_the_flags(gpu):
    V, I, J, X, xmax = _designed("rotating")
    D, kw = 200, dict(workers=1, hot_theta=0.005)
    a = _create(V, I, J, X, xmax, D, **kw)
    b = _create(V, I, J, X, xmax, D, layout=["no_deep_panels"], **kw)
    c = _create(V, I, J, X, xmax, D, layout=["no_hub_panels"], **kw)
    assert a.panel_info() == NO_PANELS == b.panel_info() and a.tile_info() == b.tile_info() == c.tile_info()
    _same_handle(a, b, "default against no_deep_panels")
    a = _create(V, I, J, X, xmax, D, **kw)
    _same_handle(a, c, "default against no_hub_panels")
    e = _create(V, I, J, X, xmax, D, layout=["deep_panels", "no_deep_panels"], **kw)      # the panels stay, the kernel is the old one
    f = _create(V, I, J, X, xmax, D, layout=["hub_panels"], **kw)
    assert e.panel_info() == f.panel_info() != NO_PANELS and e.tile_info() == f.tile_info()
    _same_handle(e, f, "deep_panels + no_deep_panels against hub_panels")
    g = _create(V, I, J, X, xmax, D, layout=["deep_panels", "no_hub_panels"], **kw)       # never wins
    assert g.panel_info() == NO_PANELS and g.tile_info()["tile_chunks"] == 0 and g.info() == c.info()


# ---- 3. many workers -----------------------------------------------------------------------------------------------------------
def test_all_workers_racing_through_the_ring(gpu):
    V, I, J, X, xmax = _designed("rotating")
    opt = _create(V, I, J, X, xmax, 200, workers=64, hot_theta=0.32, layout=["deep_panels"])    # 64 workers: the same 35 hub columns
    pi = opt.panel_info()
    assert opt.info()["hot_columns"] == 35
    assert pi["panel_columns"] == 32 and 1 <= pi["panel_blocks"] <= opt.info()["blocks"] == 16
    costs = [opt.epoch(it) / len(I) for it in range(3)]
    print("cost per epoch, 64 workers:", costs, pi)
    assert costs[0] > costs[1] > costs[2] > 0
    for name, v in opt.state().items():
        assert np.all(np.isfinite(v)), name


# ---- 4. convergence at C2's shape ----------------------------------------------------------------------------------------------
def test_the_ring_converges_like_the_column_major_hub_walk(gpu):
    """The run of test_panels_converge_like_the_column_major_hub_walk (100 k rows, 10 M nonzeros, D = 100, every worker, 5 epochs) with
    a deep_panels leg: its mean cost per epoch may exceed the no_hub_tiles leg's by at most that test's recorded margin (C2_MARGIN:
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
    dl, p1 = leg(["deep_panels"])
    coo.close()
    assert p0 == NO_PANELS and p1["panel_chunks"] > 0
    excess = float(np.max((dl - n1) / n1))
    print("cost per epoch: no_hub_tiles %s, deep_panels %s (%s); recorded margin %.5f, largest excess %.5f"
          % (np.round(n1, 6), np.round(dl, 6), p1, C2_MARGIN, excess))
    assert np.all(dl <= n1 * (1 + C2_MARGIN)), (dl, n1, C2_MARGIN)

"""CPU checks of the designed matrices (tests/designed.py), with the oracle alone.

  (a) each generator has the structure it promises;
  (b) on every structure matrix a single update is VISIBLE: replaying the array with any one nonzero left out moves some table by at
      least 10 x the replay tolerance of the one-worker GPU tests, so no position can hide a dropped or stale update;
  (c) the oracle's own `x > xmax` branch of GloveCost is exercised: adagrad_job on glove_edge_x() equals the independent Python
      model of test_oracle_kat.py bit for bit (and pGloVe's edge values likewise)."""
import numpy as np
import pytest

import oracle as O
import designed as M
from test_oracle_kat import py_update

F = np.float32


def _init_state(V, D, I, J, X, xmax, kind, seed=42):
    g = O.Glove(V, D, I, J, X, xmax, kind, seed=seed, threads=1)
    st = {k: np.ascontiguousarray(v, np.float32) for k, v in g.state().items()}
    g.close()
    return st


# ------------------------------------------------------------------ (a) structure
def test_one_column_and_one_row_structure():
    for n in (150, 300):
        V, I, J, X, xmax = M.one_column(n)
        assert V == n + 1 and np.array_equal(I, np.arange(n)) and np.all(J == n)
        V, I2, J2, X2, _ = M.one_row(n)
        assert V == n + 1 and np.array_equal(J2, np.arange(n)) and np.all(I2 == n)
        for x in (X, X2):
            assert x.dtype == np.float32 and x.min() >= F(0.02) and x.max() <= F(0.2) and xmax == float(F(0.2))
            assert x.max() / x.min() > 5                      # log-uniform over the decade, not bunched


def test_repeats_structure():
    V, I, J, X, xmax = M.repeats()
    assert V == 11 and I.max() < M.REPEAT_ROWS and J.max() < M.REPEAT_COLS
    assert 100 <= len(I) <= 140
    groups = M.back_to_back(I, J)
    assert groups.min() >= 1 and set(np.unique(groups).tolist()) >= {1, 2, 3, 4, 5}
    assert M.REPEAT_DRAWS - 4 <= len(groups) <= M.REPEAT_DRAWS      # two equal draws in a row merge into one longer group
    starts = np.concatenate([[0], np.cumsum(groups)[:-1]])
    pairs = I[starts].astype(np.int64) * 64 + J[starts]
    assert len(np.unique(pairs)) < len(pairs)                 # some pairs appear again later in the array
    assert len(np.unique(I)) == M.REPEAT_ROWS and len(np.unique(J)) >= 9
    assert X.min() >= F(0.02) and X.max() <= F(0.2)


def test_alternating_structure():
    V, I, J, X, xmax = M.alternating()
    assert V == 6 and len(I) == 80
    assert np.all(I[:40] == 0) and J[:40].tolist() == [1, 2] * 20
    assert np.all(J[40:] == 3) and I[40:].tolist() == [4, 5] * 20
    assert np.all(M.back_to_back(I, J) == 1)                  # never the same pair twice in a row: the streamed side alternates


def test_partial_structure():
    for n in M.PARTIAL_SIZES:
        V, I, J, X, xmax = M.partial(n)
        assert len(I) == n and M.is_conflict_free(I, J) and V - n >= 16
        assert X.min() > 1e-4 and X.max() <= F(0.2)
    assert {n % 128 for n in M.PARTIAL_SIZES} >= {1, 2, 63, 64, 65, 127, 0}


def test_edge_x_structure():
    V, I, J, X, xmax = M.glove_edge_x()
    assert M.is_conflict_free(I, J) and xmax == 0.3 and float(F(xmax)) != xmax          # a double fp32 cannot hold
    x3 = F(0.3)
    assert float(X[0]) > xmax > float(X[1]) and X[0] == x3 and X[1] < x3 < X[2]            # fp32(0.3) > 0.3 > its lower neighbour
    assert F(xmax) == X[0]                                     # an xmax narrowed to fp32 would compare equal: w < 1, wrong
    assert set(X[3:6].tolist()) == {F(0.6), F(300.0), F(1.0)}
    tiny = np.finfo(np.float32).tiny
    assert X[6] == F(1e-30) and X[7] == tiny and 0 < X[8] < tiny                           # subnormal, not flushed by numpy
    V, I, J, X, xmax = M.pglove_edge_x()
    assert M.is_conflict_free(I, J) and np.all((X > 0) & (X < 1))
    assert X[0] == F(0.5) and F(X[0] / F(F(1) - X[0])) == F(1)                              # l = log(1) = 0
    assert X[1] == np.nextafter(F(1), F(0)) and F(F(1) - X[1]) == F(2.0 ** -24)
    assert 0 < X[5] < np.finfo(np.float32).tiny


# ------------------------------------------------------------------ (b) a single update is visible
def _visibility(V, I, J, X, xmax, D, kind):
    """Smallest, over the nonzeros k, of the largest change (in units of the replay tolerance) that leaving k out makes to any
    table element."""
    st0 = _init_state(V, D, I, J, X, xmax, kind)
    full = {k: v.copy() for k, v in st0.items()}
    O.adagrad_job(D, I, J, X, xmax, kind, full)
    tol = {k: M.replay_tolerance(v) for k, v in full.items()}
    worst = np.inf
    keep = np.ones(len(I), bool)
    for k in range(len(I)):
        keep[k] = False
        st = {name: v.copy() for name, v in st0.items()}
        O.adagrad_job(D, I[keep], J[keep], X[keep], xmax, kind, st)
        keep[k] = True
        moved = max(float(np.max(np.abs(st[name].astype(np.float64) - full[name]) / tol[name])) for name in st)
        worst = min(worst, moved)
    return worst


@pytest.mark.parametrize("kind", [O.COST_GLOVE, O.COST_PGLOVE])
@pytest.mark.parametrize("D", [5, 6, 52, 256, 300])          # the dims of the GPU replays
@pytest.mark.parametrize("name", sorted(M.STRUCTURES))
def test_a_single_update_is_visible(name, D, kind):
    """A condition on the matrices, not a measurement of the trainer: were it not met, a replay could pass with an update lost."""
    V, I, J, X, xmax = M.STRUCTURES[name]()                   # at the size the GPU replays run (one_column, one_row: n = 300)
    worst = _visibility(V, I, J, X, xmax, D, kind)
    print("%s D=%d kind=%d: leaving one nonzero out moves a table by >= %.0f x the replay tolerance" % (name, D, kind, worst))
    assert worst >= 10.0


# ------------------------------------------------------------------ (c) the weight branch of the oracle
@pytest.mark.parametrize("D", [5, 8])
def test_oracle_takes_the_weight_branch_on_edge_x(D):
    V, I, J, X, xmax = M.glove_edge_x()
    st = _init_state(V, D, I, J, X, xmax, O.COST_GLOVE)
    py = {k: v.copy() for k, v in st.items()}
    # the inputs reach both sides of the branch, decided in fp64: fp32(0.3), its upper neighbour, 0.6, 300 and 1 lie above xmax
    assert (X.astype(np.float64) > xmax).tolist() == [True, False, True, True, True, True, False, False, False]
    cost = F(0)
    for k in range(len(I)):
        cost = py_update(O.COST_GLOVE, xmax, D, py, int(I[k]), int(J[k]), X[k], cost)
    job = O.adagrad_job(D, I, J, X, xmax, O.COST_GLOVE, st)
    assert job == float(cost)
    for name in st:
        assert np.array_equal(st[name].view(np.uint32), py[name].view(np.uint32)), name
        assert np.all(np.isfinite(st[name])), name
    # and the branch matters: with xmax narrowed to fp32 the first nonzero is weighted (0.3f / 0.3f)^0.75 = 1 too, but its lower
    # neighbour's weight changes, and with the comparison dropped 300.0 is weighted 1000^0.75
    other = _init_state(V, D, I, J, X, xmax, O.COST_GLOVE)
    O.adagrad_job(D, I, J, X, 1e9, O.COST_GLOVE, other)
    assert not np.array_equal(other["fbias"], st["fbias"])


@pytest.mark.parametrize("D", [5, 8])
def test_oracle_on_pglove_edge_x(D):
    V, I, J, X, xmax = M.pglove_edge_x()
    st = _init_state(V, D, I, J, X, xmax, O.COST_PGLOVE)
    py = {k: v.copy() for k, v in st.items()}
    cost = F(0)
    for k in range(len(I)):
        cost = py_update(O.COST_PGLOVE, xmax, D, py, int(I[k]), int(J[k]), X[k], cost)
    job = O.adagrad_job(D, I, J, X, xmax, O.COST_PGLOVE, st)
    assert job == float(cost)
    for name in st:
        assert np.array_equal(st[name].view(np.uint32), py[name].view(np.uint32)), name
        assert np.all(np.isfinite(st[name])), name

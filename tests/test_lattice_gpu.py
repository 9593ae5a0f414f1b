"""k_adagrad_runs on exact lattice walks (tests/lattice.py): the state is set so that every fp32 operation of the kernel is exact
and every stored row value is bf16-representable, so stochastic rounding is a no-op and a one-worker epoch is an integer recurrence
that lattice.walk() reproduces bit for bit.  Every comparison here is equality of words, for bf16 and fp32 handles alike:
  * focus and context equal the model; every other table keeps the bits it was given; the cost is exactly N / 2;
  * bf16 handles: extractResultF32() is the model's (focus + context) / 2, hub rows coming from their fp32 master rows.
This is what holds the code that exists only for a bf16 row read, updated and stored MORE than once to a sequential reference:
close_run()'s read-modify-write of a long row's piece, the two-source resident load and its state across a cut, emb_store's pack
order and the record strides, the bias behind the accumulator row, the re-read of a streamed row behind its own narrowed store, and
k_hub_rows on extraction.  A one-ulp tolerance sees none of it: an update is far below a bf16 ulp.
test_lattice.py shows on the CPU that every case stays inside the lattice (peak |k| <= 256, dot bound) and that a dropped update, a
dropped or doubled publish, a stale restart behind a cut and a hub row read from the bf16 table each change at least one word.
Nothing random remains: a difference is a finding, not noise."""
import numpy as np
import pytest

import geglove
from geglove import capi
import kernel_model as K
import lattice as L
from helpers import make_config, assert_state_equal

pytestmark = pytest.mark.gpu

LAYOUTS = [[], ["separate_tables"]]
CASE_IDS = [c.name for c in L.CASES]


def _create(case, D, dtype, layout, pglove=False):
    V, I, J = L.matrix(case.matrix)
    X = np.full(len(I), 0.5 if pglove else 1.0, np.float32)
    device = dict(mode="hogwild", shuffle="device", seed=5, hot=case.hot, workers=1, dtype=dtype, layout=layout,
                  learning_rate=L.learning_rate(pglove))
    if case.flush_every:
        device["flush_every"] = case.flush_every
    if case.hot_theta:
        device["hot_theta"] = case.hot_theta
    cfg = make_config(D, "pglove" if pglove else "glove", **device)
    return geglove.createOptimizer(cfg, geglove.CooMatrix(V, I, J, X, 1.0))


def _expect_path(dev, case):
    """The path the case was designed for is the one that ran."""
    V, I, J = L.matrix(case.matrix)
    info = dev.info()
    hubs = L.hub_columns(case, V, J)
    assert info["groups_in_flight"] == 1
    assert info["hot_nonzeros"] == int(hubs[J].sum()) and info["hot_columns"] == int(hubs.sum()), (case.name, info)
    if case.flush_every and hubs.any():
        assert info["flush_min"] == case.flush_every, (case.name, info["flush_min"])
    long_rows = int((np.bincount(I[~hubs[J]], minlength=V) > L.CHUNK).sum())
    assert info["long_rows"] == long_rows, (case.name, info["long_rows"])
    if (case.matrix == "long_row" and case.hot == "none") or case.matrix == "mixed":
        assert info["long_rows"] > 0 and info["shared_chunks"] > 0
    if case.matrix == "mixed":
        assert 0 < info["hot_nonzeros"] < len(I) and info["hub_chunks"] > 0


def _exact_epochs(case, D, dtype, layout, pglove=False):
    """Two epochs from the same state (iteration 0's chunk order, then iteration 1's), each against the model.  Returns the peaks."""
    V, I, J = L.matrix(case.matrix)
    N = len(I)
    dev = _create(case, D, dtype, layout, pglove)
    _expect_path(dev, case)
    fk, ck = L.rows(case.matrix, D)
    sent = L.state(fk, ck, case.sign)
    names = list(dev.state())
    assert names == list(capi.STATE_NAMES)
    peaks = []
    for it in range(2):
        what = "%s %s D=%d %s%s epoch %d" % (case.name, dtype, D, layout, " pglove" if pglove else "", it)
        for name in names:
            dev.set_state(name, sent[name])
        assert_state_equal(dev.state(), sent, exact=True, what=what + " as set")        # every value is one both formats hold
        order = dev.epoch_order(it).astype(np.int64)
        assert np.array_equal(np.sort(order), np.arange(N)), what
        cost = dev.epoch(it)
        got = dev.state()
        model = L.walk(I, J, order, fk, ck, case.sign)
        assert model.peak <= (L.PEAK_MAX if dtype == "bf16" else 2 ** 24 - 1), (what, model.peak)
        assert L.dot_bound_holds(D, model.peak), (what, model.peak)
        expect = dict(sent)
        expect["focus"], expect["context"] = L.to_f32(model.focus), L.to_f32(model.context)
        assert_state_equal(got, {k: expect[k] for k in names}, exact=True, what=what)
        assert cost == (N / 4.0 if pglove else N / 2.0), (what, cost)
        if dtype == "bf16":
            half = L.to_f32(model.focus + model.context) / np.float32(2)
            out = dev.extractResultF32()
            bad = np.nonzero(out.view(np.uint32) != half.reshape(-1).view(np.uint32))[0]
            assert bad.size == 0, (what, "extractResultF32", bad.size, "first at row", int(bad[0]) // D, "element", int(bad[0]) % D)
        peaks.append(model.peak)
    dev.close()
    return peaks


def test_rsq_of_one_is_exactly_one(gpu):
    """What the whole scheme rests on: __frsqrt_rn is the 1-ulp hardware reciprocal square root, and it must return exactly 1.0f at
    1.0f.  One nonzero, fp32 rows, accumulators 1, learning rate 1: the two rows must come back as a - b and b - a bit for bit."""
    assert L.G == 0
    I = np.array([0], np.int32); J = np.array([1], np.int32)
    D = 4
    cfg = make_config(D, "glove", mode="hogwild", shuffle="device", seed=5, hot="none", workers=1, learning_rate=1.0)
    dev = geglove.createOptimizer(cfg, geglove.CooMatrix(2, I, J, np.ones(1, np.float32), 1.0))
    fk = np.array([[3, -1, 2, 5], [0, 0, 0, 0]], np.int64); ck = np.array([[0, 0, 0, 0], [1, 4, -2, 7]], np.int64)
    sent = L.state(fk, ck)
    for name in dev.state():
        dev.set_state(name, sent[name])
    cost = dev.epoch(0)
    got = dev.state()
    dev.close()
    print("rsq(1.0f): focus row %s, context row %s (x 2^-%d), cost %r" % (
        (got["focus"][:D].astype(np.float64) * 2.0 ** L.S).tolist(), (got["context"][D:].astype(np.float64) * 2.0 ** L.S).tolist(), L.S, cost))
    expect = dict(sent)
    expect["focus"] = L.to_f32(np.array([fk[0] - ck[1], fk[1]])); expect["context"] = L.to_f32(np.array([ck[0], ck[1] - fk[0]]))
    assert_state_equal(got, {k: expect[k] for k in got}, exact=True, what="one nonzero")
    assert cost == 0.5


@pytest.mark.parametrize("layout", LAYOUTS, ids=["records", "separate_tables"])
@pytest.mark.parametrize("case", L.CASES, ids=CASE_IDS)
def test_bf16_rows_walk_the_lattice_bit_for_bit(gpu, case, layout):
    """Every bf16 lane shape (K.BF16_DIMS), inside records and in separate tables, both chunk orders."""
    peaks = [max(_exact_epochs(case, D, "bf16", layout)) for D in K.BF16_DIMS]
    print("%s bf16 %s: peak |k| %d" % (case.name, layout, max(peaks)))


@pytest.mark.parametrize("layout", LAYOUTS, ids=["records", "separate_tables"])
@pytest.mark.parametrize("case", L.CASES, ids=CASE_IDS)
def test_fp32_rows_walk_the_lattice_bit_for_bit(gpu, case, layout):
    """The fp32 AdaGrad instances with the bias in lane 63 (K.LANE63_DIMS): the one-worker replay of the existing tests (rtol 5e-5),
    tightened to equality on the same paths."""
    peaks = [max(_exact_epochs(case, D, "f32", layout)) for D in K.LANE63_DIMS]
    print("%s f32 %s: peak |k| %d" % (case.name, layout, max(peaks)))


@pytest.mark.parametrize("dtype,D", [("bf16", 260), ("f32", 254)])
def test_pglove_walks_the_lattice_bit_for_bit(gpu, dtype, D):
    """The other cost: X = 0.5 gives l = 0 and w = 0.5; with learning rate 2 the walk is the same and the cost N / 4."""
    _exact_epochs(L.CASE["mixed-auto-f3"], D, dtype, [], pglove=True)

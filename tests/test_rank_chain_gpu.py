"""Ranks on general floats are the header's fmaf chain, everywhere (ge_glove_rank_*, csrc/rank.hip): no bracket, no pair left out.
include/geglove.h states the arithmetic of a score exactly -- "s(k, c) is the fp32 fmaf chain from 0.0f over ascending d ...
z(k, c) = s(k, c) + cBias[c], one fp32 add" -- so with that chain in numpy (tests/chain_ref.py; it asserts its one condition, no
nonzero product below 2^-100) every rank, every reported score bit and the summary are determined, filters included.
test_rank_gpu.py holds general floats only inside a bracket that 80 % of the pairs decide; here all of them are held, at the tile
edges of its part A, plain and filtered, and once on every kind of handle.

That this is more than the bracket asks is shown on the CPU before the device is asked: in each case the ranks of the chain
differ from the ranks of the correctly rounded score (chain_ref.dot64) in at least one pair, so a kernel that summed otherwise
would fail.  Random columns alone would not show it at the small shapes (two scores a rounding error apart are rare among a
hundred columns), so every odd column of the first quarter is its left neighbour with every element moved by one ulp: the two
scores differ by about one rounding error and their order depends on how the sum was rounded.  At dim 1 the chain IS the
correctly rounded score (one product, one rounding), so there the two must agree, and that is asserted instead."""
import functools

import numpy as np
import pytest

import chain_ref as CH
import predict_ref as P
import rank_ref as R
from test_rank_gpu import KINDS, _handle, _set, _pairs, _filters, _rank

pytestmark = pytest.mark.gpu

# (V, D, n) of test_rank_gpu.test_exact_on_integer_tables, the shapes with more than one column; twin columns in every other one
CASES = [(2, 3, 63, False), (127, 32, 64, True), (128, 33, 65, False), (129, 50, 200, True), (300, 200, 64, False), (1000, 1024, 65, True),
         (300, 1, 200, False)]


def _tables(seed, V, D, twins):
    """General floats; column c of the first quarter, c odd, is column c - 1 with every element one ulp further from zero (and the
    same bias); with `twins` column c + V // 2 is a copy of column c."""
    F, C, fb, cb = P.float_tables(seed, V, D)
    for c in range(1, max(2, V // 4), 2):
        C[c] = np.nextafter(C[c - 1], np.float32(np.inf) * np.sign(C[c - 1])); cb[c] = cb[c - 1]
    if V == 2 and D >= 3:
        # two columns and two focus rows are four distinct pairs: too few to meet a rounding by chance, so row 0 is stated by hand.
        # a = (1, 1, 1).  b0 = (1, 2^-24, 2^-24): the chain twice meets 1 + 2^-24, a tie that rounds to even, and stays at 1; the
        # exact sum 1 + 2^-23 is representable.  b1 = (1, 1.5 * 2^-24, 0): both give 1 + 2^-23.  The chain puts column 1 first,
        # the correctly rounded scores tie and column 0 comes first.
        F[0] = 0; F[0, :3] = 1
        C[:] = 0; cb[:] = 0
        C[0, :3] = (1, 2.0 ** -24, 2.0 ** -24)
        C[1, :3] = (1, 1.5 * 2.0 ** -24, 0)
    if twins:
        m = V // 2
        C[m:2 * m] = C[:m]; cb[m:2 * m] = cb[:m]
    return F, C, fb, cb


def _targets(seed, n, V, rows=None):
    """n pairs; every other target is a column of the first quarter, where the neighbours one ulp apart are."""
    I, J = _pairs(seed, n, V, rows)
    J[::2] %= max(2, V // 4)
    return I, J


def _model(F, C, cb, I, J, filters, row_begin=0):
    """(ranks of the chain, the target's score bits, ranks of the correctly rounded score)."""
    A = F[np.asarray(I) - row_begin]
    Z = CH.chain(A, C) + cb[None, :]
    assert Z.dtype == np.float32 and np.all(np.isfinite(Z))
    Z64 = CH.dot64(A, C) + cb[None, :]
    assert Z64.dtype == np.float32
    return R.ranks(Z, J, filters), Z[np.arange(len(J)), J], R.ranks(Z64, J, filters)


def _check(h, I, J, filters, want, zt, what):
    rank, score, s = _rank(h, I, J, filters)
    bad = np.flatnonzero(rank != want)
    assert bad.size == 0, (what, "%d pairs differ; pair %d: rank %d, want %d" % (bad.size, bad[0], rank[bad[0]], want[bad[0]]))
    assert score.tobytes() == zt.tobytes(), (what, "score bits")
    assert s == R.summary(want), (what, s)


@functools.lru_cache(maxsize=None)
def _case(V, D, n, twins):
    F, C, fb, cb = _tables(2000 * V + D, V, D, twins)
    I, J = _targets(V + D + n, n, V)
    filters = _filters(7 * V + D, J, V)
    plain = _model(F, C, cb, I, J, None)
    filtered = _model(F, C, cb, I, J, filters)
    for what, (chain, _, rounded) in (("plain", plain), ("filtered", filtered)):
        differ = int((chain != rounded).sum())
        print("V %d dim %d n %d %s: the chain's rank is not the correctly rounded score's in %d pairs" % (V, D, n, what, differ))
        if D == 1:
            assert differ == 0                                       # one product, one rounding: the same arithmetic
        else:
            assert differ >= 1, "this case would not notice another order of summation"
    return F, C, fb, cb, I, J, filters, plain, filtered


@pytest.mark.parametrize("V,D,n,twins", CASES)
def test_every_rank_is_the_chains(gpu, V, D, n, twins):
    F, C, fb, cb, I, J, filters, plain, filtered = _case(V, D, n, twins)
    h = _handle(V, D)
    try:
        _set(h, F, C, fb, cb)
        _check(h, I, J, None, plain[0], plain[1], (V, D, n, "plain"))
        _check(h, I, J, filters, filtered[0], filtered[1], (V, D, n, "filtered"))
    finally:
        h.close()


@pytest.mark.parametrize("kind", list(KINDS))
def test_the_chain_on_every_kind_of_handle(gpu, kind):
    """One case per layout.  A bf16 handle rounds what set_state gives it, so its model runs on the tables get_state returns
    afterwards: focus rows and ordinary context rows widened from bf16, hub columns from their fp32 master rows -- the very
    values k_rank_stage reads (cBias stays fp32).  The model is then exact for it too; that every context row kept its fp32
    values, that the focus rows were in fact rounded, and -- as for every kind -- that the chain's ranks differ from the correctly
    rounded score's on these tables, are asserted before the ranking is asked."""
    V, D, n = 300, 40, 200
    lo, hi = KINDS[kind].get("row_range", (0, V))
    F, C, fb, cb = _tables(4343, V, D, True)
    I, J = _targets(98, n, V, rows=(100, 230))                     # rows every kind of handle owns
    filters = _filters(6, J, V)
    h = _handle(V, D, kind)
    try:
        _set(h, F, C, fb, cb, rows=KINDS[kind].get("row_range"))
        Fm, Cm, cbm = F[lo:hi], C, cb
        if kind == "bf16":
            assert h.info()["hot_columns"] > 0, "no column has an fp32 master row"
            Fm, Cm, cbm = (h.get_state(name).reshape(shape) for name, shape in (("focus", F.shape), ("context", C.shape), ("cbias", cb.shape)))
            assert Fm.dtype == np.float32 and not np.array_equal(Fm, F) and cbm.tobytes() == cb.tobytes()
            # hot="all": every context row has an fp32 master row and comes back with its fp32 values, so the neighbours one ulp
            # apart are still apart; only the focus rows were rounded
            exact = int((Cm == C).all(axis=1).sum())
            assert exact == V, "%d of %d context rows came back with their fp32 values" % (exact, V)
        for filt in (None, filters):
            chain, zt, rounded = _model(Fm, Cm, cbm, I, J, filt, row_begin=lo)
            differ = int((chain != rounded).sum())
            print("%s %s: the chain's rank is not the correctly rounded score's in %d pairs" % (kind, "filtered" if filt else "plain", differ))
            assert differ >= 1, "this case would not notice another order of summation"      # on the host, before the ranking is asked
            _check(h, I, J, filt, chain, zt, (kind, "filtered" if filt else "plain"))
    finally:
        h.close()

"""Fold-in on the device (ge_glove_fold_*, csrc/fold.hip) against the numpy restatement of the section (tests/fold_ref.py), word
for word in rows, biases and per-epoch costs.  The model is fed from ge_glove_get_state: the values the device reads in place,
whatever the handle's layout.  Handles are small (V = 300, fewer rows as dim grows) and trained for two epochs, so no table is
trivial; new rows have the lengths that meet an edge of the prefetch ring (1 .. 5) and of the 64-entry stream (63, 64, 65, 130)."""
import numpy as np
import pytest

import geglove
from geglove import capi, synth
import fold_ref as FR
import kernel_model as KM
from helpers import make_config

pytestmark = pytest.mark.gpu

V = 300
LENGTHS = (0, 1, 2, 3, 4, 5, 63, 64, 65, 130)
# name -> (method, opt, owned rows or None, device keys)
HANDLES = {
    "hogwild": ("glove", "adagrad", None, dict(mode="hogwild", shuffle="device", seed=42)),
    "hogwild-pglove": ("pglove", "adagrad", None, dict(mode="hogwild", shuffle="device", seed=42)),
    "hogwild-adam": ("glove", "adam", None, dict(mode="hogwild", shuffle="device", seed=42)),
    "separate": ("glove", "adagrad", None, dict(mode="hogwild", shuffle="device", seed=42, layout=["separate_tables"])),
    "packed": ("pglove", "adagrad", None, dict(mode="hogwild", shuffle="device", seed=42, layout=["packed_records"])),
    "bf16-hot-all": ("glove", "adagrad", None, dict(mode="hogwild", shuffle="device", seed=42, dtype="bf16", hot="all")),
    "bf16-hot-none": ("pglove", "adagrad", None, dict(mode="hogwild", shuffle="device", seed=42, dtype="bf16", hot="none")),
    "deterministic": ("glove", "adagrad", None, dict(mode="deterministic", shuffle="java", seed=42)),
    "stratified": ("glove", "adagrad", None, dict(mode="stratified", shuffle="device", seed=42)),
    "sharded": ("glove", "adagrad", (100, 200), dict(mode="hogwild", shuffle="device", seed=42, row_range=(100, 200))),
}


def _trained(name, D, vocab=V, epochs=2):
    method, opt, rows, device = HANDLES[name]
    I, J, X, xmax = synth.synthetic_coo(vocab, 8 * vocab, seed=11)
    if rows:
        keep = (I >= rows[0]) & (I < rows[1])
        I, J, X = I[keep], J[keep], X[keep]
    h = geglove.createOptimizer(make_config(D, method, opt=opt, **device), geglove.CooMatrix(vocab, I, J, X, xmax))
    for it in range(epochs):
        h.epoch(it)
    return h, method == "pglove", rows, xmax


def new_rows(lengths, lo, hi, pglove, xmax, seed, repeat_in=None):
    """(row_ptr, idx, X) of new rows of the given lengths with ids in [lo, hi); GloVe values reach past xmax."""
    rng = np.random.default_rng(seed)
    row_ptr = np.concatenate(([0], np.cumsum(lengths))).astype(np.int64)
    n = int(row_ptr[-1])
    idx = rng.integers(lo, hi, n).astype(np.int32)
    X = (0.01 + 0.9 * rng.random(n)).astype(np.float32) if pglove else (xmax * (0.05 + 1.5 * rng.random(n))).astype(np.float32)
    if repeat_in is not None:                                  # one id three times in that row
        a = int(row_ptr[repeat_in])
        idx[a + 1] = idx[a + 3] = idx[a]
    return row_ptr, idx, X


def _check(h, D, pglove, xmax, rows, side, row_ptr, idx, X, epochs, shuffle, seed, lr, state=None, init=None, vocab=V):
    state = state or h.state()
    table, bias, base = FR.frozen_side(state, side, D, vocab, rows)
    ir, ib = init if init else (None, None)
    f = capi.Folding(h._h, row_ptr, idx, X, side=side, epochs=epochs, shuffle=shuffle, lr=lr, seed=seed)
    try:
        got = f.run(ir, ib)
        assert f.kernel_ms > 0
        assert f.info == {"n_rows": len(row_ptr) - 1, "nnz": len(idx), "dim": D, "path": epochs * int(np.diff(row_ptr).max())}
    finally:
        f.close()
    want = FR.fold(D, row_ptr, idx, X, table, bias, xmax, pglove, epochs, shuffle, seed, lr if lr else 0.05, ir, ib, base)
    for what, a, b in zip(("rows", "bias", "cost"), got[:3], want[:3]):
        assert np.all(np.isfinite(b)), what
        bad = np.argwhere(FR.bits(a) != FR.bits(b))
        assert bad.size == 0, (what, side, epochs, shuffle, len(bad), bad[0], a[tuple(bad[0])], b[tuple(bad[0])])
    assert got[3].tobytes() == want[3].tobytes(), (got[3], want[3])
    return got


SHAPES = [(D, "f32") for D in KM.SHAPE_TABLE_DIMS] + [(D, "bf16") for D in KM.BF16_DIMS]      # bf16 rows exist for dim % 4 == 0 only


@pytest.mark.parametrize("D,emb", SHAPES)
def test_every_lane_shape(gpu, D, emb):
    vocab = min(V, 65536 // D)
    h, pglove, rows, xmax = _trained("bf16-hot-all" if emb == "bf16" else "hogwild", D, vocab=vocab)
    try:
        state = h.state()
        for side in ("focus", "context"):
            row_ptr, idx, X = new_rows((3, 0, 66, 1, 5), 0, vocab, pglove, xmax, seed=D)
            _check(h, D, pglove, xmax, rows, side, row_ptr, idx, X, 2, "device", 9, 0.0, state=state, vocab=vocab)
    finally:
        h.close()


@pytest.mark.parametrize("side", ["focus", "context"])
@pytest.mark.parametrize("shuffle", ["none", "device"])
def test_row_lengths_and_epochs(gpu, side, shuffle):
    D = 12
    h, pglove, rows, xmax = _trained("hogwild", D)
    try:
        state = h.state()
        row_ptr, idx, X = new_rows(LENGTHS * 3, 0, V, pglove, xmax, seed=3)
        for E in (1, 2, 5):
            _check(h, D, pglove, xmax, rows, side, row_ptr, idx, X, E, shuffle, 21, 0.1, state=state)
    finally:
        h.close()


@pytest.mark.parametrize("name", ["hogwild", "hogwild-pglove"])
def test_cost_kinds_repeated_ids_and_given_inits(gpu, name):
    D = 50
    h, pglove, rows, xmax = _trained(name, D)
    try:
        row_ptr, idx, X = new_rows((7, 0, 70, 2, 9), 0, V, pglove, xmax, seed=5, repeat_in=0)
        assert pglove or (np.any(X > xmax) and np.any(X < xmax))
        rng = np.random.default_rng(6)
        init = ((rng.standard_normal((5, D)) * 0.1).astype(np.float32), (rng.standard_normal(5) * 0.1).astype(np.float32))
        got = _check(h, D, pglove, xmax, rows, "focus", row_ptr, idx, X, 3, "device", 4, 0.05, init=init)
        assert np.array_equal(FR.bits(got[0][1]), FR.bits(init[0][1])) and got[1][1] == init[1][1] and not got[2][1].any()    # the empty row
        _check(h, D, pglove, xmax, rows, "context", row_ptr, idx, X, 3, "none", 4, 0.05, init=init)
    finally:
        h.close()


KINDS = [(name, D) for name in HANDLES for D in ((50, 6, 5) if name == "packed" else (48,) if name.startswith("bf16") else (50,))]


@pytest.mark.parametrize("name,D", KINDS)
def test_every_kind_of_handle(gpu, name, D):
    h, pglove, rows, xmax = _trained(name, D)
    try:
        state = h.state()
        if name == "bf16-hot-all":          # context rows that occur are read from their fp32 masters: not bf16 values any more
            assert np.any(state["context"].view(np.uint32) & 0xFFFF), "no master row differs from its bf16 rounding"
        lengths = (4, 0, 67, 1, 2)
        row_ptr, idx, X = new_rows(lengths, 0, V, pglove, xmax, seed=8)              # the focus side may name any column
        _check(h, D, pglove, xmax, rows, "focus", row_ptr, idx, X, 2, "device", 13, 0.0, state=state)
        lo, hi = rows if rows else (0, V)
        row_ptr, idx, X = new_rows(lengths, lo, hi, pglove, xmax, seed=9)
        _check(h, D, pglove, xmax, rows, "context", row_ptr, idx, X, 2, "device", 13, 0.0, state=state)
        if rows:                                                                      # a shard owns only its focus rows
            for bad in (lo - 1, hi, 0, V - 1):
                idx2 = idx.copy(); idx2[3] = bad
                with pytest.raises(capi.GeError) as e:
                    capi.Folding(h._h, row_ptr, idx2, X, side="context")
                assert e.value.status == capi.GE_ERR_ARG and "outside the frozen side's rows [100,200)" in str(e.value)
    finally:
        h.close()


def test_rows_are_independent_and_runs_repeat(gpu):
    D = 50
    h, pglove, rows, xmax = _trained("hogwild", D)
    try:
        row_ptr, idx, X = new_rows(LENGTHS, 0, V, pglove, xmax, seed=31)
        n = len(LENGTHS)
        kw = dict(side="focus", epochs=3, shuffle="device", lr=0.1, seed=17)

        def run(ptr, ids, x):
            f = capi.Folding(h._h, ptr, ids, x, **kw)
            try:
                a = f.run()
                b = f.run()
            finally:
                f.close()
            assert all(u.tobytes() == v.tobytes() for u, v in zip(a, b))                  # two runs, the same bytes
            return a

        base = run(row_ptr, idx, X)
        pieces = [(idx[row_ptr[r]:row_ptr[r + 1]], X[row_ptr[r]:row_ptr[r + 1]]) for r in range(n)]

        def assemble(order):
            ptr = np.concatenate(([0], np.cumsum([len(pieces[r][0]) for r in order]))).astype(np.int64)
            return ptr, np.concatenate([pieces[r][0] for r in order]), np.concatenate([pieces[r][1] for r in order])

        perm = np.random.default_rng(1).permutation(n)
        got = run(*assemble(perm))
        for k in range(3):
            assert got[k].tobytes() == base[k][perm].tobytes(), "another order"
        for r in (1, 6, 9):                                                                # alone
            got = run(*assemble([r]))
            for k in range(3):
                assert got[k].tobytes() == base[k][[r]].tobytes(), ("alone", r)
        big = np.concatenate([np.random.default_rng(2 + t).permutation(n) for t in range(10)])          # ten times as large
        got = run(*assemble(big))
        for k in range(3):
            assert got[k].tobytes() == base[k][big].tobytes(), "a larger set"
    finally:
        h.close()


def test_a_fold_in_is_a_pure_read(gpu):
    D = 50
    h, pglove, rows, xmax = _trained("hogwild-adam", D)
    try:
        snap = lambda: ([h.get_state(n).tobytes() for n in capi.ALL_STATE_NAMES], h.rng_state())
        before = snap()
        assert len(before[0]) == 12
        for side in ("focus", "context"):
            row_ptr, idx, X = new_rows(LENGTHS, 0, V, pglove, xmax, seed=41)
            _check(h, D, pglove, xmax, rows, side, row_ptr, idx, X, 2, "device", 1, 0.0)         # always AdaGrad, whatever the handle trains with
        assert snap() == before, "a fold-in wrote to the trainer"
    finally:
        h.close()


def test_refusals_that_need_the_handle(gpu):
    h, pglove, rows, xmax = _trained("deterministic", 1028, vocab=20, epochs=0)
    try:
        with pytest.raises(capi.GeError) as e:
            capi.Folding(h._h, [0, 1], [0], [0.1])
        assert e.value.status == capi.GE_ERR_ARG and "dim 1028 has no lane shape" in str(e.value)
    finally:
        h.close()
    h, pglove, rows, xmax = _trained("hogwild-pglove", 8, epochs=0)
    try:
        capi.Folding(h._h, [0, 2], [0, V - 1], [0.1, 0.9]).close()
        for side in ("focus", "context"):
            for bad in (V, 2 ** 31 - 1):
                with pytest.raises(capi.GeError) as e:
                    capi.Folding(h._h, [0, 2], [0, bad], [0.1, 0.9], side=side)
                assert e.value.status == capi.GE_ERR_ARG and "outside the frozen side's rows [0,300)" in str(e.value)
        for x in (1.0, 1.5):
            with pytest.raises(capi.GeError) as e:
                capi.Folding(h._h, [0, 2], [0, 1], [0.1, x])
            assert e.value.status == capi.GE_ERR_ARG and "not inside (0, 1)" in str(e.value)
        f = capi.Folding(h._h, [0, 2, 2], [0, 1], [0.1, 0.2], epochs=1)
        try:
            for v in (np.inf, -np.inf, np.nan):
                rows_in = np.zeros((2, 8), np.float32); rows_in[1, 7] = v
                with pytest.raises(capi.GeError) as e:
                    f.run(init_rows=rows_in)
                assert e.value.status == capi.GE_ERR_ARG and "non-finite input" in str(e.value)
                bias_in = np.zeros(2, np.float32); bias_in[0] = v
                with pytest.raises(capi.GeError) as e:
                    f.run(init_bias=bias_in)
                assert e.value.status == capi.GE_ERR_ARG and "non-finite input" in str(e.value)
            f.run()                                                                    # the set is still good
        finally:
            f.close()
    finally:
        h.close()

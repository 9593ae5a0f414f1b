"""Held-out evaluation on the device (ge_glove_eval_*, csrc/eval.hip) against the oracle, bit for bit.

Every kind of handle ge_glove_create can make is trained for two epochs (no table is trivial), its state is read once with
ge_glove_get_state, and one evaluation set of 2049 nonzeros -- repeated rows, repeated columns, one pair 65 times, values below
and above xmax -- is evaluated at every prefix length that meets an edge of the 64-nonzero wave tile or of the 1024-term sum
partition.  The reference is computed once per handle for the whole set (a prefix's terms are the set's):
  * (float)t_k of every nonzero from the oracle itself (eval_ref.oracle_terms: one one-nonzero job per k on a copy of the state);
  * residual, fp64 term and partitioned sum from the numpy restatement (eval_ref.model), which must agree with the oracle first.
Dims reach every column-piece edge (32) and both access paths (16-byte rows for dim % 4 == 0 on aligned tables, dwords
otherwise).  bf16 handles exist for dim % 4 == 0 only (the library refuses the others), so they run those dims.
Each evaluation must leave the twelve tables, the RNG state and the permutation byte-identical, and give the same bytes twice."""
import numpy as np
import pytest

import geglove
from geglove import capi, synth
import oracle as O
import eval_ref as R
from helpers import make_config, cost_kind, OPT_KIND
from test_eval_abi import eval_set

pytestmark = pytest.mark.gpu

V = 37
DIMS = (1, 3, 4, 31, 32, 33, 64, 65, 200, 300)
SIZES = (1, 63, 64, 65, 1024, 1025, 2049)
# name -> (method, opt, owned rows or None, device keys)
HANDLES = {
    "deterministic-glove": ("glove", "adagrad", None, dict(mode="deterministic", shuffle="java", seed=42)),
    "deterministic-pglove": ("pglove", "adagrad", None, dict(mode="deterministic", shuffle="java", seed=42)),
    "stratified": ("glove", "adagrad", None, dict(mode="stratified", shuffle="device", seed=42)),
    "hogwild": ("glove", "adagrad", None, dict(mode="hogwild", shuffle="device", seed=42)),
    "hogwild-packed": ("pglove", "adagrad", None, dict(mode="hogwild", shuffle="device", seed=42, layout=["packed_records"])),
    "hogwild-separate": ("glove", "adagrad", None, dict(mode="hogwild", shuffle="device", seed=42, layout=["separate_tables"])),
    "hogwild-adam": ("glove", "adam", None, dict(mode="hogwild", shuffle="device", seed=42)),
    "bf16-hot-all": ("glove", "adagrad", None, dict(mode="hogwild", shuffle="device", seed=42, dtype="bf16", hot="all")),
    "bf16-hot-none": ("pglove", "adagrad", None, dict(mode="hogwild", shuffle="device", seed=42, dtype="bf16", hot="none")),
    "sharded": ("glove", "adagrad", (10, 30), dict(mode="hogwild", shuffle="device", seed=42, row_range=(10, 30))),
}
CASES = [(name, D) for name in HANDLES for D in DIMS if not (name.startswith("bf16") and D % 4)]


def _trained(name, D, vocab=V, epochs=2):
    method, opt, rows, device = HANDLES[name]
    I, J, X, xmax = synth.synthetic_coo(vocab, 8 * vocab, seed=11)
    if rows:
        keep = (I >= rows[0]) & (I < rows[1])
        I, J, X = I[keep], J[keep], X[keep]
    h = geglove.createOptimizer(make_config(D, method, opt=opt, **device), geglove.CooMatrix(vocab, I, J, X, xmax))
    for it in range(epochs):
        h.epoch(it)
    return h, method, opt, rows, xmax


def _snapshot(h):
    names = capi.ALL_STATE_NAMES
    snap = {n: h.get_state(n).tobytes() for n in names if h._count(capi.ALL_STATE_NAMES.index(n)) > 0 and
            (h.OPT != capi.GE_OPT_ADAGRAD or not n.startswith("m2_"))}
    snap["rng_state"] = h.rng_state()
    if h._cfg.shuffle == capi.GE_SHUFFLE_JAVA:
        snap["perm"] = h.perm().tobytes()
    return snap


@pytest.mark.parametrize("name,D", CASES)
def test_residuals_terms_and_sum_match_the_oracle(gpu, name, D):
    h, method, opt, rows, xmax = _trained(name, D)
    try:
        cost = cost_kind(method)
        rb = rows[0] if rows else 0
        state = h.state()
        if name == "bf16-hot-all":          # every context row that occurs is read from its fp32 master: not a bf16 value any more
            ctx = state["context"].view(np.uint32)
            assert np.any(ctx & 0xFFFF), "no master row differs from its bf16 rounding"
        before = _snapshot(h)
        I, J, X = eval_set(V, max(SIZES), seed=1000 + D, rows=rows)
        want_res, want_term = R.model(state, D, I, J, X, xmax, cost, row_begin=rb)
        oracle32 = R.oracle_terms(state, V, D, I, J, X, xmax, cost, opt=OPT_KIND[opt], iteration=2, row_begin=rb)
        assert np.array_equal(R.bits32(want_term.astype(np.float32)), R.bits32(oracle32)), "the numpy model left the oracle"
        for n in SIZES:
            ev = capi.Evaluation(h._h, I[:n], J[:n], X[:n])
            try:
                res, term, total = ev.run()
                res2, term2, total2 = ev.run()
                only_sum = ev.run(residual=False, term=False)
                assert ev.kernel_ms() > 0
            finally:
                ev.close()
            bad = np.nonzero(R.bits32(res) != R.bits32(want_res[:n]))[0]
            assert bad.size == 0, (name, D, n, "residual", int(bad[0]), res[bad[0]], want_res[bad[0]])
            bad = np.nonzero(R.bits64(term) != R.bits64(want_term[:n]))[0]
            assert bad.size == 0, (name, D, n, "term", int(bad[0]), term[bad[0]], want_term[bad[0]])
            assert np.array_equal(R.bits32(term.astype(np.float32)), R.bits32(oracle32[:n]))
            want_total = R.partitioned_sum(want_term[:n])
            assert np.float64(total).tobytes() == np.float64(want_total).tobytes(), (name, D, n, total, want_total)
            assert res.tobytes() == res2.tobytes() and term.tobytes() == term2.tobytes() and total == total2       # two runs, the same bytes
            assert only_sum[0] is None and only_sum[1] is None and only_sum[2] == total
        assert _snapshot(h) == before, "an evaluation wrote to the trainer"
    finally:
        h.close()


def test_an_unsorted_set_comes_back_in_the_callers_order(gpu):
    """eval_set's rows arrive unsorted, so creation reorders them by focus row; a set sorted by row is taken as it is.  Both give
    the bytes of the model in the caller's order."""
    h, method, opt, rows, xmax = _trained("hogwild", 64)
    try:
        state = h.state()
        I, J, X = eval_set(V, 1500, seed=77)
        for order in (np.arange(1500), np.lexsort((J, I))):
            a, b, c = I[order], J[order], X[order]
            ev = capi.Evaluation(h._h, a, b, c)
            try:
                assert ev.reordered() == (not np.all(np.diff(a) >= 0))
                res, term, total = ev.run()
            finally:
                ev.close()
            want_res, want_term = R.model(state, 64, a, b, c, xmax, cost_kind(method))
            assert np.array_equal(R.bits32(res), R.bits32(want_res)) and np.array_equal(R.bits64(term), R.bits64(want_term))
            assert total == R.partitioned_sum(want_term)
    finally:
        h.close()


@pytest.mark.parametrize("name", ["deterministic-glove", "deterministic-pglove", "sharded"])
def test_limits_are_checked_on_the_host(gpu, name):
    h, method, opt, rows, xmax = _trained(name, 8, epochs=0)
    try:
        lo, hi = rows if rows else (0, V)
        ok = (np.array([lo, hi - 1], np.int32), np.array([0, V - 1], np.int32), np.array([0.1, 0.2], np.float32))
        capi.Evaluation(h._h, *ok).close()

        def refused(I=ok[0], J=ok[1], X=ok[2]):
            with pytest.raises(capi.GeError) as e:
                capi.Evaluation(h._h, I, J, X)
            return e.value.status == capi.GE_ERR_ARG

        bad_x = [0.0, -0.1, float("inf"), float("-inf"), float("nan")] + ([1.0, 1.5] if method == "pglove" else [])
        for x in bad_x:
            assert refused(X=np.array([0.1, x], np.float32)), x
        if method == "glove":
            capi.Evaluation(h._h, ok[0], ok[1], np.array([1.0, 7.5], np.float32)).close()       # GloVe takes any finite X > 0
        for j in (-1, V, 2 ** 31 - 1):
            assert refused(J=np.array([0, j], np.int32)), j
        for i in (lo - 1, hi, -1, V + 5):
            assert refused(I=np.array([lo, i], np.int32)), i
        assert refused(I=np.zeros(0, np.int32), J=np.zeros(0, np.int32), X=np.zeros(0, np.float32))      # n = 0
    finally:
        h.close()


@pytest.mark.parametrize("method", ["glove", "pglove"])
def test_the_terms_fold_into_the_trainers_own_epoch_cost(gpu, method):
    """Identity with the trainer itself: nonzeros (i, pi(i)) share no row and no column, so an epoch's updates leave every other
    nonzero's term alone, and a one-job deterministic epoch in matrix order adds exactly the terms evaluated before it:
    c = (float)((double)c + t_k) from 0.0f equals that epoch's cost_sum, bit for bit -- for two epochs in a row."""
    vocab, D = 64, 33
    pi = np.argsort(synth.splitmix64(5, vocab), kind="stable").astype(np.int32)
    I = np.arange(vocab, dtype=np.int32)
    X = eval_set(vocab, vocab, seed=9)[2]
    cfg = make_config(D, method, threads=1, mode="deterministic", shuffle="none", seed=42)
    h = geglove.createOptimizer(cfg, geglove.CooMatrix(vocab, I, pi, X, 0.2))
    try:
        ev = capi.Evaluation(h._h, I, pi, X)
        try:
            for it in range(2):
                _, term, _ = ev.run()
                c = np.float32(0.0)
                for t in term:
                    c = np.float32(np.float64(c) + t)
                cost = h.epoch(it)
                assert np.float64(cost).tobytes() == np.float64(c).tobytes(), (it, cost, float(c))
        finally:
            ev.close()
    finally:
        h.close()

"""The context exchange on the device (csrc/sync.hip, csrc/exchange.hip) against its numpy model (tests/exchange_ref.py), word for
word: the rank threads of this process meet in a local group (no spawn, no gloo, one process on the GPU), every rank's four
context-side tables are compared with the model as uint32 after EVERY exchange call, no element left out.  The wire is bf16 as in a
real run; the tables carry the designed words of exchange_ref (tests/test_exchange_ref.py shows what those can see)."""
import ctypes as C
import threading

import numpy as np
import pytest
import torch

import exchange_ref as R

pytestmark = pytest.mark.gpu
F = np.float32


def _masters(opt, V):
    """bool [V]: the columns whose row lives in an fp32 master row on this handle (bf16 handles; ge_context_layout.hub_index)."""
    from geglove import capi, parallel
    lay = capi.ContextLayout()
    capi.check(capi.lib().ge_glove_context_layout(opt._h, C.byref(lay)))
    if lay.dtype != capi.GE_DTYPE_BF16 or not lay.hub_index:
        return np.zeros(V, bool)
    idx = torch.as_tensor(parallel.DeviceArray(lay.hub_index, V, "<i4"), device=torch.device("cuda", 0)).cpu().numpy()
    return idx >= 0


def _against_the_model(V, D, world, wire, dtype="f32", layout=(), steps=R.STEPS, designed=True, matrix=None, nan_at=None, N=3000):
    """One case: every rank thread builds its Hogwild AdaGrad handle (a row shard of a small synthetic matrix; the context-side tables
    are V x D whatever the matrix), zeroes the edge elements, joins the group; rank 0 then plays the whole run on the model, which
    gives what set_state writes before every step and what every rank must hold after every call; every rank replays it on the device.
    Returns (differences, info): differences = [(call number, call, rank, table, words that differ, first index, device word, model word)]."""
    import geglove
    from geglove import parallel, synth
    from helpers import make_config
    I, J, X, xmax = matrix if matrix is not None else synth.synthetic_coo(V, N, seed=3)
    grp = parallel.LocalGroup(world)
    bar = threading.Barrier(world)
    start, masters, hubs, err = [None] * world, [None] * world, [None] * world, [None] * world
    script, bad, seen = [], [], [dict() for _ in range(world)]

    def body(r):
        opt = sync = None
        try:
            rows = parallel.shard_rows(V, world, r)
            si, sj, sx = parallel.shard_nonzeros(I, J, X, rows)
            cfg = make_config(D, "glove", mode="hogwild", shuffle="device", seed=42, row_range=rows, dtype=dtype, layout=list(layout))
            opt = geglove.Adagrad(geglove.CooMatrix(V, si, sj, sx, xmax), cfg, cfg.costFunction())
            t = {k: opt.get_state(k) for k in R.NAMES}
            if designed:
                R.zero_edges(t, V, D, world)
                for k in R.NAMES:
                    opt.set_state(k, t[k])
            start[r], masters[r] = {k: opt.get_state(k) for k in R.NAMES}, _masters(opt, V)
            bar.wait(timeout=300)
            sync = parallel.ContextSync(opt, world, r, wire=wire, accum_every=2, local_group=grp)
            hubs[r] = sync.hub_rows()
            bar.wait(timeout=300)
            if r == 0:
                model = R.Exchange(start, V, D, wire=wire, accum_every=2, rows=dtype, masters=masters, hubs=hubs[0])
                script.extend(R.play(model, V, D, steps=steps, designed=designed, nan_at=nan_at))
            bar.wait(timeout=600)
            for n, (call, sets, want) in enumerate(script):
                if sets is not None:
                    for k in R.NAMES:
                        opt.set_state(k, sets[r][k])
                getattr(sync, call)()
                for k in R.NAMES:
                    got = opt.get_state(k)
                    d = R.differing(got, want[r][k], nan_at if k == "context" else None)
                    if d.size:
                        bad.append((n, call, r, k, int(d.size), int(d[0]), hex(got.view(np.uint32)[d[0]]), hex(want[r][k].view(np.uint32)[d[0]])))
                    if nan_at is not None and k == "context":
                        seen[r][n] = got[nan_at]
        except Exception as e:              # noqa: BLE001 -- reported by the caller
            err[r] = e; grp.abort(); bar.abort()
        finally:
            if sync is not None: sync.close()
            if opt is not None: opt.close()

    th = [threading.Thread(target=body, args=(r,)) for r in range(world)]
    for t in th: t.start()
    for t in th: t.join(timeout=600)
    assert not any(t.is_alive() for t in th), "a rank thread did not end"
    assert all(e is None for e in err), err
    grp.close()
    assert len(script) >= len(steps) and all(np.array_equal(hubs[0], h) for h in hubs)
    return sorted(bad), dict(masters=masters, hubs=hubs[0], seen=seen, calls=[c for c, _, _ in script], start=start)


@pytest.mark.parametrize("case", R.SMALL_CASES, ids=[R.case_id(c) for c in R.SMALL_CASES])
def test_ge_sync_equals_the_numpy_model_word_for_word(gpu, case):
    """turn, turn, sync, turn, finish + begin, sync, replicate with the accumulators every second take, on a bf16 wire (one case: fp32,
    three ranks, for the group's sum order), at the smallest shapes that reach each kernel (exchange_ref.SMALL_CASES)."""
    dtype, D, layout, world, wire = case
    bad, info = _against_the_model(R.V_SMALL, D, world, wire, dtype=dtype, layout=layout)
    assert info["calls"] == ["turn", "turn", "sync", "turn", "finish", "begin", "sync", "replicate"]
    assert len(info["hubs"]) == 0                                # (a matrix this small has no busy column: the hub rows have their own test)
    assert not bad, "device and model differ (call, rank, table, words, first index, device, model): %s" % (bad[:8],)


def test_ge_sync_carries_a_nan_as_a_nan(gpu):
    """The same run with one element of rank 0's context rows set to a NaN whose payload sits in the low half only (0x7f800001; set_state
    copies without a finiteness check): narrowed by truncation, or rounded without the NaN branch, it would travel as an infinity.  Every
    rank holds a NaN there from the first land on (the payload is not compared), every other word is the model's."""
    nan_at = 7 * 32 + 5
    bad, info = _against_the_model(R.V_SMALL, 32, 2, "bf16", nan_at=nan_at)
    assert not bad, bad[:8]
    for r in range(2):
        assert set(info["seen"][r]) == set(range(len(info["calls"])))
        assert all(np.isnan(v) for n, v in info["seen"][r].items() if n >= 1 or r == 0), (r, info["seen"][r])


def test_flat4_second_pass_equals_the_model(gpu):
    """k_sync_turn_flat4 runs min(ceil(n4 / 1024), 8 CUs) blocks of 256 threads with four groups of four floats per thread, so its loop
    body repeats only when V D / 4 > 8 CUs 1024.  V is chosen on the device for 1.25 times that (plus a few rows, so that the second
    pass ends inside a slab of groups): dim 200, fat rows, two ranks, bf16 wire; two turns and a sync."""
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    D, one_pass = 200, 8 * cus * 1024
    V = -(-5 * one_pass // D) + 37                               # V D / 4 = 1.25 one_pass + 37 * 50
    assert one_pass < V * D // 4 < 2 * one_pass and (V * D // 4) % (cus * 8 * 256) != 0
    bad, info = _against_the_model(V, D, 2, "bf16", steps=("turn", "turn", "sync"))
    assert info["calls"] == ["turn", "turn", "sync"]
    assert not bad, bad[:8]


def _hub_matrix(V=2000, N=150000, world=2, extra=300):
    """synthetic_coo(V, N) plus one column that is busy (`extra` more nonzeros) inside rank 0's row block only and empty in every other
    block: a hub of the exchange (busy on some rank) that is a hub -- an fp32 master row -- on rank 0 and an ordinary bf16 row elsewhere."""
    from geglove import parallel, synth
    I, J, X, xmax = synth.synthetic_coo(V, N, seed=3)
    b, e = parallel.shard_rows(V, world, 0)
    elsewhere = np.bincount(J[(I < b) | (I >= e)], minlength=V)
    col = int(np.nonzero(elsewhere[b:e] == 0)[0][0]) + b
    free = np.setdiff1d(np.arange(b, e), I[J == col])[:extra]
    assert len(free) == extra
    I2 = np.concatenate([I, free.astype(np.int32)]); J2 = np.concatenate([J, np.full(extra, col, np.int32)])
    X2 = np.concatenate([X, np.full(extra, 0.05, np.float32)])
    order = np.argsort(I2, kind="stable")
    return (I2[order], J2[order], X2[order], xmax), col


@pytest.mark.parametrize("D", [32, 300])
def test_hub_rows_of_bf16_handles_equal_the_model(gpu, D):
    """k_hub_take<ROW16> / k_hub_land<ROW16>: two hub exchanges with moves of every row in between, then sync() and replicate(), all four
    tables against the model after every call.  The hub list must hold a row that is a master on one rank and an ordinary bf16 row on
    the other (landed there with the hashed rounding) and a row that is a master on both, or a branch of the land goes untested."""
    V = 2000
    matrix, col = _hub_matrix(V)
    bad, info = _against_the_model(V, D, 2, "bf16", dtype="bf16", steps=R.HUB_STEPS, designed=False, matrix=matrix)
    hubs, (m0, m1) = info["hubs"], info["masters"]
    assert len(hubs) > 0 and col in hubs
    assert np.any(m0[hubs] & m1[hubs]), "no hub row is a master on both ranks"
    assert np.any(m0[hubs] != m1[hubs]) and m0[col] and not m1[col], "no hub row is a master on one rank and a bf16 row on the other"
    assert info["calls"] == list(R.HUB_STEPS)
    assert not bad, bad[:8]


# ---- ge_exchange_turn_bf16, called directly ---------------------------------------------------------------------------------------------
def _loop_rows(D):
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    return -(-5 * 8 * cus * 256 // D) + 3                        # V D / 4 = 1.25 x (8 CUs blocks x 256 threads) and a few rows


@pytest.mark.parametrize("land,take", [(0, 1), (1, 0), (1, 1)])
@pytest.mark.parametrize("shape", [(1, 4), (37, 300), ("loop", 12)], ids=["1x4", "37x300", "loopx12"])
def test_exchange_turn_bf16_shapes(gpu, shape, land, take):
    """ge_exchange_turn_bf16 beyond the one shape of test_parallel_gpu's model test: a single group of four, 75 groups per row, and a table
    of 1.25 x (8 CUs x 256) groups, so that the kernel's grid-stride loop runs a second, partial pass.  Hubs (fp32 master rows) at row 0,
    at the last row and at two adjacent rows (the one-row table: none).  One element -- of a master row, or of the base in the one-row table -- is a
    NaN whose payload sits in the low half only: own and the value must come out as NaNs, not infinities (payloads are not compared)."""
    from geglove import capi
    V, D = shape
    if V == "loop":
        V = _loop_rows(D)
        n4, grid = V * D // 4, 8 * torch.cuda.get_device_properties(0).multi_processor_count * 256
        assert grid < n4 < 2 * grid and n4 % grid != 0
    rng = np.random.default_rng(100 * land + 10 * take + D)
    seed = 0x1234567
    hub_rows_at = [0, V // 2, V // 2 + 1, V - 1] if V >= 4 else []
    hub_index = np.full(V, -1, np.int32); hub_index[hub_rows_at] = np.arange(len(hub_rows_at))
    t16 = R.narrow(rng.standard_normal(V * D).astype(F))
    hub = rng.standard_normal(max(len(hub_rows_at), 1) * D).astype(F)
    is_hub = np.repeat(hub_index >= 0, D)
    t = R.widen(t16).copy()
    if hub_rows_at:
        t[is_hub] = hub[:len(hub_rows_at) * D]                   # (the rows ascend with their indices)
    b = (t + 0.01 * rng.standard_normal(V * D)).astype(F)
    w16 = R.narrow(0.02 * rng.standard_normal(V * D).astype(F)); o16 = R.narrow(0.01 * rng.standard_normal(V * D).astype(F))
    nan = np.array([0x7F800001], np.uint32).view(F)[0]
    nan_at = 1                                                   # element 1 of row 0: a master row's, or the base's
    if hub_rows_at: hub[nan_at] = nan
    else: b[nan_at] = nan
    dev = torch.device("cuda", 0)
    as_dev = lambda a: torch.from_numpy(a.view(np.int16) if a.dtype == np.uint16 else a).to(dev)
    d_t, d_b, d_w, d_o, d_hub, d_idx = map(as_dev, (t16.copy(), b.copy(), w16.copy(), o16.copy(), hub.copy(), hub_index))
    capi.check(capi.lib().ge_exchange_turn_bf16(d_t.data_ptr(), D, d_hub.data_ptr(), d_idx.data_ptr(), V, D, d_b.data_ptr(),
                                                d_w.data_ptr(), d_o.data_ptr(), land, take, seed, None))
    torch.cuda.synchronize()
    back = lambda x: x.cpu().numpy().view(np.uint16) if x.dtype == torch.int16 else x.cpu().numpy()
    exp_t16, exp_hub, exp_b, exp_o = R.turn_bf16_rows(t16, hub, hub_index.astype(np.int64), D, b, w16, o16, land, take, seed)
    got_t16, got_hub, got_b, got_o = back(d_t), back(d_hub), back(d_b), back(d_o)
    assert np.isnan(got_b[nan_at]) == np.isnan(exp_b[nan_at]) and (np.isnan(got_b[nan_at]) or not (take or not hub_rows_at))
    if take:                                                                                  # (base += own, a NaN)
        assert np.isnan(R.widen(got_o[nan_at:nan_at + 1]))[0] and np.isnan(R.widen(exp_o[nan_at:nan_at + 1]))[0]
        got_o[nan_at] = exp_o[nan_at]
    if hub_rows_at:
        assert np.isnan(got_hub[nan_at]) and np.isnan(exp_hub[nan_at])
    elif land:
        assert got_t16[nan_at] == exp_t16[nan_at]                                             # (an ordinary row's value was finite: only its base was not)
    np.testing.assert_array_equal(got_t16, exp_t16, err_msg="table")
    assert R.differing(got_b, exp_b, nan_at).size == 0, "base"
    assert R.differing(got_hub, exp_hub, nan_at if hub_rows_at else None).size == 0, "hub rows"
    np.testing.assert_array_equal(back(d_w), w16, err_msg="wire")                            # the receive buffer of the all-reduce: never written here
    np.testing.assert_array_equal(got_o, exp_o if take else o16, err_msg="own")

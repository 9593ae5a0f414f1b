"""The numpy model of the context exchange (tests/exchange_ref.py) and its designed tables, checked on the CPU: for every small case
test_exchange_gpu.py runs, that the designed inputs hold every edge they are there for, that the model has the properties the
exchange promises, and that each single fault the word-for-word comparison is there to catch changes at least one table word
somewhere in the GPU file's own step sequence.  A fresh handle's tables are stood in for by random ones of the same shapes (the
model takes them as given); the layouts of the GPU cases (fat rows, records) are the kernels' business and invisible here."""
import numpy as np
import pytest

import exchange_ref as R

F = np.float32
V = R.V_SMALL
ROW_CASES = sorted({(dtype, D, world, wire) for dtype, D, layout, world, wire in R.SMALL_CASES})
IDS = ["%s-D%d-w%d-%s" % c for c in ROW_CASES]


def start_tables(V, D, world, seed=5):
    """Stand-ins for the tables of `world` fresh handles of one seed: the same on every rank, edge elements zeroed."""
    rng = np.random.default_rng(seed)
    t = {"context": ((rng.random(V * D) - 0.5) / D).astype(F), "cbias": ((rng.random(V) - 0.5) / D).astype(F),
         "gsq_context": np.ones(V * D, F), "gsq_cbias": np.ones(V, F)}
    R.zero_edges(t, V, D, world)
    return [{k: v.copy() for k, v in t.items()} for _ in range(world)]


def model(case, fault=None, masters=None, hubs=(), V=V):
    dtype, D, world, wire = case
    return R.Exchange(start_tables(V, D, world), V, D, wire=wire, accum_every=2, rows=dtype, masters=masters, hubs=hubs, fault=fault)


def words(run):
    return [[np.concatenate([t[k].view(np.uint32) for k in R.NAMES]) for t in after] for _, _, after in run]


_RUNS = {}


def reference_run(case):
    if case not in _RUNS:
        _RUNS[case] = words(list(R.play(model(case), V, case[1])))
    return _RUNS[case]


# ---- the number formats -------------------------------------------------------------------------------------------------------------
def test_narrow_rounds_to_nearest_even_and_keeps_nans():
    w = lambda *u: np.array(u, np.uint32).view(F)
    got = R.narrow(w(0x3F808000, 0x3F818000, 0xBF808000, 0xBF818000, 0x3F807FFF, 0x3F808001, 0x3F7FFFFF, 0x00000000, 0x80000000, 0x00800000,
                     0x00008000, 0x00018000, 0x7F800000, 0x7F800001, 0xFFC00000, 0x7F7FFFFF))
    assert got.tolist() == [0x3F80, 0x3F82, 0xBF80, 0xBF82, 0x3F80, 0x3F81, 0x3F80, 0x0000, 0x8000, 0x0080,
                            0x0000, 0x0002, 0x7F80, 0x7FC0, 0xFFC0, 0x7F80]
    assert np.isnan(R.widen(got[13:15])).all() and np.isinf(R.widen(got[12:13])).all()
    x = np.random.default_rng(0).standard_normal(100000).astype(F)
    near = R.widen(R.narrow(x)).astype(np.float64)
    lo = R.widen(R.narrow(x, "truncate")).astype(np.float64)
    hi = R.widen((R.narrow(x, "truncate").astype(np.uint32) + 1).astype(np.uint16)).astype(np.float64)
    assert np.all(np.abs(near - x) <= np.minimum(np.abs(lo - x), np.abs(hi - x)))            # the nearer neighbour, whichever it is


def test_group_sums_follow_the_rank_order():
    a, b, c = (np.array([v], F) for v in (2.0 ** 24, 1.0, 1.0))
    assert R.group_sum_f32([a, b, c])[0] == F(2.0 ** 24) and R.group_sum_f32([b, c, a])[0] == F(2.0 ** 24 + 2)
    assert R.group_sum_f32([np.array([-0.0], F)]).view(np.uint32)[0] == 0                    # from +0.0f: a lone -0 comes out as +0
    h = R.narrow(np.array([1.0, 2.0 ** -8, 2.0 ** -8], F))
    assert R.widen(R.group_sum_bf16([h[:1], h[1:2], h[2:]]))[0] == F(1.0 + 2.0 ** -7)        # summed in fp32, rounded ONCE
    assert R.sqrt_f32(np.array([2.0], F))[0] == F(np.sqrt(2.0))
    assert R.merge_scale(np.array([1.0], F), np.array([-3.0], F), F(0.5))[0] == F(1)         # E = max(e, 0)
    assert R.merge_scale(np.array([1.0], F), np.array([3.0], F), F(0.0))[0] == F(1)


def test_seed_sequence():
    s = R.next_seed(0x5EED)
    assert s == (0x5EED * 1664525 + 1013904223) % 2 ** 32 and R.rank_seed(s, 0) == s and R.rank_seed(s, 3) == s ^ ((3 * 0x9E3779B1) % 2 ** 32)
    m = model(("bf16", 32, 2, "bf16"))
    m.turn(); assert m.seed == s                                 # one draw per launch of the bf16-row entry ...
    m.finish(); m.begin(); assert m.seed == R.next_seed(R.next_seed(s))
    f = model(("f32", 32, 2, "bf16"), hubs=[1, 2])
    f.turn(); assert f.seed == 0x5EED                            # ... none for fp32 tables ...
    f.hub_exchange(); assert f.seed == s                         # ... and one per hub exchange


# ---- the designed tables hold what they are for ----------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ROW_CASES, ids=IDS)
def test_every_edge_class_is_in_every_narrow_entry_at_its_first_take(case):
    """The first residual a narrow entry rounds (context rows: call 1; gradSqContext, lazy: call 2) holds every designed word exactly,
    alone on one rank and beside other ranks' words; an element of the edge block is moved by no rank, by one or by all; one rank's
    delta lies below half an fp32 ulp of the ranks' sum.  (bf16 rows hold only bf16 values, so there the classes are gradSqContext's.)"""
    dtype, D, world, wire = case
    m = model(case)
    run = R.play(m, V, D)
    next(run)
    sent = {"context": list(m.entry["context"]["sent"])}
    next(run)
    sent["gsq_context"] = list(m.entry["gsq_context"]["sent"])
    first, _ = R.edge_block(V, D, world, 0)
    n = len(R.EDGE)
    sec = (np.arange(V * D - first) // n) % (world + 2)
    for name in ("context", "gsq_context"):
        if wire != "bf16" or (name == "context" and dtype == "bf16"):
            continue
        got = np.stack([s[first:].view(np.uint32) for s in sent[name]])                      # [world, block]
        for cls, word in R.EDGE_WORDS:
            assert any(np.any(got[r][sec == r] == word) for r in range(world)), (name, cls, "alone")
            assert np.any(got[:, sec == world] == word), (name, cls, "beside the others")
        movers = (got & 0x7FFFFFFF != 0).sum(axis=0)
        assert {0, 1, world} <= set(movers.tolist()), (name, sorted(set(movers.tolist())))
        d = np.stack([s[first:] for s in sent[name]]).astype(np.float64)
        assert np.any((d != 0) & (np.abs(d) <= 2.0 ** -25 * np.abs(d.sum(axis=0))[None, :])), (name, "below the sum's ulp")


@pytest.mark.parametrize("world", [2, 3])
def test_mean_rule_elements(world):
    """cBias: elements moved by no rank, by one, by all, by +x and -x (sum 0, count 2), and a -0.0 move that must not count."""
    case = ("f32", 32, world, "bf16")
    m = model(case)
    run = R.play(m, V, 32)
    next(run)
    e = m.entry["cbias"]
    cnt, own = e["cnt"][0][V - R.MEAN_EDGE:], np.stack([o[V - R.MEAN_EDGE:] for o in e["own"]])
    assert cnt[1:7].tolist() == [1, world, 2, 1, 1, world]
    assert own[0].view(np.uint32)[4] == 0x80000000 and own[-1][4] == F(0.3)                  # the -0.0 went out and was not counted
    assert cnt[0] == 0 and cnt[7] == 0                                                        # (the designed elements have no random part in step 0)
    assert e["wire"][0][V - R.MEAN_EDGE + 3] == 0                                             # sum 0, count 2
    next(run)                                                                                # the land: the consensus moves by the mean over the movers
    got = e["base"][0][V - R.MEAN_EDGE:]
    assert got[1] == F(0.375) and got[4] == F(0.3) and got[3] == 0                            # one mover: its whole move, not 1 / world of it
    want = R.group_sum_f32([np.array([F(0.1) * F(r + 1)], F) for r in range(world)]) / F(world)
    assert got[2] == want[0]


# ---- what the exchange promises, on the model ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ROW_CASES, ids=IDS)
def test_consensus_and_replicas(case):
    """After every call the consensus (the base of an fp32 table) is the same words on every rank, and after replicate() so are the
    tables, whatever the wire.  With an fp32 wire -- and for the entries that always travel as fp32 -- a table IS the consensus after a
    sync() that found nothing in flight: the land recomputes the very difference the take sent, fl(table - c) - own = 0.  (A sync()
    behind a turn() lands on table' = fl(c' + resid), and fl(table' - c') gives resid back only up to table's rounding; what is left,
    half an ulp at most, goes out with the next take like everything else.  So that promise is checked on a run of sync() calls.)"""
    dtype, D, world, wire = case
    m = model(case)
    for call, _, after in R.play(m, V, D):
        for e in m.ent:
            if e["rows16"]:
                continue                                         # (bf16 rows: base = consensus + own in flight, per rank)
            for r in range(world):
                assert R.differing(e["base"][r], e["base"][0]).size == 0, (call, e["name"], r)
                if call == "replicate":
                    assert R.differing(m.get(r, e["name"]), e["base"][r]).size == 0, (call, e["name"], r)
    m = model(case)
    for call, _, after in R.play(m, V, D, steps=("sync",) * 4):
        for e in m.ent:
            if e["rows16"] or e["w16"] or e["taken_at"] != m.calls:
                continue
            for r in range(world):
                assert R.differing(m.get(r, e["name"]), e["base"][r]).size == 0, (m.calls, e["name"], r)
        assert wire == "bf16" or all(R.differing(after[r][k], after[0][k]).size == 0 for r in range(world) for k in ("context", "cbias"))


@pytest.mark.parametrize("case", [c for c in ROW_CASES if c[3] == "bf16"], ids=[i for c, i in zip(ROW_CASES, IDS) if c[3] == "bf16"])
def test_error_feedback_is_exact_and_bounds_the_replicas(case):
    """A bf16 wire.  (1) What narrowing drops, resid - widen(narrow(resid)), is exact in fp32: bf16 keeps the upper 8 of resid's 24
    significant bits rounded to nearest, so the difference is a multiple of resid's last place and at most half a bf16 ulp -- 2^(e-8)
    <= 2^-8 |resid| for |resid| in [2^e, 2^(e+1)), 2^-134 below the smallest normal -- i.e. at most 16 bits wide: nothing of a delta
    is ever lost, only postponed.
    (2) After sync() nothing is in flight and a rank's table is fl(c + left) with left = fl(fl(table' - c') - own) the part of the sent
    residual that narrowing dropped: |left| <= 2^-8 |sent| up to the two fp32 roundings of table' = fl(c' + sent) and of the difference,
    and fl(c + left) adds one more; each is at most half an ulp of the larger of |table| and |c| before or after the land.  So
        |table - c| <= max(2^-8 |sent|, 2^-134) + 2 ulp(max(|table|, |c|, |c'|)).
    A statement about the model (the device is held to the model's words, not to this bound)."""
    dtype, D, world, wire = case
    m = model(case)
    for call, _, after in R.play(m, V, D):
        for e in m.ent:
            if not e["w16"] or e["rows16"]:
                continue
            for r in range(world):
                s = e["sent"][r]
                if s is None:
                    continue
                with np.errstate(invalid="ignore"):
                    left32 = s - R.widen(R.narrow(s))
                left64 = s.astype(np.float64) - R.widen(R.narrow(s)).astype(np.float64)
                assert np.array_equal(left32.astype(np.float64), left64), (call, e["name"], r)
                half = np.maximum(2.0 ** -8 * np.abs(s.astype(np.float64)), 2.0 ** -134)
                assert np.all(np.abs(left64) <= half), (call, e["name"], r)
                if call == "sync" and e["taken_at"] == m.calls:
                    t, c, c0 = (x.astype(np.float64) for x in (m.get(r, e["name"]), e["base"][r], e["sent_base"][r]))
                    big = np.maximum(np.maximum(np.abs(t), np.abs(c)), np.abs(c0)).astype(F)
                    assert np.all(np.abs(t - c) <= half + 2.0 * np.spacing(big).astype(np.float64)), (e["name"], r)


# ---- every fault is seen ------------------------------------------------------------------------------------------------------------
# (the rounding, the packing and the partial group are the narrow kernels': on an fp32 wire those faults have nothing to strike)
ANY_WIRE = ("no_feedback", "base_not_landed", "mean_by_world", "lazy_wrong_calls")
FAULT_CASES = [(c, f) for c in ROW_CASES for f in R.FAULTS if c[3] == "bf16" or f in ANY_WIRE]


@pytest.mark.parametrize("case,fault", FAULT_CASES, ids=["%s-%s" % (IDS[ROW_CASES.index(c)], f) for c, f in FAULT_CASES])
def test_every_fault_changes_a_table_word(case, fault):
    """One fault at a time, over the GPU file's step sequence at each of its small shapes: some word of some rank's tables after some
    call differs from the right model's."""
    ref = reference_run(case)
    got = words(list(R.play(model(case, fault=fault), V, case[1])))
    assert any(np.any(a != b) for ga, ra in zip(got, ref) for a, b in zip(ga, ra)), fault


def test_the_designed_words_show_a_rounding_fault_at_the_first_land():
    """Two ranks, the rows' first four turns.  Rounding ties away from zero differs from nearest-even on ties only.  The first
    residual of a random move of 1e-2 is never one, so under random moves alone that fault changes no word before the third turn (by
    then the residuals are what narrowing dropped, 16 bits wide, and some of those tie); with the designed words it shows at the
    first land -- a take changes no table, so not before the second turn, which is why the sequence is several turns long."""
    case, V = ("f32", 32, 2, "bf16"), 8
    runs = {}
    for designed in (False, True):
        for fault in (None, "ties_away"):
            m = model(case, fault=fault, V=V)
            out = []
            for i in range(4):
                for r in range(2):
                    new = R.moves(m.tables(r), V, 32, 2, r, i, designed=designed)
                    for k in R.NAMES:
                        m.set(r, k, new[k])
                m.turn()
                out.append(np.concatenate([m.get(r, "context").view(np.uint32) for r in range(2)]))
            runs[designed, fault] = out
    plain = [int(np.sum(a != b)) for a, b in zip(runs[False, None], runs[False, "ties_away"])]
    diff = [int(np.sum(a != b)) for a, b in zip(runs[True, None], runs[True, "ties_away"])]
    assert plain[:2] == [0, 0] and diff[0] == 0 and diff[1] > 0, (plain, diff)


# ---- bf16 rows: master rows and the hub exchange --------------------------------------------------------------------------------------
HUB_V = 64
HUB_MASTERS = ([0, 5, 6, HUB_V - 1], [5, 9, HUB_V - 1])        # rank 0's and rank 1's hub columns: 5 and the last on both, 0, 6, 9 on one
HUB_LIST = sorted(set(HUB_MASTERS[0]) | set(HUB_MASTERS[1]))


def hub_model(D, fault=None, dtype="bf16"):
    masters = [np.isin(np.arange(HUB_V), h) for h in HUB_MASTERS]
    rng = np.random.default_rng(5)
    t = {"context": R.widen(R.narrow(((rng.random(HUB_V * D) - 0.5) / D).astype(F))), "cbias": ((rng.random(HUB_V) - 0.5) / D).astype(F),
         "gsq_context": np.ones(HUB_V * D, F), "gsq_cbias": np.ones(HUB_V, F)}      # (rows that bf16 holds: a master row starts as its bf16 entry)
    return R.Exchange([t, t], HUB_V, D, wire="bf16", accum_every=2, rows=dtype, masters=masters if dtype == "bf16" else None, hubs=HUB_LIST, fault=fault)


@pytest.mark.parametrize("D", [32, 300])
@pytest.mark.parametrize("steps", [R.HUB_STEPS, R.STEPS], ids=["hub_steps", "steps"])
@pytest.mark.parametrize("fault", R.FAULTS_BF16_ROWS)
def test_bf16_row_faults_change_a_table_word(D, steps, fault):
    """A landed ordinary row narrowed to nearest even instead of by the hash, and a hub row read from its (stale) bf16 entry instead
    of its master: both change a word in the large exchange's sequence and -- the second -- in the hub exchange's."""
    ref, got = (words(list(R.play(hub_model(D, f), HUB_V, D, steps=steps, designed=False))) for f in (None, fault))
    assert any(np.any(a != b) for ga, ra in zip(got, ref) for a, b in zip(ga, ra))


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_hub_exchange_leaves_the_hub_rows_as_the_consensus(dtype):
    """After a hub exchange every rank's hub rows of all four tables are their bases (fp32 rows and master rows: the same words;
    an ordinary bf16 entry: the hashed rounding of it, within one bf16 ulp), equal on all ranks; no other row moves."""
    D = 32
    m = hub_model(D, dtype=dtype)
    el = (np.array(HUB_LIST)[:, None] * D + np.arange(D)).reshape(-1)
    other = np.setdiff1d(np.arange(HUB_V * D), el)
    for call, sets, after in R.play(m, HUB_V, D, steps=R.HUB_STEPS[:2], designed=False):
        for r in range(2):
            for k in ("gsq_context", "context"):
                assert np.array_equal(after[r][k][other], sets[r][k][other] if dtype == "f32" or k != "context" else R.widen(R.narrow_plain(sets[r][k]))[other])
                base = m.entry[k]["base"][r]
                assert np.array_equal(base, m.entry[k]["base"][0])
                if k == "context" and dtype == "bf16":
                    ms = np.repeat(m.masters[r][HUB_LIST], D)
                    assert np.array_equal(after[r][k][el][ms], base[el][ms])
                    assert np.all(np.abs(after[r][k][el][~ms] - base[el][~ms]) <= np.abs(base[el][~ms]) * 2.0 ** -7)
                    assert np.any(after[r][k][el][~ms] != base[el][~ms])
                else:
                    assert np.array_equal(after[r][k][el], base[el])
            for k in ("cbias", "gsq_cbias"):
                assert np.array_equal(after[r][k][HUB_LIST], m.entry[k]["base"][r][HUB_LIST])

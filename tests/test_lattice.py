"""The lattice walks of tests/lattice.py, checked on the CPU: for every case test_lattice_gpu.py runs, the conditions under which the
kernel's arithmetic is exact, and that each single fault the exact comparison is there to catch changes at least one word.

The update acts on each element of a row by itself and lattice.rows(name, D) is a prefix of rows(name, 1024), so two dims cover all
the GPU file uses: the peak over 1024 elements bounds the peak of every dim, and a condition or a difference that holds in the first
four elements holds at every dim from 4 on.  The walk order is the layout rule of csrc/ge_layout.h restated (lattice.layout), under
the chunk order as laid out and under one permutation of the chunks."""
import numpy as np
import pytest

import kernel_model as K
import lattice as L

GPU_DIMS = sorted(set(K.BF16_DIMS) | set(K.LANE63_DIMS))
SMALLEST = min(GPU_DIMS)
assert SMALLEST == 4 and max(GPU_DIMS) == L.DMAX

# the fault kinds that must find a place to strike in a case (in at least one of the two chunk orders)
MUST_STRIKE = {
    "long_row-none": {"drop_update", "drop_publish", "double_publish", "stale_restart"},
    "long_row-all": {"drop_update", "drop_publish", "double_publish"},
    "hub_column-all": set(L.FAULTS), "hub_column-all-f1": set(L.FAULTS), "hub_column-all-f3": set(L.FAULTS),
    "hub_column-all-f64": set(L.FAULTS), "triples-all-f2": set(L.FAULTS), "mixed-auto-f3": set(L.FAULTS),
}


@pytest.mark.parametrize("case", L.CASES, ids=[c.name for c in L.CASES])
def test_matrix_stays_within_the_designed_size(case):
    V, I, J = L.matrix(case.matrix)
    assert V <= 400 and len(I) <= 700
    assert I.min() >= 0 and I.max() < V and J.min() >= 0 and J.max() < V


def test_matrices_have_the_designed_structure():
    V, I, J = L.matrix("long_row")
    assert np.bincount(I).max() == 300
    chunks = L.layout(V, I, J, np.zeros(V, bool))
    assert sorted(e - s for ch in chunks for (s, e, row, delta) in ch.runs if delta) == [44, 128, 128]
    assert any(len(ch.runs) > 1 and ch.runs[0][3] for ch in chunks)            # short rows share the last piece's chunk
    V, I, J = L.matrix("hub_column")
    assert len(I) == 300 and len(np.unique(J)) == 1 and len(np.unique(I)) == 300
    V, I, J = L.matrix("triples")
    same = (I[1:] == I[:-1]) & (J[1:] == J[:-1])
    assert same.sum() == 80                                                     # 40 pairs, three times each
    assert ((I[1:] != I[:-1]) & (J[1:] == J[:-1])).sum() == 10                 # ten streamed rows shared by consecutive resident rows
    for n in L.PARTIAL_SIZES:
        V, I, J = L.matrix("partial%d" % n)
        assert len(I) == n and len(np.unique(I)) == n and len(np.unique(J)) == n
    V, I, J = L.matrix("mixed")
    case = L.CASE["mixed-auto"]
    assert np.array_equal(np.nonzero(L.hub_columns(case, V, J))[0], L.MIXED_HUBS)
    chunks = L.layout(V, I, J, L.hub_columns(case, V, J))
    assert any(ch.ctx for ch in chunks) and any(d for ch in chunks for (_, _, _, d) in ch.runs if not ch.ctx) \
        and any(not d for ch in chunks for (_, _, _, d) in ch.runs)            # hub chunks, a long row, whole rows


def test_rows_are_prefixes_and_representable():
    for name in L.MATRICES:
        f, c = L.rows(name, L.DMAX)
        for D in (4, 63, 300):
            f2, c2 = L.rows(name, D)
            assert np.array_equal(f2, f[:, :D]) and np.array_equal(c2, c[:, :D])
        assert np.all(f != 0) and np.all(c != 0)
        st = L.state(f, c)
        assert len(st) == 12
        for t in ("focus", "context"):
            assert np.all(st[t].view(np.uint32) & 0xFFFF == 0)                  # bf16 holds every value
            assert np.array_equal(st[t].astype(np.float64) * 2.0 ** L.S, (f if t == "focus" else c).astype(np.float64))


@pytest.mark.parametrize("case", L.CASES, ids=[c.name for c in L.CASES])
def test_walk_meets_the_lattice_conditions(case):
    """peak <= 256 (bf16 holds every stored value), the dot bound for S at every dim, and the visibility conditions -- both rows of
    every step nonzero, every run's and piece's delta nonzero -- in the first four elements already.  The run-by-run model without
    a fault is the sequential walk."""
    for D in (SMALLEST, L.DMAX):
        for it, res in enumerate(L.check(case, D)):
            what = (case.name, D, "chunk order", it)
            assert sorted(L.walk_order(res["chunks"], res["chunk_order"]).tolist()) == list(range(len(L.matrix(case.matrix)[1]))), what
            assert res["model_equals_walk"], what
            assert res["peak"] <= L.PEAK_MAX, (what, res["peak"])
            assert res["both_nonzero"], what
            assert res["deltas_nonzero"], what
            if D == L.DMAX:
                print("%s, chunk order %d: peak |k| %d over %d elements" % (case.name, it, res["peak"], D))
                for d in GPU_DIMS:                                              # the peak over 1024 elements bounds every dim's
                    assert L.dot_bound_holds(d, res["peak"]), (what, d)
                    assert L.dot_bound_holds(d, L.PEAK_MAX), d


@pytest.mark.parametrize("case", L.CASES, ids=[c.name for c in L.CASES])
def test_every_fault_changes_a_word(case):
    """One update dropped, one run's publish dropped, a delta published twice, a run behind a cut restarted from the row as it was
    before the cut, a hub row read from its creation-time value: wherever such a fault can strike (up to six places per kind and
    chunk order), the tables differ from the clean walk in the first four elements -- so at every dim."""
    V, I, J = L.matrix(case.matrix)
    fk, ck = L.rows(case.matrix, SMALLEST)
    struck = set()
    for res in L.check(case, SMALLEST):
        clean_f, clean_c = res["walk"].focus, res["walk"].context
        for kind in L.FAULTS:
            for target in L.fault_targets(kind, res["runs"], len(I)):
                f, c, _ = L.run_model(I, J, res["chunks"], res["chunk_order"], fk, ck, case.sign, fault=(kind, target))
                assert not (np.array_equal(f, clean_f) and np.array_equal(c, clean_c)), (case.name, kind, target)
                struck.add(kind)
    assert "drop_update" in struck and "drop_publish" in struck
    assert MUST_STRIKE.get(case.name, set()) <= struck, (case.name, MUST_STRIKE[case.name] - struck)


def test_faults_are_faults():
    """The injected faults do what they say on a walk small enough to follow by hand: column 2 holds rows 0 and 1, cut after
    every nonzero (two delta runs on one resident row)."""
    I = np.array([0, 1]); J = np.array([2, 2])
    fk = np.array([[1], [1], [0]]); ck = np.array([[0], [0], [2]])
    chunks = L.layout(3, I, J, np.array([False, False, True]), flush_every=1)
    assert [ch.runs for ch in chunks] == [[(0, 1, 2, True), (1, 2, 2, True)]]
    co = np.arange(1)
    run = lambda fault=None: [t[:, 0].tolist() for t in L.run_model(I, J, chunks, co, fk, ck, 1, fault)[:2]]
    # clean: run 1 reads c = 2: f0 = 1 - 2, a = 2 - 1, delta -1 -> c = 1; run 2 reads 1: f1 = 1 - 1, a = 1 - 1, delta -1 -> c = 0
    assert run() == [[-1, 0, 0], [0, 0, 0]]
    assert run(("drop_update", 0)) == [[1, -1, 0], [0, 0, 1]]               # run 2 reads the untouched 2: f1 = 1 - 2, c = 2 - 1
    assert run(("drop_publish", 0)) == [[-1, -1, 0], [0, 0, 1]]             # run 2 reads 2 again: f1 = 1 - 2, c = 2 + (1 - 2)
    assert run(("double_publish", 0)) == [[-1, 1, 0], [0, 0, -1]]           # c = 2 - 2 after run 1; run 2: f1 = 1 - 0, c = 0 - 1
    assert run(("stale_restart", 1)) == [[-1, -1, 0], [0, 0, 0]]            # run 2 starts from 2: f1 = 1 - 2, its delta -1 onto 1
    assert run(("creation_read", 1)) == [[-1, -1, 0], [0, 0, 0]]            # the creation-time value is that same 2

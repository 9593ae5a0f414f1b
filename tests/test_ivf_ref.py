"""The inverted-file model (tests/ivf_ref.py) and the designed tables of test_ivf_gpu.py held, without a device, to what they are
designed for: the model with nprobe = L is chain_ref.topk over the whole table; the cross-list tie table really has equal score
bits in different lists with list order != id order; a designed case has |C_q| < k and one has an empty probed list; the
conditions under which the header's chain is pinned (no small product, finite partial sums) hold on every general-float table;
and the k-means centroids the trained-path tests give back by value are fixed points of the preparation."""
import numpy as np
import pytest

import chain_ref as CH
import ivf_ref as IR
import kmeans_ref as KR
import nn_ref as R

DIMS = IR.DIMS


def _finite_partial_sums(A, B):
    """Every partial sum of the chain is finite: |sum| <= sum of |products|, taken in fp64."""
    A, B = np.abs(np.asarray(A, np.float64)), np.abs(np.asarray(B, np.float64))
    assert np.all(np.isfinite(A @ B.T)) and (A @ B.T).max() < 3e38


@pytest.mark.parametrize("dim", (1, 3, 33, 200))
def test_nprobe_L_is_topk_over_the_whole_table(dim):
    n, L = 120, 5
    X = IR.twin_rows(dim, n)
    m = IR.Model(X, IR.given(R.random_rows(31 + dim, L, dim)))
    S = CH.chain(m.XH, m.XH)
    pos = np.arange(n)
    for k, ex in ((1, False), (17, True), (119, True), (120, False)):
        idx, score, count, cand = m.query_rows(pos, k, L, ex, S)
        wi, ws = CH.topk(S, k, pos if ex else None)
        assert idx.tobytes() == wi.tobytes() and score.tobytes() == ws.tobytes()
        assert np.all(count == k) and np.all(cand == n - int(ex))
    # more than the table holds: what there is, then the fill
    idx, score, count, cand = m.query_rows(pos, 128, L, True, S)
    wi, ws = CH.topk(S, 119, pos)
    assert np.array_equal(idx[:, :119], wi) and np.array_equal(score[:, :119], ws) and np.all(idx[:, 119:] == -1) and np.all(np.isneginf(score[:, 119:]))
    assert np.all(count == 119)
    # a subset: original ids come back
    keep = np.arange(1, n, 3, dtype=np.int32)
    ms = IR.Model(X, m.cen, keep)
    idx, score, _, _ = ms.query_rows(np.arange(len(keep)), 7, L)
    wi, ws = CH.topk(CH.chain(ms.XH, ms.XH), 7)
    assert np.array_equal(idx, keep[wi]) and score.tobytes() == ws.tobytes()


def test_fewer_probes_look_at_fewer_rows_and_never_find_better():
    X = IR.twin_rows(50, 300)
    m = IR.Model(X, IR.given(R.random_rows(81, 5, 50)))
    S = CH.chain(m.XH, m.XH)
    pos = np.arange(300)
    full = m.query_rows(pos, 10, 5, True, S)
    last = None
    for nprobe in (1, 2, 5):
        idx, score, count, cand = m.query_rows(pos, 10, nprobe, True, S)
        assert np.all(score <= full[1]) and (last is None or np.all(cand >= last))
        assert np.all(cand == m.sizes[m.probe(m.XH, nprobe)].sum(axis=1) - 1)      # a row's own list is its first probe
        last = cand
    assert np.all(m.probe(m.XH, 1)[:, 0] == m.label)


def test_the_twins_have_identical_prepared_rows():
    for dim in DIMS:
        XH = KR.prepare(IR.twin_rows(dim, 300), KR.COSINE)
        assert XH[:150].tobytes() == XH[150:].tobytes()


def test_the_cross_list_tie_table_is_what_it_claims():
    c = IR.case("ties")
    m, q = c.model()[0], c.vectors["e0"]
    assert m.label.tolist() == [0, 1] * 24                                        # even ids in list 0, odd ids in list 1
    table_order = np.concatenate(m.members)
    assert not np.array_equal(table_order, np.sort(table_order))                  # list order is not id order
    s = CH.chain(IR.given(q), m.XH)[0]
    assert len(set(s.view(np.uint32).tolist())) == 1 and np.isfinite(s[0]) and s[0] > 0       # one score, bit for bit, in both lists
    idx, score, count, cand = m.query_vectors(q, 16, 2)
    assert idx[0].tolist() == list(range(16)) and count[0] == 16 and cand[0] == 48
    assert set(m.label[idx[0]]) == {0, 1}


def test_the_axis_table_has_its_list_lengths_an_empty_probe_and_short_results():
    c = IR.case("axis")
    m, want = c.model()[0], IR.axis_table()[2]
    assert np.array_equal(m.label, want) and m.sizes.tolist() == [129, 1, 127, 128, 0, 0]
    assert not np.array_equal(np.concatenate(m.members), np.arange(len(c.X)))       # rows of a list are spread over the table
    away = np.array([[-1, 0, 0, 0]], np.float32)
    assert m.probe(IR.given(away), 2)[0, 0] == 5                                   # an empty probed list, first
    idx, score, count, cand = m.query_vectors(away, 16, 1)
    assert count[0] == 0 and cand[0] == 0 and np.all(idx == -1) and np.all(np.isneginf(score))
    idx, score, count, cand = m.query_rows(np.flatnonzero(m.label == 2), 128, 1, True)
    assert np.all(cand == 126) and np.all(count == 126) and np.all(idx[:, 126:] == -1) and np.all(idx[:, :126] >= 0)     # |C_q| < k
    probed = m.probe(IR.given(c.vectors["dup_and_empty"]), 2)
    assert probed[:3].tolist() == [[0, 4]] * 3 and np.all(probed[3:, 0] == 5)      # the duplicate centroid: lower id first; -e0: the empty list
    for nq in (1, 63, 64, 65):
        assert c.vectors["near3_%d" % nq].shape[0] == nq and np.all(m.probe(IR.given(c.vectors["near3_%d" % nq]), 1) == 3)


def test_the_long_list_is_one_row_longer_than_the_chunk():
    c = IR.case("long")
    m, want = c.model()[0], IR.long_list()[2]
    assert np.array_equal(m.label, want) and m.sizes.tolist() == [IR.CHUNK + 1, 50]
    last = np.flatnonzero(m.label == 0)[-1]
    assert m.query_vectors(c.vectors["mixed"][:1], 1, 1)[0][0, 0] == last          # the first vector is that row, three times as long


def test_the_chain_is_pinned_on_every_case_the_device_is_compared_with_the_model_on():
    """chain_ref.assert_no_small_product and finite partial sums on ivf_ref.cases() -- the list test_ivf_gpu.py takes every table,
    centroid set and set of query vectors from: rows against rows and against every centroid set the case uses (the given ones, or
    the k-means run of each T), every set of vectors against both.  Queries by id are rows, so rows against rows covers them.
    Not here, because they cannot be made without a device: the vectors of the trained handle in
    test_trainer_handle_entry_point_equals_the_host_rows_one, which that test compares with the device's own exact index and
    never with the model."""
    seen = set()
    for c in IR.cases():
        XH = KR.prepare(c.X if c.subset is None else c.X[c.subset], KR.COSINE)
        cens = [c.centroids(T)[0] for T in (IR.TRAIN_STEPS if c.C is None else (None,))]
        queries = [XH] + [KR.prepare(V, KR.COSINE) for V in c.vectors.values()]
        for Q in queries:
            for B in [XH] + cens:
                CH.assert_no_small_product(CH._pad4(Q), CH._pad4(B))
                _finite_partial_sums(Q, B)
        seen.add(c.name)
    assert seen == {"twin_%d" % d for d in DIMS} | {"axis", "ties", "ties_subset", "long", "batches", "trained_integers", "trained_general"}


def test_every_case_with_every_list_probed_is_topk_over_the_whole_table():
    """What lets test_ivf_gpu.py hold nprobe = L to the exact index: on every case the model then returns chain_ref.topk."""
    for c in IR.cases():
        if c.name in ("long", "batches"):
            continue                                                   # thousands of rows: the model's per-query loop is the GPU test's
        m, S = c.model(None if c.C is not None else 1)
        n = m.XH.shape[0]
        pos = np.arange(n)
        for k, ex in ((1, False), (min(33, n - 1), True)):
            idx, score, count, cand = m.query_rows(pos, k, c.L, ex, S)
            wi, ws = CH.topk(S, k, pos if ex else None)
            assert np.array_equal(idx, m.ids[wi]) and score.tobytes() == ws.tobytes(), c.name
            assert np.all(count == k) and np.all(cand == n - int(ex))


@pytest.mark.parametrize("kind", ["integers", "general"])
def test_trained_centroids_are_fixed_points_of_the_preparation(kind):
    """What lets test_ivf_gpu.py give k-means centroids back by value: preparing them again returns their bits.  And the run
    converges well inside 50 steps, so T = 50 is "until converged"."""
    c = IR.case("trained_" + kind)
    for T in IR.TRAIN_STEPS:
        cen, steps, conv = c.centroids(T)
        assert IR.given(cen).tobytes() == cen.tobytes(), (kind, T)
        assert steps == min(T, steps) and (T < 50 or (conv and 1 < steps < 50)), (kind, T, steps, conv)
        assert c.model(T)[0].sizes.sum() == len(c.X)
    assert IR.trained(c.X, c.L, IR.TRAIN_SEED + 1, 0)[0].tobytes() != c.centroids(0)[0].tobytes()

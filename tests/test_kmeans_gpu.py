"""k-means on the device against numpy (tests/kmeans_ref.py).  Exact tier: Euclid on integer rows and integer centroids, labels
and best scores with no tolerance, ties (duplicate centroids, duplicate rows) going to the lowest id, at the sizes that cross the
tile edges.  Update: given the labels the device reports, the new centroids, the sizes and the objective to the last bit, on any
input, across the piece boundary, with an empty cluster and one whose members cancel.  Bracket tier: on general rows every best
score within the bound B derived in kmeans_ref.py and no label more than the two bounds below the best centroid, every row of
every step.  Whole runs, determinism, step x t = run(t), the trainer-handle entry point bit for bit, subsets, non-finite input."""
import numpy as np
import pytest

import geglove
from geglove import capi, synth
from helpers import make_config
import chain_ref as CH
import kmeans_ref as R
import nn_ref

pytestmark = pytest.mark.gpu


def _everything(km):
    g = km.get()
    return (km.labels.tobytes(), km.best.tobytes(), km.centroids.tobytes(), km.sizes.tobytes(), g["steps"], g["converged"],
            np.float64(g["objective"]).tobytes(), np.float64(g["sum_sq"]).tobytes())


# ---- exact tier ---------------------------------------------------------------------------------------------------------

# (n, K, dim): n around the 64-row workgroup and past one objective block, K around the 128-centroid tile (every K here leaves the
# last tile partly empty), dim around the 32-column panel, the 4-float padding and the widest row
EXACT = [(1, 1, 1), (63, 2, 1), (64, 1, 3), (65, 2, 1024), (130, 127, 31), (130, 128, 33), (130, 129, 50), (1025, 257, 200), (1025, 128, 3)]


@pytest.mark.parametrize("n,K,dim", EXACT)
def test_exact_labels_and_scores_with_ties(gpu, n, K, dim):
    v = 3 if dim <= 3 else 2 if dim <= 50 else 1
    X = nn_ref.integers(100 + dim, (n, dim), -v, v)
    X[1::4] = X[0:n - 1:4]                                                # duplicate rows
    half = (K + 1) // 2
    C = nn_ref.integers(200 + K, (half, dim), -v, v)[np.arange(K) % half]          # centroid c + half is a copy of centroid c
    Z = R.exact_scores(X, C, R.EUCLID)
    want_label, want_best = R.assign(Z)
    tied = np.mean((Z == want_best[:, None]).sum(axis=1) >= 2)
    assert K < 2 or tied >= 0.9, tied                                     # nearly every row's best is shared by two or more centroids
    km = capi.Clustering.create(X, K, metric="euclid", seed=1)
    km.set_centroids(C)
    assert km.centroids.tobytes() == C.tobytes()                          # Euclid takes them as they are
    changed, objective = km.step()
    label, best = km.labels, km.best
    assert label.dtype == np.int32 and best.dtype == np.float32 and label.shape == best.shape == (n,)
    assert label.min() >= 0 and label.max() < K
    bad = np.flatnonzero((label != want_label) | (best != want_best))
    assert bad.size == 0, "row %d: got (%d, %r), want (%d, %r)" % (bad[0], label[bad[0]], best[bad[0]], want_label[bad[0]], want_best[bad[0]])
    assert best.tobytes() == want_best.tobytes()
    assert label.max() < half                                             # the copy with the higher id never wins
    assert changed == n and objective == R.objective(want_best)
    assert np.array_equal(km.sizes, np.bincount(want_label, minlength=K))
    assert km.centroids.tobytes() == R.update(X, want_label, C, R.EUCLID).tobytes()


# ---- update, bit for bit ------------------------------------------------------------------------------------------------

def _designed_clusters():
    """dim 9, K = 6 unit centres on the axes.  Clusters 1 .. 4 get 1023, 1024, 1025 and 2049 noisy members, cluster 5 none; the two
    rows +e_7 and -e_7 score the same against every centre, so both go to the lowest id, cluster 0, whose other members there are
    none: under cosine they cancel.  Positions are shuffled, so a cluster's members are spread over the table."""
    dim, K = 9, 6
    C = np.zeros((K, dim), np.float32)
    C[np.arange(K), np.arange(K)] = 1
    sizes = [2, 1023, 1024, 1025, 2049, 0]
    rows, planted = [np.eye(dim, dtype=np.float32)[7:8], -np.eye(dim, dtype=np.float32)[7:8]], [0, 0]
    for c in range(1, 5):
        noise = 0.05 * nn_ref.uniform(40 + c, (sizes[c], dim))
        rows.append((C[c][None, :] * (1 + c) + noise).astype(np.float32))       # norms differ from cluster to cluster
        planted += [c] * sizes[c]
    X, planted = np.concatenate(rows), np.array(planted)
    order = np.argsort(synth.splitmix64(77, len(X)), kind="stable")
    return X[order], planted[order], C, np.array(sizes)


@pytest.mark.parametrize("metric", [R.COSINE, R.EUCLID])
def test_update_objective_and_sizes_to_the_last_bit(gpu, metric):
    X, planted, C, sizes = _designed_clusters()
    if metric == R.EUCLID:
        C = C * np.arange(1, 7, dtype=np.float32)[:, None]             # centre c at (1 + c) e_c, where its members lie
        C[0] = 0; C[5] = -C[5]                                           # 0: nearest to +-e_7 among the ties' lowest id; 5: far from every row
    K = len(C)
    XH = R.prepare(X, metric)
    km = capi.Clustering.create(X, K, metric=metric, seed=3)
    km.set_centroids(C)
    for step in range(2):
        before = km.centroids
        if step == 0:
            assert before.tobytes() == R.prepare(C, metric).tobytes()
        changed, objective = km.step()
        label, best = km.labels, km.best
        if step == 0:
            assert changed == len(X) and np.array_equal(np.bincount(label, minlength=K), sizes)
            assert np.array_equal(label, planted)
        assert np.array_equal(km.sizes, np.bincount(label, minlength=K))
        want = R.update(XH, label, before, metric)
        got = km.centroids
        assert got.tobytes() == want.tobytes(), np.flatnonzero((got != want).any(axis=1))
        for c in np.flatnonzero(np.bincount(label, minlength=K) == 0):
            assert got[c].tobytes() == before[c].tobytes()               # an empty cluster keeps its centroid
        if step == 0:                                                    # (the moved centroids of step 1 may draw +-e_7 apart)
            assert got[5].tobytes() == before[5].tobytes()
            if metric == R.COSINE:
                assert got[0].tobytes() == before[0].tobytes()           # and so does the one whose members cancel
        assert objective == R.objective(best) == km.get()["objective"]
    assert km.get()["steps"] == 2


@pytest.mark.parametrize("n", [1023, 1024, 1025])
def test_objective_across_the_block_boundary(gpu, n):
    X = nn_ref.random_rows(n, n, 5)
    for metric in (R.COSINE, R.EUCLID):
        km = capi.Clustering.create(X, 4, metric=metric, seed=n)
        cen = km.centroids
        _, objective = km.step()
        assert objective == R.objective(km.best)
        XH = R.prepare(X, metric).astype(np.float64)
        sum_sq = km.get()["sum_sq"]
        assert sum_sq == R.partition_sum(R.seq_sum(XH * XH, 1))
        if metric == R.EUCLID:
            # the inertia follows: |x - c|^2 = |x|^2 - 2 t and every z is within B of its t; the fp64 sums of n terms add n 2^-53 each
            inertia = float(((XH - cen.astype(np.float64)[km.labels]) ** 2).sum())
            slack = 2 * n * float(R.bound(XH, cen, metric).max()) + 1e-12 * (sum_sq + 2 * abs(objective))
            assert abs((sum_sq - 2 * objective) - inertia) <= slack


# ---- bracket tier -------------------------------------------------------------------------------------------------------

def _general_rows(kind, dim):
    if kind == "random":
        return nn_ref.random_rows(31 + dim, 1500, dim)
    return nn_ref.planted(17 + dim, 30, 50, dim, 0.8)[0]


@pytest.mark.parametrize("dim", [50, 200])
@pytest.mark.parametrize("kind", ["random", "planted"])
@pytest.mark.parametrize("metric", [R.COSINE, R.EUCLID])
def test_every_row_of_every_step_within_the_bound(gpu, metric, kind, dim):
    X = _general_rows(kind, dim)
    n, K, seed = len(X), 130, 11                                          # two centroid tiles, the second nearly empty
    XH = R.prepare(X, metric)
    km = capi.Clustering.create(X, K, metric=metric, seed=seed)
    first = km.centroids
    assert first.tobytes() == XH[R.initial_positions(seed, n, K)].tobytes()      # the keyed sample of the prepared rows
    worst = 0.0
    for step in range(3):
        before = km.centroids
        changed, objective = km.step()
        label, best = km.labels, km.best
        worst = max(worst, R.check_bracket(XH, before, metric, label, best))
        assert objective == R.objective(best)
        assert km.centroids.tobytes() == R.update(XH, label, before, metric).tobytes()
        assert (changed == n) if step == 0 else (0 <= changed < n)
    print("%s %s dim %d: worst |best - t| = %.3f B" % (metric, kind, dim, worst))


# ---- chain tier ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dim", [33, 200])
@pytest.mark.parametrize("metric", [R.COSINE, R.EUCLID])
def test_labels_and_best_are_the_chain_bit_for_bit(gpu, metric, dim):
    """General floats, no bound: z = chain(xh, cen) + h with one fp32 add, the chain the header's "fp32 fmaf chain from 0.0f over
    ascending d" in numpy (tests/chain_ref.py; test_chain_ref.py shows that it differs from any other order of summation in most
    scores at these dims), h from kmeans_ref.bias.  K = 130 is two centroid tiles; centroid c + 65 is a copy of centroid c, so
    every row's best is an exact tie that must go to the lower id."""
    n, K = 300, 130
    X = nn_ref.random_rows(800 + dim, n, dim)
    C = nn_ref.random_rows(900 + dim, K, dim)
    C[:40] = X[:40]                                                       # some centroids are rows
    C[K // 2:] = C[:K // 2]
    XH, cen = R.prepare(X, metric), R.prepare(C, metric)
    Z = CH.chain(XH, cen) + R.bias(cen, metric)[None, :]
    assert Z.dtype == np.float32 and np.all(np.isfinite(Z))
    want_label, want_best = R.assign(Z)
    assert want_label.max() < K // 2 and len(set(want_label.tolist())) > 10
    km = capi.Clustering.create(X, K, metric=metric, seed=1)
    km.set_centroids(C)
    assert km.centroids.tobytes() == cen.tobytes()
    km.step()
    label, best = km.labels, km.best
    bad = np.flatnonzero((label != want_label) | (best.view(np.uint32) != want_best.view(np.uint32)))
    assert bad.size == 0, "%d of %d rows differ from the model; row %d: got (%d, %r), want (%d, %r)" % (
        bad.size, n, bad[0], label[bad[0]], best[bad[0]], want_label[bad[0]], want_best[bad[0]])
    assert label.tobytes() == want_label.tobytes() and best.tobytes() == want_best.tobytes()


# ---- whole runs ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("metric", [R.COSINE, R.EUCLID])
def test_planted_clusters_are_recovered_from_their_centres(gpu, metric):
    seed, clusters, size, dim = 5, 20, 50, 50
    X, planted = nn_ref.planted(seed, clusters, size, dim, 0.1)
    centres = nn_ref.uniform(seed, (clusters, dim))
    centres /= np.linalg.norm(centres, axis=1, keepdims=True)
    km = capi.Clustering.create(X, clusters, metric=metric)
    km.set_centroids(centres.astype(np.float32))
    steps, converged = km.run(10)
    assert converged and steps <= 3 and km.get()["converged"] and km.get()["steps"] == steps
    assert np.array_equal(km.labels, planted)                             # the identity map: centroid c is centre c
    assert np.array_equal(km.sizes, np.full(clusters, size))


@pytest.mark.parametrize("metric", [R.COSINE, R.EUCLID])
def test_keyed_sample_converges_and_two_handles_agree(gpu, metric):
    X, _ = nn_ref.planted(6, 12, 80, 20, 0.5)
    a = capi.Clustering.create(X, 12, metric=metric, seed=2024)
    b = capi.Clustering.create(X, 12, metric=metric, seed=2024)
    steps, converged = a.run(100)
    assert converged and 1 <= steps < 100
    assert b.run(100) == (steps, True)
    assert _everything(a) == _everything(b)
    changed, _ = a.step()                                                 # a converged handle stays where it is
    assert changed == 0 and a.labels.tobytes() == b.labels.tobytes() and a.centroids.tobytes() == b.centroids.tobytes()
    c = capi.Clustering.create(X, 12, metric=metric, seed=2025)           # another seed, another sample
    assert c.centroids.tobytes() != capi.Clustering.create(X, 12, metric=metric, seed=2024).centroids.tobytes()
    assign_ms, update_ms = a.kernel_ms
    assert assign_ms > 0 and update_ms > 0


def test_steps_equal_a_run(gpu):
    X = nn_ref.random_rows(8, 3000, 24)
    for metric in (R.COSINE, R.EUCLID):
        a = capi.Clustering.create(X, 40, metric=metric, seed=9)
        b = capi.Clustering.create(X, 40, metric=metric, seed=9)
        trail = [a.step() for _ in range(3)]
        assert trail[0][0] == 3000 and all(ch > 0 for ch, _ in trail)      # not converged yet: the run below takes all three steps
        assert b.run(3) == (3, False)
        assert _everything(a) == _everything(b)
        assert b.get()["objective"] == trail[-1][1]
        with pytest.raises(capi.GeError) as e:
            b.run(0)
        assert e.value.status == capi.GE_ERR_ARG and "max_iter" in str(e.value)


# ---- entry points -------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("mode,dim", [("hogwild", 50), ("deterministic", 24)])
def test_trainer_handle_entry_point_equals_the_host_rows_one(gpu, mode, dim):
    V, N, K = 3000, 40000, 33
    I, J, Xc, xmax = synth.synthetic_coo(V, N, seed=77)
    m = geglove.CooMatrix(V, I, J, Xc, xmax)
    cfg = make_config(dim, method="pglove", mode=mode, shuffle="java" if mode == "deterministic" else "device", seed=5)
    opt = geglove.Adagrad(m, cfg, cfg.costFunction())
    for it in range(3):
        opt.epoch(it)
    before = opt.state()
    rows = opt.extractResultF32().reshape(V, dim)
    keep = np.arange(1, V, 3, dtype=np.int32)
    for subset in (None, keep):
        for metric in ("cosine", "euclid"):
            on_handle = capi.Clustering.create_glove(opt._h, K, subset=subset, metric=metric, seed=4)
            on_rows = capi.Clustering.create(rows, K, subset=subset, metric=metric, seed=4)
            assert on_handle.get() == on_rows.get() and on_handle.get()["n"] == (V if subset is None else len(keep))
            assert on_handle.centroids.tobytes() == on_rows.centroids.tobytes()
            assert on_handle.run(3) == on_rows.run(3)
            assert _everything(on_handle) == _everything(on_rows)
    after = opt.state()
    for name in before:
        assert before[name].tobytes() == after[name].tobytes(), name
    assert rows.tobytes() == opt.extractResultF32().tobytes()
    opt.close()


@pytest.mark.parametrize("metric", ["cosine", "euclid"])
def test_a_subset_equals_its_packed_rows(gpu, metric):
    X = nn_ref.random_rows(21, 2000, 10)
    keep = np.flatnonzero(synth.splitmix64(22, 2000) % np.uint64(3) != 0).astype(np.int32)
    a = capi.Clustering.create(X, 9, subset=keep, metric=metric, seed=6)
    b = capi.Clustering.create(np.ascontiguousarray(X[keep]), 9, metric=metric, seed=6)
    assert a.get()["n"] == len(keep) == b.get()["n"]
    assert a.run(4) == b.run(4)
    assert _everything(a) == _everything(b)


def test_non_finite_input_is_refused_and_reading_before_a_step(gpu):
    X = nn_ref.random_rows(9, 500, 6)
    for bad in (np.nan, np.inf, -np.inf):
        for metric in ("cosine", "euclid"):
            Z = X.copy(); Z[123, 4] = bad
            with pytest.raises(capi.GeError) as e:
                capi.Clustering.create(Z, 5, metric=metric)
            assert e.value.status == capi.GE_ERR_ARG and "non-finite input" in str(e.value)
            km = capi.Clustering.create(X, 5, metric=metric)
            kept = km.centroids
            with pytest.raises(capi.GeError) as e:
                km.set_centroids(Z[120:125])
            assert e.value.status == capi.GE_ERR_ARG and "non-finite input" in str(e.value)
            assert km.centroids.tobytes() == kept.tobytes()               # a refused table changes nothing
    km = capi.Clustering.create(X, 5)
    with pytest.raises(capi.GeError) as e:
        km.labels
    assert e.value.status == capi.GE_ERR_STATE
    Z = X.copy(); Z[20] = 0                                               # a zero row is harmless under cosine: z = 0 against everything
    km = capi.Clustering.create(Z, 5, seed=1)
    before = km.centroids
    km.step()
    assert np.all(np.isfinite(km.best)) and km.best[20] == 0 and km.labels[20] == 0       # every centroid ties at 0: the lowest id
    R.check_bracket(R.prepare(Z, R.COSINE), before, R.COSINE, km.labels, km.best)         # and the other rows are not poisoned

"""The yardstick of the inverted-file tests: the "Inverted-file index" section of include/geglove.h in numpy, built from
chain_ref.chain (the score), kmeans_ref.prepare / assign / update (rows, lists, training) and chain_ref.topk (the probe order).
Never the library itself.  Also here: the designed tables the GPU tests use, so that test_ivf_ref.py can hold them to what they
are designed for without a device."""
import numpy as np

import chain_ref as CH
import kmeans_ref as KR
import nn_ref as R

F32 = np.float32
CHUNK = 4096          # csrc/ivf.hip IVF_CHUNK: rows of a list one work item scans
BATCH_ENTRIES = 1 << 24   # csrc/ivf.hip IVF_BATCH_ENTRIES: partial-list entries per batch of queries


class Model:
    """The index over the rows X[subset] with the PREPARED centroids `cen` (fp32 [L, dim])."""

    def __init__(self, X, cen, subset=None):
        X = np.ascontiguousarray(X, F32)
        self.ids = np.arange(X.shape[0], dtype=np.int32) if subset is None else np.asarray(subset, np.int32)
        self.XH = KR.prepare(X[self.ids], KR.COSINE)
        self.cen = np.ascontiguousarray(cen, F32)
        self.L = self.cen.shape[0]
        Z = CH.chain(self.XH, self.cen)
        assert np.all(np.isfinite(Z))
        self.label, _ = KR.assign(Z)
        self.sizes = np.bincount(self.label, minlength=self.L).astype(np.int32)
        self.members = [np.flatnonzero(self.label == c) for c in range(self.L)]        # ascending position

    def probe(self, QH, nprobe):
        """int32 [nq, nprobe]: the first nprobe centroids of every prepared query in the total order."""
        Z = CH.chain(QH, self.cen)
        assert np.all(np.isfinite(Z))
        return CH.topk(Z, nprobe)[0]

    def query(self, QH, k, nprobe, self_pos=None, S=None):
        """(index, score, count, candidates) for the prepared queries QH; self_pos[q]: the position query q must not return.
        S: the scores of the queries against every indexed row, when the caller has them."""
        QH = np.ascontiguousarray(QH, F32)
        nq = QH.shape[0]
        if S is None:
            S = CH.chain(QH, self.XH)
        S = CH.ranked(S)
        assert np.all(np.isfinite(S))
        probed = self.probe(QH, nprobe)
        idx = np.full((nq, k), -1, np.int32)
        score = np.full((nq, k), -np.inf, F32)
        count = np.zeros(nq, np.int32)
        cand = np.zeros(nq, np.int32)
        for q in range(nq):
            C = np.sort(np.concatenate([self.members[c] for c in probed[q]]))           # the union; lists are disjoint
            if self_pos is not None:
                C = C[C != self_pos[q]]
            cand[q] = C.size
            order = C[np.argsort(-S[q, C], kind="stable")][:k]                          # score descending, then position = id ascending
            count[q] = order.size
            idx[q, :order.size] = self.ids[order]
            score[q, :order.size] = S[q, order]
        return idx, score, count, cand

    def query_rows(self, pos, k, nprobe, exclude_self=False, S=None):
        pos = np.asarray(pos, np.int64)
        return self.query(self.XH[pos], k, nprobe, pos if exclude_self else None, None if S is None else S[pos])

    def query_vectors(self, V, k, nprobe):
        return self.query(KR.prepare(V, KR.COSINE), k, nprobe)


def given(C):
    """Centroids given by value, as the index prepares them."""
    return KR.prepare(np.ascontiguousarray(C, F32), KR.COSINE)


def trained(X, L, seed, T, subset=None):
    """(centroids, steps, converged) of ge_kmeans_create + ge_kmeans_run(T) under GE_KM_COSINE: the keyed sample, then at most T
    steps (assign, update), stopping after a step that changed no label.  T = 0: the sample itself."""
    X = np.ascontiguousarray(X, F32)
    XH = KR.prepare(X if subset is None else X[np.asarray(subset)], KR.COSINE)
    cen = XH[KR.initial_positions(seed, XH.shape[0], L)].copy()
    label = np.full(XH.shape[0], -1, np.int32)
    steps, changed = 0, 1
    while steps < T and changed:
        new, _ = KR.assign(CH.chain(XH, cen))
        changed = int(np.sum(new != label))
        label = new
        cen = KR.update(XH, label, cen, KR.COSINE)
        steps += 1
    return cen, steps, changed == 0 and steps > 0


# ---------------------------------------------------------------------------------------------------------------------
# The designed tables.
# ---------------------------------------------------------------------------------------------------------------------
def twin_rows(dim, n, seed=0):
    """nn_ref.random_rows whose second half is the first half scaled by 2: the prepared twins have identical bits (doubling is
    exact in fp32 and in the fp64 norm), sit in the same list and tie in every score."""
    X = R.random_rows(7000 + 13 * dim + n + seed, n, dim)
    h = n // 2
    X[h:2 * h] = X[:h] * F32(2.0)
    return X


def axis_table(dim=4):
    """Lists of length 129, 1, 127, 128 around the axes e0 .. e3, in shuffled row order, and six centroids: e0 .. e3, a second e0
    (id 4: every row prefers the lower id, so its list is empty) and -e0 (id 5: no row lies near it, its list is empty too, and a
    query at -e0 probes it first).  Returns (rows, centroids as given, the list every row is built for)."""
    from geglove import synth
    lengths = (129, 1, 127, 128)
    want = np.repeat(np.arange(4), lengths)
    X = np.zeros((want.size, dim), np.float64)
    X[np.arange(want.size), want] = 1.0
    X += 0.1 * R.uniform(4711, X.shape)
    X *= np.exp2(R.integers(4712, (want.size, 1), -2, 2).astype(np.float64))
    order = np.argsort(synth.splitmix64(4713, want.size), kind="stable")
    C = np.zeros((6, dim), F32)
    C[[0, 1, 2, 3, 4], [0, 1, 2, 3, 0]] = 1.0
    C[5, 0] = -1.0
    return X[order].astype(F32), C, want[order].astype(np.int32)


def near_axis(axis, count, seed, dim=4, sign=1.0):
    """`count` query vectors near sign * e_axis."""
    V = 0.05 * R.uniform(seed, (count, dim))
    V[:, axis] += sign
    return V.astype(F32)


def cross_list_ties(pairs=24, dim=3):
    """Rows (a, b, 0) 2^s and (a, -b, 0) 2^s alternating, a = 3, b = 1: every prepared first component has the same bits, so the
    query e0 scores all of them alike.  Centroids along (1, 1) and (1, -1): even ids fall into list 0, odd ids into list 1, and
    the table in list order (0, 2, 4, .. then 1, 3, 5, ..) is not in id order.  Returns (rows, centroids, the query)."""
    X = np.zeros((2 * pairs, dim), F32)
    for i in range(pairs):
        s = F32(2.0) ** (i % 5 - 2)
        X[2 * i] = (3 * s, 1 * s) + (0,) * (dim - 2)
        X[2 * i + 1] = (3 * s, -1 * s) + (0,) * (dim - 2)
    C = np.zeros((2, dim), F32)
    C[0, :2] = (1, 1)
    C[1, :2] = (1, -1)
    q = np.zeros((1, dim), F32)
    q[0, 0] = 1
    return X, C, q


def long_list():
    """One list one row longer than the scan's chunk (THIS DEPENDS ON IVF_CHUNK = 4096 in csrc/ivf.hip) and one of 50 rows."""
    n0, n1, dim = CHUNK + 1, 50, 4
    want = np.repeat(np.arange(2), (n0, n1))
    X = np.zeros((want.size, dim), np.float64)
    X[np.arange(want.size), want] = 1.0
    X += 0.2 * R.uniform(99, X.shape)
    from geglove import synth
    order = np.argsort(synth.splitmix64(98, want.size), kind="stable")
    C = np.zeros((2, dim), F32)
    C[[0, 1], [0, 1]] = 1.0
    return X[order].astype(F32), C, want[order].astype(np.int32)


# ---------------------------------------------------------------------------------------------------------------------
# The cases: every table, centroid source and set of query vectors that test_ivf_gpu.py sends to the device, made once here.
# test_ivf_gpu.py takes its inputs from `case(name)` and nowhere else; test_ivf_ref.py walks `cases()` and holds every one of
# them to the conditions under which the header's chain is pinned.  The one input that cannot be made without a device -- the
# vectors of a trained handle (test_trainer_handle_entry_point_equals_the_host_rows_one) -- is not here: that test compares the
# device with the device (handle entry point against host rows entry point, inverted file against exact index), never with the
# model.
# ---------------------------------------------------------------------------------------------------------------------
DIMS = (1, 3, 4, 31, 32, 33, 50, 200, 1024)         # below / at / above the panel of 32 columns, no multiple of 4, the limit
TRAIN_SEED, TRAIN_STEPS = 1234, (0, 1, 50)


class Case:
    """rows X, subset (or None), and either C (centroids as given, L of them) or train = L (centroids trained with TRAIN_SEED for
    each T of TRAIN_STEPS); vectors: name -> query vectors sent by value.  Queries by id take their rows from X."""

    def __init__(self, name, X, C=None, train=None, subset=None, vectors=None):
        self.name, self.X, self.C, self.train, self.subset, self.vectors = name, X, C, train, subset, dict(vectors or {})
        self.L = train if C is None else C.shape[0]
        for a in [X] + list(self.vectors.values()) + ([] if C is None else [C]):
            a.setflags(write=False)
        self._cen, self._model = {}, {}

    def centroids(self, T=None):
        """The prepared centroids: of the given ones, or of the run of at most T steps -> (centroids, steps, converged)."""
        if T not in self._cen:
            self._cen[T] = (given(self.C), 0, False) if self.C is not None else trained(self.X, self.L, TRAIN_SEED, T, self.subset)
        return self._cen[T]

    def model(self, T=None):
        """(Model, its all-pairs scores), made once."""
        if T not in self._model:
            m = Model(self.X, self.centroids(T)[0], self.subset)
            S = CH.chain(m.XH, m.XH)
            S.setflags(write=False)
            self._model[T] = (m, S)
        return self._model[T]


def _make_cases():
    from geglove import synth
    out = []
    for dim in DIMS:
        n = 300
        X = twin_rows(dim, n)
        subset = np.flatnonzero(synth.splitmix64(11 + dim, n) % np.uint64(4) != 0).astype(np.int32) if dim in (33, 200) else None
        ids = np.arange(n) if subset is None else subset
        vectors = {"mixed": np.concatenate([R.random_rows(900 + dim, 60, dim), X[ids[[0, len(ids) // 2, len(ids) - 1]]]])}     # 60 that are no rows, three that are
        if dim == 50:
            vectors["seventy"] = R.random_rows(17, 70, dim)
        out.append(Case("twin_%d" % dim, X, C=R.random_rows(31 + dim, 5, dim), subset=subset, vectors=vectors))
    X, C, _ = axis_table()
    vectors = {"near3_%d" % nq: near_axis(3, nq, 500 + nq) for nq in (1, 63, 64, 65)}
    vectors["dup_and_empty"] = np.concatenate([near_axis(0, 3, 71), np.array([[-1, 0, 0, 0]], F32), near_axis(0, 2, 72, sign=-1.0)])
    out.append(Case("axis", X, C=C, vectors=vectors))
    X, C, q = cross_list_ties()
    out.append(Case("ties", X, C=C, vectors={"e0": q}))
    out.append(Case("ties_subset", X, C=C, subset=np.array([i for i in range(48) if i % 5 != 1], np.int32), vectors={"e0": q}))
    X, C, want = long_list()
    last = np.flatnonzero(want == 0)[-1:]                             # the last row of the long list: alone in the second chunk
    out.append(Case("long", X, C=C, vectors={"mixed": np.concatenate([X[last] * F32(3), R.random_rows(6, 5, 4)])}))
    out.append(Case("batches", R.random_rows(4004, 2000, 4), C=R.random_rows(4005, 16, 4)))          # by value it sends its own rows
    X = R.integers(61, (700, 8), -4, 4)
    X[5] = 0                                                          # a zero row is harmless
    out.append(Case("trained_integers", X, train=8, vectors={"forty": R.random_rows(63, 40, 8)}))
    X = R.planted(62, 12, 50, 50, noise=0.8)[0]
    X[5] = 0
    out.append(Case("trained_general", X, train=12, vectors={"forty": R.random_rows(63, 40, 50)}))
    return out


_CASES = None


def cases():
    global _CASES
    if _CASES is None:
        _CASES = _make_cases()
    return _CASES


def case(name):
    return {c.name: c for c in cases()}[name]

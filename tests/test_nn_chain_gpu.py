"""k_nn_score_select held to the header's score bit for bit: "an fp32 fmaf chain from 0 in ascending d", computed in numpy
(tests/chain_ref.py) on general floats, then the header's total order.  out_index and out_score are compared as bytes: no bound,
no slot left out.  test_chain_ref.py asserts, without a device, that the model differs from a split, a reversed or an unfused
sum in more than half of the scores at every dim >= 31 used here, so a tile that summed otherwise fails.

Also here: every list capacity <CAP> of the kernel made to compact again and again (integer scores, exact), and what a score that
overflows does."""
import functools

import numpy as np
import pytest

from geglove import capi, synth
import chain_ref as CH
import kmeans_ref as KR
import nn_ref as R

pytestmark = pytest.mark.gpu

KS = (1, 16, 17, 32, 33, 64, 65, 128)               # both sides of every edge of nn_cap_of: CAP 32 | 64 | 128 | 256
DIMS = (1, 3, 4, 31, 32, 33, 50, 200, 1024)         # below / at / above the panel of 32 columns, no multiple of 4, the limit
SIZES = (127, 128, 129, 300)                        # the candidate tile holds 128
NQS = (1, 63, 64, 65, None)                         # the query tile holds 64; None = every row
MODEL_METRIC = {"cosine": KR.COSINE, "dot": KR.EUCLID}     # kmeans_ref.prepare: EUCLID leaves the rows as they are, as DOT does


def _cases():
    """(dim, n, metric, nq, k, exclude_self): 16 on the 300-row tables -- every k with and without exclude_self -- and one per
    (dim, small table), k, query count, metric and exclude_self rotating through their values."""
    out = []
    wide = ((200, "cosine"), (33, "dot"), (50, "cosine"), (200, "dot"))
    for i, k in enumerate(KS):
        for j, ex in enumerate((False, True)):
            dim, metric = wide[(i + 2 * j) % 4]
            out.append((dim, 300, metric, NQS[(2 * i + j) % 5], k, ex))
    t = 0
    for dim in DIMS:
        for n in SIZES[:3]:
            ex = t % 3 == 1
            k = KS[(3 * t + 1) % 8]
            while k > n - int(ex):
                k = KS[KS.index(k) - 1]
            out.append((dim, n, ("dot", "cosine")[t % 2], NQS[(t + 1) % 5], k, ex))
            t += 1
    return out


CASES = _cases()
# the covering the issue asks for, checked where the list is built
assert {c[0] for c in CASES} == set(DIMS) and {c[1] for c in CASES} == set(SIZES) and {c[3] for c in CASES} == set(NQS)
assert {c[4] for c in CASES} == set(KS) and {(c[4], c[5]) for c in CASES if c[1] == 300} == {(k, ex) for k in KS for ex in (False, True)}
assert all(c[4] <= c[1] - int(c[5]) for c in CASES) and len(CASES) == 43


def _rows(dim, n):
    """nn_ref.random_rows with the second half a copy of the first: every row but the last of an odd table has a twin with the
    same scores against everything, so every list holds exact ties that the id rule must break."""
    X = R.random_rows(5000 + 7 * dim + n, n, dim)
    h = n // 2
    X[h:2 * h] = X[:h]
    return X


@functools.lru_cache(maxsize=None)
def _table(dim, n, metric):
    """The rows, the prepared rows and the model's scores of every row against every row (read-only; a score depends on its
    two rows only, so any set of queries takes its rows from this matrix)."""
    X = _rows(dim, n)
    XH = KR.prepare(X, MODEL_METRIC[metric])
    S = CH.chain(XH, XH)
    assert np.all(np.isfinite(S))
    for a in (X, XH, S):
        a.setflags(write=False)
    return X, XH, S


def _same_bytes(got, want, what):
    gi, gs = got
    wi, ws = want
    assert gi.dtype == np.int32 and gs.dtype == np.float32 and gi.shape == wi.shape and gs.shape == ws.shape
    if gi.tobytes() == wi.tobytes() and gs.tobytes() == ws.tobytes():
        return
    bad_s, bad_i = gs.view(np.uint32) != ws.view(np.uint32), gi != wi
    q, e = np.argwhere(bad_s | bad_i)[0]
    raise AssertionError("%s: %d of %d scores and %d indices differ from the model; first at query %d slot %d: got (%d, %r), want (%d, %r)"
                         % (what, bad_s.sum(), gs.size, bad_i.sum(), q, e, gi[q, e], gs[q, e], wi[q, e], ws[q, e]))


@pytest.mark.parametrize("dim,n,metric,nq,k,exclude_self", CASES)
def test_scores_and_order_are_the_chain_bit_for_bit(gpu, dim, n, metric, nq, k, exclude_self):
    X, _, S = _table(dim, n, metric)
    nn = capi.Neighbors.create(X, metric=metric)
    if nq is None:
        qp = np.arange(n, dtype=np.int32)
        got = nn.query_rows(None, k, exclude_self=exclude_self)
    else:
        qp = (synth.splitmix64(dim * 1000 + n + k, nq) % np.uint64(n)).astype(np.int32)
        qp[0] = n - 1                                             # the last row: past the twins of an odd table
        got = nn.query_rows(qp, k, exclude_self=exclude_self)
    want = CH.topk(S[qp], k, qp if exclude_self else None)
    _same_bytes(got, want, "dim %d n %d %s nq %s k %d exclude_self %d" % (dim, n, metric, nq, k, exclude_self))
    if k >= 2:
        assert np.any(want[1][:, 1:] == want[1][:, :-1]), "the case holds no tie"


@pytest.mark.parametrize("metric", ["cosine", "dot"])
def test_query_vectors_bit_for_bit(gpu, metric):
    """Vectors that are no rows of the table (and three that are) are prepared like rows; k = 33 is <128>."""
    dim, n, k = 50, 300, 33
    X, XH, _ = _table(dim, n, metric)
    V = np.concatenate([R.random_rows(4242, 62, dim), X[[0, 151, 299]]])
    want = CH.topk(CH.chain(KR.prepare(V, MODEL_METRIC[metric]), XH), k)
    _same_bytes(capi.Neighbors.create(X, metric=metric).query_vectors(V, k), want, "query_vectors %s" % metric)


@pytest.mark.parametrize("metric", ["cosine", "dot"])
def test_an_index_over_a_subset_bit_for_bit(gpu, metric):
    """Ids differ from positions: the order is by ascending ORIGINAL id, the excluded row is the query's own id."""
    dim, n, k = 33, 300, 17
    X = _rows(dim, n)
    keep = np.flatnonzero(synth.splitmix64(11, n) % np.uint64(3) != 0).astype(np.int32)
    assert 150 < len(keep) < 250 and not np.array_equal(keep, np.arange(len(keep)))
    XH = KR.prepare(X[keep], MODEL_METRIC[metric])
    S = CH.chain(XH, XH)
    nn = capi.Neighbors.create(X, subset=keep, metric=metric)
    for exclude_self in (False, True):
        qp = np.arange(0, len(keep), 3)
        wi, ws = CH.topk(S[qp], k, qp if exclude_self else None)
        assert np.any(ws[:, 1:] == ws[:, :-1])
        _same_bytes(nn.query_rows(keep[qp], k, exclude_self=exclude_self), (keep[wi], ws), "subset %s exclude_self %d" % (metric, exclude_self))


# ---------------------------------------------------------------------------------------------------------------------
# Every list capacity made to compact.
# ---------------------------------------------------------------------------------------------------------------------
N_COMPACT = 128 * 3 * 1024 - 50
QUERIES = np.array([(1, 0), (-1, 0), (0, 1), (0, -1), (1, 1), (-1, 1), (1, -1), (0, 0)], np.float32)


@functools.lru_cache(maxsize=None)
def _compact_table(sawtooth):
    c = np.arange(N_COMPACT, dtype=np.int64)
    X = np.ones((N_COMPACT, 2), np.float32)
    X[:, 0] = (c * 7919) % 1009 if sawtooth else c
    X.setflags(write=False)
    return X


@pytest.mark.parametrize("sawtooth", [False, True])
def test_every_list_capacity_compacts(gpu, sawtooth):
    """DOT, dim 2, 393 166 rows (c, 1) (or ((7919 c) mod 1009, 1)), eight query vectors, every k of KS; integer scores below 2^24,
    so nn_ref.exact_topk is the truth.

    The launch: query_impl cuts the candidates into ranges of whole 128-candidate tiles, `want` = min(tiles, 1024, ceil(2048 /
    query tiles)) of them.  Here tiles = ceil(393166 / 128) = 3072 and eight queries are one query tile, so want = 1024, a range is
    3072 / 1024 = 3 tiles = 384 candidates -- more than the largest capacity, 256 -- and there are 1024 ranges (the last one 50
    candidates short).  nn has no getter for the number of ranges: THIS TEST DEPENDS ON THE CAP OF 1024 RANGES in query_impl; with
    another cap the ranges may hold fewer candidates than a list and <256> would not compact.

    What the queries do on the ascending table: (1, 0) and (1, 1) score c (+ 1), ascending with the position: every candidate
    beats every threshold, a list fills and compacts every CAP - k insertions, and in the merge every one of the 1024 lists
    displaces the running one.  (-1, 0), (-1, 1): only the first k of a range ever enter.  (0, 1), (0, -1), (0, 0): all scores
    equal, ids alone decide.  On the sawtooth table scores repeat every 1009 rows, 1009 and 384 coprime: ties in mid-list, in every
    range, between ranges."""
    X = _compact_table(sawtooth)
    assert (N_COMPACT + 127) // 128 == 3072 and 3 * 128 > 256
    S = QUERIES.astype(np.int64) @ X.astype(np.int64).T
    nn = capi.Neighbors.create(X, metric="dot")
    for k in KS:
        want = R.exact_topk(S, k)
        _same_bytes(nn.query_vectors(QUERIES, k), want, "compaction sawtooth %d k %d" % (sawtooth, k))


# ---------------------------------------------------------------------------------------------------------------------
# Overflow.
# ---------------------------------------------------------------------------------------------------------------------
BIG = np.float32(2.0 ** 100)


def test_overflowed_scores_rank_as_infinities(gpu):
    """DOT on finite rows built from +-2^100.  No row mixes signs, so no partial sum meets an infinity of the other sign: the
    scores are +-inf, +-2^101, 0 whether a tile fuses or not (asserted on the model).  +inf comes first, by id; then the finite
    scores; -inf last, by id; no NaN anywhere.  Every capacity."""
    pattern = np.array([(BIG, BIG), (-BIG, -BIG), (1, 1), (0, 0), (-1, -1), (BIG, 0), (0, -BIG)], np.float32)
    X = pattern[np.arange(203) % 7]
    Q = np.array([(BIG, BIG), (-BIG, -BIG), (1, 0), (0, BIG)], np.float32)
    S = CH.chain(Q, X)
    assert S.tobytes() == CH.unfused(Q, X).tobytes() and not np.isnan(S).any()
    assert np.isposinf(S[0]).sum() == 58 and np.isneginf(S[0]).sum() == 58 and np.isfinite(S[2]).all()
    nn = capi.Neighbors.create(X, metric="dot")
    for k in KS:
        gi, gs = nn.query_vectors(Q, k)
        assert not np.isnan(gs).any()
        _same_bytes((gi, gs), CH.topk(S, k), "overflow k %d" % k)
    gi, gs = nn.query_vectors(Q, 128)
    plus = np.flatnonzero(np.isposinf(S[0]))
    assert np.array_equal(gi[0, :58], plus) and np.all(np.isposinf(gs[0, :58])) and np.all(np.isfinite(gs[0, 58:]))
    # by row id with exclude_self: row 0 = (BIG, BIG) against the table is row 0 of S
    gi, gs = nn.query_rows([0, 1], 65, exclude_self=True)
    _same_bytes((gi, gs), CH.topk(S[:2], 65, np.array([0, 1])), "overflow by row id")


def test_a_table_whose_every_score_is_minus_infinity(gpu):
    X = np.full((300, 2), -BIG, np.float32)
    nn = capi.Neighbors.create(X, metric="dot")
    for k in KS:
        gi, gs = nn.query_vectors(np.array([(BIG, BIG), (BIG, 0)], np.float32), k)
        assert np.array_equal(gi, np.tile(np.arange(k, dtype=np.int32), (2, 1))) and np.all(np.isneginf(gs))


def test_a_partial_sum_of_plus_infinity_absorbs_a_finite_product(gpu):
    """The one input that tells a fused tile from an unfused one at overflow: query (2^100, 2^100), candidate (2^100, -2^100).
    The header's chain is fmaf(2^100, 2^100, 0) = +inf, then fmaf(2^100, -2^100, +inf) = +inf: inside the fused operation the
    product -2^200 is finite.  A product rounded on its own is -inf, +inf - inf is NaN, and a NaN is reported as -inf.
    Row 77 is that candidate, every other row scores -inf: the chain puts 77 first with +inf, from every capacity."""
    X = np.full((130, 2), -BIG, np.float32)
    X[77] = (BIG, -BIG)
    q = np.array([(BIG, BIG)], np.float32)
    assert np.isposinf(CH.chain(q, X[77:78])[0, 0]) and np.isnan(CH.unfused(q, X[77:78])[0, 0])
    nn = capi.Neighbors.create(X, metric="dot")
    seen = {}
    for k in (1, 17, 33, 65):                                    # <32>, <64>, <128>, <256>
        gi, gs = nn.query_vectors(q, k)
        at = np.flatnonzero(gi[0] == 77)
        seen[k] = float(gs[0, at[0]]) if at.size else None
        print("overflow, capacity of k = %d: candidate (2^100, -2^100) scores %r at slot %s" % (k, seen[k], at.tolist()))
        assert not np.isnan(gs).any()
    for k, s in seen.items():
        assert s == np.inf, "k = %d: the score of (2^100, 2^100) . (2^100, -2^100) is %r, the header's chain gives +inf" % (k, s)
        gi, gs = nn.query_vectors(q, k)
        want_i = np.concatenate([[77], np.delete(np.arange(130), 77)])[:k].astype(np.int32)
        assert np.array_equal(gi[0], want_i) and gs[0, 0] == np.inf and np.all(np.isneginf(gs[0, 1:]))

"""The alignment model (tests/align_ref.py) against itself, without a device: on every designed family the sorted walk and the
synchronous rounds give the same one-to-one set, that set has no blocking pair, the mutual pairs are the pairs of round 1, and
the family has the structure it is named for; on general floats the chain differs from the correctly rounded dot product in
qualifying scores, so a tile that summed otherwise would be caught by the byte comparison of test_align_gpu.py."""
import numpy as np
import pytest

import align_ref as A
import chain_ref as CH
import match_ref as M


def _check(S, T, what):
    """Both assignments on one family; returns (p, q, s, mate_a, mate_b, assigning rounds)."""
    nA, nB = S.shape
    p, q, s = A.candidates(S, T)
    assert np.all(np.diff(p * nB + q) > 0)                                             # ascending (a, b), no candidate twice
    mate_a, mate_b, pair = A.greedy(nA, nB, p, q, s)
    r_a, r_b, count, first = A.rounds(nA, nB, p, q, s)
    assert np.array_equal(mate_a, r_a) and np.array_equal(mate_b, r_b), what           # (i) equals (ii)
    assert A.blocking_pairs(p, q, s, mate_a, mate_b) == [], what
    got_a, got_b = mate_a[mate_a >= 0], mate_b[mate_b >= 0]
    assert np.unique(got_a).size == got_a.size and np.unique(got_b).size == got_b.size, what       # one-to-one
    assert all(mate_b[y] == x for x, y in enumerate(mate_a) if y >= 0) and got_a.size == got_b.size
    assert sorted(first) == A.mutual_pairs(nA, nB, p, q, s), what                      # the mutual pairs are round 1's
    free_a, free_b = mate_a < 0, mate_b < 0
    assert not np.any(free_a[p] & free_b[q]), what                                     # no candidate with both ends free
    return p, q, s, mate_a, mate_b, count


@pytest.mark.parametrize("shape", A.TILE_SHAPES)
def test_tile_tables_qualify_between_one_and_twenty_percent(shape):
    nA, nB, dim = shape
    for metric in A.METRICS:
        X, source, target, S, T, share = A.tile_case(nA, nB, dim, metric)
        n, h = nA + nB, (nA + nB) // 2
        assert np.array_equal(X[h:2 * h], X[:h]) and np.any(X[:h] != 0)                # the second half copies the first
        assert np.array_equal(np.sort(np.concatenate([source, target])), np.arange(n)) and (source.size, target.size) == (nA, nB)
        p, q, s, mate_a, mate_b, _ = _check(S, T, (shape, metric))
        assert p.size == round(share * nA * nB) and A.SHARE[0] <= share <= A.SHARE[1], (shape, metric, share)
        assert np.any(s == T)                                                          # T is attained
        out = A.align_scores(S, source, target, T)
        assert out[7]["candidates"] == p.size and out[7]["assigned"] == int((mate_a >= 0).sum()) >= 1
        assert np.all(np.isin(out[0], source)) and np.all(np.isin(out[1], target))
    if min(nA, nB) > 1:                                                                # a row and its copy lie in different sets somewhere
        twins = np.isin(np.arange(h), source) & np.isin(np.arange(h, 2 * h), target)
        assert twins.any()


def test_general_floats_tell_the_chain_from_the_rounded_dot():
    differ = 0
    for (nA, nB, dim), metric in (((193, 300, 200), "cosine"), ((193, 300, 200), "dot"), ((65, 129, 33), "dot"), ((129, 65, 31), "cosine")):
        X, source, target, S, T, _ = A.tile_case(nA, nB, dim, metric)
        XH = M.KR.prepare(X, M.MODEL_METRIC[metric])
        R = CH.dot64(XH[source], XH[target])
        hit = S >= T
        d = int((S[hit].view(np.uint32) != R[hit].view(np.uint32)).sum())
        assert d > 0, (nA, nB, dim, metric)
        differ += d
    assert differ >= 100


def test_threshold_family_holds_scores_at_and_one_ulp_below():
    X, source, target, S, T = A.threshold_case()
    assert M.below(T) == T - 1 and np.all(source % 2 == 0) and np.all(target % 2 == 1)
    at, under = int((S == T).sum()), int((S == M.below(T)).sum())
    assert at >= 10 and under >= 10
    p, q, s, *_ = _check(S, T, "at T")
    assert p.size == int((S >= T).sum()) and int((s == T).sum()) == at and not np.any(s == M.below(T))
    p2, *_ = _check(S, M.below(T), "one ulp below T")
    assert p2.size == p.size + under


def test_all_ties_pair_in_id_order_one_pair_per_round():
    X, source, target, S, T = A.ties_case()
    assert np.all(X == X[0]) and np.all(S == T) and S.shape == (64, 80)
    p, q, s, mate_a, mate_b, count = _check(S, T, "ties")
    assert p.size == 64 * 80 and np.array_equal(mate_a, np.arange(64)) and count == 64             # the bound's worst case
    out = A.align_scores(S, source, target, T)
    assert np.array_equal(out[3], 64 + np.arange(64)) and out[7]["mutual"] == 1 and out[7]["ambiguous_sources"] == 64


def test_weighted_chain_hands_out_second_choices_one_round_each():
    X, source, target, S, T, perm = A.chain_case()
    pairs = source.size
    assert X.shape == (600, 599) and pairs == target.size == 300 and np.any(np.diff(perm) < 0)
    p, q, s, mate_a, mate_b, count = _check(S, T, "chain")
    assert p.size == 599 and sorted(s.tolist()) == list(range(2, 601))                 # exactly the edges, each scoring its weight
    assert count >= 250                                                                # here: one round per pair
    out = A.align_scores(S, source, target, T)
    assert out[7]["assigned"] == pairs and pairs - out[7]["mutual"] >= 290
    # s_i is assigned t_i, and for every i >= 1 that is its second choice: t_(i-1) scores higher
    where_a, where_b = {int(r): k for k, r in enumerate(source)}, {int(r): k for k, r in enumerate(target)}
    for i in range(pairs):
        x, y = where_a[int(perm[2 * i])], where_b[int(perm[2 * i + 1])]
        assert mate_a[x] == y
        if i:
            assert S[x, where_b[int(perm[2 * i - 1])]] > S[x, y] >= T


def test_star_gives_the_hub_to_one_source_and_fills_the_other_targets():
    X, source, target, S, T, perm = A.star_case()
    p, q, s, mate_a, mate_b, count = _check(S, T, "star")
    hub = int(np.searchsorted(target, perm[300]))
    assert target[hub] == perm[300] and p.size == 600 and np.all(np.argmax(S, axis=1) == hub)      # everyone's first choice
    assert np.all(mate_b >= 0) and int((mate_a >= 0).sum()) == 41 and int((mate_a == hub).sum()) == 1
    assert source[mate_b[hub]] == perm[299]                                            # the best of them
    assert count >= 2                                                                  # the cascade: second choices come after the hub is gone


def test_extremes_nothing_and_everything():
    X, source, target, S, _, _ = A.tile_case(65, 129, 33, "cosine")
    hi, lo = np.nextafter(S.max(), np.float32(np.inf)), np.nextafter(S.min(), np.float32(-np.inf))
    out = A.align_scores(S, source, target, hi)
    assert out[0].size == 0 and np.all(out[3] == -1) and np.all(out[6] == -1) and not out[5].any() and not out[4].any()
    assert out[7] == {"candidates": 0, "assigned": 0, "mutual": 0, "sources_with_candidates": 0, "targets_with_candidates": 0,
                      "ambiguous_sources": 0}
    p, q, s, mate_a, mate_b, _ = _check(S, lo, "everything")
    assert p.size == 65 * 129 and int((mate_a >= 0).sum()) == 65

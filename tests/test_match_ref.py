"""The matching model (tests/match_ref.py) against itself, without a device: the scores are symmetric in bits, every designed
family has the structure it is named for, and on general floats the chain differs from the correctly rounded dot product in
qualifying scores, so a tile that summed otherwise would be caught by the byte comparison of test_match_gpu.py."""
import numpy as np
import pytest

import chain_ref as CH
import match_ref as M


def test_scores_are_symmetric_in_bits():
    for dim, n, metric in ((200, 300, "cosine"), (33, 129, "dot"), (3, 65, "cosine"), (1, 193, "dot")):
        S = M.tile_case(dim, n, metric)[1]
        assert S.view(np.uint32).tobytes() == np.ascontiguousarray(S.T).view(np.uint32).tobytes(), (dim, n, metric)
    for S in (M.path_case()[1], M.threshold_case()[1]):
        assert S.tobytes() == np.ascontiguousarray(S.T).tobytes()


@pytest.mark.parametrize("dim", M.TILE_DIMS)
def test_tile_tables_qualify_between_one_and_twenty_percent(dim):
    for n in M.TILE_SIZES:
        for metric in M.METRICS:
            X, S, T, share = M.tile_case(dim, n, metric)
            h = n // 2
            assert np.array_equal(X[h:2 * h], X[:h]) and np.any(X[:h] != 0)                 # the second half copies the first
            a, b, s, label, summary = M.match_scores(S, np.arange(n), T)
            pairs = n * (n - 1) // 2
            assert summary["pairs"] == a.size == round(share * pairs) and M.SHARE[0] <= share <= M.SHARE[1], (dim, n, metric, share)
            assert np.any(s == T)                                                           # T is attained
            assert np.all(a < b) and np.all(np.diff(a.astype(np.int64) * n + b) > 0)        # ascending (a, b), no pair twice
            # a row and its copy score the same against everything, so they share a label whenever either has a pair
            twin = label[h:2 * h] == label[:h]
            paired = np.isin(np.arange(h), np.concatenate([a, b]))
            assert np.all(twin[paired])


def test_general_floats_tell_the_chain_from_the_rounded_dot():
    differ = 0
    for dim, n, metric in ((200, 300, "cosine"), (200, 193, "dot"), (33, 300, "dot"), (31, 129, "cosine")):
        X, S, T, _ = M.tile_case(dim, n, metric)
        XH = M.KR.prepare(X, M.MODEL_METRIC[metric])
        R = CH.dot64(XH, XH)
        p, q = np.triu_indices(n, 1)
        hit = S[p, q] >= T
        d = int((S[p, q][hit].view(np.uint32) != R[p, q][hit].view(np.uint32)).sum())
        assert d > 0, (dim, n, metric)
        differ += d
    assert differ >= 100


def test_threshold_family_holds_scores_at_and_one_ulp_below():
    X, S, T = M.threshold_case()
    n = X.shape[0]
    p, q = np.triu_indices(n, 1)
    upper = S[p, q]
    assert M.below(T) == T - 1 and np.array_equal(X, np.rint(X))                           # one ulp is 1 up there
    at, under = int((upper == T).sum()), int((upper == M.below(T)).sum())
    assert at >= 10 and under >= 10
    a, b, s, label, summary = M.match_scores(S, np.arange(n), T)
    assert summary["pairs"] == int((upper >= T).sum()) and int((s == T).sum()) == at and not np.any(s == M.below(T))
    a2, b2, s2, _, summary2 = M.match_scores(S, np.arange(n), M.below(T))
    assert summary2["pairs"] == summary["pairs"] + under


def test_path_is_one_component_with_exactly_its_edges():
    X, S, perm = M.path_case()
    assert X.shape == (511, 512) and np.all(X.sum(axis=1) == 2)
    a, b, s, label, summary = M.match_scores(S, np.arange(511), 1.0)
    edges = sorted((int(min(perm[r], perm[r + 1])), int(max(perm[r], perm[r + 1]))) for r in range(510))
    assert list(zip(a.tolist(), b.tolist())) == edges and np.all(s == 1) and a.size == 510
    assert summary == {"pairs": 510, "components": 1, "groups": 1, "grouped_rows": 511, "largest": 511}
    assert np.all(label == 0)
    assert np.any(np.diff(perm) < 0)                                                       # the ids do not follow the path


def test_forest_has_a_joined_pair_of_paths_a_star_and_isolated_rows():
    X, S, perm, edges, (A, B, star, iso) = M.forest_case()
    n = X.shape[0]
    a, b, s, label, summary = M.match_scores(S, np.arange(n), 1.0)
    assert a.size == len(edges) == 399 and np.all(s == 1)
    assert summary == {"pairs": 399, "components": 32, "groups": 2, "grouped_rows": 401, "largest": 300}
    both = perm[list(A) + list(B)]
    assert np.all(label[both] == both.min()) and np.all(label[perm[list(star)]] == perm[list(star)].min())
    assert np.array_equal(label[perm[list(iso)]], perm[list(iso)])                         # a row without a pair labels itself
    # a subset that leaves out vertex 40 of the first path cuts the joined component in two
    subset = np.setdiff1d(np.arange(n), [perm[40]])
    a2, b2, s2, label2, summary2 = M.match_scores(S[np.ix_(subset, subset)], subset, 1.0)
    assert summary2["pairs"] == 397 and summary2["groups"] == 3 and summary2["largest"] == 300 - 41
    head = perm[0:40]
    at = np.searchsorted(subset, head)
    assert np.all(label2[at] == head.min())

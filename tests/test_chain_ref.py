"""The numpy model of the header's score (tests/chain_ref.py) held to what it claims, on the CPU, before any GPU test relies on
it: exact on integers, fused where fusing shows, and -- the condition of the byte comparisons in test_nn_chain_gpu.py,
test_pca_chain_gpu.py and the chain tests of k-means and predict -- different from the sums a wrong tile would give."""
import numpy as np
import pytest

import chain_ref as CH
import kmeans_ref as KR
import nn_ref as R

CHAIN_DIMS = [31, 32, 33, 50, 200, 1024]        # every dim >= 31 at which a GPU test compares bytes with `chain`


def test_chain_is_the_exact_product_on_integers():
    for dim in (1, 3, 4, 5, 33, 200):
        A, B = R.integers(dim, (37, dim), -8, 8), R.integers(dim + 1000, (41, dim), -8, 8)
        want = A.astype(np.int64) @ B.astype(np.int64).T
        assert np.abs(want).max() < 2 ** 24
        for S in (CH.chain(A, B), CH.descending(A, B), CH.unfused(A, B), CH.dot64(A, B)):
            assert S.dtype == np.float32 and S.shape == (37, 41)
            assert np.array_equal(S.astype(np.int64), want) and np.array_equal(S, np.rint(S))


def test_fused_and_unfused_differ_in_the_last_bit_by_hand():
    """d = 0: 2^-12 * 2^-12 = 2^-24, exact either way.  d = 1: (1 + 2^-12)^2 = 1 + 2^-11 + 2^-24.  Fused, the sum
    1 + 2^-11 + 2^-23 is a float and nothing is rounded.  Unfused, the product is a tie and rounds to even, 1 + 2^-11; adding
    2^-24 is a tie again and rounds to even again: 1 + 2^-11, one ulp below."""
    a = np.array([[2.0 ** -12, 1 + 2.0 ** -12]], np.float32)
    assert CH.chain(a, a)[0, 0] == np.float32(1 + 2.0 ** -11 + 2.0 ** -23)
    assert CH.unfused(a, a)[0, 0] == np.float32(1 + 2.0 ** -11)
    assert np.nextafter(CH.unfused(a, a)[0, 0], np.float32(2)) == CH.chain(a, a)[0, 0]
    # and the order of d shows: 2^24 + 1 - 2^24 is 0 ascending (the 1 is lost), 1 descending
    b = np.array([[2.0 ** 12, 1.0, -2.0 ** 12]], np.float32)
    c = np.array([[2.0 ** 12, 1.0, 2.0 ** 12]], np.float32)
    assert CH.chain(b, c)[0, 0] == 0 and CH.descending(b, c)[0, 0] == 1


def test_chain_pads_to_four_and_refuses_small_products():
    A, B = R.random_rows(1, 5, 7), R.random_rows(2, 6, 7)
    A8, B8 = np.zeros((5, 8), np.float32), np.zeros((6, 8), np.float32)
    A8[:, :7], B8[:, :7] = A, B
    assert CH.chain(A, B).tobytes() == CH.chain(A8, B8).tobytes()
    tiny = np.array([[1.0, 2.0 ** -60]], np.float32)
    with pytest.raises(AssertionError):
        CH.chain(tiny, tiny)
    CH.chain(tiny, np.array([[1.0, 0.0]], np.float32))          # a zero product is no small product


def test_overflow_as_the_header_states_it():
    """(2^100, 2^100) . (2^100, -2^100): the chain reaches +inf at d = 0 and fmaf(2^100, -2^100, +inf) = +inf (the product is
    finite inside the fused operation); a product rounded on its own is -inf and +inf - inf is NaN."""
    q = np.array([[2.0 ** 100, 2.0 ** 100]], np.float32)
    c = np.array([[2.0 ** 100, -2.0 ** 100], [-2.0 ** 100, 2.0 ** 100], [2.0 ** 100, 2.0 ** 100], [-2.0 ** 100, -2.0 ** 100]], np.float32)
    assert np.array_equal(CH.chain(q, c)[0], np.array([np.inf, -np.inf, np.inf, -np.inf], np.float32))
    u = CH.unfused(q, c)[0]
    assert np.isnan(u[0]) and np.isnan(u[1]) and u[2] == np.inf and u[3] == -np.inf


def test_topk_is_the_total_order():
    S = R.integers(3, (50, 90), -3, 3)                           # many ties
    self_pos = np.arange(50) % 90
    for k in (1, 7, 89):
        for sp in (None, self_pos):
            a, b = CH.topk(S, k, sp), R.stable_topk(S, k, sp)
            assert np.array_equal(a[0], b[0]) and a[1].tobytes() == b[1].tobytes()
    Z = np.array([[-0.0, 0.0, np.nan, -np.inf, 1.0, np.nan, 0.0]], np.float32)
    idx, score = CH.topk(Z, 7)
    assert idx.tolist() == [[4, 0, 1, 6, 2, 3, 5]]               # -0 = +0 by id; NaN = -inf by id
    assert score.tobytes() == np.array([[1.0, -0.0, 0.0, 0.0, -np.inf, -np.inf, -np.inf]], np.float32).tobytes()
    idx, _ = CH.topk(Z, 3, np.array([4]))
    assert idx.tolist() == [[0, 1, 6]]
    assert CH.ranks(Z, np.array([1])).tolist() == [2] and CH.ranks(Z, np.array([2])).tolist() == [5]
    assert CH.ranks(Z, np.array([2]), excluded=(Z == 1)).tolist() == [4]


@pytest.mark.parametrize("metric", [KR.COSINE, KR.EUCLID])
@pytest.mark.parametrize("dim", CHAIN_DIMS)
def test_the_model_tells_the_chain_from_its_rivals(dim, metric):
    """On the rows the GPU tests use, at least half of the 70 x 300 scores must differ from fp32(fp64 dot), from the
    descending-d chain and from the unfused chain: a tile that computed one of those could not pass a comparison of bytes."""
    X = KR.prepare(R.random_rows(700 + dim, 300, dim), metric)   # EUCLID: the rows themselves, as the DOT metric scores them
    Q = X[:70]
    S = CH.chain(Q, X)
    assert np.all(np.isfinite(S))
    for name, rival in (("fp64 dot", CH.dot64), ("descending d", CH.descending), ("unfused", CH.unfused)):
        share = float(np.mean(rival(Q, X) != S))
        print("dim %d %s: %.2f of the scores differ from %s" % (dim, metric, share, name))
        assert share >= 0.5, "the model does not discriminate against %s at dim %d" % (name, dim)

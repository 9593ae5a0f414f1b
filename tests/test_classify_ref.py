"""CPU-only checks of the classification yardstick (tests/classify_ref.py) against independent statements of itself: its exp and
log against the math library, its gradient against a textbook fp64 softmax gradient within a bound derived from the chain
length, its L-BFGS on the planted family the GPU test runs (so that test asserts nothing the model does not reach alone), and
the case list the GPU test shares, which asserts its own coverage of the tile edges."""
import math
import struct

import numpy as np
import pytest

import classify_ref as R
import nn_ref


def _ulps(got, want):
    return float((np.abs(got - want) / np.spacing(np.abs(want))).max())


def test_cexp_against_the_math_library():
    t = -np.concatenate([np.linspace(0.0, 708.0, 100001), 50.0 * (0.5 + 0.5 * nn_ref.uniform(1, (100000,))) ** 3, [0.0, 708.0, 1e-300, 1e-17]])
    got, want = R.cexp(t), np.array([math.exp(v) for v in t.tolist()])
    worst = _ulps(got, want)
    print("cexp: %.2f ulp at worst over %d points of [-708, 0]" % (worst, t.size))
    assert worst <= 2.0
    assert R.cexp(np.array([0.0, -0.0])).tolist() == [1.0, 1.0]
    assert R.cexp(np.array([-708.0000001, -1e4, -np.inf])).tolist() == [0.0, 0.0, 0.0]
    assert np.all(np.diff(R.cexp(np.linspace(-700.0, 0.0, 20001))) > 0)


def test_clog_against_the_math_library():
    S = np.concatenate([np.linspace(1.0, 1024.0, 100001), 1.0 + (0.5 + 0.5 * nn_ref.uniform(2, (100000,))) ** 6, [1.0, 1.0 + 2.0 ** -52, 2.0, 1024.0]])
    got, want = R.clog(S), np.array([math.log(v) for v in S.tolist()])
    nz = want > 0
    worst, absolute = _ulps(got[nz], want[nz]), float(np.abs(got - want).max())
    print("clog: %.2f ulp, %.3g absolute at worst over %d points of [1, 1024]" % (worst, absolute, S.size))
    assert worst <= 4.0 and absolute <= 9e-16
    assert R.clog(np.array([1.0]))[0] == 0.0


def _f32(v):
    return struct.unpack("f", struct.pack("f", v))[0]


def test_a_row_against_a_scalar_loop():
    """One softmax row and its loss term and residuals, spelled with Python floats."""
    k = R.build_case(R.CASES[1])
    XH, W, labels = k["XH"], k["W"], k["labels"]
    mem = R.members(labels, k["train"])
    Z = R.logits(XH[mem], W)
    l, Rr = R.residuals(Z, labels[mem])
    fact = [float(math.factorial(j)) for j in range(14)]
    for t in (0, 5, len(mem) - 1):
        z = [float(v) for v in Z[t]]
        m = max(z)
        e = []
        for v in z:
            tt = v - m
            kk = float(round(tt * R.INVLN2))                  # Python rounds halves to even, as rint
            r = (tt - kk * R.LN2HI) - kk * R.LN2LO
            p = 1.0 / fact[13]
            for j in range(12, -1, -1):
                p = p * r + 1.0 / fact[j]
            e.append(math.ldexp(p, int(kk)))
        S = 0.0
        for v in e:
            S = S + v
        f, kk = math.frexp(S)
        if f < R.SQRT_HALF:
            f, kk = 2.0 * f, kk - 1
        s = (f - 1.0) / (f + 1.0)
        w = s * s
        q = 1.0 / 25.0
        for j in range(23, 0, -2):
            q = q * w + 1.0 / float(j)
        y = int(labels[mem[t]])
        assert l[t] == float(kk) * R.LN2HI + (float(kk) * R.LN2LO + (2.0 * s) * q) - (z[y] - m)
        for c in range(len(z)):
            qc = e[c] / S
            pf = 0.0 if qc < 2.0 ** -60 else _f32(qc)
            assert Rr[t, c] == _f32(pf - (1.0 if c == y else 0.0))


def test_the_cut_leaves_exact_zeros():
    k = R.under_the_cut_case()
    Z = R.logits(k["XH"], k["W"])
    T, E, S, PF = R.softmax(Z)
    assert (E / S[:, None] < 2.0 ** -60).sum() >= 4 and np.all(E > 0)      # under the cut, yet not zero before it
    l, Rr = R.residuals(Z, k["labels"])
    assert Rr[3].tolist() == [-1.0, 1.0, 0.0] and l[3] == 99.0              # the true class lost by 99: its loss is the gap
    assert R.evaluate(k["XH"], k["labels"], None, k["W"], 0.0) is not None
    assert R.evaluate(k["XH"], k["labels"], None, np.full_like(k["W"], 3e38), 0.0) is None     # finite weights, a logit that overflows


@pytest.mark.parametrize("case", R.CASES, ids=[c[0] for c in R.CASES])
def test_gradient_against_a_plain_fp64_softmax_gradient(case):
    """|g - g64| <= (1024 + Dp) 2^-23 mean_t sum |r| |x| per element: a chain of at most 1024 members rounds once per step
    (1024 2^-24 of the sum of magnitudes), the residuals are rounded to fp32 (2^-24) and inherit the logit chain's Dp roundings
    through the softmax, whose derivative is at most 1; the factor 2 is the slack the fp64 piece sums and the l2 term share."""
    k = R.build_case(case)
    f, g = R.evaluate(k["XH"], k["labels"], k["train"], k["W"], 1e-4)
    g64, mag = R.plain_gradient(k["XH"], k["labels"], k["train"], k["W"], 1e-4)
    Dp = k["XH"].shape[1]
    bound = (1024 + Dp) * 2.0 ** -23 * mag
    worst = float((np.abs(g - g64) / np.maximum(bound, 1e-300)).max())
    print("%s: the worst element is %.3g of its bound" % (k["name"], worst))
    assert np.all(np.abs(g - g64) <= bound)
    assert math.isfinite(f) and f > 0


def test_lbfgs_on_the_planted_family():
    X, y = R.planted(7, 600, 12, 5)
    train = (np.arange(600) % 5 != 4).astype(np.uint8)
    XH = R.features(X, R.COSINE)
    assert R.features_in_range(XH)
    fit = R.Fit(XH, y, train, 5)
    ran, stop = fit.run(200)
    print("planted: %d iterations, %d evaluations, loss %.17g" % (ran, fit.evaluations, fit.f))
    assert stop == R.GRADIENT and ran == fit.iterations < 200
    assert np.all(np.diff(fit.losses) <= 0) and abs(fit.losses[0] - math.log(5)) <= 1e-13        # zero weights: every row loses log C
    label, prob = R.predict(XH, fit.weights())
    test = R.score(y, label, 1 - train, 5)
    assert test["count"] == 120 and test["accuracy"] == 1.0 and test["macro_f1"] == 1.0
    assert R.score(y, label, train, 5)["accuracy"] == 1.0
    assert np.all(prob > 0.2) and np.all(prob <= 1)
    # run(a) then run(b) is run(a + b)
    one, two = R.Fit(XH, y, train, 5), R.Fit(XH, y, train, 5)
    one.run(6)
    two.run(2); two.run(4)
    assert one.theta.tobytes() == two.theta.tobytes() and one.evaluations == two.evaluations and one.stop == two.stop == R.MAXITER


def test_score_against_a_double_loop():
    labels = np.array([0, 1, 2, -1, 1, 1, 0, 2, -1, 0], np.int32)
    pred = np.array([0, 2, 2, 1, 1, 0, 0, 2, 0, 1], np.int32)
    mask = np.array([1, 1, 1, 1, 0, 1, 1, 1, 1, 1], np.uint8)
    s = R.score(labels, pred, mask, 4)
    tp, fp, fn = [0] * 4, [0] * 4, [0] * 4
    for p in range(10):
        if labels[p] < 0 or not mask[p]:
            continue
        if labels[p] == pred[p]:
            tp[labels[p]] += 1
        else:
            fn[labels[p]] += 1; fp[pred[p]] += 1
    assert (s["tp"].tolist(), s["fp"].tolist(), s["fn"].tolist()) == (tp, fp, fn) and s["count"] == 7 and s["correct"] == 4
    f1 = [2 * tp[c] / (2 * tp[c] + fp[c] + fn[c]) for c in range(3)]           # class 3 never appears: not in the mean
    assert s["macro_f1"] == (0.0 + f1[0] + f1[1] + f1[2]) / 3.0 and s["accuracy"] == 4 / 7
    assert R.score(labels, pred, np.zeros(10, np.uint8), 4)["macro_f1"] == 0.0


def test_the_case_list_covers_the_edges():
    """Every C, dim and n_T the tile edges ask for, both normalisations, a subset, a class without members, positions that are
    unlabelled and labelled positions that do not train, and features inside [2^-20, 2^20]."""
    built = [R.build_case(c) for c in R.CASES]
    assert {k["classes"] for k in built} >= R.EDGES["C"]
    assert {k["dim"] for k in built} >= R.EDGES["dim"]
    assert {len(R.members(k["labels"], k["train"])) for k in built} >= R.EDGES["n_T"]
    assert {k["normalize"] for k in built} == {R.COSINE, R.RAW}
    assert any(k["subset"] is not None for k in built) and any(k["empty"] for k in built)
    for k in built:
        mem = R.members(k["labels"], k["train"])
        assert len(mem) == k["n_t"] and R.features_in_range(k["XH"]) and np.all(np.isfinite(k["W"]))
        n = len(k["labels"])
        if k["n_t"] > 1:
            assert n > k["n_t"] and (k["labels"] < 0).any() and ((k["labels"] >= 0) & (k["train"] == 0)).any()
            assert np.diff(mem).max() > 1                                      # the members are not one run of positions
        if k["empty"]:
            assert not (k["labels"][mem] == 1).any()
        if k["subset"] is not None:
            assert np.all(np.diff(k["subset"]) > 0) and len(k["subset"]) == n < len(k["rows"])
    cut = R.under_the_cut_case()
    T, E, S, PF = R.softmax(R.logits(cut["XH"], cut["W"]))
    assert (PF == 0).any()

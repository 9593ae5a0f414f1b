"""Softmax regression on the device against numpy (tests/classify_ref.py), byte for byte: the loss and the gradient after
set_weights at the tile edges of every kernel (the case list of classify_ref, whose coverage test_classify_ref.py asserts), the
labels and probabilities of a prediction with a designed tie, whole L-BFGS runs replayed word for word, the planted family, the
score counts, determinism, the trainer-handle entry point and the errors."""
import numpy as np
import pytest

import geglove
from geglove import capi, synth
from helpers import make_config
import classify_ref as R

pytestmark = pytest.mark.gpu

ALL = R.CASES + [None]                                                     # None: the row under the 2^-60 cut
IDS = [c[0] for c in R.CASES] + ["cut"]


def _build(case):
    return R.under_the_cut_case() if case is None else R.build_case(case)


def _create(k, **kw):
    return capi.Classifier.create(k["rows"], k["labels"], k["classes"], train=k["train"], subset=k["subset"], normalize=k["normalize"], **kw)


@pytest.mark.parametrize("case", ALL, ids=IDS)
def test_eval_is_the_model_byte_for_byte(gpu, case):
    k = _build(case)
    clf = _create(k, l2=1e-4)
    g0 = clf.get()
    assert (g0["n"], g0["dim"], g0["classes"], g0["n_train"]) == (len(k["labels"]), k["dim"], k["classes"], k["n_t"])
    assert not clf.weights.any() and (g0["iterations"], g0["stop"], g0["evaluations"]) == (0, "none", 0)
    clf.set_weights(k["W"])
    assert clf.weights.tobytes() == k["W"].tobytes()
    loss, grad = clf.eval()
    want_loss, want_grad = R.evaluate(k["XH"], k["labels"], k["train"], k["W"], 1e-4)
    print("%s: loss %.17g (model %.17g), %d gradient words differ" % (k["name"], loss, want_loss, int((grad != want_grad).sum())))
    assert loss == want_loss
    bad = np.argwhere(grad.view(np.uint64) != want_grad.view(np.uint64))
    assert bad.size == 0, "g[%d][%d]: got %r, want %r (%d differ)" % (bad[0][0], bad[0][1], grad[tuple(bad[0])], want_grad[tuple(bad[0])], len(bad))
    again_loss, again_grad = clf.eval()                                    # a pure read, and the same bytes
    assert again_loss == loss and again_grad.tobytes() == grad.tobytes()
    assert clf.get() == dict(g0) and clf.weights.tobytes() == k["W"].tobytes()


@pytest.mark.parametrize("case", ALL, ids=IDS)
def test_predict_is_the_model_byte_for_byte(gpu, case):
    """The weights of the class that wins most often are copied over another class: wherever it would win, the two tie and the
    lower id is reported."""
    k = _build(case)
    W = k["W"].copy()
    often = int(np.bincount(R.predict(k["XH"], W)[0], minlength=k["classes"]).argmax())
    other = k["classes"] - 1 if often != k["classes"] - 1 else 0
    W[other] = W[often]
    lo, hi = min(often, other), max(often, other)
    clf = _create(k)
    clf.set_weights(W)
    label, prob = clf.predict()
    want_label, want_prob = R.predict(k["XH"], W)
    assert label.dtype == np.int32 and prob.dtype == np.float32 and label.shape == prob.shape == (len(k["labels"]),)
    assert label.tobytes() == want_label.tobytes()
    assert prob.tobytes() == want_prob.tobytes()
    assert (want_label == lo).any() and not (label == hi).any()            # the tie happens, and never goes to the higher id
    s = clf.score(confusion=True)
    want = R.score(k["labels"], want_label, None, k["classes"])
    for name in ("tp", "fp", "fn", "confusion"):
        assert np.array_equal(s[name], want[name]), name
    assert (s["count"], s["correct"], s["accuracy"], s["macro_f1"]) == (want["count"], want["correct"], want["accuracy"], want["macro_f1"])
    assert s["count"] == int((k["labels"] >= 0).sum())


@pytest.mark.parametrize("name,start", [("c3-d3", False), ("c17-d31", True)])
def test_twelve_iterations_replay_word_for_word(gpu, name, start):
    """From the zero start and from given weights; the second case has a class without members."""
    k = R.build_case([c for c in R.CASES if c[0] == name][0])
    clf = _create(k, l2=1e-3, tolerance=0.0)
    fit = R.Fit(k["XH"], k["labels"], k["train"], k["classes"], l2=1e-3, tolerance=0.0, weights=k["W"] if start else None)
    if start:
        clf.set_weights(k["W"])
    for chunk in (5, 7):                                                   # the state survives between the calls
        got, want = clf.run(chunk), fit.run(chunk)
        assert got == want == (chunk, "maxiter")
        g = clf.get()
        print("%s: %d iterations, %d evaluations, loss %.17g" % (name, g["iterations"], g["evaluations"], g["loss"]))
        assert (g["iterations"], g["stop"], g["evaluations"], g["loss"]) == (fit.iterations, fit.stop, fit.evaluations, fit.f)
        assert clf.weights.tobytes() == fit.weights().tobytes()
    loss, grad = clf.eval()
    assert loss == fit.f and grad.ravel().tobytes() == fit.g.tobytes()     # the master copy itself, through the gradient at it
    assert fit.evaluations > 12


def test_the_planted_family(gpu):
    X, y = R.planted(7, 600, 12, 5)
    train = (np.arange(600) % 5 != 4).astype(np.uint8)
    XH = R.features(X, R.COSINE)
    runs = []
    for _ in range(2):
        clf = capi.Classifier.create(X, y, 5, train=train)
        ran, stop = clf.run(200)
        label, prob = clf.predict()
        runs.append((ran, stop, clf.get(), clf.weights.tobytes(), label.tobytes(), prob.tobytes()))
    assert runs[0] == runs[1]                                              # two runs, the same bytes
    assert stop == "gradient" and 1 <= ran < 200
    test = clf.score(1 - train, confusion=True)
    assert test["count"] == 120 and test["accuracy"] == 1.0 and test["macro_f1"] == 1.0
    assert np.array_equal(test["confusion"], np.diag(np.bincount(y[train == 0], minlength=5)))
    assert clf.score(train)["count"] == 480
    fit = R.Fit(XH, y, train, 5)
    assert fit.run(200) == (ran, stop)
    g = clf.get()
    assert (g["iterations"], g["evaluations"], g["loss"]) == (fit.iterations, fit.evaluations, fit.f)
    assert clf.weights.tobytes() == fit.weights().tobytes()
    logits_ms, softmax_ms, gradient_ms = clf.kernel_ms
    assert logits_ms > 0 and softmax_ms > 0 and gradient_ms > 0


def test_score_over_a_mask(gpu):
    k = R.build_case(R.CASES[3])
    clf = _create(k)
    clf.set_weights(k["W"])
    label, _ = clf.predict()
    mask = (synth.splitmix64(5, len(label)) % np.uint64(3) == 0).astype(np.uint8)
    got, want = clf.score(mask, confusion=True), R.score(k["labels"], label, mask, k["classes"])
    for name in ("tp", "fp", "fn", "confusion"):
        assert np.array_equal(got[name], want[name]), name
    assert (got["count"], got["correct"], got["accuracy"], got["macro_f1"]) == (want["count"], want["correct"], want["accuracy"], want["macro_f1"])
    assert 0 < got["count"] < int((k["labels"] >= 0).sum())
    none = clf.score(np.zeros(len(label), np.uint8))
    assert (none["count"], none["accuracy"], none["macro_f1"]) == (0, 0.0, 0.0)


def test_trainer_handle_entry_point_equals_the_host_rows_one(gpu):
    V, N, dim, classes = 3000, 40000, 24, 7
    I, J, Xc, xmax = synth.synthetic_coo(V, N, seed=77)
    m = geglove.CooMatrix(V, I, J, Xc, xmax)
    cfg = make_config(dim, method="pglove", mode="deterministic", shuffle="java", seed=5)
    opt = geglove.Adagrad(m, cfg, cfg.costFunction())
    for it in range(3):
        opt.epoch(it)
    before = opt.state()
    rows = opt.extractResultF32().reshape(V, dim)
    keep = np.arange(1, V, 3, dtype=np.int32)
    for subset in (None, keep):
        n = V if subset is None else len(keep)
        labels = (synth.splitmix64(9, n) % np.uint64(classes + 1)).astype(np.int32) - 1
        train = (synth.splitmix64(10, n) % np.uint64(4) != 0).astype(np.uint8)
        for normalize in ("cosine", "none"):
            on_handle = capi.Classifier.create_glove(opt._h, labels, classes, train=train, subset=subset, normalize=normalize)
            on_rows = capi.Classifier.create(rows, labels, classes, train=train, subset=subset, normalize=normalize)
            assert on_handle.get() == on_rows.get() and on_handle.get()["n"] == n
            assert on_handle.run(3) == on_rows.run(3)
            assert on_handle.get() == on_rows.get() and on_handle.weights.tobytes() == on_rows.weights.tobytes()
            a, b = on_handle.predict(), on_rows.predict()
            assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes()
    after = opt.state()
    for name in before:
        assert before[name].tobytes() == after[name].tobytes(), name
    assert rows.tobytes() == opt.extractResultF32().tobytes()
    opt.close()


def test_a_non_finite_logit_is_a_state_error(gpu):
    """Huge finite weights: an argument the caller controls, refused with a message; the handle stays as it was."""
    k = R.under_the_cut_case()
    clf = _create(k)
    clf.set_weights(np.full_like(k["W"], 3e38))
    before = clf.get()
    for call in (clf.eval, clf.predict, lambda: clf.run(3)):
        with pytest.raises(capi.GeError) as e:
            call()
        assert e.value.status == capi.GE_ERR_STATE and "non-finite logit" in str(e.value)
    assert clf.get() == before
    clf.set_weights(k["W"])
    assert clf.eval()[0] == R.evaluate(k["XH"], k["labels"], None, k["W"], 1e-4)[0]
    with pytest.raises(capi.GeError) as e:
        clf.set_weights(np.where(np.arange(9).reshape(3, 3) == 4, np.inf, k["W"]).astype(np.float32))
    assert e.value.status == capi.GE_ERR_ARG and "non-finite input" in str(e.value)
    assert clf.weights.tobytes() == k["W"].tobytes()


def test_non_finite_rows_are_refused(gpu):
    k = R.build_case(R.CASES[1])
    for bad in (np.nan, np.inf, -np.inf):
        rows = k["rows"].copy()
        rows[77, 1] = bad
        with pytest.raises(capi.GeError) as e:
            capi.Classifier.create(rows, k["labels"], k["classes"], train=k["train"], normalize=k["normalize"])
        assert e.value.status == capi.GE_ERR_ARG and "non-finite input" in str(e.value)

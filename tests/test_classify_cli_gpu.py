"""`device: { classify: labels.tsv }` through the CLI on tests/golden/tiny.nt, with a labels file written from the dict keys:
<name>.classes.tsv next to the other two files -- the same banner, one `#` line with C, train, test, iterations, stop, loss and the
test figures, C `#` lines with the classes and their counts, one line per line of the dict file; the roles equal the seeded mask;
the summary's figures are those of the file's own lines; the output filters select the rows; without the key the output directory
is what it was; invalid values are configuration errors."""
import math
import os
import re

import numpy as np
import pytest

from geglove import capi
from test_cli_gpu import GOLD
from test_pca_cli_gpu import NAME, _log, _run

pytestmark = pytest.mark.gpu
FILTERED = "output:\n  uri: [ http://ex.org/authors/ ]\n"
EVERYTHING = "output:\n  uri: []\n  blank: []\n  literal: []\n"
TEXT = 5e-7                                  # %11.6E: half a unit of the seventh significant digit, relative


def _base():
    base = open(os.path.join(GOLD, "tiny.config.yml")).read()
    assert FILTERED in base and "  seed: 42" in base
    return base


def _with(base, output, extra):
    return base.replace(FILTERED, output).replace("  seed: 42", "  seed: 42\n" + extra)


def _class_of(key, kind):
    """Three classes whose ids are NOT in the order in which they first appear: ranks of the names in byte order."""
    return "writer" if "/authors/" in key else "paper" if "/papers/" in key else "Text" if kind == "LITERAL" else "other"


def _dict(cwd):
    dic = (cwd / "out" / (NAME + ".dict.tsv")).read_text().splitlines()
    head = dic.index("key\ttype")
    return [l.split("\t") for l in dic[head + 1:]]


def _labels_file(cwd, keys, skip=(), extra=()):
    lines = ["# key\tclass", ""]
    lines += ["%s\t%s" % (k, _class_of(k, t)) for i, (k, t) in enumerate(keys) if i not in skip]
    lines += list(extra)
    os.makedirs(cwd, exist_ok=True)
    (cwd / "labels.tsv").write_text("\n".join(lines) + "\n")


def _read(cwd):
    out = cwd / "out"
    dic = (out / (NAME + ".dict.tsv")).read_text().splitlines()
    vec = (out / (NAME + ".vectors.tsv")).read_text().splitlines()
    cls = (out / (NAME + ".classes.tsv")).read_text().splitlines()
    head = dic.index("key\ttype")
    assert cls[:head] == vec[:head] == dic[:head]                  # the same banner lines
    keys = [l.split("\t") for l in dic[head + 1:]]
    X = np.array([[float(x) for x in l.split("\t")] for l in vec[head:]], np.float32)
    summary = cls[head][2:].split("\t")
    assert cls[head].startswith("# ") and len(summary) == 8
    C = int(summary[0])
    classes = [l[2:].split("\t") for l in cls[head + 1:head + 1 + C]]
    assert all(l.startswith("# ") for l in cls[head + 1:head + 1 + C]) and not any(l.startswith("#") for l in cls[head + 1 + C:])
    rows = [l.split("\t") for l in cls[head + 1 + C:]]
    return dic[:head], keys, X, summary, classes, rows


def _check(keys, summary, classes, rows, fraction, skip=()):
    """The file against itself: structure, the class table, the roles against the seeded mask, and the summary's figures recomputed
    from the rows.  Returns (labels, train, test, predicted)."""
    n = len(keys)
    C, n_train, n_test, iterations = (int(v) for v in summary[:4])
    names = sorted({_class_of(k, t) for i, (k, t) in enumerate(keys) if i not in skip}, key=lambda s: s.encode())
    assert C == len(names) == len(classes) and [c[1] for c in classes] == names and [int(c[0]) for c in classes] == list(range(C))
    assert len(rows) == n and all(len(r) == 5 for r in rows) and [int(r[0]) for r in rows] == list(range(n))
    assert all(re.fullmatch(r"\d\.\d{6}E[+-]\d{2}", r[2]) for r in rows)                       # the number format of the vectors file
    predicted = np.array([int(r[1]) for r in rows])
    prob = np.array([float(r[2]) for r in rows])
    assert predicted.min() >= 0 and predicted.max() < C and np.all(prob >= 1.0 / C * (1 - 2 * TEXT)) and np.all(prob <= 1)
    labels = np.array([-1 if i in skip else names.index(_class_of(k, t)) for i, (k, t) in enumerate(keys)])
    assert [r[4] for r in rows] == [str(v) if v >= 0 else "-" for v in labels]
    labelled = np.flatnonzero(labels >= 0)
    pick = capi.holdout_mask(42, len(labelled), fraction) if fraction > 0 else np.zeros(len(labelled), np.uint8)
    role = np.array(["-"] * n, dtype=object)
    role[labelled] = np.where(pick != 0, "test", "train")
    assert [r[3] for r in rows] == role.tolist()                                             # the roles equal the mask
    train, test = role == "train", role == "test"
    assert (n_train, n_test) == (int(train.sum()), int(test.sum()))
    assert 1 <= iterations <= 200 and summary[4] in ("gradient", "maxiter", "linesearch")
    over = test if n_test > 0 else train                                                     # no test vertex: the figures of the training set
    tp = [int(((labels == c) & (predicted == c) & over).sum()) for c in range(C)]
    fp = [int(((labels != c) & (predicted == c) & over).sum()) for c in range(C)]
    fn = [int(((labels == c) & (predicted != c) & over).sum()) for c in range(C)]
    assert [[int(v) for v in c[2:]] for c in classes] == [list(v) for v in zip(tp, fp, fn)]
    loss, accuracy, macro = (float(v) for v in summary[5:])
    assert all("%.17g" % float(v) == v for v in summary[5:])                                 # text that parses back to the same double
    assert accuracy == sum(tp) / int(over.sum())
    f1 = [2.0 * tp[c] / (2 * tp[c] + fp[c] + fn[c]) for c in range(C) if tp[c] + fp[c] + fn[c] > 0]
    total = 0.0
    for v in f1:
        total = total + v
    assert macro == total / len(f1)
    assert 0 < loss <= math.log(C)                                                           # Armijo, from the zero start where f = log C
    return labels, train.astype(np.uint8), test.astype(np.uint8), predicted


def _mirror_loss(X, labels, train, C, normalize="cosine", l2=None, iterations=200):
    clf = capi.Classifier.create(X, labels, C, train=train, normalize=normalize, l2=l2)
    ran, stop = clf.run(iterations)
    return clf.get()["loss"], ran, stop, clf.predict()[0]


def test_classes_of_every_written_vertex(gpu, tmp_path):
    """The summary's loss against capi.Classifier on the WRITTEN vectors.  Those carry seven significant digits, so the fit the
    CLI ran saw slightly different rows; no margin is fixed in advance: the mirror is run on the written vectors and on five
    copies moved by half a unit of the seventh digit (the text's own error) in seeded directions, and 4 x the largest loss
    difference among them is allowed.  Measured on an MI355X: the largest difference among the moved copies 8.89e-08 at a
    loss of 0.0296, the CLI's loss 1.32e-08 from the mirror's."""
    plain = _run(tmp_path / "plain", _with(_base(), EVERYTHING, ""))
    keys0 = _dict(tmp_path / "plain")
    cwd = tmp_path / "run"
    _labels_file(cwd, keys0, skip=(1,), extra=["http://ex.org/authors/nobody\twriter"])
    r = _run(cwd, _with(_base(), EVERYTHING, "  classify: labels.tsv"))
    assert sorted(os.listdir(cwd / "out")) == sorted(NAME + s for s in (".classes.tsv", ".dict.tsv", ".vectors.tsv"))
    banner, keys, X, summary, classes, rows = _read(cwd)
    assert keys == keys0
    line = "Classify: labels.tsv (test 0.2, l2 1.0E-4, cosine, at most 200 iterations)"
    assert "# " + line in banner and line in _log(r.stdout, "Graph Embeddings")
    assert len(keys) >= 6 and {t for _, t in keys} >= {"URI", "LITERAL"}
    labels, train, test, predicted = _check(keys, summary, classes, rows, 0.2, skip=(1,))
    assert labels[1] == -1 and rows[1][3:] == ["-", "-"] and int(summary[0]) >= 3
    warn = [l for l in r.stdout.splitlines() if " WARN " in l]
    assert len(warn) == 1 and warn[0].endswith(":: 1 keys of labels.tsv are skipped: 1 unknown, 0 not written")
    done = _log(r.stdout, "Classify")
    assert len(done) == 1 and re.fullmatch(r"fitted %d classes on %d vertices in %d iterations \(%s\), (test|training) accuracy \S+ over \d+; wrote out/%s\.classes\.tsv"
                                           % (int(summary[0]), int(train.sum()), int(summary[3]), summary[4], re.escape(NAME)), done[0]), done
    # the loss against the mirror on the written vectors
    C = int(summary[0])
    want, ran, stop, label = _mirror_loss(X, labels, train, C)
    moved = []
    for s in range(5):
        sign = np.where(capi.holdout_mask(100 + s, X.size, 0.5).reshape(X.shape) != 0, 1.0, -1.0)
        moved.append(_mirror_loss((X.astype(np.float64) * (1.0 + TEXT * sign)).astype(np.float32), labels, train, C)[0])
    spread = max(abs(v - want) for v in moved)
    print("cli classes: loss %s, mirror %.17g, largest difference among the moved copies %.3g, the CLI's %.3g" % (summary[5], want, spread, abs(float(summary[5]) - want)))
    assert abs(float(summary[5]) - want) <= 4 * spread


def test_output_filters_and_the_other_keys(gpu, tmp_path):
    # a type filter, no normalisation, three iterations, no test split, a stronger penalty
    _run(tmp_path / "plain", _with(_base(), "output:\n  uri: []\n", ""))
    keys0 = _dict(tmp_path / "plain")
    cwd = tmp_path / "uris"
    _labels_file(cwd, keys0)
    extra = "  classify: labels.tsv\n  classify_test: 0\n  classify_l2: 0.01\n  classify_iterations: 3\n  classify_normalize: none"
    r = _run(cwd, _with(_base(), "output:\n  uri: []\n", extra))
    banner, keys, X, summary, classes, rows = _read(cwd)
    assert "# Classify: labels.tsv (test 0.0, l2 0.01, none, at most 3 iterations)" in banner
    assert len(keys) >= 6 and {t for _, t in keys} == {"URI"}
    labels, train, test, predicted = _check(keys, summary, classes, rows, 0.0)      # positions refer to the filtered dict
    assert int(summary[2]) == 0 and int(summary[3]) <= 3 and not test.any() and train.all()
    assert "WARN" not in r.stdout
    # a prefix filter that keeps the three authors: one class is left, which is an error; the labels of the others are "not written"
    cwd = tmp_path / "authors"
    _labels_file(cwd, keys0)
    r = _run(cwd, _with(_base(), FILTERED, "  classify: labels.tsv"), expect=1)
    assert "classify: 1 classes among the written vertices, at least 2 are needed" in r.stderr
    # a key that appears twice
    cwd = tmp_path / "twice"
    _labels_file(cwd, keys0, extra=["%s\tpaper" % keys0[0][0]])
    r = _run(cwd, _with(_base(), "output:\n  uri: []\n", "  classify: labels.tsv"), expect=1)
    assert "appears twice" in r.stderr
    r = _run(tmp_path / "missing", _with(_base(), "output:\n  uri: []\n", "  classify: nothing.tsv"), expect=1)
    assert "cannot open the labels file nothing.tsv" in r.stderr


def test_without_the_key_nothing_changes(gpu, tmp_path):
    base = _base()
    for name, text in (("plain", base), ("again", base), ("others", _with(base, FILTERED, "  classify_test: 0.5\n  classify_normalize: none"))):
        r = _run(tmp_path / name, text)
        assert sorted(os.listdir(tmp_path / name / "out")) == [NAME + ".dict.tsv", NAME + ".vectors.tsv"]
        assert "Classify" not in r.stdout
    for f in (NAME + ".dict.tsv", NAME + ".vectors.tsv"):
        want = (tmp_path / "plain" / "out" / f).read_bytes()
        assert (tmp_path / "again" / "out" / f).read_bytes() == want == (tmp_path / "others" / "out" / f).read_bytes()
        assert b"Classify" not in want


def test_bad_values_are_configuration_errors(gpu, tmp_path):
    base = _base()
    test = "Invalid configuration: Invalid device.classify_test, choose a fraction from 0 to 0.9"
    l2 = "Invalid configuration: Invalid device.classify_l2, choose a number from 0 up"
    iterations = "Invalid configuration: Invalid device.classify_iterations, choose a number from 1 up"
    for extra, message in (("  classify_test: 0.95", test), ("  classify_test: -0.1", test), ("  classify_test: half", test), ("  classify_test: nan", test),
                           ("  classify_l2: -1", l2), ("  classify_l2: inf", l2), ("  classify_l2: small", l2),
                           ("  classify_iterations: 0", iterations), ("  classify_iterations: 2.5", iterations), ("  classify_iterations: soon", iterations),
                           ("  classify_normalize: euclid", "Invalid configuration: Invalid device.classify_normalize, choose one of: cosine, none")):
        r = _run(tmp_path, _with(base, FILTERED, "  classify: labels.tsv\n" + extra), expect=1)
        assert message in r.stderr
        assert not os.path.exists(tmp_path / "out")

"""`device: { clusters: K }` through the CLI on tests/golden/tiny.nt: <name>.clusters.tsv next to the other two files -- same
banner, one `#` line with K, steps, converged and the objective, one line per line of the dict file -- with the labels and scores
capi.Clustering gives on the written vectors; the output filters select the rows; without the key the output directory is what it
was; invalid values are configuration errors."""
import os
import re

import numpy as np
import pytest

from geglove import capi
import kmeans_ref as R
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


def _read(cwd):
    out = cwd / "out"
    dic = (out / (NAME + ".dict.tsv")).read_text().splitlines()
    vec = (out / (NAME + ".vectors.tsv")).read_text().splitlines()
    clu = (out / (NAME + ".clusters.tsv")).read_text().splitlines()
    head = dic.index("key\ttype")
    assert clu[:head] == vec[:head] == dic[:head]                  # the same banner lines
    keys = [l.split("\t") for l in dic[head + 1:]]
    X = np.array([[float(x) for x in l.split("\t")] for l in vec[head:]], np.float32)
    assert clu[head].startswith("# ") and not any(l.startswith("#") for l in clu[head + 1:])
    K, steps, converged, objective = clu[head][2:].split("\t")
    rows = [l.split("\t") for l in clu[head + 1:]]
    return dic[:head], keys, X, (int(K), int(steps), int(converged), objective), rows


def _check(X, summary, rows, K, metric, iterations=50):
    """The file against capi.Clustering on the written vectors, same seed, K, metric and iteration limit.  The written vectors
    carry 7 significant digits, so a score moves by at most 2 * 5e-7 |x| |c| (Euclid: and 5e-7 |c|^2) on top of the bound B of
    the scores themselves and of the score's own text."""
    n = len(X)
    assert len(rows) == n and all(len(r) == 3 for r in rows)
    assert [int(r[0]) for r in rows] == list(range(n))
    assert all(re.fullmatch(r"-?\d\.\d{6}E[+-]\d{2}", r[2]) for r in rows)                    # the number format of the vectors file
    label = np.array([int(r[1]) for r in rows])
    score = np.array([float(r[2]) for r in rows])
    assert label.min() >= 0 and label.max() < K
    km = capi.Clustering.create(X, K, metric=metric, seed=42)
    steps, converged = km.run(iterations)
    assert summary[:3] == (K, steps, int(converged)), summary
    assert np.array_equal(label, km.labels)
    want = km.best.astype(np.float64)
    XH = R.prepare(X, metric)
    scale = R.norms(XH) * R.norms(km.centroids)[label] + (R.norms(km.centroids)[label] ** 2 if metric == R.EUCLID else 0)
    margin = 2 * ((XH.shape[1] + 2) * R.U + 2 * TEXT) * scale + TEXT * np.abs(want)
    print("cli clusters: %d lines, K %d, scores within %.3g of the margin" % (n, K, (np.abs(score - want) / margin).max()))
    assert np.all(np.abs(score - want) <= margin)
    assert "%.17g" % float(summary[3]) == summary[3]
    assert abs(float(summary[3]) - km.get()["objective"]) <= margin.sum()
    return label


def test_clusters_of_every_written_vertex(gpu, tmp_path):
    r = _run(tmp_path, _with(_base(), EVERYTHING, "  clusters: 3"))
    assert sorted(os.listdir(tmp_path / "out")) == sorted(NAME + s for s in (".clusters.tsv", ".dict.tsv", ".vectors.tsv"))
    banner, keys, X, summary, rows = _read(tmp_path)
    line = "Clusters: 3 (cosine, at most 50 iterations)"
    assert "# " + line in banner and line in _log(r.stdout, "Graph Embeddings")
    assert len(keys) >= 6 and {t for _, t in keys} >= {"URI", "LITERAL"}
    label = _check(X, summary, rows, 3, R.COSINE)
    assert len(set(label.tolist())) > 1
    done = _log(r.stdout, "Clusters")
    assert len(done) == 1 and re.fullmatch(r"wrote 3 cosine clusters of %d vertices after %d iterations \((not )?converged\) to out/%s\.clusters\.tsv"
                                           % (len(keys), summary[1], re.escape(NAME)), done[0]), done
    assert "WARN" not in r.stdout


def test_output_filters_metric_and_iterations(gpu, tmp_path):
    # a type filter, Euclid, one iteration
    r = _run(tmp_path / "uris", _with(_base(), "output:\n  uri: []\n", "  clusters: 2\n  clusters_metric: euclid\n  clusters_iterations: 1"))
    banner, keys, X, summary, rows = _read(tmp_path / "uris")
    assert "# Clusters: 2 (euclid, at most 1 iterations)" in banner
    assert len(keys) >= 6 and {t for _, t in keys} == {"URI"}
    _check(X, summary, rows, 2, R.EUCLID, iterations=1)              # positions refer to the filtered dict: X holds its rows only
    assert summary[1] == 1
    # a prefix filter that keeps three vertices: K shrinks to three, with a warning
    r = _run(tmp_path / "authors", _with(_base(), FILTERED, "  clusters: 5"))
    _, keys, X, summary, rows = _read(tmp_path / "authors")
    assert [k for k, _ in keys] == ["http://ex.org/authors/a1", "http://ex.org/authors/a2", "http://ex.org/authors/a3"]
    _check(X, summary, rows, 3, R.COSINE)
    warn = [l for l in r.stdout.splitlines() if " WARN " in l]
    assert len(warn) == 1 and warn[0].endswith(":: only 3 vertices are written: 3 clusters instead of 5")


def test_without_the_key_nothing_changes(gpu, tmp_path):
    base = _base()
    for name, text in (("plain", base), ("again", base), ("zero", _with(base, FILTERED, "  clusters: 0\n  clusters_metric: euclid"))):
        r = _run(tmp_path / name, text)
        assert sorted(os.listdir(tmp_path / name / "out")) == [NAME + ".dict.tsv", NAME + ".vectors.tsv"]
        assert "Clusters" not in r.stdout
    for f in (NAME + ".dict.tsv", NAME + ".vectors.tsv"):
        want = (tmp_path / "plain" / "out" / f).read_bytes()
        assert (tmp_path / "again" / "out" / f).read_bytes() == want == (tmp_path / "zero" / "out" / f).read_bytes()
        assert b"Clusters" not in want


def test_bad_values_are_configuration_errors(gpu, tmp_path):
    base = _base()
    number = "Invalid configuration: Invalid device.clusters, choose a number from 1 to 65536 (0 = off)"
    for extra, message in (("  clusters: 65537", number), ("  clusters: -3", number), ("  clusters: 2.5", number), ("  clusters: many", number),
                           ("  clusters: 3\n  clusters_metric: dot", "Invalid configuration: Invalid device.clusters_metric, choose one of: cosine, euclid"),
                           ("  clusters: 3\n  clusters_iterations: 0", "Invalid configuration: Invalid device.clusters_iterations, choose a number from 1 up"),
                           ("  clusters: 3\n  clusters_iterations: soon", "Invalid configuration: Invalid device.clusters_iterations, choose a number from 1 up")):
        r = _run(tmp_path, _with(base, FILTERED, extra), expect=1)
        assert message in r.stderr
        assert not os.path.exists(tmp_path / "out")

"""`device: { neighbors: K }` through the CLI on tests/golden/tiny.nt: <name>.neighbors.tsv next to the other two files -- same
banner, one line per line of the dict file, positions in that file -- with scores that are the cosines of the written vectors;
the output filters select the candidates; without the key the output directory is what it was."""
import os
import re

import numpy as np
import pytest

import nn_ref as R
from test_cli_gpu import GOLD
from test_pca_cli_gpu import NAME, _log, _run

pytestmark = pytest.mark.gpu
FILTERED = "output:\n  uri: [ http://ex.org/authors/ ]\n"
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
    nbr = (out / (NAME + ".neighbors.tsv")).read_text().splitlines()
    head = dic.index("key\ttype")
    assert nbr[:head] == vec[:head] == dic[:head]                  # the same banner lines
    keys = [l.split("\t") for l in dic[head + 1:]]
    X = np.array([[float(x) for x in l.split("\t")] for l in vec[head:]])
    rows = [l.split("\t") for l in nbr[head:]]
    return dic[:head], keys, X, rows


def _check_rows(X, rows, K, dim=8):
    """Every line against the cosines of the written vectors: 7 significant digits of both rows move a cosine by at most
    2 * 5e-7, on top of the bound B of the scores themselves."""
    n = len(X)
    assert len(rows) == n and all(len(r) == 1 + 2 * K for r in rows)
    assert [int(r[0]) for r in rows] == list(range(n))
    idx = np.array([[int(x) for x in r[1::2]] for r in rows]).reshape(n, K)
    assert all(re.fullmatch(r"-?\d\.\d{6}E[+-]\d{2}", x) for r in rows for x in r[2::2])       # the number format of the vectors file
    score = np.array([[float(x) for x in r[2::2]] for r in rows]).reshape(n, K)
    assert idx.min() >= 0 and idx.max() < n and not np.any(idx == np.arange(n)[:, None])        # no line lists its own position
    assert all(len(set(r)) == K for r in idx.tolist())
    Y = X / np.linalg.norm(X, axis=1, keepdims=True)
    T = Y @ Y.T
    margin = R.bound(dim) + 2 * TEXT
    t = np.take_along_axis(T, idx, axis=1)
    err = np.abs(score - t)
    print("cli neighbours: %d lines, K %d, scores within %.3g of B + 2 * 5e-7" % (n, K, err.max() / margin))
    assert np.all(err <= margin)
    assert np.all(score[:, 1:] <= score[:, :-1])
    U = T.copy()
    U[np.arange(n), np.arange(n)] = -np.inf
    np.put_along_axis(U, idx, -np.inf, axis=1)
    if K < n - 1:
        assert np.all(U.max(axis=1) <= t.min(axis=1) + 2 * margin)     # not beaten, with the doubled margin
    else:
        assert np.all(np.isneginf(U))


def test_neighbors_of_every_written_vertex(gpu, tmp_path):
    everything = "output:\n  uri: []\n  blank: []\n  literal: []\n"
    r = _run(tmp_path, _with(_base(), everything, "  neighbors: 5"))
    assert sorted(os.listdir(tmp_path / "out")) == sorted(NAME + s for s in (".dict.tsv", ".neighbors.tsv", ".vectors.tsv"))
    banner, keys, X, rows = _read(tmp_path)
    assert "# Nearest neighbours: 5 (cosine)" in banner and "Nearest neighbours: 5 (cosine)" in _log(r.stdout, "Graph Embeddings")
    assert len(keys) >= 6 and {t for _, t in keys} >= {"URI", "LITERAL"}
    _check_rows(X, rows, 5)
    assert _log(r.stdout, "Neighbors") == ["wrote 5 cosine neighbours of %d vertices to out/%s.neighbors.tsv" % (len(keys), NAME)]
    assert "WARN" not in r.stdout


def test_output_filters_select_the_candidates(gpu, tmp_path):
    # a type filter: the URIs only
    r = _run(tmp_path / "uris", _with(_base(), "output:\n  uri: []\n", "  neighbors: 5"))
    _, keys, X, rows = _read(tmp_path / "uris")
    assert len(keys) >= 6 and {t for _, t in keys} == {"URI"}
    _check_rows(X, rows, 5)                                         # positions refer to the filtered dict: X holds its rows only
    # a prefix filter that keeps three vertices: K shrinks to two, with a warning
    r = _run(tmp_path / "authors", _with(_base(), FILTERED, "  neighbors: 5\n  neighbors_metric: cosine"))
    _, keys, X, rows = _read(tmp_path / "authors")
    assert [k for k, _ in keys] == ["http://ex.org/authors/a1", "http://ex.org/authors/a2", "http://ex.org/authors/a3"]
    _check_rows(X, rows, 2)
    warn = [l for l in r.stdout.splitlines() if " WARN " in l]
    assert len(warn) == 1 and warn[0].endswith(":: only 3 vertices are written: listing 2 neighbours instead of 5")
    # dot products of the same vectors
    r = _run(tmp_path / "dot", _with(_base(), "output:\n  uri: []\n", "  neighbors: 3\n  neighbors_metric: dot"))
    banner, keys, X, rows = _read(tmp_path / "dot")
    assert "# Nearest neighbours: 3 (dot)" in banner
    idx = np.array([[int(x) for x in row[1::2]] for row in rows])
    score = np.array([[float(x) for x in row[2::2]] for row in rows])
    t = np.take_along_axis(X @ X.T, idx, axis=1)
    scale = np.linalg.norm(X, axis=1)[:, None] * np.linalg.norm(X, axis=1)[idx]
    assert np.all(np.abs(score - t) <= (R.bound(8) + 2 * TEXT) * scale + TEXT * np.abs(t))       # the cosine bound times the two norms, and the score's own text


def test_without_the_key_nothing_changes(gpu, tmp_path):
    base = _base()
    for name, text in (("plain", base), ("again", base), ("zero", _with(base, FILTERED, "  neighbors: 0"))):
        _run(tmp_path / name, text)
        assert sorted(os.listdir(tmp_path / name / "out")) == [NAME + ".dict.tsv", NAME + ".vectors.tsv"]
    for f in (NAME + ".dict.tsv", NAME + ".vectors.tsv"):
        want = (tmp_path / "plain" / "out" / f).read_bytes()
        assert (tmp_path / "again" / "out" / f).read_bytes() == want == (tmp_path / "zero" / "out" / f).read_bytes()
        assert b"Nearest neighbours" not in want


def test_bad_values_are_configuration_errors(gpu, tmp_path):
    base = _base()
    for extra, message in (("  neighbors: 129", "Invalid configuration: Invalid device.neighbors, choose a number from 1 to 128 (0 = off)"),
                           ("  neighbors: -3", "Invalid configuration: Invalid device.neighbors, choose a number from 1 to 128 (0 = off)"),
                           ("  neighbors: 5\n  neighbors_metric: euclid", "Invalid configuration: Invalid device.neighbors_metric, choose one of: cosine, dot")):
        r = _run(tmp_path, _with(base, FILTERED, extra), expect=1)
        assert message in r.stderr
        assert not os.path.exists(tmp_path / "out")

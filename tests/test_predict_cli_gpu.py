"""`device: { predict: K }` through the CLI: tests/golden/tiny.config.yml with the key lists, for every kept vertex, its K best
missing links among the kept vertices -- the columns of its row that the trainer saw and the vertex itself left out -- in
<name>.links.tsv.  Deterministic mode: the tables are the oracle pipeline's, so every listed entry must pass the checks
predict_ref.py derives from them.  Without the key no such file appears and nothing else changes."""
import os

import numpy as np
import pytest

import oracle as O
import predict_ref as P
from geglove import capi
from test_cli_gpu import GOLD, _graph_from_host
from test_pca_cli_gpu import NAME, _run, _files, _log

pytestmark = pytest.mark.gpu
BASE = open(os.path.join(GOLD, "tiny.config.yml")).read()
K = 5


def _with(extra):
    return BASE.replace("  seed: 42", "  seed: 42\n" + extra)


def _oracle_case(fraction=0.0, maxiter=3, tolerance=1e-4):
    """The tables of the oracle pipeline, the kept vertices, and per kept vertex the columns of its row the trainer saw."""
    g, keys, _ = _graph_from_host()
    V = g["V"]
    coo = O.bca_build(V, g["out"], g["inn"], 0.1, 1e-3, True, O.NORM_NONE)
    I, J, X = np.asarray(coo["I"]), np.asarray(coo["J"]), np.asarray(coo["X"], np.float32)
    seen = np.ones(len(I), bool) if fraction == 0 else ~capi.holdout_mask(42, len(I), fraction).astype(bool)
    m = O.Glove(V, 8, I[seen], J[seen], X[seen], coo["max"], O.COST_PGLOVE, seed=42, threads=1)
    prev = 0.0
    for _ in range(maxiter):
        train = m.epoch()
        diff = abs(prev - train)
        prev = train
        if diff <= tolerance:
            break
    state = {k: np.asarray(v, np.float32) for k, v in m.state().items()}
    kept = np.array([i for i, k in enumerate(keys) if k.startswith("http://ex.org/authors/")], np.int32)
    lists = [np.unique(J[seen][I[seen] == i]) for i in kept]
    return V, state["focus"].reshape(V, 8), state["context"].reshape(V, 8), state["cbias"].reshape(V), kept, lists


def _check_links(tmp_path, stdout, extra_banner, fraction):
    V, F, C, cb, kept, lists = _oracle_case(fraction)
    n = len(kept)
    text = (tmp_path / "out" / (NAME + ".links.tsv")).read_text().splitlines()
    vec, dic = _files(tmp_path)
    head = dic.splitlines().index("key\ttype")
    banner = "# Predict: the %d best missing links of every kept vertex, known nonzeros filtered" % K
    assert text[:head] == dic.splitlines()[:head] == vec.splitlines()[:head] and banner in text[:head]
    assert all(b in text[:head] for b in extra_banner)
    body = [l.split("\t") for l in text[head:]]
    assert len(body) == n == len(dic.splitlines()) - head - 1 and n > 1
    assert [int(f[0]) for f in body] == list(range(n))                               # dict positions, dict order
    index = np.full((n, K), -1, np.int32)
    score = np.full((n, K), -np.inf, np.float32)
    count = np.zeros(n, np.int32)
    for k, f in enumerate(body):
        assert len(f) % 2 == 1 and (len(f) - 1) // 2 <= K, f
        count[k] = (len(f) - 1) // 2
        for t in range(count[k]):
            pos, z = int(f[1 + 2 * t]), f[2 + 2 * t]
            assert 0 <= pos < n and z == "%.9g" % np.float32(float(z)), f              # text that parses back to the same float
            index[k, t] = kept[pos]
            score[k, t] = np.float32(float(z))
    keep = P.candidates(n, V, P.csr(lists), kept, kept)
    for k in range(n):                                                               # no filtered column, never the row itself
        got = index[k, :count[k]]
        assert kept[k] not in got and not np.any(np.isin(got, lists[k])) and np.all(np.isin(got, kept))
    t, E = P.bound(F, C, cb, kept)
    model, ok = P.decided(t, E, keep, K)
    print("%d kept vertices, %d candidates in all, %.0f %% of the slots decided" % (n, keep.sum(), 100 * ok.mean()))
    assert keep.sum() > 0, "the fixture leaves no candidate: nothing is listed"
    P.check_within_bound(index, score, count, t, E, keep, model, ok)
    log = _log(stdout, "Predict")
    assert log == ["wrote %d predicted links of %d vertices to out/%s.links.tsv" % (count.sum(), n, NAME)]
    assert banner[2:] in _log(stdout, "Graph Embeddings")


def test_links_file_passes_the_checks_of_the_oracle_pipeline(gpu, tmp_path):
    r = _run(tmp_path, _with("  predict: %d" % K))
    _check_links(tmp_path, r.stdout, [], 0.0)


def test_under_holdout_the_kept_nonzeros_are_the_filter(gpu, tmp_path):
    r = _run(tmp_path, _with("  holdout: 0.1\n  predict: %d" % K))
    _check_links(tmp_path, r.stdout, [], 0.1)


def test_without_the_key_nothing_changes(gpu, tmp_path):
    plain = _run(tmp_path / "plain", BASE)
    off = _run(tmp_path / "off", _with("  predict: 0"))
    on = _run(tmp_path / "on", _with("  predict: %d" % K))
    names = sorted([NAME + ".vectors.tsv", NAME + ".dict.tsv"])
    assert sorted(os.listdir(tmp_path / "plain" / "out")) == sorted(os.listdir(tmp_path / "off" / "out")) == names
    assert sorted(os.listdir(tmp_path / "on" / "out")) == sorted(names + [NAME + ".links.tsv"])
    for name in names:
        assert (tmp_path / "plain" / "out" / name).read_bytes() == (tmp_path / "off" / "out" / name).read_bytes()
    strip = lambda out: [l.split(" :: ", 1)[-1] for l in out.splitlines()]       # the time of day goes
    assert strip(plain.stdout) == strip(off.stdout) and not _log(plain.stdout, "Predict") and "# Predict" not in _files(tmp_path / "plain")[0]
    # the prediction reads: the vectors of the run that predicts are those of the run that does not, banner line apart
    rows = lambda text: [l for l in text.splitlines() if not l.startswith("# Predict: ")]
    assert rows(_files(tmp_path / "on")[0]) == rows(_files(tmp_path / "plain")[0])
    assert rows(_files(tmp_path / "on")[1]) == rows(_files(tmp_path / "plain")[1])


def test_bad_values_are_configuration_errors(gpu, tmp_path):
    for i, bad in enumerate(("129", "-1", "1.5", "many")):
        cwd = tmp_path / ("bad%d" % i)
        r = _run(cwd, _with("  predict: " + bad), expect=1)
        assert "Invalid configuration: Invalid device.predict, choose a number of links to predict per vertex from 1 to 128 (0 = off)" in r.stderr
        assert not os.path.exists(cwd / "out")
    r = _run(tmp_path / "ranks", _with("  predict: 5\n  gpus: 2"), expect=1)
    assert "Invalid configuration: device.predict runs on one rank only, set device.gpus: 1" in r.stderr and not os.path.exists(tmp_path / "ranks" / "out")

"""`device: { holdout: F }` through the CLI: tests/golden/tiny.config.yml with the new key trains on the nonzeros
ge_holdout_mask keeps, evaluates the held-out ones after every epoch and writes <name>.holdout.tsv, whose two cost columns the
oracle pipeline reproduces exactly; without the key (or with 0) the output directory is what it was."""
import os
import re
import subprocess

import numpy as np
import pytest

import oracle as O
import eval_ref as R
from geglove import capi
from test_cli_gpu import EXE, GOLD, _graph_from_host
from test_pca_cli_gpu import NAME, _run, _files, _log

pytestmark = pytest.mark.gpu
BASE = open(os.path.join(GOLD, "tiny.config.yml")).read()


def _with(extra):
    return BASE.replace("  seed: 42", "  seed: 42\n" + extra)


def _oracle_history(fraction, maxiter=3, tolerance=1e-4):
    g, _, _ = _graph_from_host()
    coo = O.bca_build(g["V"], g["out"], g["inn"], 0.1, 1e-3, True, O.NORM_NONE)
    I, J, X = np.asarray(coo["I"]), np.asarray(coo["J"]), np.asarray(coo["X"], np.float32)
    held = capi.holdout_mask(42, len(I), fraction).astype(bool)
    assert 0 < held.sum() < len(I)
    m = O.Glove(g["V"], 8, I[~held], J[~held], X[~held], coo["max"], O.COST_PGLOVE, seed=42, threads=1)     # the FULL matrix's max
    rows, prev = [], 0.0
    for it in range(maxiter):
        train = m.epoch()
        _, term = R.model(m.state(), 8, I[held], J[held], X[held], coo["max"], O.COST_PGLOVE)
        rows.append((it, train, R.partitioned_sum(term) / int(held.sum())))
        diff = abs(prev - train)
        prev = train
        if diff <= tolerance:
            break
    return rows, int(held.sum()), len(I)


def test_holdout_file_reproduces_the_oracle_pipeline(gpu, tmp_path):
    r = _run(tmp_path, _with("  holdout: 0.2"))
    want, n_held, n_all = _oracle_history(0.2)
    text = (tmp_path / "out" / (NAME + ".holdout.tsv")).read_text().splitlines()
    vec, dic = _files(tmp_path)
    head = dic.splitlines().index("key\ttype")
    banner = "# Holdout: 0.2 (%d of %d nonzeros)" % (n_held, n_all)
    assert text[:head] == dic.splitlines()[:head] == vec.splitlines()[:head] and banner in text[:head]
    body = [l.split("\t") for l in text[head:]]
    assert len(body) == len(want) and all(len(f) == 3 for f in body)            # one row per epoch the tolerance stop let run
    for f, (it, train, holdout) in zip(body, want):
        assert int(f[0]) == it
        assert np.float64(float(f[1])).tobytes() == np.float64(train).tobytes(), (it, f[1], train)
        assert np.float64(float(f[2])).tobytes() == np.float64(holdout).tobytes(), (it, f[2], holdout)
        assert f[1] == "%.17g" % train and f[2] == "%.17g" % holdout
    epochs = _log(r.stdout, "Optimizer")
    lines = [l for l in epochs if l.startswith("epoch ")]
    assert len(lines) == len(want)
    for l, (it, train, holdout) in zip(lines, want):
        assert l.startswith("epoch %d  cost %.9g  holdout %.9g  " % (it + 1, train, holdout)), l
    assert banner[2:] in _log(r.stdout, "Graph Embeddings")
    assert _log(r.stdout, "Holdout") == ["wrote %d epochs to out/%s.holdout.tsv" % (len(want), NAME)]


def test_row_count_follows_the_tolerance_stop(gpu, tmp_path):
    """A tolerance no epoch can miss stops after the first epoch: one row; tolerance 0 runs all of maxiter."""
    for tol, label in (("1e9", "stop"), ("0", "all")):
        cwd = tmp_path / label
        _run(cwd, _with("  holdout: 0.2").replace("tolerance: 1e-4", "tolerance: " + tol))
        text = (cwd / "out" / (NAME + ".holdout.tsv")).read_text().splitlines()
        body = [l for l in text if re.match(r"\d+\t", l)]
        want, _, _ = _oracle_history(0.2, tolerance=float(tol))
        assert len(body) == len(want) == (1 if label == "stop" else 3)


def test_without_the_key_nothing_changes(gpu, tmp_path):
    plain = _run(tmp_path / "plain", BASE)
    off = _run(tmp_path / "off", _with("  holdout: 0"))
    assert sorted(os.listdir(tmp_path / "plain" / "out")) == sorted(os.listdir(tmp_path / "off" / "out")) == \
        sorted([NAME + ".vectors.tsv", NAME + ".dict.tsv"])
    assert _files(tmp_path / "plain") == _files(tmp_path / "off")
    strip = lambda out: [l.split(" :: ", 1)[-1] for l in out.splitlines()]       # the time of day goes; a banner line may span two
    assert strip(plain.stdout) == strip(off.stdout) and "holdout" not in plain.stdout.lower()


def test_bad_values_are_configuration_errors(gpu, tmp_path):
    for i, bad in enumerate(("0.6", "-0.1", "0.5000001", "lots")):
        cwd = tmp_path / ("bad%d" % i)
        r = _run(cwd, _with("  holdout: " + bad), expect=1)
        assert "Invalid configuration: Invalid device.holdout, choose a fraction from 0 to 0.5 (0 = off)" in r.stderr
        assert not os.path.exists(cwd / "out")
    r = _run(tmp_path / "ranks", _with("  holdout: 0.2\n  gpus: 2"), expect=1)
    assert "Invalid configuration: device.holdout runs on one rank only" in r.stderr and not os.path.exists(tmp_path / "ranks" / "out")

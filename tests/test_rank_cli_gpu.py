"""`device: { rank: Q }` through the CLI: tests/golden/tiny.config.yml with `holdout: 0.1` and `rank: 50` trains on the kept
nonzeros, ranks the first 50 held-out ones among all columns with the row's kept nonzeros filtered out, and writes
<name>.rank.tsv.  Deterministic mode: the tables are the oracle pipeline's, so every rank must lie in the bracket rank_ref.py
derives from them.  Without the key no such file appears and nothing else changes."""
import os

import numpy as np
import pytest

import oracle as O
import rank_ref as R
from geglove import capi
from test_cli_gpu import GOLD, _graph_from_host
from test_pca_cli_gpu import NAME, _run, _files, _log

pytestmark = pytest.mark.gpu
BASE = open(os.path.join(GOLD, "tiny.config.yml")).read()
Q = 50


def _with(extra):
    return BASE.replace("  seed: 42", "  seed: 42\n" + extra)


def _oracle_case(fraction, maxiter=3, tolerance=1e-4):
    g, _, _ = _graph_from_host()
    V = g["V"]
    coo = O.bca_build(V, g["out"], g["inn"], 0.1, 1e-3, True, O.NORM_NONE)
    I, J, X = np.asarray(coo["I"]), np.asarray(coo["J"]), np.asarray(coo["X"], np.float32)
    held = capi.holdout_mask(42, len(I), fraction).astype(bool)
    m = O.Glove(V, 8, I[~held], J[~held], X[~held], coo["max"], O.COST_PGLOVE, seed=42, threads=1)
    prev = 0.0
    for _ in range(maxiter):
        train = m.epoch()
        diff = abs(prev - train)
        prev = train
        if diff <= tolerance:
            break
    state = {k: np.asarray(v, np.float32) for k, v in m.state().items()}
    n = min(Q, int(held.sum()))
    rI, rJ = I[held][:n], J[held][:n]
    kI, kJ = I[~held], J[~held]
    filters = R.csr([np.unique(kJ[kI == i]) for i in rI])
    return V, state["focus"].reshape(V, 8), state["context"].reshape(V, 8), state["cbias"].reshape(V), rI, rJ, filters, int(held.sum())


def test_rank_file_lies_in_the_bracket_of_the_oracle_pipeline(gpu, tmp_path):
    r = _run(tmp_path, _with("  holdout: 0.1\n  rank: %d" % Q))
    V, F, C, cb, rI, rJ, filters, n_held = _oracle_case(0.1)
    n = len(rI)
    assert n == min(Q, n_held) and n > 0
    text = (tmp_path / "out" / (NAME + ".rank.tsv")).read_text().splitlines()
    vec, dic = _files(tmp_path)
    head = dic.splitlines().index("key\ttype")
    banner = "# Rank: %d held-out nonzeros among all columns, training nonzeros filtered" % Q
    assert text[:head] == dic.splitlines()[:head] == vec.splitlines()[:head] and banner in text[:head]
    top = text[head].split("\t")
    body = [l.split("\t") for l in text[head + 1:]]
    assert len(top) == 6 and len(body) == n and all(len(f) == 4 for f in body)
    assert [int(f[0]) for f in body] == rI.tolist() and [int(f[1]) for f in body] == rJ.tolist()      # the first held-out nonzeros, matrix order
    rank = np.array([int(f[2]) for f in body])
    score = np.array([float(f[3]) for f in body])
    assert all(f[3] == "%.9g" % np.float32(float(f[3])) for f in body)
    lo, hi, tj, Ej = R.bracket(F, C, cb, rI, rJ, filters)
    print("lo == hi for %.0f %% of the %d pairs" % (100 * np.mean(lo == hi), n))
    bad = np.flatnonzero((rank < lo) | (rank > hi))
    assert bad.size == 0, "pair %d: rank %d outside [%d, %d]" % (bad[0], rank[bad[0]], lo[bad[0]], hi[bad[0]])
    assert np.all(np.abs(score - tj) <= Ej)
    want = R.summary(rank)
    assert top[0] == "%.17g" % want["mrr"] and top[1] == "%.17g" % want["mean_rank"]
    assert [int(x) for x in top[2:]] == [want["hits1"], want["hits10"], want["hits100"], n]
    log = _log(r.stdout, "Rank")
    assert len(log) == 1 and log[0].startswith("ranked %d held-out nonzeros: mrr %.6g, " % (n, want["mrr"])) and log[0].endswith("wrote out/%s.rank.tsv" % NAME)
    assert banner[2:] in _log(r.stdout, "Graph Embeddings")


def test_without_the_key_nothing_changes(gpu, tmp_path):
    plain = _run(tmp_path / "plain", _with("  holdout: 0.1"))
    off = _run(tmp_path / "off", _with("  holdout: 0.1\n  rank: 0"))
    on = _run(tmp_path / "on", _with("  holdout: 0.1\n  rank: %d" % Q))
    names = sorted([NAME + ".vectors.tsv", NAME + ".dict.tsv", NAME + ".holdout.tsv"])
    assert sorted(os.listdir(tmp_path / "plain" / "out")) == sorted(os.listdir(tmp_path / "off" / "out")) == names
    assert sorted(os.listdir(tmp_path / "on" / "out")) == sorted(names + [NAME + ".rank.tsv"])
    assert _files(tmp_path / "plain") == _files(tmp_path / "off")
    strip = lambda out: [l.split(" :: ", 1)[-1] for l in out.splitlines()]       # the time of day goes
    assert strip(plain.stdout) == strip(off.stdout) and not _log(plain.stdout, "Rank") and "# Rank" not in _files(tmp_path / "plain")[0]
    # the ranking reads: the vectors of the run that ranks are those of the run that does not, banner line apart
    rows = lambda text: [l for l in text.splitlines() if not l.startswith("# Rank: ")]
    assert rows(_files(tmp_path / "on")[0]) == rows(_files(tmp_path / "plain")[0])


def test_bad_values_are_configuration_errors(gpu, tmp_path):
    for i, bad in enumerate(("-1", "1.5", "lots")):
        cwd = tmp_path / ("bad%d" % i)
        r = _run(cwd, _with("  holdout: 0.1\n  rank: " + bad), expect=1)
        assert "Invalid configuration: Invalid device.rank, choose a number of held-out nonzeros to rank (0 = off)" in r.stderr
        assert not os.path.exists(cwd / "out")
    r = _run(tmp_path / "alone", _with("  rank: 5"), expect=1)
    assert "Invalid configuration: device.rank ranks held-out nonzeros, set device.holdout" in r.stderr and not os.path.exists(tmp_path / "alone" / "out")

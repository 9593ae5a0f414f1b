"""`device: { pca: apply }` through the CLI: tests/golden/tiny.config.yml (which carries `pca: { variance: 0.95 }`, as the
reference's shipped configurations do) with the new key writes the k leading components instead of the dim-wide vectors --
same banner, same headers, same file name -- and the numbers are the numpy PCA of the oracle pipeline's vectors."""
import os
import re
import subprocess

import numpy as np
import pytest

import oracle as O
import pca_ref as R
from test_cli_gpu import EXE, GOLD, _graph_from_host

pytestmark = pytest.mark.gpu
NAME = "tiny_pglove_partial_directed_0.1_0.001_adagrad_pca_8"


def _run(cwd, config_text, expect=0):
    os.makedirs(cwd / "tests" / "golden", exist_ok=True)
    (cwd / "tests" / "golden" / "tiny.nt").write_bytes(open(os.path.join(GOLD, "tiny.nt"), "rb").read())
    (cwd / "run.yml").write_text(config_text)
    r = subprocess.run([EXE, "-c", "run.yml"], cwd=cwd, capture_output=True, text=True, timeout=120)
    assert r.returncode == expect, r.stderr + r.stdout
    return r


def _files(cwd):
    return ((cwd / "out" / (NAME + ".vectors.tsv")).read_text(), (cwd / "out" / (NAME + ".dict.tsv")).read_text())


def _log(stdout, who):
    return [l.split(" :: ", 1)[1] for l in stdout.splitlines() if re.match(r"\d\d:\d\d:\d\d INFO  %s +:: " % re.escape(who), l)]


def _oracle_vectors():
    g, keys, _ = _graph_from_host()
    coo = O.bca_build(g["V"], g["out"], g["inn"], 0.1, 1e-3, True, O.NORM_NONE)
    m = O.Glove(g["V"], 8, coo["I"], coo["J"], coo["X"], coo["max"], O.COST_PGLOVE, seed=42, threads=1)
    m.optimize(3, 1e-4)
    return m.extract(), [i for i, k in enumerate(keys) if k.startswith("http://ex.org/authors/")]


def test_apply_writes_the_leading_components(gpu, tmp_path):
    base = open(os.path.join(GOLD, "tiny.config.yml")).read()
    plain = _run(tmp_path / "plain", base)
    applied = _run(tmp_path / "applied", base.replace("  seed: 42", "  seed: 42\n  pca: apply"))
    vec0, dic0 = _files(tmp_path / "plain")
    vec1, dic1 = _files(tmp_path / "applied")                       # the same file name: _pca_<dim> keeps the configured dim
    assert _log(plain.stdout, "Graph Embeddings") == _log(applied.stdout, "Graph Embeddings")       # banner and prefix line
    assert "# PCA Minimum Variance: 0.95" in vec1.splitlines()
    assert dic1 == dic0
    head = dic1.splitlines().index("key\ttype")
    assert vec1.splitlines()[:head] == vec0.splitlines()[:head] == dic1.splitlines()[:head]
    body = vec1.splitlines()[head:]
    assert len(body) == len(dic1.splitlines()) - head - 1 == 3

    # the yardstick: numpy's PCA of the oracle pipeline's vectors (deterministic mode: the CLI's vectors are those, bit for bit)
    vectors, want = _oracle_vectors()
    X = vectors.astype(np.float32)
    assert np.array_equal(X.astype(np.float64), vectors)
    ref = R.numpy_pca(X, 0.95)
    k, lam = ref["k"], ref["lam"]
    gap = np.min(-np.diff(lam[:k + 1]))
    assert gap / lam[0] >= 1e-3 and k < 8 and R.share_margin(lam, k) >= 1e-4, (lam, k)       # the fixture decides k and its directions
    fields = [l.split("\t") for l in body]
    assert all(len(f) == k for f in fields)
    assert all(re.fullmatch(r"-?\d\.\d{6}E[+-]\d{2}", x) for f in fields for x in f)         # %11.6E
    got = np.array([[float(x) for x in f] for f in fields])
    # |cov - cov_ref| <= the covariance bound entry by entry, so its 2-norm is at most the bound's: the projection bound with that,
    # plus the text's half unit in the seventh digit
    bound = R.transform_bound(ref, ref["cov"] + R.cov_bound(X))[want]
    text = 0.5e-6 * 10.0 ** np.array([[int(x[-3:]) for x in f] for f in fields])
    err = np.abs(got - ref["out"][want])
    print("cli pca: k %d, error at most %.3g of the bound" % (k, np.max(err / (bound + text))))
    assert np.all(err <= bound + text)
    share = lam[:k].sum() / lam.sum()
    assert _log(applied.stdout, "PCA") == ["kept %d of 8 components (%.6f of the variance >= 0.95)" % (k, share)]
    assert _log(plain.stdout, "PCA") == []


def test_apply_without_a_pca_block_is_a_configuration_error(gpu, tmp_path):
    base = open(os.path.join(GOLD, "tiny.config.yml")).read()
    no_block = base.replace("pca:\n  variance: 0.95\n", "").replace("  seed: 42", "  seed: 42\n  pca: apply")
    assert "variance" not in no_block
    r = _run(tmp_path, no_block, expect=1)
    assert "Invalid configuration: device.pca: apply needs a pca block" in r.stderr
    assert not os.path.exists(tmp_path / "out")
    r = _run(tmp_path, base.replace("  seed: 42", "  seed: 42\n  pca: whiten"), expect=1)
    assert "Invalid configuration: Invalid device.pca" in r.stderr


def test_without_the_key_nothing_changes(gpu, tmp_path):
    base = open(os.path.join(GOLD, "tiny.config.yml")).read()
    _run(tmp_path / "plain", base)
    _run(tmp_path / "off", base.replace("  seed: 42", "  seed: 42\n  pca: off"))
    assert _files(tmp_path / "plain") == _files(tmp_path / "off")
    vec, dic = _files(tmp_path / "plain")
    head = dic.splitlines().index("key\ttype")
    vectors, want = _oracle_vectors()
    body = vec.splitlines()[head:]
    assert len(body) == len(want)
    for l, i in zip(body, want):
        assert l.split("\t") == [O.format_11_6E(v) for v in vectors[i]]          # the full dim-wide vectors, byte for byte

"""`device: { foldin: F }` through the CLI: tests/golden/tiny.config.yml with the new key withholds the rows of the vertices
ge_foldin_mask names, trains on the rest, folds the late vertices in after the last epoch and writes <name>.foldin.tsv; the
vectors file carries every vertex, the late ones as (folded focus + trained context) / 2 -- recomputed here through
capi.Folding on an identically trained handle."""
import os
import re

import numpy as np
import pytest

import geglove
import oracle as O
from geglove import capi
from helpers import make_config
from test_cli_gpu import GOLD, _graph_from_host
from test_pca_cli_gpu import _run, _log

pytestmark = pytest.mark.gpu
# every vertex of the graph is written, so the late ones are among them whichever the seed names
BASE = open(os.path.join(GOLD, "tiny.config.yml")).read().replace("  uri: [ http://ex.org/authors/ ]", "  uri: []\n  blank: []\n  literal: []")
assert "  literal: []" in BASE
F, E = 0.2, 7


def _with(extra):
    return BASE.replace("  seed: 42", "  seed: 42\n" + extra)


def _folded_pipeline():
    """The CLI's pipeline in Python: (keys, late vertices, their row lengths, vectors [V, 8] as fp32, cost [late, E])."""
    g, keys, _ = _graph_from_host()
    V = g["V"]
    coo = O.bca_build(V, g["out"], g["inn"], 0.1, 1e-3, True, O.NORM_NONE)
    I, J, X = np.asarray(coo["I"]), np.asarray(coo["J"]), np.asarray(coo["X"], np.float32)
    mask = capi.foldin_mask(42, V, F).astype(bool)
    late = np.flatnonzero(mask)
    assert 0 < len(late) < V
    held = mask[I]
    cfg = make_config(8, "pglove", threads=1, maxiter=3, tolerance=1e-4, mode="deterministic", shuffle="java", seed=42)
    h = geglove.createOptimizer(cfg, geglove.CooMatrix(V, I[~held], J[~held], X[~held], coo["max"]))      # the FULL matrix's max
    try:
        h.optimize()
        lens = np.array([int(np.sum(I == v)) for v in late])
        row_ptr = np.concatenate(([0], np.cumsum(lens))).astype(np.int64)
        idx = np.concatenate([J[I == v] for v in late]).astype(np.int32)              # each row in matrix order
        Xs = np.concatenate([X[I == v] for v in late]).astype(np.float32)
        f = capi.Folding(h._h, row_ptr, idx, Xs, side="focus", epochs=E, shuffle="device", lr=0.0, seed=42)
        try:
            rows, bias, cost, _ = f.run()
        finally:
            f.close()
        state = h.state()
        focus, context = state["focus"].reshape(V, 8).copy(), state["context"].reshape(V, 8)
        focus[late] = rows
        vectors = ((focus + context) / np.float32(2)).astype(np.float32)
    finally:
        h.close()
    return keys, late, lens, vectors, cost


def test_late_vertices_are_folded_in_and_written(gpu, tmp_path):
    r = _run(tmp_path, _with("  foldin: %g\n  foldin_epochs: %d" % (F, E)))
    keys, late, lens, vectors, cost = _folded_pipeline()
    name = re.search(r"Writing files with prefix: (\S+)", r.stdout).group(1)
    vec = (tmp_path / "out" / (name + ".vectors.tsv")).read_text().splitlines()
    dic = (tmp_path / "out" / (name + ".dict.tsv")).read_text().splitlines()
    fold = (tmp_path / "out" / (name + ".foldin.tsv")).read_text().splitlines()
    head = dic.index("key\ttype")
    banner = "# Foldin: %g, %d epochs (%d of %d vertices late)" % (F, E, len(late), len(keys))
    assert fold[:head] == dic[:head] == vec[:head] and banner in fold[:head]
    assert banner[2:] in _log(r.stdout, "Graph Embeddings")
    # the list: exactly the masked vertices, ascending, with their keys, row lengths and first and last costs
    body = [l.split("\t") for l in fold[head:]]
    assert [int(f[0]) for f in body] == late.tolist() and [f[1] for f in body] == [keys[v] for v in late]
    assert [int(f[2]) for f in body] == lens.tolist()
    for f, c in zip(body, cost):
        assert f[3] == "%.9g" % c[0] and f[4] == "%.9g" % c[-1], (f, c)
    assert _log(r.stdout, "Foldin") == ["folded %d late vertices in from %d withheld nonzeros; wrote out/%s.foldin.tsv" % (len(late), lens.sum(), name)]
    # the vectors: every vertex, the late ones with their folded focus rows
    written_keys = [l.split("\t")[0] for l in dic[head + 1:]]
    assert sorted(written_keys) == sorted(keys) and len(vec) - head == len(keys)
    got = {k: l.split("\t") for k, l in zip(written_keys, vec[head:])}
    assert np.any(lens > 0)
    for v in range(len(keys)):
        want = ["%.6E" % x for x in vectors[v].astype(np.float64)]
        assert got[keys[v]] == want, (v, v in late, got[keys[v]], want)


def test_without_the_key_nothing_changes(gpu, tmp_path):
    plain = _run(tmp_path / "plain", BASE)
    off = _run(tmp_path / "off", _with("  foldin: 0"))
    assert sorted(os.listdir(tmp_path / "plain" / "out")) == sorted(os.listdir(tmp_path / "off" / "out"))
    assert not [f for f in os.listdir(tmp_path / "off" / "out") if f.endswith(".foldin.tsv")]
    for f in os.listdir(tmp_path / "plain" / "out"):
        assert (tmp_path / "plain" / "out" / f).read_bytes() == (tmp_path / "off" / "out" / f).read_bytes()
    assert "foldin" not in plain.stdout.lower()


def test_bad_values_are_configuration_errors(gpu, tmp_path):
    for i, bad in enumerate(("0.6", "-0.1", "0.5000001", "some")):
        cwd = tmp_path / ("bad%d" % i)
        r = _run(cwd, _with("  foldin: " + bad), expect=1)
        assert "Invalid configuration: Invalid device.foldin, choose a fraction from 0 to 0.5 (0 = off)" in r.stderr
        assert not os.path.exists(cwd / "out")
    for i, bad in enumerate(("0", "1025", "-3", "2.5")):
        r = _run(tmp_path / ("epochs%d" % i), _with("  foldin: 0.2\n  foldin_epochs: " + bad), expect=1)
        assert "Invalid configuration: Invalid device.foldin_epochs, choose a number from 1 to 1024" in r.stderr
    r = _run(tmp_path / "both", _with("  foldin: 0.2\n  holdout: 0.2"), expect=1)
    assert "Invalid configuration: device.foldin and device.holdout split the matrix differently" in r.stderr
    r = _run(tmp_path / "ranks", _with("  foldin: 0.2\n  gpus: 2"), expect=1)
    assert "Invalid configuration: device.foldin runs on one rank only" in r.stderr and not os.path.exists(tmp_path / "ranks" / "out")

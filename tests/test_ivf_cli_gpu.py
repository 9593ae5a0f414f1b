"""`device: { neighbors_lists: L, neighbors_probes: P, neighbors_iterations: T }` through the CLI on tests/golden/tiny.nt: with
P = L the neighbour lines of <name>.neighbors.tsv are the exact run's, byte for byte; with fewer probes a line lists what its
probed lists hold, a prefix-free subset of the exact order; the banner names L, P and T; without the keys nothing changes; the
bad combinations are configuration errors with their messages."""
import os

import pytest

from test_cli_gpu import GOLD
from test_pca_cli_gpu import NAME, _log, _run

pytestmark = pytest.mark.gpu
FILTERED = "output:\n  uri: [ http://ex.org/authors/ ]\n"
EVERYTHING = "output:\n  uri: []\n  blank: []\n  literal: []\n"


def _base():
    base = open(os.path.join(GOLD, "tiny.config.yml")).read()
    assert FILTERED in base and "  seed: 42" in base
    return base


def _with(base, output, extra):
    return base.replace(FILTERED, output).replace("  seed: 42", "  seed: 42\n" + extra)


def _neighbor_file(cwd):
    """(banner lines, neighbour lines) of <name>.neighbors.tsv; the dict file's banner tells where the lines begin."""
    dic = (cwd / "out" / (NAME + ".dict.tsv")).read_text().splitlines()
    head = dic.index("key\ttype")
    raw = (cwd / "out" / (NAME + ".neighbors.tsv")).read_bytes().split(b"\n")
    assert [l.decode() for l in raw[:head]] == dic[:head]
    return dic[:head], raw[head:]


def test_every_list_probed_gives_the_exact_file(gpu, tmp_path):
    exact = _run(tmp_path / "exact", _with(_base(), EVERYTHING, "  neighbors: 5"))
    banner_e, lines_e = _neighbor_file(tmp_path / "exact")
    n = len(lines_e) - 1
    assert n >= 8
    for name, extra, line in (("ivf", "  neighbors: 5\n  neighbors_lists: 3\n  neighbors_probes: 3\n  neighbors_iterations: 4", "Neighbour lists: 3 (3 probed, at most 4 iterations)"),
                              ("one", "  neighbors: 5\n  neighbors_lists: 1", "Neighbour lists: 1 (1 probed, at most 10 iterations)")):
        r = _run(tmp_path / name, _with(_base(), EVERYTHING, extra))
        banner, lines = _neighbor_file(tmp_path / name)
        assert lines == lines_e, name                                  # byte for byte
        assert "# " + line in banner and "# Nearest neighbours: 5 (cosine)" in banner and [b for b in banner if "Neighbour lists" not in b] == banner_e
        assert line in _log(r.stdout, "Graph Embeddings")
        assert _log(r.stdout, "Neighbors")[0].startswith("wrote 5 cosine neighbours of %d vertices to out/%s.neighbors.tsv from " % (n, NAME))
        for f in (".dict.tsv", ".vectors.tsv"):                        # the other files differ in the banner line only
            a = (tmp_path / name / "out" / (NAME + f)).read_text().splitlines()
            b = (tmp_path / "exact" / "out" / (NAME + f)).read_text().splitlines()
            assert [l for l in a if "Neighbour lists" not in l] == b
    # more lists than vertices are kept: as many lists as vertices, every one probed
    r = _run(tmp_path / "many", _with(_base(), EVERYTHING, "  neighbors: 5\n  neighbors_lists: 4096\n  neighbors_probes: 128\n  neighbors_iterations: 0"))
    if n <= 128:
        assert _neighbor_file(tmp_path / "many")[1] == lines_e


def test_fewer_probes_list_what_the_probed_lists_hold(gpu, tmp_path):
    _run(tmp_path / "exact", _with(_base(), EVERYTHING, "  neighbors: 5"))
    _, lines_e = _neighbor_file(tmp_path / "exact")
    _run(tmp_path / "ivf", _with(_base(), EVERYTHING, "  neighbors: 5\n  neighbors_lists: 4\n  neighbors_probes: 1"))
    banner, lines = _neighbor_file(tmp_path / "ivf")
    assert "# Neighbour lists: 4 (1 probed, at most 10 iterations)" in banner and len(lines) == len(lines_e) and lines[-1] == b""
    for k, (a, e) in enumerate(zip(lines[:-1], lines_e[:-1])):
        a, e = a.split(b"\t"), e.split(b"\t")
        assert a[0] == e[0] == str(k).encode() and len(a) % 2 == 1 and len(a) <= len(e)
        got = list(zip(a[1::2], a[2::2]))
        assert len(set(g[0] for g in got)) == len(got) and str(k).encode() not in [g[0] for g in got]
        scores = [float(s) for _, s in got]
        assert scores == sorted(scores, reverse=True)
        # whatever it lists with a score above the exact run's fifth is in the exact run's line, with the same text
        floor = float(e[-1])
        assert all(g in list(zip(e[1::2], e[2::2])) for g in got if float(g[1]) > floor)


def test_without_the_keys_nothing_changes(gpu, tmp_path):
    """`neighbors_lists: 0` is off: the three files are those of a run without the key, byte for byte.  That the exact path itself
    still writes what it wrote before the key existed -- K pairs on every line, the cosines of the written vectors, the unchanged
    banner and log line -- is what tests/test_nn_cli_gpu.py holds, unchanged, on the same graph; here every line of the exact file
    is also counted: 1 + 2 K fields."""
    base = _base()
    for name, text in (("plain", _with(base, FILTERED, "  neighbors: 2")), ("zero", _with(base, FILTERED, "  neighbors: 2\n  neighbors_lists: 0"))):
        _run(tmp_path / name, text)
    for f in (".dict.tsv", ".vectors.tsv", ".neighbors.tsv"):
        want = (tmp_path / "plain" / "out" / (NAME + f)).read_bytes()
        assert (tmp_path / "zero" / "out" / (NAME + f)).read_bytes() == want and b"Neighbour lists" not in want
    head = (tmp_path / "plain" / "out" / (NAME + ".dict.tsv")).read_text().splitlines().index("key\ttype")
    lines = (tmp_path / "plain" / "out" / (NAME + ".neighbors.tsv")).read_text().splitlines()[head:]
    assert len(lines) == 3 and all(len(l.split("\t")) == 1 + 2 * 2 for l in lines)


def test_bad_combinations_are_configuration_errors(gpu, tmp_path):
    base = _base()
    lists = "Invalid configuration: Invalid device.neighbors_lists, choose a number from 1 to 65536 (0 = off)"
    probes = "Invalid configuration: Invalid device.neighbors_probes, choose a number from 1 to the smaller of device.neighbors_lists and 128"
    iters = "Invalid configuration: Invalid device.neighbors_iterations, choose a number from 0 to 1024"
    for extra, message in (("  neighbors_lists: 4", "Invalid configuration: device.neighbors_lists needs device.neighbors"),
                           ("  neighbors: 3\n  neighbors_metric: dot\n  neighbors_lists: 4", "Invalid configuration: device.neighbors_lists needs device.neighbors_metric: cosine"),
                           ("  neighbors: 3\n  neighbors_probes: 2", "Invalid configuration: device.neighbors_probes and device.neighbors_iterations need device.neighbors_lists"),
                           ("  neighbors: 3\n  neighbors_iterations: 2", "Invalid configuration: device.neighbors_probes and device.neighbors_iterations need device.neighbors_lists"),
                           ("  neighbors: 3\n  neighbors_lists: 65537", lists), ("  neighbors: 3\n  neighbors_lists: -4", lists),
                           ("  neighbors: 3\n  neighbors_lists: four", lists),
                           ("  neighbors: 3\n  neighbors_lists: 4\n  neighbors_probes: 5", probes), ("  neighbors: 3\n  neighbors_lists: 4\n  neighbors_probes: 0", probes),
                           ("  neighbors: 3\n  neighbors_lists: 400\n  neighbors_probes: 129", probes),
                           ("  neighbors: 3\n  neighbors_lists: 4\n  neighbors_iterations: 1025", iters), ("  neighbors: 3\n  neighbors_lists: 4\n  neighbors_iterations: -1", iters)):
        r = _run(tmp_path, _with(base, FILTERED, extra), expect=1)
        assert message in r.stderr, (extra, r.stderr)
        assert not os.path.exists(tmp_path / "out")

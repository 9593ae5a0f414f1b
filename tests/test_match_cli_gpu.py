"""`device: { match: T }` through the CLI on a small bibliographic graph with planted duplicate authors (written by the test):
<name>.matches.tsv and <name>.entities.tsv next to the other two files, their lines held to capi.Matching on the WRITTEN vectors;
without the key the output directory is what it was; an overflow is the documented run-time error.

The written vectors carry seven significant digits (relative error e <= 5e-7 per component), so the stage inside the CLI saw
slightly different rows.  A cosine moves by at most 2 e |x||y| / (|x||y|) from the products and 2 e from the two norms, 4 e = 2e-6
in all; the chains' own rounding adds at most (8 + 2) 2^-24 < 6e-7 at dim 8 and the score's text 5e-7: scores are compared
within 4e-6, and T is put in the middle of a gap of the written vectors' scores at least 2e-5 wide, so that the SET of pairs, the
groups and every key are compared exactly."""
import os
import re

import numpy as np
import pytest

from geglove import capi
from test_cli_gpu import GOLD
from test_pca_cli_gpu import _log, _run

pytestmark = pytest.mark.gpu
NAME = "dups"
AUTHORS = 12
SCORE_TOLERANCE, GAP = 4e-6, 2e-5


def _graph():
    """Authors a0 .. a11 write papers p_i and p_(i+1); author d_i is a planted duplicate of a_i: same name, same papers."""
    lines = []
    for i in range(AUTHORS):
        for who in ("a%d" % i, "d%d" % i):
            lines.append('<http://ex.org/authors/%s> <http://xmlns.com/foaf/0.1/name> "Author Number %d" .' % (who, i))
            for p in (i, (i + 1) % AUTHORS):
                lines.append("<http://ex.org/papers/p%d> <http://purl.org/dc/elements/1.1/creator> <http://ex.org/authors/%s> ." % (p, who))
    for p in range(AUTHORS):
        lines.append('<http://ex.org/papers/p%d> <http://purl.org/dc/elements/1.1/title> "Paper %d on things" .' % (p, p))
        lines.append("<http://ex.org/papers/p%d> <http://purl.org/dc/terms/references> <http://ex.org/papers/p%d> ." % (p, (p + 5) % AUTHORS))
    return "\n".join(lines) + "\n"


def _config(extra=""):
    base = open(os.path.join(GOLD, "tiny.config.yml")).read()
    assert "graph: tests/golden/tiny.nt" in base and "output:\n  uri: [ http://ex.org/authors/ ]" in base and "  seed: 42" in base
    base = base.replace("graph: tests/golden/tiny.nt", "graph: dups.nt").replace("output:\n", "output:\n  name: %s\n" % NAME)
    return base.replace("  seed: 42", "  seed: 42\n" + extra if extra else "  seed: 42")


def _go(cwd, extra="", expect=0):
    os.makedirs(cwd, exist_ok=True)
    (cwd / "dups.nt").write_text(_graph())
    return _run(cwd, _config(extra), expect=expect)


def _written(cwd):
    dic = (cwd / "out" / (NAME + ".dict.tsv")).read_text().splitlines()
    vec = (cwd / "out" / (NAME + ".vectors.tsv")).read_text().splitlines()
    head = dic.index("key\ttype")
    keys = [l.split("\t")[0] for l in dic[head + 1:]]
    X = np.array([[float(x) for x in l.split("\t")] for l in vec[head:]], np.float32)
    assert X.shape[0] == len(keys) == 2 * AUTHORS
    return dic[:head], keys, X


def _threshold(X, metric="cosine"):
    """T in the middle of the widest gap among the 5th to 40th best scores of the written vectors."""
    m = capi.Matching.from_rows(X, metric=metric)
    a, b, s, _, _ = m.run(-3.0e38 if metric == "dot" else -2.0)
    assert s.size == X.shape[0] * (X.shape[0] - 1) // 2
    top = np.sort(s.astype(np.float64))[::-1][4:40]
    gaps = top[:-1] - top[1:]
    at = int(np.argmax(gaps))
    assert gaps[at] >= GAP, gaps[at]
    return float(np.float32((top[at] + top[at + 1]) / 2))


def test_matches_and_entities_of_the_written_vertices(gpu, tmp_path):
    plain = _go(tmp_path / "plain")
    banner, keys, X = _written(tmp_path / "plain")
    assert sorted(os.listdir(tmp_path / "plain" / "out")) == [NAME + ".dict.tsv", NAME + ".vectors.tsv"] and "Match" not in plain.stdout
    T = _threshold(X)
    cwd = tmp_path / "match"
    r = _go(cwd, "  match: %r" % T)
    assert sorted(os.listdir(cwd / "out")) == sorted(NAME + s for s in (".dict.tsv", ".entities.tsv", ".matches.tsv", ".vectors.tsv"))
    # without the key the other outputs are what they are with it, but for the banner's line
    for f in (".dict.tsv", ".vectors.tsv"):
        with_key = (cwd / "out" / (NAME + f)).read_text().splitlines()
        assert [l for l in with_key if not l.startswith("# Match: ")] == (tmp_path / "plain" / "out" / (NAME + f)).read_text().splitlines()
        assert sum(l.startswith("# Match: ") for l in with_key) == 1
    banner2, keys2, X2 = _written(cwd)
    assert keys2 == keys and X2.tobytes() == X.tobytes()
    a, b, s, label, summary = capi.Matching.from_rows(X).run(T)
    assert summary["pairs"] >= 5 and summary["groups"] >= 1
    assert np.abs(capi.Matching.from_rows(X).run(-2.0)[2].astype(np.float64) - T).min() >= GAP / 2 - 1e-7       # nothing near T
    matches = (cwd / "out" / (NAME + ".matches.tsv")).read_text().splitlines()
    entities = (cwd / "out" / (NAME + ".entities.tsv")).read_text().splitlines()
    head = len(banner2)
    assert matches[:head] == entities[:head] == banner2 and any(l.startswith("# Match: pairs scoring at least ") for l in banner2)
    rows = [l.split("\t") for l in matches[head:]]
    assert [(r_[0], r_[1]) for r_ in rows] == [(keys[i], keys[j]) for i, j in zip(a.tolist(), b.tolist())]                 # (a, b) order, by key
    assert all(re.fullmatch(r"-?\d\.\d{6}E[+-]\d{2}", r_[2]) for r_ in rows)                                           # the number format of the vectors file
    assert np.abs(np.array([float(r_[2]) for r_ in rows]) - s.astype(np.float64)).max() <= SCORE_TOLERANCE
    want = []
    for root in sorted(set(label.tolist())):
        members = [keys[i] for i in np.flatnonzero(label == root).tolist()]
        if len(members) >= 2:
            want.append("\t".join(members))
    assert entities[head:] == want and len(want) == summary["groups"]
    done = _log(r.stdout, "Match")
    assert len(done) == 1 and done[0].startswith("matched %d cosine pairs scoring at least " % summary["pairs"])
    assert ("%d entities of %d vertices, the largest of %d; wrote out/%s.matches.tsv and out/%s.entities.tsv"
            % (summary["groups"], summary["grouped_rows"], summary["largest"], NAME, NAME)) in done[0]
    # an overflow is a run-time error that names the number found and the key to raise; neither file is written
    cwd = tmp_path / "overflow"
    r = _go(cwd, "  match: %r\n  match_max_pairs: %d" % (T, summary["pairs"] - 1), expect=1)
    assert ("match: %d pairs reach device.match" % summary["pairs"]) in r.stderr and "raise device.match or device.match_max_pairs" in r.stderr
    assert sorted(os.listdir(cwd / "out")) == [NAME + ".dict.tsv", NAME + ".vectors.tsv"]
    # exactly the number found is no overflow
    cwd = tmp_path / "exact"
    _go(cwd, "  match: %r\n  match_max_pairs: %d" % (T, summary["pairs"]))
    assert (cwd / "out" / (NAME + ".matches.tsv")).read_text().splitlines()[head:] == matches[head:]


def test_without_the_key_nothing_changes_and_bad_keys_are_configuration_errors(gpu, tmp_path):
    for name in ("plain", "again"):
        r = _go(tmp_path / name)
        assert sorted(os.listdir(tmp_path / name / "out")) == [NAME + ".dict.tsv", NAME + ".vectors.tsv"] and "Match" not in r.stdout
    for f in (NAME + ".dict.tsv", NAME + ".vectors.tsv"):
        want = (tmp_path / "plain" / "out" / f).read_bytes()
        assert (tmp_path / "again" / "out" / f).read_bytes() == want and b"Match" not in want
    for extra, message in (("  match_metric: dot", "device.match_metric and device.match_max_pairs need device.match"),
                           ("  match_max_pairs: 5", "device.match_metric and device.match_max_pairs need device.match"),
                           ("  match: nan", "Invalid device.match, choose a finite score threshold"),
                           ("  match: 0.5\n  match_metric: euclid", "Invalid device.match_metric, choose one of: cosine, dot"),
                           ("  match: 0.5\n  match_max_pairs: 0", "Invalid device.match_max_pairs, choose a number from 1 to 268435456")):
        r = _go(tmp_path / "bad", extra, expect=1)
        assert "Invalid configuration: " + message in r.stderr
        assert not os.path.exists(tmp_path / "bad" / "out")

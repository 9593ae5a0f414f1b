"""`device: { align: T, align_source: P, align_target: Q }` through the CLI on the planted-duplicates graph of
test_match_cli_gpu.py (authors a*, duplicates d*): <name>.alignment.tsv next to the other two files, its lines held to scores
recomputed with capi.Alignment on the WRITTEN vectors; without the key the output directory is what it was; an empty set and an
overflow are the documented run-time errors.

The written vectors carry seven significant digits, so the stage inside the CLI saw slightly different rows (the bound of
test_match_cli_gpu.py applies: scores within 4e-6) and near-ties may resolve differently: equality with a rerun on the written
vectors is NOT claimed.  T sits in the middle of a gap at least 2e-5 wide of the written vectors' cross scores, so the candidate
SET is the same, and the file is held to what every assignment of that set must satisfy up to the tolerance: right prefixes,
one-to-one, scores of the named pairs, no candidate with both ends free, no candidate ahead of both its ends' pairs by more than
the tolerance, and a `mutual` mark only where each end is the other's best up to the tolerance."""
import os
import re

import numpy as np
import pytest

from geglove import capi
from test_match_cli_gpu import AUTHORS, GAP, NAME, SCORE_TOLERANCE, _go, _written
from test_pca_cli_gpu import _log

pytestmark = pytest.mark.gpu
SOURCE, TARGET = "http://ex.org/authors/a", "http://ex.org/authors/d"
KEYS = "  align_source: %s\n  align_target: %s" % (SOURCE, TARGET)


def _sets(keys):
    source = np.array([i for i, k in enumerate(keys) if k.startswith(SOURCE)], np.int32)
    target = np.array([i for i, k in enumerate(keys) if k.startswith(TARGET)], np.int32)
    assert source.size == target.size == AUTHORS
    return source, target


def _cross_scores(X, source, target):
    """{(source id, target id): score} of every cross pair of the written vectors."""
    a, b, s = capi.Alignment.from_rows(X, source, target).run(-2.0)[:3]
    assert s.size == source.size * target.size
    return {(int(x), int(y)): float(v) for x, y, v in zip(a, b, s)}


def _threshold(cross):
    """T in the middle of the widest gap among the 5th to 40th best cross scores of the written vectors."""
    top = np.sort(np.array(list(cross.values()), np.float64))[::-1][4:40]
    gaps = top[:-1] - top[1:]
    at = int(np.argmax(gaps))
    assert gaps[at] >= GAP, gaps[at]
    return float(np.float32((top[at] + top[at + 1]) / 2))


def test_alignment_of_the_written_vertices(gpu, tmp_path):
    plain = _go(tmp_path / "plain")
    banner, keys, X = _written(tmp_path / "plain")
    assert sorted(os.listdir(tmp_path / "plain" / "out")) == [NAME + ".dict.tsv", NAME + ".vectors.tsv"] and "Align" not in plain.stdout
    source, target = _sets(keys)
    cross = _cross_scores(X, source, target)
    T = _threshold(cross)
    assert min(abs(v - T) for v in cross.values()) >= GAP / 2 - 1e-7                                          # nothing near T
    cwd = tmp_path / "align"
    r = _go(cwd, "  align: %r\n%s" % (T, KEYS))
    assert sorted(os.listdir(cwd / "out")) == sorted(NAME + s for s in (".alignment.tsv", ".dict.tsv", ".vectors.tsv"))
    # without the key the other outputs are what they are with it, but for the banner's line
    for f in (".dict.tsv", ".vectors.tsv"):
        with_key = (cwd / "out" / (NAME + f)).read_text().splitlines()
        assert [l for l in with_key if not l.startswith("# Align: ")] == (tmp_path / "plain" / "out" / (NAME + f)).read_text().splitlines()
        assert sum(l.startswith("# Align: ") for l in with_key) == 1
    banner2, keys2, X2 = _written(cwd)
    assert keys2 == keys and X2.tobytes() == X.tobytes()
    lines = (cwd / "out" / (NAME + ".alignment.tsv")).read_text().splitlines()
    head = len(banner2)
    assert lines[:head] == banner2
    assert ("# Align: %s to %s, pairs scoring at least " % (SOURCE, TARGET)) in "\n".join(banner2) and "(cosine, at most 16777216 pairs)" in "\n".join(banner2)
    rows = [l.split("\t") for l in lines[head:]]
    at = {k: i for i, k in enumerate(keys)}
    candidates = {pair: v for pair, v in cross.items() if v >= T}
    assert len(candidates) >= 5 and len(rows) >= 1 and all(len(r_) == 4 for r_ in rows)
    assert all(r_[0].startswith(SOURCE) and r_[1].startswith(TARGET) and r_[3] in ("0", "1") for r_ in rows)
    assert all(re.fullmatch(r"-?\d\.\d{6}E[+-]\d{2}", r_[2]) for r_ in rows)                                  # the number format of the vectors file
    pairs = [(at[r_[0]], at[r_[1]]) for r_ in rows]
    assert [x for x, _ in pairs] == sorted(x for x, _ in pairs)                                               # ascending source id
    assert len({x for x, _ in pairs}) == len(pairs) == len({y for _, y in pairs})                             # one to one
    assert all(pair in candidates for pair in pairs)
    assert max(abs(float(r_[2]) - cross[pair]) for r_, pair in zip(rows, pairs)) <= SCORE_TOLERANCE
    of_a, of_b = {x: cross[(x, y)] for x, y in pairs}, {y: cross[(x, y)] for x, y in pairs}
    slack = 2 * SCORE_TOLERANCE
    for (x, y), v in candidates.items():
        assert x in of_a or y in of_b, (keys[x], keys[y])                                                      # no candidate with both ends free
        assert not (v > of_a.get(x, -np.inf) + slack and v > of_b.get(y, -np.inf) + slack), (keys[x], keys[y])  # none ahead of both ends' pairs
    for r_, (x, y) in zip(rows, pairs):
        rivals = [v for (p, q), v in candidates.items() if (p == x) != (q == y)]                               # the other candidates of either end
        if r_[3] == "1":
            assert all(cross[(x, y)] >= v - slack for v in rivals), r_                                         # the best of both ends, up to the tolerance
        else:
            assert any(cross[(x, y)] <= v + slack for v in rivals), r_                                         # not clearly the best of both
    mutual = sum(r_[3] == "1" for r_ in rows)
    done = _log(r.stdout, "Align")
    assert done == ["aligned %d of %d %s with %d %s (%d candidates, %d mutual); wrote out/%s.alignment.tsv"
                    % (len(rows), AUTHORS, SOURCE, AUTHORS, TARGET, len(candidates), mutual, NAME)]
    # an overflow is a run-time error that names the number found and the key to raise; no file is written
    cwd = tmp_path / "overflow"
    r = _go(cwd, "  align: %r\n%s\n  align_max_pairs: %d" % (T, KEYS, len(candidates) - 1), expect=1)
    assert ("align: %d pairs reach device.align" % len(candidates)) in r.stderr and "raise device.align or device.align_max_pairs" in r.stderr
    assert sorted(os.listdir(cwd / "out")) == [NAME + ".dict.tsv", NAME + ".vectors.tsv"]
    # exactly the number found is no overflow
    cwd = tmp_path / "exact"
    _go(cwd, "  align: %r\n%s\n  align_max_pairs: %d" % (T, KEYS, len(candidates)))
    assert (cwd / "out" / (NAME + ".alignment.tsv")).read_text().splitlines()[head:] == lines[head:]


def test_an_empty_set_is_a_run_time_error_and_bad_keys_are_configuration_errors(gpu, tmp_path):
    cwd = tmp_path / "empty"
    r = _go(cwd, "  align: 0.5\n  align_source: %s\n  align_target: http://ex.org/nobody/" % SOURCE, expect=1)
    assert "no written vertex has a key that begins with device.align_target: http://ex.org/nobody/" in r.stderr
    assert sorted(os.listdir(cwd / "out")) == [NAME + ".dict.tsv", NAME + ".vectors.tsv"]
    alone = "device.align_source, device.align_target, device.align_metric and device.align_max_pairs need device.align"
    for extra, message in ((KEYS, alone), ("  align_metric: dot", alone),
                           ("  align: 0.5", "device.align needs device.align_source and device.align_target"),
                           ("  align: 0.5\n  align_source: %s\n  align_target: %sbc" % (SOURCE, SOURCE), "device.align_source and device.align_target overlap"),
                           ("  align: nan\n" + KEYS, "Invalid device.align, choose a finite score threshold"),
                           ("  align: 0.5\n%s\n  align_metric: euclid" % KEYS, "Invalid device.align_metric, choose one of: cosine, dot"),
                           ("  align: 0.5\n%s\n  align_max_pairs: 0" % KEYS, "Invalid device.align_max_pairs, choose a number from 1 to 268435456")):
        r = _go(tmp_path / "bad", extra, expect=1)
        assert "Invalid configuration: " + message in r.stderr
        assert not os.path.exists(tmp_path / "bad" / "out")

"""ge_bca_build on graphs designed for the bounds of its LDS kernel and for its re-run paths (tests/bca_ref.py).

Bar: BIT-EXACT against the oracle, as in test_bca_parity_gpu.py -- row_ptr, I, J, X as uint32, max.  What this file adds is
that every case also reads the builder's path report (GE_BCA_TIMING) and holds it to what the walk model predicts: how many
bookmarks k_bca<true> handed to k_bca<false> (more than 512 nodes touched over both passes, or more than 384 at once in the
TreeMap), how many rows were re-run because the pool had no room, how often the global-memory tables grew.  A case whose graph
no longer takes the path it was built for fails, it does not pass by testing something else.

Measured on an MI355X: the 56 cases of this file take 13 s together, none more than 2.3 s (the docstrings of the one-wave tests
have the figures that decided their bookmark ranges).
"""
import functools
import re

import numpy as np
import pytest

import geglove
import oracle as O
import bca_ref as R
from test_bca_parity_gpu import NORMS, _cfg, _check

pytestmark = pytest.mark.gpu

REPORT = re.compile(r"\[ge_bca_build\] rows (\d+): handed over (\d+) \(LDS bounds\), re-run for the pool (\d+), "
                    r"table growths (\d+), tables (lds|global)\n")


def _report(capfd):
    """The path report of the one build since the last call: dict(rows, H, R, G, tables)."""
    found = REPORT.findall(capfd.readouterr().err)
    assert len(found) == 1, found
    n, h, r, g, tables = found[0]
    return dict(rows=int(n), H=int(h), R=int(r), G=int(g), tables=tables)


@functools.lru_cache(maxsize=None)
def _design(name):
    return R.design(name)


@functools.lru_cache(maxsize=None)
def _composite():
    return R.composite()


@functools.lru_cache(maxsize=None)
def _oracle(key, directed, normalize):
    g, eps = (_composite()[0], R.COMPOSITE_EPS) if key == "composite" else _design(key)[:2]
    return O.bca_build(g["V"], g["out"], g["inn"], R.ALPHA, eps, directed, NORMS[normalize])


@functools.lru_cache(maxsize=None)
def _paths(key, directed):
    """Per bookmark: (size of the un-normalised row, handed over by the LDS kernel?).  A walk touches every node of its row and no
    other, so the oracle's row size IS the touched count; the TreeMap never holds more nodes than the walk touches, so only the
    bookmarks with more than 384 entries need the model's peak."""
    g, eps = (_composite()[0], R.COMPOSITE_EPS) if key == "composite" else _design(key)[:2]
    n = np.diff(_oracle(key, directed, "none")["row_ptr"])
    big = n > R.LDS_MAX
    for b in np.nonzero((n > R.LDS_AC) & ~big)[0]:
        s = R.stats(g, int(b), R.ALPHA, eps, directed)
        assert s["union"] == n[b]
        big[b] = R.handed_over(s)
    return n, big


def _default_pool(n_rows):
    """Entries of the first pool when nothing is configured and the build is too small to be sampled (ge_bca_build)."""
    return max(128 * n_rows, 1 << 16)


def _same_bytes(a, b):
    np.testing.assert_array_equal(a.row_ptr, b.row_ptr)
    np.testing.assert_array_equal(a.I, b.I)
    np.testing.assert_array_equal(a.J, b.J)
    np.testing.assert_array_equal(a.X.view(np.uint32), b.X.view(np.uint32))
    assert a.max() == b.max()


# ---- each design alone ----------------------------------------------------------------------------------------------------------
# what the issue states for the roots, held as literals beside the model's count: bookmarks handed over, directed / undirected
# (undirected, every leaf of the 385-leaf star walks to the root and from there to all 385 leaves: 386 bookmarks leave)
H_LITERAL = {"comb511": (0, 0), "comb512": (0, 0), "comb513": (1, 1), "star383": (0, 0), "star384": (0, 0), "star385": (1, 386),
             "split511": (0, None), "split512": (0, None), "split513": (1, None), "comb1241": (1, 1), "tree512": (0, 0), "tree513": (1, 1),
             "star64": (0, 0), "star65": (0, 0), "star128": (0, 0), "holes128": (0, 0), "bowtie70": (0, 0)}


@pytest.mark.parametrize("directed", [True, False])
@pytest.mark.parametrize("name", sorted(R.DESIGNS))
def test_design_alone(gpu, monkeypatch, capfd, name, directed):
    """Default path, none / unity / counts, each built twice -- without and with the report -- and both held to the oracle."""
    g, eps, _ = _design(name)
    n, big = _paths(name, directed)
    want_h, want_g = int(big.sum()), int(n.max() > 1024)          # the global-memory tables start at 2 048 slots = 1 024 nodes
    lit = H_LITERAL[name][0 if directed else 1]
    if lit is not None:
        assert want_h == lit
    assert want_g == (name == "comb1241")
    for normalize in ("none", "unity", "counts"):
        monkeypatch.delenv("GE_BCA_TIMING", raising=False)
        quiet = _check(g, epsilon=eps, directed=directed, normalize=normalize)
        assert "[ge_bca_build]" not in capfd.readouterr().err
        monkeypatch.setenv("GE_BCA_TIMING", "1")
        loud = _check(g, epsilon=eps, directed=directed, normalize=normalize)
        rep = _report(capfd)
        r = rep.pop("R")                 # which rows a full pool refuses depends on the order the wavefronts reach it; whether any, not
        assert rep == dict(rows=g["V"], H=want_h, G=want_g, tables="lds"), (name, directed, normalize, rep)
        assert (r > 0) == (n[~big].sum() > _default_pool(g["V"]))
        _same_bytes(quiet, loud)


# ---- the composite --------------------------------------------------------------------------------------------------------------
def _check_low(directed, normalize, device=None, row_range=None):
    """The composite's bookmarks [0, n_low) (or row_range) on the device against the same rows of the oracle's full build."""
    g, n_low, _ = _composite()
    rb, re_ = row_range or (0, n_low)
    dev = geglove.BookmarkColoring(g, _cfg(R.ALPHA, R.COMPOSITE_EPS, directed, normalize, device), row_range=(rb, re_))
    ref = _oracle("composite", directed, normalize)
    rp = ref["row_ptr"]
    lo, hi = int(rp[rb]), int(rp[re_])
    want_ptr = np.clip(rp, lo, hi) - lo
    np.testing.assert_array_equal(dev.row_ptr, want_ptr)
    assert dev.coOccurrenceCount() == hi - lo
    np.testing.assert_array_equal(dev.I, ref["I"][lo:hi])
    np.testing.assert_array_equal(dev.J, ref["J"][lo:hi])
    assert np.array_equal(dev.X.view(np.uint32), ref["X"][lo:hi].view(np.uint32)), "paint values differ"
    # BookmarkColoring.setMax over the bookmarks of the range: Math.max(0, bcv.max()), an empty row giving 1
    sizes = np.diff(rp[rb:re_ + 1])
    assert sizes.min() > 0
    assert dev.max() == max(0.0, float(ref["X"][lo:hi].max()))
    return dev


def _refused(n, big, cap):
    """One wavefront, bookmarks in ascending order: every row the LDS kernel keeps takes its un-normalised size from the pool counter,
    whether it fits or not, so from the first row that does not fit onward every row is refused."""
    used = 0
    kept = np.nonzero(~big)[0]
    for i, b in enumerate(kept):
        if used + n[b] > cap:
            return len(kept) - i
        used += n[b]
    return 0


def _windows(directed):
    """The bookmark ranges of the one-wave runs.  Directed: all of [0, n_low) in one build.  Undirected, where every leaf of a star
    walks to its root and on to all the other leaves (386 handed-over rows of 770 pops each for the 385 star alone), the whole range
    took 21 s under one wavefront and 37 s with half a pool: instead one window per design -- the last 8 vertices of the design
    before it, the path between them, the root and the 11 vertices behind it -- so that every root still runs on tables that a
    known kind of row has just used: the 512 comb after handed-over star leaves, the 512 split after the 513 split's handed-over
    in-neighbours, the 1241 comb (the growth) after rows at the bound, the full tree row after plain comb leaves."""
    g, n_low, roots = _composite()
    if directed:
        return [(0, n_low)]
    return [(max(0, r - 11), r + 12) for r in roots.values()]


@pytest.mark.parametrize("pool", ["default", "half"])
@pytest.mark.parametrize("normalize", ["none", "unity"])
@pytest.mark.parametrize("directed", [True, False])
def test_composite_under_one_wave(gpu, monkeypatch, capfd, directed, normalize, pool):
    """One wavefront runs 513 comb, 385 star, 512 comb, 384 star, 513 split, 512 split, 1241 comb and the full tree row in this
    order on one set of tables: a row at a bound follows a handed-over row, an exact replay follows ranking, and with half a pool
    the one second launch carries the big rows AND the refused rows and grows its tables once, for the 1241 comb.
    H, R and G of every build are the model's.  Measured on an MI355X: directed, all 4 583 bookmarks in one build, 0.2 - 0.3 s on
    the default pool and 0.55 - 0.6 s with half a pool; undirected, the eight windows of _windows() together, 1.2 s (1.6 - 2.3 s for
    the case that also computes the oracle's build and the model's peaks, once per session)."""
    g, n_low, roots = _composite()
    n_all, big_all = _paths("composite", directed)
    assert all(big_all[roots[k]] for k in ("comb513", "star385", "split513", "comb1241"))
    assert not any(big_all[roots[k]] for k in ("comb512", "star384", "split512", "tree512"))
    monkeypatch.setenv("GE_BCA_WAVES", "1")
    monkeypatch.setenv("GE_BCA_TIMING", "1")
    grown = 0
    for rb, re_ in _windows(directed):
        n, big = n_all[rb:re_], big_all[rb:re_]
        device, cap = None, _default_pool(re_ - rb)
        if pool == "half":
            cap = int(n[~big].sum()) // 2                      # half of what reaches the pool: handed-over rows do not
            device = {"bca_pool_entries": cap}
            assert cap >= 64                                   # (the smallest pool the builder accepts)
        want_r = _refused(n, big, cap)
        if pool == "half":
            assert 0 < want_r < len(n)
        want_g = int(n.max() > 1024)
        if want_g:
            assert big.sum() >= 1 and (pool == "default" or want_r > 0)     # the launch that grows carries big rows, and refused ones
        grown += want_g
        capfd.readouterr()
        _check_low(directed, normalize, device, (rb, re_))
        rep = _report(capfd)
        assert rep == dict(rows=re_ - rb, H=int(big.sum()), R=want_r, G=want_g, tables="lds"), ((rb, re_), rep)
    assert grown == 1


@pytest.mark.parametrize("normalize", ["none", "unity"])
@pytest.mark.parametrize("directed", [True, False])
def test_composite_default_waves(gpu, monkeypatch, capfd, directed, normalize):
    """The same rows with the wavefronts the builder chooses: same bytes, same hand-overs, one growth."""
    g, n_low, _ = _composite()
    n, big = _paths("composite", directed)
    monkeypatch.setenv("GE_BCA_TIMING", "1")
    capfd.readouterr()
    _check_low(directed, normalize)
    rep = _report(capfd)
    r = rep.pop("R")
    assert rep == dict(rows=n_low, H=int(big[:n_low].sum()), G=1, tables="lds"), rep
    assert (r > 0) == (n[:n_low][~big[:n_low]].sum() > _default_pool(n_low))


@pytest.mark.parametrize("pool", ["default", "half"])
@pytest.mark.parametrize("normalize", ["none", "unity"])
@pytest.mark.parametrize("directed", [True, False])
def test_composite_global_tables(gpu, monkeypatch, capfd, directed, normalize, pool):
    """GE_BCA_TABLES=global: k_bca<false> runs every bookmark; its tables grow once in the main loop, for the 1241 comb.  With half
    a pool one launch reports a table overflow AND refused rows: the overflow must win (grow, run again), or the 1241 comb's row
    -- which never reached the pool -- stays empty."""
    g, n_low, _ = _composite()
    n = _paths("composite", directed)[0][:n_low]
    monkeypatch.setenv("GE_BCA_TABLES", "global")
    monkeypatch.setenv("GE_BCA_TIMING", "1")
    capfd.readouterr()
    _check_low(directed, normalize, {"bca_pool_entries": int(n.sum()) // 2} if pool == "half" else None)
    rep = _report(capfd)
    assert (rep["rows"], rep["H"], rep["G"], rep["tables"]) == (n_low, 0, 1, "global"), rep
    assert (rep["R"] > 0) == (n.sum() > (int(n.sum()) // 2 if pool == "half" else _default_pool(n_low)))


@pytest.mark.parametrize("directed", [True, False])
def test_composite_split_by_row_range(gpu, monkeypatch, directed):
    """Two shards, cut inside the 384 star, concatenate to the whole."""
    g, n_low, roots = _composite()
    cut = roots["star384"] + 100
    full = _check_low(directed, "none")
    a = _check_low(directed, "none", row_range=(0, cut))
    b = _check_low(directed, "none", row_range=(cut, n_low))
    np.testing.assert_array_equal(np.concatenate([a.I, b.I]), full.I)
    np.testing.assert_array_equal(np.concatenate([a.J, b.J]), full.J)
    np.testing.assert_array_equal(np.concatenate([a.X, b.X]).view(np.uint32), full.X.view(np.uint32))
    assert max(a.max(), b.max()) == full.max()

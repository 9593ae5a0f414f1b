"""The walk model of tests/bca_ref.py against the oracle, and every designed graph against the bound it was built for (CPU only).

Nothing here tests the device kernel.  It pins the two things tests/test_bca_designed_gpu.py leans on: that the model's
key -> value maps are the oracle's rows bit for bit (so its touched / peak counts describe the walk the oracle and the kernel
perform), and that each design still lands where it was designed to land -- a design that drifts off its bound fails here
instead of quietly testing nothing on the device.
"""
import numpy as np
import pytest

import oracle as O
import bca_ref as R
from geglove import synth


def _oracle_rows(g, eps, directed, normalize=O.NORM_NONE, alpha=R.ALPHA):
    ref = O.bca_build(g["V"], g["out"], g["inn"], alpha, eps, directed, normalize)
    return ref, ref["row_ptr"]


def _assert_model_equals_oracle(g, eps, directed, alpha=R.ALPHA, rows=None):
    ref, rp = _oracle_rows(g, eps, directed, alpha=alpha)
    bad = 0
    for b in (range(g["V"]) if rows is None else rows):
        J = ref["J"][rp[b]:rp[b + 1]].tolist(); X = ref["X"][rp[b]:rp[b + 1]].view(np.uint32).tolist()
        want = R.row(g, b, alpha, eps, directed)
        got = dict(zip(J, X))
        assert len(got) == len(J)
        bad += got != {k: int(np.float32(v).view(np.uint32)) for k, v in want.items()}
    assert bad == 0, "%d rows differ from the oracle" % bad


@pytest.mark.parametrize("directed", [True, False])
def test_model_equals_oracle_on_a_random_graph(directed):
    g = synth.synthetic_graph(300, 4.0, seed=9, weights=(1.0, 2.0, 0.5))
    _assert_model_equals_oracle(g, R.EPS, directed)


@pytest.mark.parametrize("directed", [True, False])
@pytest.mark.parametrize("name", sorted(R.DESIGNS))
def test_model_equals_oracle_on_every_design(name, directed):
    g, eps, _ = R.design(name)
    _assert_model_equals_oracle(g, eps, directed)


@pytest.mark.parametrize("directed", [True, False])
def test_model_equals_oracle_on_the_composite(directed):
    g, n_low, _ = R.composite()
    _assert_model_equals_oracle(g, R.COMPOSITE_EPS, directed)


@pytest.mark.parametrize("name", sorted(R.DESIGNS))
def test_design_lands_on_its_bound(name):
    g, eps, expect = R.design(name)
    for directed, want in expect.items():
        s = R.stats(g, 0, R.ALPHA, eps, directed)
        assert {k: s[k] for k in want} == want, (name, directed, s)
        ref, rp = _oracle_rows(g, eps, directed)
        assert rp[1] - rp[0] == want["row"]                       # the oracle's row has the size the model counts
    assert set(expect) >= {True}


def test_designs_straddle_the_lds_bounds():
    """The hand-over rule of k_bca<true> applied to the model's counts: 511 / 512 / 384 stay, 513 / 385 leave."""
    leave = {n for n in R.DESIGNS if R.handed_over(R.stats(R.design(n)[0], 0, R.ALPHA, R.design(n)[1], True))}
    assert leave == {"comb513", "star385", "split513", "comb1241", "tree513"}
    leave_u = {n for n in R.DESIGNS if False in R.DESIGNS[n][2]
               and R.handed_over(R.stats(R.design(n)[0], 0, R.ALPHA, R.design(n)[1], False))}
    assert leave_u == {"comb513", "star385", "comb1241", "tree513"}


@pytest.mark.parametrize("directed", [True, False])
def test_composite_keeps_every_design_on_its_bound(directed):
    """In the composite (one epsilon, 1e-4, for all) each design's root touches what it touches alone and stays on its side of both bounds."""
    g, n_low, roots = R.composite()
    assert list(roots) == R.COMPOSITE_ORDER and n_low <= 5000 and g["V"] <= 30000
    for name, root in roots.items():
        alone_g, alone_eps, expect = R.design(name)
        if directed not in expect:
            continue
        s = R.stats(g, root, R.ALPHA, R.COMPOSITE_EPS, directed)
        assert (s["union"], s["row"]) == (expect[directed]["union"], expect[directed]["row"]), (name, s)
        assert R.handed_over(s) == R.handed_over(expect[directed]), (name, s)
        if name.startswith("star"):
            assert s["peak"] == expect[directed]["peak"]
    # the far leaves are above the consecutive region, and nothing else is
    idx = np.concatenate([g["out"][1], g["inn"][1]])
    assert sorted(set(idx[idx >= n_low].tolist())) == [R.TREE_STRIDE * k for k in range(3, 15)]


@pytest.mark.parametrize("normalize", [O.NORM_NONE, O.NORM_UNITY])
@pytest.mark.parametrize("directed", [True, False])
@pytest.mark.parametrize("name", ["tree512", "tree513"])
def test_tree_rows_differ_from_the_plain_order(name, directed, normalize):
    """Nine or more keys in bin 0 from table length 64 on: the oracle's row is not the (bin, put sequence) order that ranking gives,
    so the kernel can only match it through its exact replay -- at 512 entries, with every LDS view of the emission full."""
    g, eps, _ = R.design(name)
    ref, rp = _oracle_rows(g, eps, directed, normalize)
    got = ref["J"][rp[0]:rp[1]].tolist()
    # the reverse pass from the root finds no in-neighbour: the merged map is the forward map, key for key
    plain = R.plain_order(R.walk(g, 0, R.ALPHA, eps, 0 if directed else 2)[2])
    if normalize != O.NORM_NONE:
        plain.remove(0)
    assert sorted(got) == sorted(plain)
    assert got != plain
    far = [k for k in got if k % R.TREE_STRIDE == 0 and k]
    assert len(far) == (12 if name == "tree512" else 13)

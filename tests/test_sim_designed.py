"""The designed label families of tests/sim_ref.py hold what they are for, so that a green run of
tests/test_sim_designed_gpu.py means something.  CPU only: the oracle and the Python models.  Conditions, not
measurements."""
import functools

import numpy as np
import pytest

import oracle as O
import sim_ref as R


@functools.lru_cache(maxsize=None)
def jaro_details(L):
    """The Python model's details of every pair i < j of jw_sparse(L): 465 pairs at every L, under a second each L."""
    labs = [R.units(s) for s in R.jw_sparse(L)]
    return {(i, j): R.py_jaro_winkler(labs[i], labs[j], details=True) for i in range(len(labs)) for j in range(i + 1, len(labs))}


@pytest.mark.parametrize("L", R.LENGTH_CLASSES)
def test_jw_sparse_reaches_every_mask_word_the_window_edges_and_the_transposition_walk(L):
    labels = R.jw_sparse(L); ix = R.jw_sparse_index(L); det = jaro_details(L)
    assert len(labels) <= 48 and max(len(R.units(s)) for s in labels) == L
    assert sum(d.last_min >= 32 and d.last_max >= 32 for d in det.values()) >= 20
    assert sum(d.transpositions >= 4 for d in det.values()) >= 10
    if L == 1024:
        assert sum(d.last_min >= 992 and d.last_max >= 992 for d in det.values()) >= 20          # the last of the 32 words
    # the c = 32 exchange has matches on both sides of position 32 in both strings.  Its partner is the base; at
    # L = 64 a shift by 32 leaves the window of 31, so there it is the c = 31 exchange (units one position apart)
    pair = (ix["base"], ix["swap32"]) if L > 64 else (ix["swap31"], ix["swap32"])
    d = det[pair]
    matched_min = [mi for mi, xi in enumerate(d.idx) if xi != -1]; matched_max = [xi for xi in d.idx if xi != -1]
    assert min(matched_min) < 32 <= max(matched_min) and min(matched_max) < 32 <= max(matched_max)
    assert L == 64 or d.transpositions == 64                           # every exchanged unit, across the word boundary
    # a unit at distance exactly `range` matches, one at `range + 1` does not
    rng = L // 2 - 1
    base = R.units(labels[0])
    at_range = det[(0, ix["rot%d" % rng])]
    assert any(xi != -1 and abs(mi - xi) == rng for mi, xi in enumerate(at_range.idx))
    rot = R.units(labels[ix["rot%d" % (rng + 1)]])
    beyond = det[(0, ix["rot%d" % (rng + 1)])]
    assert any(abs(mi - rot.index(c)) == rng + 1 and beyond.idx[mi] == -1 for mi, c in enumerate(base))
    assert not any(xi != -1 and abs(mi - xi) > rng for d in det.values() for mi, xi in enumerate(d.idx))
    # a flagged candidate is skipped and the search runs on: some unit is matched past an equal, earlier one in its window
    rnd = [k for name, k in ix.items() if name.startswith("random")]
    skipped = 0
    for i in rnd:
        for j in rnd:
            if i < j:
                a, b = R.units(labels[i]), R.units(labels[j])
                mx, mn = (a, b) if len(a) > len(b) else (b, a)
                r = max(len(mx) // 2 - 1, 0)
                skipped += any(xi != -1 and c in mx[max(mi - r, 0):xi] for (mi, c), xi in zip(enumerate(mn), det[(i, j)].idx))
    assert skipped >= 10


@pytest.mark.parametrize("L", R.LENGTH_CLASSES)
def test_oracle_equals_the_python_jaro_winkler_on_jw_sparse(L):
    """Every pair i < j at every L: 465 of 465 (the model looks candidates up by unit, which keeps 1024 units cheap)."""
    tab = R.table("jw_sparse%d" % L, "jarowinkler"); det = jaro_details(L)
    assert len(det) == 465
    for (i, j), d in det.items():
        assert tab.sim[i, j] == d.value, (i, j)


def test_jw_gate_sits_on_the_gate_and_on_the_length_bound():
    labels = R.jw_gate(); info = R.jw_gate_info(); tab = R.table("jw_gate", "jarowinkler")
    seven = float(np.float32(0.7))
    jaro = [v for _, _, v in info["gate"]]
    assert seven in jaro and seven < 0.7
    assert any(0.7 < v < 0.7 + 1e-6 for v in jaro) and any(0.7 - 1e-6 < v <= 0.7 for v in jaro)
    assert sum(v > 0.7 for v in jaro) >= 3 and sum(v < seven for v in jaro) >= 3
    for i, j, v in info["gate"]:
        d = R.py_jaro_winkler(R.units(labels[i]), R.units(labels[j]), details=True)
        assert d.jaro == v and tab.sim[i, j] == d.value
        assert (d.value > d.jaro) == (v > 0.7)                     # the boost is visible exactly above the gate
    one_ten = info["gate"][-1]
    assert (labels[one_ten[0]], labels[one_ten[1]]) == ("a", "a" + "b" * 9) and tab.sim[one_ten[0], one_ten[1]] == seven
    # prefix pairs: the reference value against the kernel's double bound, whose margin is 1e-6
    over = [tab.sim[i, j] - R.jw_length_bound(len(R.units(labels[i])), len(R.units(labels[j]))) for i, j in info["prefix"]]
    assert len(over) > 300
    assert max(over) < 1e-6                                        # 6.6e-8 here
    assert max(over) > 0 and sum(abs(x) < 1e-7 for x in over) >= 10
    for i, j in info["prefix"]:
        assert labels[j].startswith(labels[i]) and tab.sim[i, j] == R.py_jaro_winkler(R.units(labels[i]), R.units(labels[j]))


@pytest.mark.parametrize("L", R.LENGTH_CLASSES)
def test_lev_edges_distances_are_the_designed_ones(L):
    labels = R.lev_edges(L); cases = R.lev_edges_cases(L); tab = R.table("lev_edges%d" % L, "levenshtein")
    assert L == 64 or len(labels) <= 48
    assert {m for m, *_ in cases} == {1, 2, 7, 8, 10, 63, 64, L}
    assert {p for *_, p in cases} >= {"end", "start", "spread", "cut"}
    assert "" in labels
    lib = O.lib()
    for m, d, b, p, place in cases:
        x, y = O.utf16(labels[b]), O.utf16(labels[p])
        y_ = y if len(y) else np.zeros(1, np.uint16)
        assert len(x) == m and len(x) - len(y) == (d if place == "cut" else 0)
        assert lib.geo_sim_levenshtein_distance(O._p(x, O.C.c_uint16), len(x), O._p(y_, O.C.c_uint16), len(y)) == d, (m, d, place)
        if m <= 64 or place in ("end", "cut") and d in (1, m):      # the Python DP takes 0.5 s per 1024 x 1024 pair
            assert R.py_levenshtein(list(x), list(y)) == d
        assert tab.sim[min(b, p), max(b, p)] == 1.0 - d / m
    if L == 64:
        assert {(m, d) for m, d, *_ in cases} >= {(10, 1), (10, 5), (10, 9), (10, 10), (63, 31), (64, 32), (64, 63), (7, 3), (2, 1), (1, 1)}


FILTER_CASES = [("jw_sparse64", "jarowinkler", 3, 0.67), ("jw_sparse256", "jarowinkler", 3, 0.5), ("jw_sparse1024", "jarowinkler", 3, 0.9),
                ("jw_sparse64", "levenshtein", 3, 0.5), ("jw_sparse256", "levenshtein", 3, 0.05),
                ("jw_gate", "jarowinkler", 3, float(np.float32(0.7))), ("lev_edges64", "levenshtein", 3, 0.8), ("lev_edges256", "levenshtein", 3, 0.5),
                ("lev_edges1024", "levenshtein", 3, 0.7), ("profile_edges", "ngram_cosine", 1, 0.5), ("profile_edges", "ngram_cosine", 4, 0.0),
                ("profile_edges", "ngram_jaccard", 2, 0.25), ("profile_edges", "ngram_jaccard", 3, -1.0), ("profile_edges", "token_cosine", 3, 0.5),
                ("profile_edges", "token_jaccard", 3, 0.0)]


@pytest.mark.parametrize("name,method,ngram,threshold", FILTER_CASES)
def test_the_filtered_table_is_the_oracles_compare_group(name, method, ngram, threshold):
    tab = R.table(name, method, ngram)
    for form, src, tgt, upper in R.splits(len(tab.labels)):
        ref = O.compare_group(O.sim_cfg(method, threshold, ngram=ngram), tab.labels, src, tgt, upper_triangle=upper)
        exp = R.expected(tab, threshold, src, tgt, upper=upper)
        assert len(ref[0]) > 0
        for a, b in zip(exp, ref):
            np.testing.assert_array_equal(a.view(np.uint32) if a.dtype == np.float32 else a, b.view(np.uint32) if b.dtype == np.float32 else b, err_msg=form)


def test_profile_edges_hold_their_edges():
    labels = list(R.profile_edges())
    assert len(R.py_ngrams(labels[0], 1)) == 1024 and len(R.units(labels[0])) == 1024
    p = R.py_ngrams(labels[1], 1)
    assert len(p) == 1023 and sorted(p.values())[-2:] == [1, 2]
    assert not set(R.py_ngrams("abcdef", 2)) & set(R.py_ngrams("uvwxyz", 2))
    assert "ab  cd" != "ab \t cd" and R.py_ngrams("ab  cd", 2) == R.py_ngrams("ab \t cd", 2)
    assert len("a    b") == 6 and R.py_ngrams("a    b", 4) == {} and len(R.py_ngrams("a    b", 3)) == 1
    assert np.isnan(R.table("profile_edges", "ngram_cosine", 4).sim[labels.index("a    b"), labels.index("abcdefabc")])     # raw length passes the guard
    assert R.table("profile_edges", "ngram_cosine", 4).sim[labels.index("abc"), labels.index("abcdefabc")] == 0.0          # the guard itself
    assert np.isnan(R.table("profile_edges", "ngram_jaccard", 3).sim[labels.index("a"), labels.index("ab")])
    assert R.py_tokens("the of and") == {} and R.py_tokens("x y z q") == {}
    assert R.py_tokens("graph embedding") == R.py_tokens("graph embedding ") == R.py_tokens("graph embedding  ")
    assert R.py_tokens("graph x") == {tuple(map(ord, "graph")): 1}
    assert tuple(map(ord, "deep\tlearning")) in R.py_tokens("deep\tlearning graph")
    # the oracle's profiles are the models'
    for method, ngram, model in (("ngram_jaccard", 2, R.py_jaccard), ("ngram_cosine", 1, R.py_cosine), ("token_jaccard", 3, R.py_jaccard), ("token_cosine", 3, R.py_cosine)):
        tab = R.table("profile_edges", method, ngram)
        prof = [R.py_tokens(s) if method.startswith("token") else R.py_ngrams(s, ngram) for s in labels]
        for i in range(len(labels)):
            for j in range(i + 1, len(labels)):
                if method == "ngram_cosine" and min(len(R.units(labels[i])), len(R.units(labels[j]))) < ngram:
                    assert tab.sim[i, j] == 0.0
                else:
                    np.testing.assert_equal(tab.sim[i, j], model(prof[i], prof[j]), err_msg="%s %d %d" % (method, i, j))


def test_numeric_own_vertex_cases_are_the_references():
    cases = R.numeric_own_vertex()
    assert len(cases) >= 6
    for c in cases:
        i, j, s = O.compare_group(O.sim_cfg("numeric", **R.NUMERIC_CFG), c["labels"], c["source"], c["target"], c["source_vertex"],
                                  c["target_vertex"], upper_triangle=c["upper"])
        assert list(zip(i, j)) == c["pairs"], c["name"]
    first = cases[0]
    i, j, s = O.compare_group(O.sim_cfg("numeric", **R.NUMERIC_CFG), first["labels"], first["source"], first["target"], first["source_vertex"],
                              first["target_vertex"])
    assert s[0] == np.float32(0.70710677)

"""Known answers for the literal-similarity restatement (oracle/ge_oracle_sim.c), SURVEY.md 8f rank 4.

PARITY UNPINNED: the reference ships no tests.  Token*, Numeric and Date* follow the reference's own sources and are
checked against values derived by hand from them; JaroWinkler / Levenshtein / n-gram profiles live in
info.debatty:java-string-similarity (not under /root/reference, version "RELEASE") and are checked against the two
values that library's README prints, the textbook Jaro-Winkler examples, and an independent Python model."""
import numpy as np
import pytest

import oracle as O
from sim_ref import py_cosine, py_jaccard, py_jaro_winkler, py_levenshtein, py_ngrams, py_tokens


def sim(method, a, b, **kw):
    v, threw = O.sim_pair(O.sim_cfg(method, **kw), a, b)
    assert not threw
    return v


# ---- known answers ---------------------------------------------------------------------------------------------
def test_jaro_winkler_readme_and_textbook_values():
    # java-string-similarity README: jw.similarity("My string", "My tsring") / ("My string", "My ntrisg")
    assert float(np.float32(sim("jarowinkler", "My string", "My tsring"))) == 0.9740740656852722
    assert float(np.float32(sim("jarowinkler", "My string", "My ntrisg"))) == 0.8962963223457336
    for a, b, want in (("MARTHA", "MARHTA", 0.9611), ("DIXON", "DICKSONX", 0.8133), ("DWAYNE", "DUANE", 0.84), ("CRATE", "TRACE", 0.7333)):
        assert abs(sim("jarowinkler", a, b) - want) < 1e-4
    assert sim("jarowinkler", "abc", "abc") == 1.0
    assert sim("jarowinkler", "abc", "xyz") == 0.0
    assert sim("jarowinkler", "", "xyz") == 0.0
    assert sim("jarowinkler", "abc", "") == 0.0
    # the library's prefix is NOT capped at four characters, its weight is min(0.1, 1 / max length)
    assert sim("jarowinkler", "abcdefghij", "abcdefghix") == pytest.approx(0.9333333 + 0.1 * 9 * (1 - 0.9333333), abs=1e-6)


def test_levenshtein_known_distances():
    def dist(a, b):
        x, y = O.utf16(a), O.utf16(b)
        x_ = x if len(x) else np.zeros(1, np.uint16); y_ = y if len(y) else np.zeros(1, np.uint16)
        return O.lib().geo_sim_levenshtein_distance(O._p(x_, O.C.c_uint16), len(x), O._p(y_, O.C.c_uint16), len(y))
    assert dist("kitten", "sitting") == 3
    assert dist("My string", "My $tring") == 1            # README of the library
    assert dist("flaw", "lawn") == 2
    assert dist("", "abc") == 3 and dist("abc", "") == 3 and dist("abc", "abc") == 0
    assert sim("levenshtein", "kitten", "sitting") == 1.0 - 3 / 7
    assert sim("levenshtein", "", "") == 1.0


def test_token_profiles_follow_the_tokenator():
    # "the" / "a" are stop words, one-character tokens are dropped, only ' ' separates, trim() strips the rest
    assert sim("token_jaccard", "the quick brown fox", "a quick red fox jumps") == 2 / 5
    assert sim("token_cosine", "deep deep learning", "deep learning of graphs") == 3 / (np.sqrt(5.0) * np.sqrt(3.0))
    assert py_tokens("x the\tcat  sat\n on a mat") == {tuple(map(ord, t)): 1 for t in ("the\tcat", "sat", "mat")}   # a tab does not split; "the\tcat" is no stop word
    assert sim("token_jaccard", "x the\tcat  sat\n on a mat", "sat mat") == 2 / 3
    assert np.isnan(sim("token_jaccard", "a of", "the an"))                                    # 0 / 0.0
    assert sim("token_jaccard", "a of", "a of") == 1.0                                         # equals() first
    assert np.isnan(sim("token_cosine", "a", "b c"))


def test_ngram_profiles():
    assert sim("ngram_jaccard", "abcd", "bcde", ngram=2) == 0.5
    assert sim("ngram_jaccard", "a  b\t\tc", "a b c", ngram=2) == 1.0              # whitespace runs collapse before shingling
    assert sim("ngram_cosine", "ab", "abc", ngram=3) == 0.0                        # PreComputedNgramCosine: shorter than k -> 0
    assert np.isnan(sim("ngram_jaccard", "ab", "cd", ngram=3))                     # ... but the Jaccard variant has no such guard
    assert sim("ngram_cosine", "abab", "abba", ngram=2) == pytest.approx(3 / (np.sqrt(5.0) * np.sqrt(3.0)))


def test_numeric_including_its_quirks():
    assert sim("numeric", "1985^^http://x#int", "1990^^http://x#int", smooth=0.5) == 6 ** -0.5
    assert sim("numeric", "7", "7") == 1.0 and sim("numeric", "", "7") == 0.0
    assert sim("numeric", "10", "13", smooth=0.5, distance=1.0) == 3 ** -0.5       # ||10-13| - 1| + 1 = 3
    assert sim("numeric", "12", "x3", smooth=0.5) == 0.0                            # NumberFormatException -> 0
    assert sim("numeric", "2147483648", "1", smooth=0.5) == 0.0                     # outside int
    assert sim("numeric", "5", "9") == 1.0                                          # smooth defaults to 1: x ** 0
    # Numeric.java:33 takes the '^' position of s1 for s2 as well: "1990" + "1" is cut to "1990" ...
    assert sim("numeric", "1985^^t", "19901", smooth=0.5) == 6 ** -0.5
    # ... and a shorter s2 makes String.substring throw: the CompareJob dies
    v, threw = O.sim_pair(O.sim_cfg("numeric", smooth=0.5), "1985^^t", "19")
    assert threw


def test_dates():
    assert sim("date_days", "20200101", "20200131", smooth=0.5) == 31 ** -0.5
    assert sim("date_days", "20200101", "20200230", smooth=0.5) == 0.0              # BASIC_ISO_DATE is STRICT
    assert sim("date_days", "20200101Z", "20200102+0100", smooth=0.5) == 2 ** -0.5  # optional offset
    assert sim("date_days", "2020-01-01", "2020-01-03", smooth=0.5, pattern="yyyy-MM-dd") == 3 ** -0.5
    assert sim("date_days", "2019-02-28", "2019-02-30", smooth=0.5, pattern="yyyy-MM-dd") == 1.0 ** -0.5   # SMART clamps Feb 30 to Feb 28
    assert sim("date_months", "2020-01-31^^xsd:date", "2020-03-30", smooth=0.5, pattern="yyyy-MM-dd") == 2 ** -0.5   # one whole month
    assert sim("date_years", "2020-01-31", "2010-03-30", smooth=0.5, pattern="yyyy-MM-dd") == 10 ** -0.5             # -9 whole years
    assert sim("date_years", "2020-01-31", "2010-03-30", smooth=0.5, pattern="yyyy-MM-dd", time="backwards") == 0.0  # d1 after d2
    assert sim("date_years", "2020-01-31", "2010-03-30", smooth=0.5, pattern="yyyy-MM-dd", time="forwards") == 10 ** -0.5
    assert sim("date_days", "19700101", "19700101") == 1.0 and sim("date_days", "", "19700101") == 0.0
    assert sim("date_days", "1600-02-29", "1600-03-01", smooth=0.5, pattern="uuuu-MM-dd") == 2 ** -0.5     # 1600 is a leap year
    assert sim("date_days", "20200301", "20190301", smooth=0.5) == 367 ** -0.5                                # across Feb 29 2020
    assert O.lib().geo_sim_pattern_supported(b"yyyy-MM-dd") == 1 and O.lib().geo_sim_pattern_supported(b"d/M/yyyy") == 1
    assert O.lib().geo_sim_pattern_supported(b"yyyy-MMM-dd") == 0 and O.lib().geo_sim_pattern_supported(b"MM-dd") == 0
    assert sim("date_days", "3/1/2020", "13/1/2020", smooth=0.5, pattern="d/M/yyyy") == 11 ** -0.5
    assert sim("date_days", "20200103", "20200101", smooth=0.5, pattern="yyyyMMdd") == 3 ** -0.5             # adjacent value parsing


def test_compare_group_job_order_and_rules():
    labels = ["jan jansen", "jan janssen", "piet", "pieter", "jan jansen"]
    i, j, s = O.compare_group(O.sim_cfg("jarowinkler", 0.8), labels, [0, 1, 2, 3, 4], [0, 1, 2, 3, 4], upper_triangle=True)
    assert list(zip(i, j)) == [(0, 1), (0, 4), (1, 4), (2, 3)]                       # job i, then j > i
    assert s[1] == 1.0                                                               # equal labels on two vertices
    # rectangular group: every job starts at target 0 and skips its own vertex only
    i, j, s = O.compare_group(O.sim_cfg("levenshtein", 0.5), labels, [0, 2], [0, 1, 2, 3], source_vertex=[10, 12], target_vertex=[10, 11, 12, 13])
    assert list(zip(i, j)) == [(0, 1), (1, 3)]
    # a Numeric job that throws loses ALL its results, also the ones found before the throw
    nums = ["1985^^t", "1986^^t", "19", "1984^^t"]
    i, j, s = O.compare_group(O.sim_cfg("numeric", 0.1, smooth=0.5), nums, [0, 1, 2, 3], [0, 1, 2, 3], upper_triangle=True)
    assert list(zip(i, j)) == []          # jobs 0 and 1 meet "19"; job 2 ("19", no '^') parses "1984^^t" whole -> NumberFormatException -> 0
    i, j, s = O.compare_group(O.sim_cfg("numeric", 0.1, smooth=0.5), nums, [3, 1, 0], [3, 1, 0], upper_triangle=True)
    assert list(zip(i, j)) == [(0, 1), (0, 2), (1, 2)]


@pytest.mark.parametrize("seed", range(3))
def test_restatement_against_python_models(seed):
    rng = np.random.default_rng(seed)
    alphabet = list("abcde ") + ["é", "\t", "𝄞"]
    words = ["".join(rng.choice(alphabet, size=rng.integers(0, 14))) for _ in range(40)]
    for a in words[:20]:
        for b in words[20:]:
            assert sim("jarowinkler", a, b) == py_jaro_winkler(list(O.utf16(a)), list(O.utf16(b)))
            m = max(len(O.utf16(a)), len(O.utf16(b)))
            want = 1.0 if a == b else (1.0 if m == 0 else 1.0 - py_levenshtein(list(O.utf16(a)), list(O.utf16(b))) / m)
            assert sim("levenshtein", a, b) == want
            for k in (2, 3):
                np.testing.assert_equal(sim("ngram_jaccard", a, b, ngram=k), 1.0 if a == b else py_jaccard(py_ngrams(a, k), py_ngrams(b, k)))
            np.testing.assert_equal(sim("token_jaccard", a, b), 1.0 if a == b else py_jaccard(py_tokens(a), py_tokens(b)))
            np.testing.assert_equal(sim("token_cosine", a, b), 1.0 if a == b else py_cosine(py_tokens(a), py_tokens(b)))

"""Independent Python models of the string metrics, designed label families for the similarity kernels, and the
oracle's double similarity of every pair of a family, computed once per process.

TEST INFRASTRUCTURE ONLY.  The families are built from UTF-16 code units so that every match is intended: a base of
distinct units `0x100 + u`, one surrogate pair, a tab and a space where the family allows them.  `launch()` in
csrc/similarity.hip picks the mask width W = 2 / 8 / 32 words from the longest label in use, hence the length class
L in {64, 256, 1024} of the string families.  A family at L = 256 or 1024 holds at most 48 labels: the oracle's
all-pairs walk over them is what a test pays for, once."""
import collections
import ctypes as C
import functools

import numpy as np

import oracle as O

f32 = np.float32

# ---- independent Python models ---------------------------------------------------------------------------------
JaroDetail = collections.namedtuple("JaroDetail", "value matches transpositions last_min last_max jaro idx")
JaroDetail.__doc__ = """value: the Jaro-Winkler similarity; matches; transpositions: mismatches of the two matched sequences
BEFORE halving; last_min / last_max: largest flagged position in the shorter / longer string (-1: none); jaro: the float
Jaro value as a double; idx[mi]: position in the longer string matched to unit mi of the shorter one, or -1."""


def py_jaro_winkler(s1, s2, details=False):
    f = f32
    if s1 == s2:
        n = len(s1)
        return JaroDetail(1.0, n, 0, n - 1, n - 1, 1.0, list(range(n))) if details else 1.0
    mx, mn = (s1, s2) if len(s1) > len(s2) else (s2, s1)
    rng = max(len(mx) // 2 - 1, 0)
    where = {}
    for xi, c in enumerate(mx):
        where.setdefault(c, []).append(xi)
    flags = [False] * len(mx); idx = [-1] * len(mn)
    for mi, c in enumerate(mn):
        lo, hi = max(mi - rng, 0), min(mi + rng + 1, len(mx))
        for xi in where.get(c, ()):                        # ascending: the first free equal unit inside the window
            if xi >= hi:
                break
            if xi >= lo and not flags[xi]:
                flags[xi] = True; idx[mi] = xi; break
    ms1 = [mn[i] for i in range(len(mn)) if idx[i] != -1]
    ms2 = [mx[i] for i in range(len(mx)) if flags[i]]
    m = len(ms1)
    if m == 0:
        return JaroDetail(0.0, 0, 0, -1, -1, 0.0, idx) if details else 0.0
    t2 = sum(a != b for a, b in zip(ms1, ms2))
    t = t2 // 2
    prefix = 0
    for a, b in zip(s1, s2):
        if a != b:
            break
        prefix += 1
    mf = f(m)
    j = float(f(f(f(mf / f(len(s1))) + f(mf / f(len(s2)))) + f(f(mf - f(t)) / mf)) / f(3))
    v = j + min(0.1, 1.0 / len(mx)) * prefix * (1 - j) if j > 0.7 else j
    if not details:
        return v
    return JaroDetail(v, m, t2, max(i for i in range(len(mn)) if idx[i] != -1), max(i for i in range(len(mx)) if flags[i]), j, idx)


def py_levenshtein(a, b):
    prev = list(range(len(b) + 1))
    for i, ca in enumerate(a):
        cur = [i + 1]
        for j, cb in enumerate(b):
            cur.append(min(cur[j] + 1, prev[j + 1] + 1, prev[j] + (ca != cb)))
        prev = cur
    return prev[-1]


STOP = {"the", "of", "and", "a", "an", "to", "in", "is", "you", "that", "it", "for", "on", "from", "are", "as", "with", "at", "or", "by", "but", "if"}


def py_tokens(s):
    """Tokenator over UTF-16 code units (String.length / charAt / trim count units: an astral character is two)."""
    u = [int(x) for x in O.utf16(s)]
    stop = {tuple(ord(c) for c in w) for w in STOP}
    out, start = {}, 0
    for pos, ch in enumerate(u):
        if ch == 32 or pos == len(u) - 1:
            a, b = start, pos + 1
            while a < b and u[a] <= 32: a += 1
            while b > a and u[b - 1] <= 32: b -= 1
            tok = tuple(u[a:b])
            start = pos + 1
            if len(tok) > 1 and tok not in stop:
                out[tok] = out.get(tok, 0) + 1
    return out


def py_ngrams(s, k):
    """k-grams over UTF-16 code units (java.lang.String.substring), whitespace runs collapsed first."""
    u, t = [int(x) for x in O.utf16(s)], []
    for c in u:
        ws = c == 32 or 9 <= c <= 13
        if ws and t and t[-1] == 32 and prev_ws:
            continue
        t.append(32 if ws else c); prev_ws = ws
    out = {}
    for i in range(len(t) - k + 1):
        g = tuple(t[i:i + k]); out[g] = out.get(g, 0) + 1
    return out


def py_jaccard(p, q):
    u = len(set(p) | set(q))
    return (len(p) + len(q) - u) / u if u else float("nan")


def py_cosine(p, q):
    dot = sum(c * q.get(g, 0) for g, c in p.items())
    n = np.sqrt(float(sum(c * c for c in p.values()))) * np.sqrt(float(sum(c * c for c in q.values())))
    return dot / n if n else float("nan")


def jw_length_bound(n1, n2):
    """The most a pair can reach from its lengths alone, in double: every unit of the shorter label matched in order.
    The kernel prunes a pair when this is below threshold - 1e-6."""
    nmn, nmx = min(n1, n2), max(n1, n2)
    jmax = (nmn / n1 + nmn / n2 + 1.0) / 3.0
    return jmax + min(0.1, 1.0 / nmx) * nmn * (1.0 - jmax)


# ---- label families --------------------------------------------------------------------------------------------
HI, LO = 0xD834, 0xDD1E                                   # U+1D11E as two code units
LENGTH_CLASSES = (64, 256, 1024)


def units(s):
    return [int(x) for x in O.utf16(s)]


def text(u):
    """Code units -> str; a lone surrogate raises (the families keep their one pair whole)."""
    return np.asarray(u, np.uint16).tobytes().decode("utf-16-le")


def _alphabet(n, off=0):
    return [0x100 + off + u for u in range(n)]


@functools.lru_cache(maxsize=None)
def _jw_sparse(L):
    rng = np.random.default_rng(L)
    base = _alphabet(L)
    base[5], base[6] = 9, 32                                # a tab and a space: ordinary units to Jaro and Levenshtein
    base[40:42] = [HI, LO]                                  # no rotation, exchange or cut below separates the pair
    out = [("base", base)]
    for r in dict.fromkeys((1, 2, 31, 32, 33, L // 2 - 2, L // 2 - 1, L // 2)):
        out.append(("rot%d" % r, base[r:] + base[:r]))
    rev = base[::-1]
    rev[L - 42:L - 40] = [HI, LO]                           # the reverse, with the surrogate pair left in order
    out.append(("reverse", rev))
    for c in (31, 32, 33, 63, 64, 65):
        if 2 * c <= L:
            out.append(("swap%d" % c, base[c:2 * c] + base[:c] + base[2 * c:]))
    keep = [p for p in (31, 32, 63, 64, L - 1) if p < L]
    for k in (1, 2):
        lab = _alphabet(L, k * L)
        for p in keep:
            lab[p] = base[p]
        out.append(("only%d" % k, lab))
    out.append(("cut%d" % (L - 1), base[:L - 1]))
    lengths = [L, L - 1] + ([31, 32, 33] if L == 64 else []) + [int(x) for x in rng.integers(L - 40, L + 1, size=10)]
    symbols = _alphabet(40)
    for k, n in enumerate(lengths):
        out.append(("random%d_%d" % (k, n), [int(x) for x in rng.choice(symbols, size=n)]))
    if L == 64:
        out += [("cut%d" % n, base[:n]) for n in (31, 32, 33)]
    assert len(out) <= 48
    return [text(u) for _, u in out], {name: k for k, (name, _) in enumerate(out)}


def jw_sparse(L):
    """Labels that set match flags in every mask word and make the window and the transposition walk decide."""
    return list(_jw_sparse(L)[0])


def jw_sparse_index(L):
    """name -> position: base, rot<r>, reverse, swap<c>, only<k>, cut<n>, random<k>_<n>."""
    return dict(_jw_sparse(L)[1])


def jaro_float(n1, n2, m, t):
    """The float Jaro value of m matches with t (halved) transpositions, as a double."""
    f = f32
    mf = f(m)
    return float(f(f(f(mf / f(n1)) + f(mf / f(n2))) + f(f(mf - f(t)) / mf)) / f(3))


def _gate_pair(n1, n2, m, t, salt):
    """Two labels of n1 <= n2 units with exactly m matches and 2t mismatches among them: the common units, the last t
    adjacent pairs exchanged in the second label, then units that match nothing."""
    common = _alphabet(m, 64)
    other = list(common)
    for k in range(t):
        a = m - 2 - 2 * k
        other[a], other[a + 1] = other[a + 1], other[a]
    return common + _alphabet(n1 - m, 200 + 64 * salt), other + _alphabet(n2 - m, 232 + 64 * salt)


@functools.lru_cache(maxsize=None)
def _jw_gate():
    base = _alphabet(64)
    base[3] = 9
    prefix_lengths = list(range(1, 25)) + [32, 33, 64]
    labels = [base[:n] for n in prefix_lengths]
    prefix_pairs = [(a, b) for a in range(len(labels)) for b in range(a + 1, len(labels))]
    # every attainable float Jaro value near 0.7 of labels up to 64 units (up to 24 the nearest value above 0.7 is
    # 3.1e-5 away; (18, 25, 15, 5) is the shortest shape that reaches the float right above 0.7)
    seven = float(f32(0.7))
    found = {}
    for n2 in range(1, 65):
        n1, m, t = np.meshgrid(np.arange(1, n2 + 1), np.arange(1, n2 + 1), np.arange(0, 33), indexing="ij")
        ok = (m <= n1) & (2 * t <= m) & ((t == 0) | (n2 >= 4))     # a window of 0 cannot match exchanged neighbours
        n1, m, t = n1[ok], m[ok], t[ok]
        mf = m.astype(f32)
        j = ((((mf / n1.astype(f32)) + (mf / f32(n2))) + ((mf - t.astype(f32)) / mf)) / f32(3)).astype(np.float64)
        near = np.abs(j - 0.7) < 1e-3
        for a, b, c, v in zip(n1[near], m[near], t[near], j[near]):
            assert float(v) == jaro_float(int(a), n2, int(b), int(c))
            found.setdefault(float(v), []).append((int(a), n2, int(b), int(c)))
    values = sorted(found)
    at = values.index(seven)
    gate = []
    for v in values[at - 3:at + 4]:                         # 0.7f, and the three attainable values on either side
        for shape in found[v][:2]:
            a, b = _gate_pair(*shape, salt=len(gate))
            d = py_jaro_winkler(a, b, details=True)
            if d.jaro == v and (d.matches, d.transpositions) == (shape[2], 2 * shape[3]):
                gate.append((len(labels), len(labels) + 1, v)); labels += [a, b]
    one, ten = [ord("a")], [ord("a")] + [ord("b")] * 9      # the issue's own example: 2.1f / 3 = 0.7f, no boost
    gate.append((len(labels), len(labels) + 1, seven)); labels += [one, ten]
    return [text(u) for u in labels], {"prefix": prefix_pairs, "gate": gate}


def jw_gate():
    """Short labels: prefixes of one base (every pair of them attains the length bound of the prune) and pairs whose
    float Jaro value is 0.7f or one of its attainable neighbours."""
    return list(_jw_gate()[0])


def jw_gate_info():
    """{"prefix": [(i, j)], "gate": [(i, j, float Jaro value)]} over positions in jw_gate()."""
    return _jw_gate()[1]


def _substituted(base, where, off):
    lab = list(base)
    for k, p in enumerate(where):
        lab[p] = 0x100 + off + k
    return lab


@functools.lru_cache(maxsize=None)
def _lev_edges(L):
    labels, cases, seen = [[]], [], {(): 0}                 # position 0: the empty label

    def add(lab):
        if tuple(lab) not in seen:
            seen[tuple(lab)] = len(labels); labels.append(list(lab))
        return seen[tuple(lab)]

    full = L == 64
    fresh = 2048                                            # substitutes: units no base holds, never reused
    for m in dict.fromkeys((1, 2, 7, 8, 10, 63, 64, L)):
        base = _alphabet(m)
        if m >= 8:
            base[3] = 32
        if m >= 63:
            base[40:42] = [HI, LO]
        b = add(base)
        if m == L or full:
            ds = sorted({1, m // 2, m - 1, m} - {0})
        else:
            ds = sorted({1, m // 2} - {0})
        for d in ds:
            places = {"end": range(m - d, m), "start": range(d), "spread": [(2 * k + 1) * m // (2 * d) for k in range(d)]}
            if not (m == L or full):
                places = {"end": places["end"]} if d == 1 else {"spread": places["spread"]}
            for name, where in places.items():
                where = list(where)
                if HI in [base[p] for p in where] and LO not in [base[p] for p in where]:
                    where[[base[p] for p in where].index(HI)] -= 1                  # never half a surrogate pair
                if LO in [base[p] for p in where] and HI not in [base[p] for p in where]:
                    where[[base[p] for p in where].index(LO)] += 1
                if len(set(where)) != d or min(where) < 0 or max(where) >= m:
                    continue
                cases.append((m, d, b, add(_substituted(base, where, fresh)), name)); fresh += d
        # shorter partners: the length difference is the distance; around every give_up the thresholds 1 - d/m produce
        cuts = set()
        for d in ([0] + ds if (m == L or full) else []):
            cuts |= {k for k in (d - 1, d, d + 1, d + 2) if 0 < k <= m}
        cuts.add(1)
        if m <= 10 and full:
            cuts = set(range(1, m + 1))
        for k in sorted(cuts):
            if base[m - k - 1:m - k] == [HI]:
                continue
            cases.append((m, k, b, add(base[:m - k]), "cut"))
    assert L == 64 or len(labels) <= 48, len(labels)
    return [text(u) for u in labels], cases


def lev_edges(L):
    """Bases of m distinct units with partners at a known distance d: substitutions at the end, at the start and
    spread out, prefixes shorter by d, a disjoint partner (d = m) and the empty label."""
    return list(_lev_edges(L)[0])


def lev_edges_cases(L):
    """[(m, d, position of the base, position of the partner, placement)]"""
    return list(_lev_edges(L)[1])


@functools.lru_cache(maxsize=None)
def profile_edges():
    """Profiles at the capacity of the kernel's LDS lists (1024 distinct grams at ngram = 1), empty, equal and disjoint
    profiles, and the Tokenator's arms."""
    full = _alphabet(1024)
    repeat = list(full); repeat[5] = repeat[4]
    return (text(full), text(repeat),
            # the first third is the source side of the rectangular split: it holds one of each kind
            "graph embedding learning", "deep graph learning deep vectors", "glove vectors", "abcabcabc",
            "abcdef", "graph embedding", "deep\tlearning graph", "ab  cd",
            "uvwxyz",                                         # gram set disjoint from "abcdef"
            "ab \t cd",                                       # another label, the profile of "ab  cd"
            "", "a", "ab", "abc",                             # shorter than ngram
            "a    b",                                         # raw length 6, collapsed length 3
            "the of and", "x y z q",                          # stop words only; one-unit tokens only
            "graph embedding ", "graph embedding  ", "graph x",                       # the pos == n - 1 arm
            "deep learning graph",                            # a tab does not split a token
            "\U0001D11E\U0001D11E graph", "\U0001D11E graph",
            "graph embedding learning deep", "graph graph graph embedding", "knowledge graph embedding learning deep vectors glove",
            "abcdefabc", "bcdefa uvw")


def family(name):
    if name == "jw_gate":
        return jw_gate()
    if name == "profile_edges":
        return list(profile_edges())
    for L in LENGTH_CLASSES:
        if name == "jw_sparse%d" % L:
            return jw_sparse(L)
        if name == "lev_edges%d" % L:
            return lev_edges(L)
    raise KeyError(name)


NUMERIC_CFG = dict(threshold=0.1, smooth=0.5)


def numeric_own_vertex():
    """Numeric jobs and short targets: a target shorter than the job's '^' position kills the job (String.substring
    throws) unless the job never reaches it: its own vertex, below the diagonal, empty.  Each case: labels, source /
    target positions, source / target vertices, upper_triangle, and the pairs the reference keeps."""
    T, U, S = "1985^^t", "1986^^t", "19"
    case = lambda name, labels, src, tgt, sv, tv, upper, pairs: dict(name=name, labels=labels, source=src, target=tgt,
                                                                      source_vertex=sv, target_vertex=tv, upper=upper, pairs=pairs)
    return [
        case("short target on the job's own vertex", [T, S, U], [0], [1, 2], [5], [5, 6], False, [(0, 1)]),
        case("short target on another vertex", [T, S, U], [0], [1, 2], [5], [7, 6], False, []),
        case("own short target, then a foreign one", [T, S, U, S], [0], [1, 2, 3], [5], [5, 6, 7], False, []),
        case("two short targets, both on the own vertex", [T, S, U, "1"], [0], [1, 2, 3], [5], [5, 6, 5], False, [(0, 1)]),
        case("short label before the source position", [S, T, U], [0, 1, 2], [0, 1, 2], [1, 2, 3], [1, 2, 3], True, [(1, 2)]),
        case("short label after the source position", [T, U, S], [0, 1, 2], [0, 1, 2], [1, 2, 3], [1, 2, 3], True, []),
        case("short label after, on the job's own vertex", [T, U, S], [0, 1, 2], [0, 1, 2], [1, 2, 1], [1, 2, 1], True, [(0, 1)]),
        case("an empty label never kills", [T, "", U], [0], [1, 2], [5], [7, 6], False, [(0, 1)]),
        case("length equal to the '^' position", [T, "1990", U], [0], [1, 2], [5], [7, 6], False, [(0, 0), (0, 1)]),
    ]


# ---- the oracle's double similarity of every pair, once ----------------------------------------------------------
Table = collections.namedtuple("Table", "labels sim have")
_TABLES = {}


def table(name, method, ngram=3):
    """sim[i, j] = metric.similarity(labels[i], labels[j]) in double, NaN included, for every i < j -- and for every
    ordered pair where the family is short (Jaro's matching is not symmetric at equal lengths)."""
    key = (name, method, ngram)
    if key in _TABLES:
        return _TABLES[key]
    labels = family(name)
    enc = [np.ascontiguousarray(O.utf16(s) if s else np.zeros(1, np.uint16)) for s in labels]
    lens = [len(O.utf16(s)) for s in labels]
    n = len(labels)
    sim = np.full((n, n), np.nan); have = np.zeros((n, n), bool)
    cfg = O.sim_cfg(method, ngram=ngram)
    lib = O.lib(); threw = C.c_int(0)
    both = max(lens) <= 64
    for i in range(n):
        for j in range(0 if both else i + 1, n):
            if i == j:
                continue
            sim[i, j] = lib.geo_sim_pair(C.byref(cfg), O._p(enc[i], C.c_uint16), lens[i], O._p(enc[j], C.c_uint16), lens[j], C.byref(threw))
            assert not threw.value
            have[i, j] = True
    sim.setflags(write=False); have.setflags(write=False)
    _TABLES[key] = Table(labels, sim, have)
    return _TABLES[key]


def expected(tab, threshold, source, target, source_vertex=None, target_vertex=None, upper=False, job_range=None):
    """The CompareJob loop over the table, filtered in double, in job order -> (i, j, float32 similarity)."""
    sv = list(source) if source_vertex is None else source_vertex
    tv = list(target) if target_vertex is None else target_vertex
    lo, hi = (0, len(source)) if job_range is None else job_range
    oi, oj, os_ = [], [], []
    for i in range(lo, hi):
        for j in range(i + 1 if upper else 0, len(target)):
            if tv[j] == sv[i]:
                continue
            assert tab.have[source[i], target[j]], "pair (%d, %d) is not in the table" % (source[i], target[j])
            v = tab.sim[source[i], target[j]]
            if v >= threshold:
                oi.append(i); oj.append(j); os_.append(v)
    return np.array(oi, np.int32), np.array(oj, np.int32), np.array(os_, np.float64).astype(np.float32)


def splits(n):
    """The two group forms every family runs in: the square upper triangle, and a rectangular split whose pairs all
    lie in the table's upper half (sources before targets)."""
    k = n // 3
    return [("square", list(range(n)), list(range(n)), True), ("rect", list(range(k)), list(range(k, n)), False)]


def attained(tab, count=8):
    """`count` (or all, if fewer) distinct similarities in (0, 1] that pairs i < j attain, spread over the sorted values."""
    v = np.unique(tab.sim[np.triu(tab.have, 1) & (tab.sim > 0) & (tab.sim <= 1)])
    if len(v) <= count:
        return [float(x) for x in v]
    return [float(v[k]) for k in np.unique(np.linspace(0, len(v) - 1, count).round().astype(int))]

"""A plain model of one Bookmark Coloring walk, and graphs designed to land on the bounds of the builder's LDS kernel.

The model restates DirectedWeighted.doWork / UndirectedWeighted.doWork with a dict for the TreeMap and Python floats (fp64) for
the paint; it knows nothing of tables, wavefronts or java.util.HashMap order, so it yields key -> value maps, not rows.  What it
adds to the oracle is what the oracle does not report: how many nodes a bookmark touches and how many sit in the TreeMap at once --
the two quantities that decide whether k_bca<true> keeps a bookmark (<= 512 touched over both passes, <= 384 at once) or hands it
to k_bca<false>.  tests/test_bca_designed.py holds the model to the oracle bit for bit and every design to its place on a bound.
"""
import heapq

import numpy as np

from geglove import synth

ALPHA, EPS = 0.1, 1e-3
LDS_MAX, LDS_AC = 512, 384            # csrc/bca.hip: nodes per bookmark, nodes at once in the TreeMap
F32 = np.float32


# ---- the walk -------------------------------------------------------------------------------------------------------------------
def _adj(graph):
    """Neighbour lists (id, weight / total in fp64) per mode and the sequential fp64 totals, once per graph."""
    a = graph.get("_adj")
    if a is None:
        def lists(csr):
            ptr, idx, w = csr
            idx = np.asarray(idx).tolist(); w = np.asarray(w, F32).astype(np.float64).tolist(); ptr = np.asarray(ptr).tolist()
            return [list(zip(idx[ptr[v]:ptr[v + 1]], w[ptr[v]:ptr[v + 1]])) for v in range(graph["V"])]
        out, inn = lists(graph["out"]), lists(graph["inn"])

        def total(*parts):
            t = 0.0
            for part in parts:
                for _, w in part:
                    t += w
            return t
        # the heaviest edge per list: where even that one's share is below epsilon the whole spread is dropped, which a pop of
        # a 385-leaf star's root with a trace of paint would otherwise spend 385 steps to find out (exact: x -> spread * (x / total)
        # is monotone for x >= 0, total > 0; lists with a negative weight get no such bound)
        def heaviest(part):
            return max((w for _, w in part), default=0.0) if all(w >= 0 for _, w in part) else float("inf")
        t_out, t_in, t_und = [total(o) for o in out], [total(i) for i in inn], [total(o, i) for o, i in zip(out, inn)]

        # (double) weight / totalWeight per edge, once: the same fp64 quotient at every pop (x / 0 as Java has it: inf or NaN)
        def shares(part, t):
            with np.errstate(divide="ignore", invalid="ignore"):
                return [(nb, w / t if t != 0 else float(np.float64(w) / np.float64(t))) for nb, w in part]
        a = graph["_adj"] = ([shares(o, t) for o, t in zip(out, t_out)], [shares(i, t) for i, t in zip(inn, t_in)],
                             [shares(o + i, t) for o, i, t in zip(out, inn, t_und)], t_out, t_in, t_und,
                             [heaviest(o) for o in out], [heaviest(i) for i in inn])
    return a


def walk(graph, bookmark, alpha, eps, mode):
    """One pass.  mode 0: out-neighbours, 1: in-neighbours, 2: undirected (out then in, one total).
    Returns (nodes touched, in order; peak TreeMap size after any insertion; BCV as {node: float32}, in put order)."""
    out, inn, und, t_out, t_in, t_und, h_out, h_in = _adj(graph)
    tree = {bookmark: 1.0}
    order = [bookmark]                                          # the TreeMap's keys as a heap: a key is pushed when it enters the map
    touched, seen, peak, bcv = [bookmark], {bookmark}, 1, {}
    while tree:
        f = heapq.heappop(order)                                # pollFirstEntry()
        wet = tree.pop(f)
        bcv[f] = F32(bcv.get(f, F32(0)) + F32(alpha * wet))     # put(key, getOrDefault(key, 0f) + (float)(alpha * wet))
        if wet < eps:
            continue
        if mode == 0:
            nbrs, total, heavy = out[f], t_out[f], h_out[f]
        elif mode == 1:
            nbrs, total, heavy = inn[f], t_in[f], h_in[f]
        else:
            nbrs, total, heavy = und[f], t_und[f], max(h_out[f], h_in[f])
        if mode != 2 and (not nbrs or total == 0):
            continue
        spread = (1 - alpha) * wet
        if total > 0 and spread * (heavy / total) < eps:
            continue
        for nb, share in nbrs:
            pt = spread * share
            if pt < eps:
                continue
            if nb in tree:
                tree[nb] = tree[nb] + pt
            else:
                tree[nb] = pt
                heapq.heappush(order, nb)
                if nb not in seen:
                    seen.add(nb); touched.append(nb)
                peak = max(peak, len(tree))
    return touched, peak, bcv


def row(graph, b, alpha=ALPHA, eps=EPS, directed=True):
    """The un-normalised row of bookmark b as {key: float32}: forward BCV, the reverse BCV merged in with Float.sum."""
    if not directed:
        return walk(graph, b, alpha, eps, 2)[2]
    f = dict(walk(graph, b, alpha, eps, 0)[2])
    for k, v in walk(graph, b, alpha, eps, 1)[2].items():
        f[k] = F32(f[k] + v) if k in f else v
    return f


def stats(graph, b, alpha=ALPHA, eps=EPS, directed=True):
    """fwd: nodes the forward pass touches; union: forward and reverse together (what the LDS table must hold); peak: the largest
    TreeMap of either pass; row: entries of the un-normalised row."""
    if not directed:
        t, peak, bcv = walk(graph, b, alpha, eps, 2)
        return dict(fwd=len(t), union=len(t), peak=peak, row=len(bcv))
    tf, pf, bf = walk(graph, b, alpha, eps, 0)
    tr, pr, br = walk(graph, b, alpha, eps, 1)
    return dict(fwd=len(tf), union=len(set(tf) | set(tr)), peak=max(pf, pr), row=len(set(bf) | set(br)))


def handed_over(s):
    return s["union"] > LDS_MAX or s["peak"] > LDS_AC


def java_hash(k):
    return (k ^ (k >> 16)) & 0xFFFFFFFF


def plain_order(bcv):
    """Iteration order of a java.util.HashMap that only ever grew by load factor and whose bins are plain lists: (bin, put sequence)."""
    cap = 16
    while len(bcv) > cap // 4 * 3:
        cap <<= 1
    keys = list(bcv)
    return sorted(keys, key=lambda k: (java_hash(k) & (cap - 1), keys.index(k)))


# ---- edge lists -----------------------------------------------------------------------------------------------------------------
def comb(base, a, cs):
    """Root `base`; then mid_1, its cs[0] leaves, mid_2, its leaves, ... at ascending ids.  Leaves pop before the next mid spreads,
    so the TreeMap stays small while the touched count grows.  Returns (edges, ids used, [mids])."""
    assert len(cs) == a
    edges, mids, v = [], [], base + 1
    for c in cs:
        mids.append(v); edges.append((base, v, 1.0))
        edges += [(v, v + 1 + k, 1.0) for k in range(c)]
        v += 1 + c
    return edges, v - base, mids


def star(base, k, weights=(1.0,)):
    return [(base, base + 1 + i, weights[i % len(weights)]) for i in range(k)], k + 1


def infan(base, first, r):
    """r vertices first..first+r-1, each with one edge -> base: only the reverse pass from `base` reaches them."""
    return [(first + i, base, 1.0) for i in range(r)], r


def bowtie(base, n_out, n_in):
    """`base` with n_out out-neighbours and n_in in-neighbours: undirected, both neighbour loops run more than one 64-lane step."""
    e = [(base, base + 1 + i, 1.0) for i in range(n_out)] + [(base + 1 + n_out + i, base, 1.0) for i in range(n_in)]
    return e, 1 + n_out + n_in


def make_graph(V, edges):
    src = np.array([e[0] for e in edges], np.int64); dst = np.array([e[1] for e in edges], np.int64)
    out, inn = synth.edges_to_csr(V, src, dst, np.array([e[2] for e in edges], np.float32))
    return dict(V=V, out=out, inn=inn)


def _comb_design(cs, base=0):
    def build(base=base):
        e, n, _ = comb(base, len(cs), cs)
        return e, n
    return build


def _split_design(r):
    def build(base=0):
        e, n, _ = comb(base, 7, [60] * 7)
        e2, n2 = infan(base, base + n, r)
        return e + e2, n + n2
    return build


def _star_design(k, weights=(1.0,)):
    return lambda base=0: star(base, k, weights)


TREE_STRIDE = 2048


def tree_edges(base, far):
    """comb(base, 7, [72]*6 + [60]) whose last mid also points at the far leaves: multiples of 2048, which share bin 0 of every
    table length from 64 to 1024 -- the row of `base` is emitted by the exact java.util.HashMap replay."""
    e, n, mids = comb(base, 7, [72] * 6 + [60])
    return e + [(mids[-1], f, 1.0) for f in far], n


def _tree_design(n_far):
    def build(base=0):
        assert base == 0
        e, n = tree_edges(0, [TREE_STRIDE * k for k in range(1, n_far + 1)])
        return e, TREE_STRIDE * n_far + 1
    return build


def _exp(union, peak, row=None, fwd=None):
    d = dict(union=union, peak=peak, row=union if row is None else row)
    if fwd is not None:
        d["fwd"] = fwd
    return d


# name -> (builder(base) -> (edges, ids used), epsilon, expected stats of the root: {directed flag: dict})
DESIGNS = {
    "comb511": (_comb_design([72] * 6 + [71]), EPS, {True: _exp(511, 78, fwd=511), False: _exp(511, 79)}),
    "comb512": (_comb_design([72] * 6 + [72]), EPS, {True: _exp(512, 78, fwd=512), False: _exp(512, 79)}),
    "comb513": (_comb_design([72] * 6 + [73]), EPS, {True: _exp(513, 78, fwd=513), False: _exp(513, 79)}),
    "star383": (_star_design(383), EPS, {True: _exp(384, 383, fwd=384), False: _exp(384, 383)}),
    "star384": (_star_design(384), EPS, {True: _exp(385, 384, fwd=385), False: _exp(385, 384)}),
    "star385": (_star_design(385), EPS, {True: _exp(386, 385, fwd=386), False: _exp(386, 385)}),
    "split511": (_split_design(83), EPS, {True: _exp(511, 83, fwd=428)}),
    "split512": (_split_design(84), EPS, {True: _exp(512, 84, fwd=428)}),
    "split513": (_split_design(85), EPS, {True: _exp(513, 85, fwd=428)}),
    "comb1241": (_comb_design([30] * 40), 1e-4, {True: _exp(1241, 69, fwd=1241), False: _exp(1241, 70)}),
    "tree512": (_tree_design(12), EPS, {True: _exp(512, 78, fwd=512), False: _exp(512, 79)}),
    "tree513": (_tree_design(13), EPS, {True: _exp(513, 78, fwd=513), False: _exp(513, 79)}),
    # the neighbour loops run 64 lanes per step: one full step, one step and one lane, two full steps
    "star64": (_star_design(64), EPS, {True: _exp(65, 64), False: _exp(65, 64)}),
    "star65": (_star_design(65), EPS, {True: _exp(66, 65), False: _exp(66, 65)}),
    "star128": (_star_design(128), EPS, {True: _exp(129, 128), False: _exp(129, 128)}),
    # weights 1, 0.001, 1, ...: 0.9 * 0.001 / 64.064 < eps, so every second lane of both steps is pruned (ballot compaction with holes)
    "holes128": (_star_design(128, (1.0, 0.001)), EPS, {True: _exp(65, 64), False: _exp(65, 64)}),
    # 70 out- and 70 in-neighbours: the undirected pop runs two steps of the first loop and two of the second
    "bowtie70": (lambda base=0: bowtie(base, 70, 70), EPS, {True: _exp(141, 70, fwd=71), False: _exp(141, 140)}),
}


def design(name):
    """(graph, epsilon, expected) of one design standing alone, root = vertex 0."""
    build, eps, expect = DESIGNS[name]
    edges, n = build()
    return make_graph(n, edges), eps, expect


COMPOSITE_EPS = 1e-4       # the 1241 comb needs it; the other designs are built for 1e-3 and are checked in the composite at 1e-4 too
COMPOSITE_ORDER = ["comb513", "star385", "comb512", "star384", "split513", "split512", "comb1241", "tree512"]


def composite():
    """The designs of COMPOSITE_ORDER end to end at ascending bases, a 3-vertex path (a -> b -> c, connected to nothing else) between
    neighbours; the far leaves of the tree row lie above everything else.  Returns (graph, n_low, {name: root vertex})."""
    edges, roots, v = [], {}, 0
    for i, name in enumerate(COMPOSITE_ORDER):
        roots[name] = v
        if name.startswith("tree"):
            n_far = 12
            lo = v + 500 + 1                                    # the comb of the tree row uses 500 ids
            k0 = (lo + TREE_STRIDE - 1) // TREE_STRIDE
            far = [TREE_STRIDE * k for k in range(k0, k0 + n_far)]
            e, n = tree_edges(v, far)
            V = far[-1] + 1
        else:
            e, n = DESIGNS[name][0](v)
        edges += e
        v += n
        if i + 1 < len(COMPOSITE_ORDER):
            edges += [(v, v + 1, 1.0), (v + 1, v + 2, 1.0)]
            v += 3
    assert v <= far[0] and far[-1] < 65536                      # java_hash(2048 k) = 2048 k: bin 0 of every table length up to 2048
    return make_graph(V, edges), v, roots

"""CPU-only checks of the ranking section of include/geglove.h: the exported symbols and the summary structure, the argument
errors that need no device, the `device.rank` key of the C++ host's bean, and the numpy yardstick (tests/rank_ref.py) against a
brute-force double loop."""
import ctypes as C
import os
import re

import numpy as np

from geglove import capi
import rank_ref as R

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
i32p, i64p = C.POINTER(C.c_int32), C.POINTER(C.c_int64)


def test_header_symbols_are_exported():
    header = open(os.path.join(REPO, "include", "geglove.h")).read()
    declared = set(re.findall(r"\b(ge_glove_rank_\w+|ge_rank_\w+)\s*\(", header))
    assert declared == {"ge_glove_rank_create", "ge_glove_rank_run", "ge_rank_last_kernel_ms", "ge_rank_last_phase_ms", "ge_rank_get",
                        "ge_rank_summary_size", "ge_rank_destroy"}
    L = capi.lib()
    for name in declared:
        assert name in capi.SYMBOLS and getattr(L, name) is not None


def test_summary_structure_matches_the_library():
    assert capi.lib().ge_rank_summary_size() == C.sizeof(capi.RankSummary) == 48
    assert [n for n, _ in capi.RankSummary._fields_] == ["n", "mrr", "mean_rank", "hits1", "hits10", "hits100"]


def _create(h, I, J, n, ptr, idx, out=True):
    L = capi.lib()
    I = None if I is None else np.asarray(I, np.int32)
    J = None if J is None else np.asarray(J, np.int32)
    ptr = None if ptr is None else np.asarray(ptr, np.int64)
    idx = None if idx is None else np.asarray(idx, np.int32)
    p = lambda a, t: None if a is None else a.ctypes.data_as(t)
    r = C.c_void_p()
    st = L.ge_glove_rank_create(h, p(I, i32p), p(J, i32p), n, p(ptr, i64p), p(idx, i32p), C.byref(r) if out else None)
    assert r.value is None
    return st, L.ge_last_error().decode()


def test_limits_are_refused_without_a_device():
    """Everything that needs no handle is checked before the handle is looked at, so a null handle reaches each message."""
    ARG = capi.GE_ERR_ARG
    I, J = [0, 1, 2], [2, 1, 0]
    ptr, idx = [0, 2, 2, 3], [0, 5, 1]
    assert _create(None, I, J, 3, ptr, idx) == (ARG, "null ge_glove handle")              # a well-formed set gets as far as the handle
    assert _create(None, I, J, 3, None, None) == (ARG, "null ge_glove handle")
    # null arguments
    assert _create(None, I, J, 3, ptr, idx, out=False)[0] == ARG
    assert _create(None, None, J, 3, ptr, idx) == (ARG, "null rank arrays")
    assert _create(None, I, None, 3, ptr, idx) == (ARG, "null rank arrays")
    assert _create(None, I, J, 3, ptr, None) == (ARG, "filter_idx is null")
    # n
    for n in (0, -1, 2 ** 31):
        st, msg = _create(None, I, J, n, None, None)
        assert st == ARG and "1 <= n < 2^31" in msg, (n, msg)
    # ids out of range
    st, msg = _create(None, [0, -1, 2], J, 3, ptr, idx)
    assert st == ARG and "pair 1: focus row -1 out of range" in msg
    st, msg = _create(None, I, [2, 1, -3], 3, ptr, idx)
    assert st == ARG and "pair 2: column -3 out of range" in msg
    st, msg = _create(None, I, J, 3, ptr, [-1, 5, 1])
    assert st == ARG and "pair 0: filter id -1 out of range" in msg
    # a descending and a repeated filter id
    for bad in ([5, 0, 1], [5, 5, 1]):
        st, msg = _create(None, I, J, 3, ptr, bad)
        assert st == ARG and "pair 0: the filter list is not strictly ascending at entry 1" in msg, (bad, msg)
    # the offsets
    st, msg = _create(None, I, J, 3, [1, 2, 2, 3], idx)
    assert st == ARG and "filter_ptr[0] is 1, not 0" in msg
    st, msg = _create(None, I, J, 3, [0, 2, 1, 3], idx)
    assert st == ARG and "filter_ptr decreases at [2]" in msg
    # the other entry points
    L = capi.lib()
    ms = C.c_float()
    assert L.ge_glove_rank_run(None, None, None, None) == ARG
    assert L.ge_rank_last_kernel_ms(None, C.byref(ms)) == ARG
    assert L.ge_rank_last_phase_ms(None, None, None, None) == ARG
    assert L.ge_rank_get(None, None, None, None, None) == ARG
    L.ge_rank_destroy(None)                                           # harmless


def test_host_configuration_key(tmp_path):
    """`device: { rank: Q }` in the C++ host's bean: an integer >= 0, 0 = off; it needs `holdout` and inherits its refusal of
    several ranks; the banner gains its line only when the key is set."""
    capi._share_hip_runtime_with_torch()
    host = C.CDLL(os.path.join(REPO, "graph-embeddings_amd", "lib", "libgehost.so"))
    host.geh_config_summary.restype = C.c_char_p
    base = "graph: g.nt\nmethod: glove\ndim: 4\nbca:\n  alpha: 0.1\n  epsilon: 0.001\noutput:\n  uri: []\n"
    bad = "ERR\nInvalid configuration: Invalid device.rank, choose a number of held-out nonzeros to rank (0 = off)"
    alone = "ERR\nInvalid configuration: device.rank ranks held-out nonzeros, set device.holdout"
    line = lambda q: "# Rank: %d held-out nonzeros among all columns, training nonzeros filtered" % q
    cases = {"": (None, None), "device:\n  rank: 0\n": (None, None), "device:\n  holdout: 0.2\n": (None, None),
             "device:\n  holdout: 0.2\n  rank: 0\n": (None, None),
             "device:\n  holdout: 0.2\n  rank: 50\n": (None, line(50)), "device:\n  rank: 7\n  holdout: 0.5\n": (None, line(7)),
             "device:\n  rank: 50\n": (alone, None), "device:\n  rank: 50\n  holdout: 0\n": (alone, None),
             "device:\n  holdout: 0.2\n  rank: -1\n": (bad, None), "device:\n  holdout: 0.2\n  rank: 1.5\n": (bad, None),
             "device:\n  holdout: 0.2\n  rank: lots\n": (bad, None), "device:\n  rank: -3\n": (bad, None),
             "device:\n  holdout: 0.2\n  rank: 99999999999\n": (bad, None),
             "device:\n  holdout: 0.2\n  rank: 5\n  gpus: 2\n": ("ERR\nInvalid configuration: device.holdout runs on one rank only, set device.gpus: 1", None)}
    for i, (extra, (err, want)) in enumerate(cases.items()):
        p = tmp_path / ("c%d.yml" % i)
        p.write_text(base + extra)
        out = host.geh_config_summary(str(p).encode(), 1).decode()
        if err:
            assert out == err, (extra, out)
        else:
            assert out.startswith("OK\n") and ("# Rank" in out) == (want is not None) and (want is None or want in out.splitlines()), (extra, out)


def test_the_yardstick_against_a_double_loop():
    """7 pairs x 5 columns with ties, -0 beside +0, a NaN, and filters: empty, holding the target, every column, ending at V - 1."""
    Z = np.array([[1, 1, 1, 1, 1],
                  [3, 2, 2, 5, 2],
                  [0.0, -0.0, 0.0, -1, 0.0],
                  [np.nan, 4, np.nan, -np.inf, 4],
                  [2, 9, 9, 9, 1],
                  [5, 4, 3, 2, 1],
                  [1, 2, 3, 4, 5]], np.float64)
    J = np.array([2, 4, 1, 0, 2, 4, 0])
    lists = [[], [1, 4], [0, 1, 2, 3, 4], [3, 4], [1], [0, 2, 4], [4]]
    for filters in (None, R.csr(lists)):
        want = []
        for k in range(7):
            z = [(-np.inf if np.isnan(v) else v) for v in Z[k]]
            gone = set() if filters is None else set(lists[k])
            rank = 1
            for c in range(5):
                if c == J[k] or c in gone:
                    continue
                if z[c] > z[J[k]] or (z[c] == z[J[k]] and c < J[k]):
                    rank += 1
            want.append(rank)
        assert R.ranks(Z, J, filters).tolist() == want, (filters, want)
    assert R.ranks(Z, J).tolist() == [3, 5, 2, 3, 2, 5, 5]
    assert R.ranks(Z, J, R.csr(lists)).tolist() == [3, 4, 1, 2, 1, 3, 4]
    ptr, idx = R.csr(lists)
    assert ptr.tolist() == [0, 0, 2, 7, 9, 10, 13, 14] and ptr.dtype == np.int64 and idx.dtype == np.int32


def test_summary_of_the_yardstick():
    s = R.summary([1, 2, 4, 200, 10, 11])
    assert s == {"n": 6, "mrr": ((((((0.0 + 1.0) + 0.5) + 0.25) + 1.0 / 200) + 0.1) + 1.0 / 11) / 6, "mean_rank": 228.0 / 6,
                 "hits1": 1, "hits10": 4, "hits100": 5}

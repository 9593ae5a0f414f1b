"""The generator's recipe (include/geglove.h, "Synthetic co-occurrence matrix") in numpy: the yardstick ge_synth_coo is held to,
bit for bit.  Integer and bit operations only, so there is nothing to round: I, J, X and the draw count must be equal bytes.

model(V, row_begin, row_end, nnz, seed) -> (I, J, X, draws), or raises TooDense when the budget of 8 M + 1024 draws does not
hold M = nnz - rows distinct valid keys.  draws = t* + 1, t* = the draw that delivered the M-th key (0 for M = 0).
The draws are evaluated in steps for memory's sake only; the result does not depend on the step (test_synth_abi.py checks that).
Results are cached per argument tuple and returned read-only: the tests share them.
"""
import functools

import numpy as np

from geglove.synth import splitmix64

M32 = np.uint64(0xFFFFFFFF)
U64 = 0xFFFFFFFFFFFFFFFF
X_MAX = np.float32(0.2)


class TooDense(ValueError):
    pass


def check_args(V, row_begin, row_end, nnz):
    """The library's limits; returns (row_begin, row_end) with 0,0 resolved."""
    if V < 1:
        raise ValueError("vocab_size")
    if (row_begin, row_end) == (0, 0):
        row_end = V
    if not 0 <= row_begin < row_end <= V:
        raise ValueError("row range")
    rows = row_end - row_begin
    if not rows <= nnz < 2 ** 31:
        raise ValueError("nnz")
    if nnz - rows > rows * (V - 1):
        raise ValueError("cells")
    return row_begin, row_end


def relabel(V, seed):
    return np.argsort(splitmix64(seed ^ 0x77777777, V), kind="stable").astype(np.int64)


def sigma(seed, row_begin):
    return (seed + 0x1000003 * (row_begin + 1)) & U64


def draws(V, row_begin, row_end, seed, t0, n, rl=None):
    """Draws t0 .. t0 + n - 1: (i, j, valid, c) -- c is what the value is made from."""
    rows = row_end - row_begin
    B = int(V).bit_length()
    rl = relabel(V, seed) if rl is None else rl
    s = sigma(seed, row_begin)
    a = splitmix64(s, n, t0); b = splitmix64(s ^ 0x5A5A5A5A, n, t0); c = splitmix64(s ^ 0x0F0F0F0F, n, t0)
    i = row_begin + (((a >> np.uint64(32)) * np.uint64(rows)) >> np.uint64(32)).astype(np.int64)
    k = (((b >> np.uint64(32)) * np.uint64(B)) >> np.uint64(32)).astype(np.int64)
    lo = (b & M32).astype(np.int64)
    r = (np.int64(1) << k) - 1 + (lo >> (32 - k))            # k = 0: lo >> 32 = 0 on an int64, r = 0
    ok = r < V
    j = rl[np.minimum(r, V - 1)]
    ok &= j != i
    return i, j, ok, c


def value(c):
    """x of a draw from its c: 2^-e (1 + 23 random mantissa bits), e in 3 .. 12, capped at 0.2f."""
    e = 3 + (((c >> np.uint64(32)) * np.uint64(10)) >> np.uint64(32)).astype(np.uint32)
    bits = ((np.uint32(127) - e) << np.uint32(23)) | (c & np.uint64(0x7FFFFF)).astype(np.uint32)
    return np.minimum(bits.view(np.float32), X_MAX)


def _model(V, row_begin, row_end, nnz, seed, step):
    row_begin, row_end = check_args(V, row_begin, row_end, nnz)
    rows = row_end - row_begin
    M = nnz - rows
    budget = 8 * M + 1024
    rl = relabel(V, seed)
    keys = np.zeros(0, np.int64); ts = np.zeros(0, np.int64); cs = np.zeros(0, np.uint64)      # first occurrences so far
    T = 0
    while len(keys) < M:
        if T >= budget:
            raise TooDense("%d of %d distinct keys within %d draws" % (len(keys), M, budget))
        n = min(step or max(1024, M + M // 4), budget - T)
        i, j, ok, c = draws(V, row_begin, row_end, seed, T, n, rl)
        t = np.arange(T, T + n, dtype=np.int64)
        k_all = np.concatenate([keys, ((i - row_begin) * V + j)[ok]])
        t_all = np.concatenate([ts, t[ok]]); c_all = np.concatenate([cs, c[ok]])
        _, first = np.unique(k_all, return_index=True)       # index of the first occurrence: earlier entries win
        first.sort()
        keys, ts, cs = k_all[first], t_all[first], c_all[first]          # ascending t
        T += n
    keys, ts, cs = keys[:M], ts[:M], cs[:M]
    n_draws = int(ts[-1]) + 1 if M else 0
    d = np.arange(rows, dtype=np.int64)
    key = np.concatenate([d * V + (row_begin + d), keys])
    x = np.concatenate([np.full(rows, X_MAX, np.float32), value(cs)])
    o = np.argsort(key, kind="stable")
    key, x = key[o], x[o]
    out = ((row_begin + key // V).astype(np.int32), (key % V).astype(np.int32), x, n_draws)
    for a in out[:3]:
        a.flags.writeable = False
    return out


@functools.lru_cache(maxsize=None)
def model(V, row_begin, row_end, nnz, seed=0xC0FFEE, step=0):
    return _model(V, row_begin, row_end, nnz, seed, step)


def hub_column(J, V, seed=0xC0FFEE):
    """(the column of rank 0, its count, the largest count of any column): rank 0 draws the most, so the first two are the hub."""
    cnt = np.bincount(J, minlength=V)
    hub = int(relabel(V, seed)[0])
    return hub, int(cnt[hub]), int(cnt.max())

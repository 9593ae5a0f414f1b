"""GE_MODE_STRATIFIED restated in numpy from include/geglove.h alone: the partition, the schedule, the keyed bijections and the
sequential order an epoch equals.  The tests hold the device (ge_glove_epoch_order, ge_glove_info) to this file, and the oracle
replays the order it gives."""
import numpy as np

M64 = (1 << 64) - 1
C = (0x9E3779B1, 0x85EBCA6B, 0xC2B2AE35, 0x27D4EB2F)
SHUFFLE_NONE, SHUFFLE_DEVICE = "none", "device"


def default_p(rows, nnz):
    """cfg.strata == 0: the largest power of two P with 8 P^2 <= nnz and P <= rows; at least 1, at most 2048."""
    P = 1
    while P < 2048 and 2 * P <= rows and 8 * (2 * P) * (2 * P) <= nnz:
        P *= 2
    return P


def keys(seed, iteration, salt):
    """K(salt): four 32-bit round keys from SplitMix64 of (seed, iteration, salt)."""
    z = ((seed & M64) * 0x9E3779B97F4A7C15 + (iteration & 0xFFFFFFFF) * 0xD1B54A32D192ED03 + 0x632BE59BD9B4E019
         + salt * 0xA0761D6478BD642F) & M64
    out = []
    for _ in range(4):
        z = (z + 0x9E3779B97F4A7C15) & M64
        t = z
        t = ((t ^ (t >> 30)) * 0xBF58476D1CE4E5B9) & M64
        t = ((t ^ (t >> 27)) * 0x94D049BB133111EB) & M64
        t ^= t >> 31
        out.append(t & 0xFFFFFFFF)
    return out


def bijection(n, key):
    """B(n, key) as the array [B(0), ..., B(n-1)]: a cycle-walked keyed bijection of [0, n)."""
    if n == 0:
        return np.zeros(0, np.int64)
    b = 0
    while (1 << b) < n:
        b += 1
    m = (1 << b) - 1
    sh = b // 2 if b > 1 else 1

    def R(y):
        for q in range(4):
            y = (y + key[q]) & m
            y = (y * C[q]) & m
            y = y ^ (y >> sh)
        return y

    y = R(np.arange(n, dtype=np.uint64))
    while True:
        out = y >= n
        if not out.any():
            return y.astype(np.int64)
        y[out] = R(y[out])


def partition(I, J, P):
    """(rb, cb) per nonzero: rb = (r(I[k]) * P) // N with r(i) the nonzeros in rows below i; likewise the columns."""
    I = np.asarray(I, np.int64); J = np.asarray(J, np.int64)
    N = len(I)
    if N == 0:
        return np.zeros(0, np.int64), np.zeros(0, np.int64)
    V = int(max(I.max(), J.max())) + 1
    r = np.concatenate(([0], np.cumsum(np.bincount(I, minlength=V))))
    c = np.concatenate(([0], np.cumsum(np.bincount(J, minlength=V))))
    return (r[I] * P) // N, (c[J] * P) // N


class Model:
    """The layout of one handle: tiles[T] = the nonzeros (indices into I / J / X) of tile T = a * P + b in ascending k."""

    def __init__(self, I, J, P):
        self.P, self.N = P, len(I)
        self.I, self.J = np.asarray(I, np.int64), np.asarray(J, np.int64)
        rb, cb = partition(I, J, P)
        assert self.N == 0 or (rb.max() < P and cb.max() < P)
        tile = rb * P + cb
        order = np.argsort(tile, kind="stable")
        counts = np.bincount(tile, minlength=P * P) if self.N else np.zeros(P * P, np.int64)
        self.off = np.concatenate(([0], np.cumsum(counts)))
        self.sorted = order
        self.counts = counts.reshape(P, P)

    def tile(self, a, b):
        T = a * self.P + b
        return self.sorted[self.off[T]:self.off[T + 1]]

    def sub_epoch(self, s):
        """[(tile id, its nonzeros)] of sub-epoch s, a ascending."""
        P = self.P
        return [(a * P + (a + s) % P, self.tile(a, (a + s) % P)) for a in range(P)]

    @property
    def path(self):
        """strata_path = sum over sub-epochs of the largest tile."""
        P = self.P
        a = np.arange(P)
        return int(sum(self.counts[a, (a + s) % P].max() for s in range(P)))

    @property
    def ideal(self):
        return -(-self.N // self.P)

    def sub_epoch_order(self, seed, iteration, shuffle):
        if shuffle == SHUFFLE_NONE:
            return list(range(self.P))
        return [int(v) for v in bijection(self.P, keys(seed, iteration, 0))]

    def jobs(self, seed, iteration, shuffle):
        """The tiles of epoch `iteration` in the order of the sequential equivalent, each as the array of its nonzeros in the
        order its wavefront walks them (empty tiles included: a job with cost 0)."""
        out = []
        for s in self.sub_epoch_order(seed, iteration, shuffle):
            for T, nz in self.sub_epoch(s):
                if shuffle == SHUFFLE_DEVICE and len(nz):
                    nz = nz[bijection(len(nz), keys(seed, iteration, T + 1))]
                out.append(nz)
        return out

    def epoch_order(self, seed, iteration, shuffle):
        jobs = self.jobs(seed, iteration, shuffle)
        return np.concatenate(jobs).astype(np.int64) if jobs else np.zeros(0, np.int64)

    def launches(self):
        """Sub-epochs that hold a nonzero: what an epoch launches."""
        P = self.P
        a = np.arange(P)
        return int(sum(self.counts[a, (a + s) % P].max() > 0 for s in range(P)))

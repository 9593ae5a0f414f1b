"""The yardstick of the clustering tests: the "Clustering" section of include/geglove.h in numpy, operation for operation.
Never the library itself.

Sums whose order the header fixes are taken in that order: `seq_sum` adds slices one after the other from 0.0 (np.cumsum would
do the same but starts from its first element, which loses the sign of a -0.0).

The bound B(dim, row, centroid) on |z - t|, t the fp64 value of xh . cen - 0.5 |cen|^2 (cosine: of xh . cen), xh the PREPARED
row (an fp32 vector, which `prepare` gives bit for bit), u = 2^-24 the unit roundoff of fp32:
    s   the fmaf chain of length dim rounds once per step:  |s - xh . cen| <= gamma_dim sum_d |xh_d| |cen_d| <= gamma_dim |xh| |cen|,
        gamma_dim = dim u / (1 - dim u) <= (dim + 1/2) u at dim <= 1024;
    h   q is an fp64 chain (relative error <= (dim + 1) 2^-53), then one product by -0.5 (exact) and one rounding to fp32:
        |h + 0.5 |cen|^2| <= (u + dim 2^-52) 0.5 |cen|^2;   cosine: h = 0 exactly;
    z   one fp32 add:  |z - (s + h)| <= u (|s| + |h|) <= u (1 + gamma_dim) |xh| |cen| + u (1 + 2 u) 0.5 |cen|^2.
Together |z - t| <= ((dim + 1/2) u + u (1 + dim u + u)) |xh| |cen| + (2 u + 2 u^2 + dim 2^-52) 0.5 |cen|^2, which at dim <= 1024 is
below
    B = (dim + 2) u |xh| |cen| + 1.5 u |cen|^2          (cosine: B = (dim + 2) u |xh| |cen|, z = s + 0.0f being exact).
The chain's bound needs products that do not underflow: `bound` asserts that the smallest nonzero |xh_d| times the smallest
nonzero |cen_d| is a normal fp32 number.

Two centroids whose t differ by more than 2 B keep their order under any z within B of t; closer ones may come out either way."""
import numpy as np

from geglove import synth

U = 2.0 ** -24
TINY = float(np.finfo(np.float32).tiny)
PIECE = 1024
INIT_KEY = 0x4B4D45414E53
COSINE, EUCLID = "cosine", "euclid"


def seq_sum(A, axis):
    """The sum along `axis` in ascending index order, from 0.0, in the dtype of A."""
    A = np.moveaxis(np.asarray(A), axis, 0)
    s = np.zeros(A.shape[1:], A.dtype)
    for a in A:
        s = s + a
    return s


def prepare(X, metric):
    """The prepared rows, fp32: cosine divides by the fp64 norm accumulated in ascending d and rounds once; a zero row stays zero."""
    X = np.ascontiguousarray(X, np.float32)
    if metric == EUCLID:
        return X.copy()
    X64 = X.astype(np.float64)
    nrm = np.sqrt(seq_sum(X64 * X64, 1))
    out = np.zeros_like(X)
    nz = nrm > 0
    out[nz] = (X64[nz] / nrm[nz, None]).astype(np.float32)
    return out


def bias(cen, metric):
    """h_c, fp32."""
    cen = np.asarray(cen, np.float32)
    if metric == COSINE:
        return np.zeros(cen.shape[0], np.float32)
    c64 = cen.astype(np.float64)
    return (-0.5 * seq_sum(c64 * c64, 1)).astype(np.float32)


def exact_scores(XH, cen, metric):
    """z for inputs on which every product, partial sum and the final add are exact in fp32 (asserted): then the fmaf chain
    equals the fp64 matrix product.  Returns fp32 [n, K]."""
    XH = np.asarray(XH, np.float32).astype(np.float64)
    C = np.asarray(cen, np.float32).astype(np.float64)
    h = bias(cen, metric).astype(np.float64)
    assert np.array_equal(XH, np.rint(XH)) and np.array_equal(C, np.rint(C)), "the exact tier takes integers"
    assert (np.abs(XH) @ np.abs(C).T).max() < 2 ** 23, "a partial sum may not be exact"
    assert np.array_equal(2 * h, np.rint(2 * h)) and np.abs(h).max(initial=0) < 2 ** 22
    if metric == EUCLID:
        assert np.array_equal(h, -0.5 * (C * C).sum(axis=1))
    Z = XH @ C.T + h[None, :]
    assert np.array_equal(Z.astype(np.float32).astype(np.float64), Z), "a z is not representable"
    return Z.astype(np.float32)


def assign(Z):
    """label and best by the definition: the first centroid of a stable sort of -z, a NaN counting as -inf."""
    Z = np.array(Z, np.float32)
    Z[np.isnan(Z)] = -np.inf
    label = np.empty(Z.shape[0], np.int32)
    for p in range(Z.shape[0]):
        label[p] = np.argsort(-Z[p], kind="stable")[0]
    return label, Z[np.arange(Z.shape[0]), label]


def cluster_sums(XH, labels, K):
    """S_c[d] in fp64 over the stated partition, and n_c."""
    X64 = np.asarray(XH, np.float32).astype(np.float64)
    S = np.zeros((K, X64.shape[1]), np.float64)
    count = np.zeros(K, np.int64)
    for c in range(K):
        members = np.flatnonzero(np.asarray(labels) == c)             # ascending position
        count[c] = members.size
        pieces = [seq_sum(X64[members[i:i + PIECE]], 0) for i in range(0, members.size, PIECE)]
        if pieces:
            S[c] = seq_sum(np.stack(pieces), 0)
    return S, count


def update(XH, labels, cen, metric):
    """The centroids after the update (fp32), from the prepared rows, the labels and the centroids before it."""
    cen = np.asarray(cen, np.float32)
    S, count = cluster_sums(XH, labels, cen.shape[0])
    out = cen.copy()
    for c in range(cen.shape[0]):
        if count[c] == 0:
            continue
        if metric == EUCLID:
            out[c] = (S[c] / np.float64(count[c])).astype(np.float32)
        else:
            m = np.sqrt(seq_sum(S[c] * S[c], 0))
            if m == 0:
                continue
            out[c] = (S[c] / m).astype(np.float32)
    return out


def partition_sum(v):
    """The fp64 sum over blocks of 1024 positions, each from 0.0 in ascending order, then over the blocks in ascending order."""
    v = np.asarray(v, np.float64)
    blocks = [seq_sum(v[i:i + PIECE], 0) for i in range(0, v.size, PIECE)]
    return float(seq_sum(np.array(blocks, np.float64), 0))


def objective(best):
    """The partition sum of the best scores (fp32 values, widened exactly)."""
    return partition_sum(np.asarray(best, np.float32).astype(np.float64))


def initial_positions(seed, n, K):
    """The K positions with the smallest (SM(seed ^ INIT_KEY, p), p), in that order."""
    key = synth.splitmix64((seed ^ INIT_KEY) & (2 ** 64 - 1), n)
    return np.argsort(key, kind="stable")[:K].astype(np.int64)


def norms(A):
    A = np.asarray(A, np.float32).astype(np.float64)
    return np.sqrt((A * A).sum(axis=1))


def bound(XH, cen, metric):
    """B[p, c] of the docstring; asserts the inputs keep clear of the subnormal range."""
    XH, cen = np.asarray(XH, np.float32), np.asarray(cen, np.float32)
    ax, ac = np.abs(XH[XH != 0]).astype(np.float64), np.abs(cen[cen != 0]).astype(np.float64)
    assert ax.size == 0 or ac.size == 0 or ax.min() * ac.min() >= TINY, "a product may underflow: rescale the input"
    dim = XH.shape[1]
    assert 1 <= dim <= 1024
    nx, nc = norms(XH), norms(cen)
    B = (dim + 2) * U * nx[:, None] * nc[None, :]
    if metric == EUCLID:
        B = B + 1.5 * U * (nc * nc)[None, :]
    return B


def truth(XH, cen, metric):
    """t[p, c] in fp64."""
    X64, C64 = np.asarray(XH, np.float32).astype(np.float64), np.asarray(cen, np.float32).astype(np.float64)
    T = X64 @ C64.T
    if metric == EUCLID:
        T = T - 0.5 * (C64 * C64).sum(axis=1)[None, :]
    return T


def check_bracket(XH, cen, metric, labels, best):
    """For EVERY row: best within B of t(label), and t(label) >= max_c t - 2 B.  Returns the largest |best - t| / B seen."""
    T, B = truth(XH, cen, metric), bound(XH, cen, metric)
    n, K = T.shape
    labels = np.asarray(labels)
    assert labels.shape == (n,) and labels.min() >= 0 and labels.max() < K
    rows = np.arange(n)
    t, b = T[rows, labels], B[rows, labels]
    err = np.abs(np.asarray(best, np.float32).astype(np.float64) - t)
    assert np.all(err <= b), "a best score is %.3g B from the fp64 value of its label" % (err / np.maximum(b, 1e-300)).max()
    # the winner c* against any rival c: z(c*) >= z(c), |z - t| <= B for both, so t(c*) >= t(c) - B(c*) - B(c)
    assert np.all(t[:, None] >= T - b[:, None] - B), "a row's label loses to another centroid by more than the two bounds"
    assert np.all(t >= T.max(axis=1) - 2 * B.max(axis=1)), "a label is more than 2 B below the best centroid"
    return float((err / np.maximum(b, 1e-300)).max())

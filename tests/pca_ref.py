"""The yardstick of the PCA tests: numpy in fp64 on the same fp32 input, the designed inputs, and the derived tolerances.
Never the library itself.  (u32 = 2^-24, u64 = 2^-53: the unit roundoffs of the two formats.)"""
import numpy as np

from geglove import synth

U32 = 2.0 ** -24
U64 = 2.0 ** -53

# (n, D, ratio, offset): variances fall geometrically, so the spectrum is well separated and 0.95 lies between two shares
DESIGNED = ((20000, 48, 0.8, 0.0), (20000, 48, 0.8, 100.0), (50000, 200, 0.93, 0.3))


def unit_uniform(seed, shape):
    """Uniform with mean 0 and variance 1 from SplitMix64."""
    n = int(np.prod(shape))
    u = (synth.splitmix64(seed, n) >> np.uint64(11)).astype(np.float64) * (1.0 / 9007199254740992.0)
    return ((u - 0.5) * np.sqrt(12.0)).reshape(shape)


def orthogonal(seed, D):
    q, r = np.linalg.qr(unit_uniform(seed, (D, D)))
    return q * np.sign(np.diag(r))            # a unique factor, whatever LAPACK's sign convention


def designed_input(n, D, ratio, offset, seed=2024):
    """X = ((Z * s) @ Q.T + offset) as fp32, s[d] = ratio^(d/2)."""
    Z = unit_uniform(seed, (n, D))
    Q = orthogonal(seed ^ 0x51ED, D)
    s = ratio ** (np.arange(D) / 2.0)
    return ((Z * s) @ Q.T + offset).astype(np.float32)


def spd(D, ratio=0.8, seed=7):
    """Q diag(ratio^d) Q^T, symmetric to the last bit."""
    Q = orthogonal(seed + D, D)
    C = (Q * ratio ** np.arange(D)) @ Q.T
    return (C + C.T) / 2


def fix_signs(W):
    """In every column the entry of largest magnitude is positive (lowest index on a tie)."""
    W = W.copy()
    big = np.argmax(np.abs(W), axis=0)
    W[:, W[big, np.arange(W.shape[1])] < 0] *= -1
    return W


def k_rule(lam, variance, max_components=0):
    """Smallest k >= 1 with the leading k eigenvalues summing to >= variance * total, in fp64, in that order."""
    total = 0.0
    for v in lam:
        total += float(v)
    k = 1
    if total > 0:
        cum, k = 0.0, len(lam)
        for c, v in enumerate(lam):
            cum += float(v)
            if cum >= variance * total:
                k = c + 1
                break
    return min(k, max_components) if max_components > 0 else k


def eig_desc(C):
    lam, W = np.linalg.eigh(C)
    lam, W = lam[::-1].copy(), W[:, ::-1].copy()
    return np.maximum(lam, 0.0), fix_signs(W)


def numpy_pca(X, variance=0.95):
    X = np.asarray(X, np.float32).astype(np.float64)
    n = X.shape[0]
    mean = X.sum(axis=0) / n
    Xc = X - mean
    cov = (Xc.T @ Xc) / (n - 1)
    lam, W = eig_desc(cov)
    k = k_rule(lam, variance)
    return dict(mean=mean, cov=cov, lam=lam, W=W, k=k, Xc=Xc, out=Xc @ W[:, :k])


def share_margin(lam, k, variance=0.95):
    """Distance of `variance` from the cumulative shares at k - 1 and at k (k must be unambiguous before it is asserted)."""
    total = lam.sum()
    if total == 0:
        return 1.0
    cum = np.cumsum(lam) / total
    below = variance - (cum[k - 2] if k >= 2 else 0.0)
    return min(below, cum[k - 1] - variance)


def mean_bound(X):
    """Any fp64 summation of n terms: n * 2 u64 * sum|x| / n."""
    return 2 * U64 * np.abs(X.astype(np.float64)).sum(axis=0)


def cov_bound(X):
    """n * 2 u64 * sqrt(M_aa M_bb) / (n - 1) with M the UNCENTRED sums of squares: covers a one-pass and a two-pass scheme."""
    X = X.astype(np.float64)
    n = X.shape[0]
    M = (X * X).sum(axis=0)
    return n * 2 * U64 * np.sqrt(np.outer(M, M)) / (n - 1)


def transform_bound(ref, cov_lib):
    """Per row: (D + 2) u32 |x - mean| + |x - mean| (2 |dC|_2 + 4 D 2 u64 lmax) / gap; gap = the smallest difference of consecutive
    numpy eigenvalues among the first k + 1."""
    D = ref["cov"].shape[0]
    norms = np.linalg.norm(ref["Xc"], axis=1)
    first = (D + 2) * U32 * norms
    lead = ref["lam"][:ref["k"] + 1]
    if len(lead) < 2:
        return first[:, None]
    gap = np.min(-np.diff(lead))
    dC = np.linalg.norm(cov_lib - ref["cov"], 2)
    second = norms * (2 * dC + 4 * D * 2 * U64 * ref["lam"][0]) / gap
    return (first + second)[:, None]


def solver_ratios(C, lam, W):
    """Scaled residual |C W - W L|_max / (D 2 u64 lmax) and scaled orthogonality |W^T W - I|_max / (D 2 u64)."""
    D = C.shape[0]
    lmax = max(float(np.max(np.abs(lam))), np.finfo(float).tiny)
    resid = np.max(np.abs(C @ W - W * lam)) / (D * 2 * U64 * lmax)
    orth = np.max(np.abs(W.T @ W - np.eye(D))) / (D * 2 * U64)
    return resid, orth
